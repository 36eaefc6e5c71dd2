/*
 * shims_hevc_res.hip — ffhip_hevc_residual_pictures_dev(): validates what the host can see of a picture set (depth, format, the
 * planes' pointers, alignment and lengths, the size groups, and that no res range of the call overlaps a coeffs range or another
 * plane's res range) and launches the residual kernel (kernels/hevc_res_pic.hip) on the caller's stream.  The records themselves are
 * device data and are checked by the kernel against the lengths.
 */
#include <algorithm>
#include <stdint.h>
#include <vector>

#include "kernels/common.h"
#include "kernels/h264_kernels.h"

extern "C" int ffhip_hevc_res_tu_record_size(void) { return (int)sizeof(FFHipHevcResTU); }

namespace {
struct Span { /* the bytes a range occupies: [lo, hi) */
    uintptr_t lo, hi;
};
} // namespace

extern "C" int ffhip_hevc_residual_pictures_dev(int bit_depth, int chroma_format_idc, int npics, const FFHipHevcResPic *pics, void *stream)
{
    if ((bit_depth != 8 && bit_depth != 10 && bit_depth != 12) || chroma_format_idc < 0 || chroma_format_idc > 3) {
        ffhip_set_error("ffhip_hevc_residual_pictures_dev: bit depth %d (8, 10 or 12), chroma format %d (0..3)", bit_depth, chroma_format_idc);
        return FFHIP_EINVAL;
    }
    if (npics <= 0 || !pics) {
        ffhip_set_error("ffhip_hevc_residual_pictures_dev: npics = %d, or a NULL picture array", npics);
        return FFHIP_EINVAL;
    }
    const int nplanes = chroma_format_idc ? 3 : 1;
    std::vector<Span> res, coe; /* the used planes' ranges */
    for (int i = 0; i < npics; i++)
        for (int p = 0; p < nplanes; p++) {
            const FFHipHevcResPlane &D = pics[i].plane[p];
            if (D.ncoeffs < 0 || D.nres < 0 || D.size_start[0] != 0) {
                ffhip_set_error("ffhip_hevc_residual_pictures_dev: picture %d plane %d: ncoeffs %d / nres %d negative, or size_start[0] = %d "
                                "(must be 0)", i, p, D.ncoeffs, D.nres, D.size_start[0]);
                return FFHIP_EINVAL;
            }
            for (int s = 0; s < 4; s++)
                if (D.size_start[s + 1] < D.size_start[s]) {
                    ffhip_set_error("ffhip_hevc_residual_pictures_dev: picture %d plane %d: size_start decreases at %d", i, p, s + 1);
                    return FFHIP_EINVAL;
                }
            if (!D.size_start[4])
                continue; /* no records: the plane is not looked at */
            if (!D.coeffs || !D.res || !D.tus || (((uintptr_t)D.coeffs | (uintptr_t)D.res | (uintptr_t)D.tus) & 15)) {
                ffhip_set_error("ffhip_hevc_residual_pictures_dev: picture %d plane %d: coeffs, res and tus must be non-NULL and 16-byte "
                                "aligned", i, p);
                return FFHIP_EINVAL;
            }
            res.push_back({ (uintptr_t)D.res, (uintptr_t)(D.res + D.nres) });
            coe.push_back({ (uintptr_t)D.coeffs, (uintptr_t)(D.coeffs + D.ncoeffs) });
        }
    /* no res range may overlap another res range or any coeffs range of the call: the res spans are sorted by start (empty ones
     * overlap nothing), neighbours checked with a running maximum of the ends, and each coeffs span is one binary search */
    res.erase(std::remove_if(res.begin(), res.end(), [](const Span &x) { return x.lo == x.hi; }), res.end());
    std::sort(res.begin(), res.end(), [](const Span &x, const Span &y) { return x.lo < y.lo; });
    std::vector<uintptr_t> hi_max(res.size());
    for (size_t k = 0; k < res.size(); k++) {
        if (k && hi_max[k - 1] > res[k].lo) {
            ffhip_set_error("ffhip_hevc_residual_pictures_dev: two res ranges of the call overlap");
            return FFHIP_EINVAL;
        }
        hi_max[k] = k ? std::max(hi_max[k - 1], res[k].hi) : res[k].hi;
    }
    for (const Span &s : coe) {
        if (s.lo == s.hi)
            continue;
        const size_t n = (size_t)(std::lower_bound(res.begin(), res.end(), s.hi, [](const Span &x, uintptr_t v) { return x.lo < v; }) -
                                  res.begin());
        if (n && hi_max[n - 1] > s.lo) {
            ffhip_set_error("ffhip_hevc_residual_pictures_dev: a res range overlaps a coeffs range of the call");
            return FFHIP_EINVAL;
        }
    }
    if (!ffhip_have_device())
        return FFHIP_ENOSYS;
    return ffhip_launch_hevc_residual_pictures(bit_depth, chroma_format_idc, npics, pics, (hipStream_t)stream);
}
