/*
 * shims_hevc_inter.hip — ffhip_hevc_inter_pictures_dev(): validates what the host can see of a picture set (geometry, planes, the
 * DPB tables, reference / destination overlap) and launches the inter reconstruction (kernels/hevc_inter_pic.hip) on the caller's
 * stream.  The records themselves are device data and are checked by the kernel.
 */
#include <algorithm>
#include <stdint.h>
#include <vector>

#include "kernels/common.h"
#include "kernels/h264_kernels.h"

extern "C" int ffhip_hevc_inter_pu_record_size(void) { return (int)sizeof(FFHipHevcInterPU); }
extern "C" int ffhip_hevc_inter_tu_record_size(void) { return (int)sizeof(FFHipHevcInterTU); }
extern "C" int ffhip_hevc_inter_slice_record_size(void) { return (int)sizeof(FFHipHevcInterSlice); }

namespace {
struct Span { /* the bytes a plane occupies: [lo, hi) */
    uintptr_t lo, hi;
};
Span plane_span(const void *base, ptrdiff_t stride, int w_bytes, int rows)
{
    const uintptr_t b = (uintptr_t)base;
    return { b, b + (uintptr_t)((ptrdiff_t)(rows - 1) * stride + w_bytes) };
}
} // namespace

extern "C" int ffhip_hevc_inter_pictures_dev(int bit_depth, int chroma_format_idc, int width, int height, int log2_ctb_size, int npics,
                                             const FFHipHevcInterPic *pics, void *stream)
{
    if ((bit_depth != 8 && bit_depth != 10 && bit_depth != 12) || chroma_format_idc < 0 || chroma_format_idc > 3 || log2_ctb_size < 4 ||
        log2_ctb_size > 6) {
        ffhip_set_error("ffhip_hevc_inter_pictures_dev: bit depth %d (8, 10 or 12), chroma format %d (0..3), log2 CTB size %d (4..6)",
                        bit_depth, chroma_format_idc, log2_ctb_size);
        return FFHIP_EINVAL;
    }
    if (width <= 0 || height <= 0 || width > 65535 || height > 65535 || (width | height) & 7) {
        ffhip_set_error("ffhip_hevc_inter_pictures_dev: picture size %d x %d (multiples of 8, at most 65535)", width, height);
        return FFHIP_EINVAL;
    }
    if (npics <= 0 || !pics) {
        ffhip_set_error("ffhip_hevc_inter_pictures_dev: npics = %d, or a NULL picture array", npics);
        return FFHIP_EINVAL;
    }
    const int ps = bit_depth > 8 ? 2 : 1, nplanes = chroma_format_idc ? 3 : 1;
    const unsigned amask = 4u * ps - 1; /* four samples per access */
    int pw[3], ph[3];
    for (int p = 0; p < 3; p++) {
        pw[p] = p && chroma_format_idc != 3 ? width >> 1 : width;
        ph[p] = p && chroma_format_idc == 1 ? height >> 1 : height;
    }
    for (int i = 0; i < npics; i++) {
        const FFHipHevcInterPic &P = pics[i];
        if (!P.pus || !P.pu_ctb_start || (P.nslices > 0 && !P.slices) || P.nslices < 0 || P.nrefs < 0 || P.nrefs > 16) {
            ffhip_set_error("ffhip_hevc_inter_pictures_dev: picture %d: NULL PU / slice tables, nslices = %d or nrefs = %d (0..16)", i,
                            P.nslices, P.nrefs);
            return FFHIP_EINVAL;
        }
        for (int p = 0; p < nplanes; p++) {
            const FFHipHevcInterPlane &D = P.plane[p];
            if (!D.base || !D.tus || !D.tu_ctb_start || !D.res) {
                ffhip_set_error("ffhip_hevc_inter_pictures_dev: picture %d plane %d: a NULL pointer", i, p);
                return FFHIP_EINVAL;
            }
            if ((((uintptr_t)D.base | (size_t)D.stride) & amask) || D.stride < (ptrdiff_t)pw[p] * ps) {
                ffhip_set_error("ffhip_hevc_inter_pictures_dev: picture %d plane %d: base and stride must be %u-byte aligned, the stride at "
                                "least the plane's width", i, p, amask + 1);
                return FFHIP_EINVAL;
            }
            for (int r = 0; r < P.nrefs; r++) {
                const uint8_t *b = P.ref[r].base[p];
                const ptrdiff_t s = P.ref[r].stride[p];
                if (!b || (((uintptr_t)b | (size_t)s) & (ps - 1)) || s < (ptrdiff_t)pw[p] * ps) {
                    ffhip_set_error("ffhip_hevc_inter_pictures_dev: picture %d reference %d plane %d: NULL, misaligned or a stride below "
                                    "the width", i, r, p);
                    return FFHIP_EINVAL;
                }
            }
        }
    }
    /* no reference plane of the call may be a destination plane of the call: a launch's pictures are predicted side by side.  The
     * destination spans are sorted by start with a running maximum of their ends, so each reference span is one binary search */
    std::vector<Span> dst;
    dst.reserve((size_t)npics * nplanes);
    for (int i = 0; i < npics; i++)
        for (int p = 0; p < nplanes; p++)
            dst.push_back(plane_span(pics[i].plane[p].base, pics[i].plane[p].stride, pw[p] * ps, ph[p]));
    std::sort(dst.begin(), dst.end(), [](const Span &x, const Span &y) { return x.lo < y.lo; });
    std::vector<uintptr_t> hi_max(dst.size());
    for (size_t k = 0; k < dst.size(); k++)
        hi_max[k] = k ? std::max(hi_max[k - 1], dst[k].hi) : dst[k].hi;
    for (int j = 0; j < npics; j++)
        for (int r = 0; r < pics[j].nrefs; r++)
            for (int q = 0; q < nplanes; q++) {
                const Span s = plane_span(pics[j].ref[r].base[q], pics[j].ref[r].stride[q], pw[q] * ps, ph[q]);
                /* the destinations that start before s ends; one of them overlaps s iff the largest end among them is past s.lo */
                const size_t n = (size_t)(std::lower_bound(dst.begin(), dst.end(), s.hi, [](const Span &x, uintptr_t v) { return x.lo < v; }) -
                                          dst.begin());
                if (n && hi_max[n - 1] > s.lo) {
                    ffhip_set_error("ffhip_hevc_inter_pictures_dev: picture %d reference %d plane %d overlaps a plane the call writes", j, r, q);
                    return FFHIP_EINVAL;
                }
            }
    if (!ffhip_have_device())
        return FFHIP_ENOSYS;
    return ffhip_launch_hevc_inter_pictures(bit_depth, chroma_format_idc, width, height, log2_ctb_size, npics, pics, (hipStream_t)stream);
}
