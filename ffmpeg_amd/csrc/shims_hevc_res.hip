/*
 * shims_hevc_res.hip — ffhip_hevc_residual_pictures_dev(): the host checks (depth, format, the planes' pointers, alignment and
 * lengths, the size groups, and that no res range of the call overlaps a coeffs range or another plane's res range) and the launch of
 * the residual kernel (kernels/hevc_res_pic.hip) on the caller's stream.  The records themselves are device data and are checked by
 * the kernel against the lengths.
 */
#include "kernels/common.h"
#include "kernels/h264_kernels.h"
#include "kernels/picture_check.h"

extern "C" int ffhip_hevc_res_tu_record_size(void) { return (int)sizeof(FFHipHevcResTU); }

extern "C" int ffhip_hevc_residual_pictures_dev(int bit_depth, int chroma_format_idc, int npics, const FFHipHevcResPic *pics, void *stream)
{
    static const char who[] = "ffhip_hevc_residual_pictures_dev";
    if (const int r = ffhip_check_hevc_format(who, bit_depth, chroma_format_idc))
        return r;
    if (const int r = ffhip_check_count(who, npics, pics, "picture"))
        return r;
    const int nplanes = chroma_format_idc ? 3 : 1;
    FFHipSpanSet res; /* the used planes' res ranges, and their coeffs ranges in the order of the call */
    std::vector<FFHipSpan> coe;
    for (int i = 0; i < npics; i++)
        for (int p = 0; p < nplanes; p++) {
            const FFHipHevcResPlane &D = pics[i].plane[p];
            if (D.ncoeffs < 0 || D.nres < 0 || D.size_start[0] != 0) {
                ffhip_set_error("%s: picture %d plane %d: ncoeffs %d / nres %d negative, or size_start[0] = %d (must be 0)", who, i, p, D.ncoeffs,
                                D.nres, D.size_start[0]);
                return FFHIP_EINVAL;
            }
            for (int s = 0; s < 4; s++)
                if (D.size_start[s + 1] < D.size_start[s]) {
                    ffhip_set_error("%s: picture %d plane %d: size_start decreases at %d", who, i, p, s + 1);
                    return FFHIP_EINVAL;
                }
            if (!D.size_start[4])
                continue; /* no records: the plane is not looked at */
            if (!D.coeffs || !D.res || !D.tus || (((uintptr_t)D.coeffs | (uintptr_t)D.res | (uintptr_t)D.tus) & 15)) {
                ffhip_set_error("%s: picture %d plane %d: coeffs, res and tus must be non-NULL and 16-byte aligned", who, i, p);
                return FFHIP_EINVAL;
            }
            res.add(ffhip_plane_span(D.res, 0, (ptrdiff_t)D.nres * (ptrdiff_t)sizeof(*D.res), 1));
            coe.push_back(ffhip_plane_span(D.coeffs, 0, (ptrdiff_t)D.ncoeffs * (ptrdiff_t)sizeof(*D.coeffs), 1));
        }
    /* no res range may overlap another res range or any coeffs range of the call (coeffs ranges may be shared: they are only read) */
    if (res.seal()) {
        ffhip_set_error("%s: two res ranges of the call overlap", who);
        return FFHIP_EINVAL;
    }
    for (const FFHipSpan &s : coe)
        if (res.hits(s)) {
            ffhip_set_error("%s: a res range overlaps a coeffs range of the call", who);
            return FFHIP_EINVAL;
        }
    if (!ffhip_have_device())
        return FFHIP_ENOSYS;
    return ffhip_launch_hevc_residual_pictures(bit_depth, chroma_format_idc, npics, pics, (hipStream_t)stream);
}
