/*
 * shims_h264_inter.hip — ffhip_h264_inter_pictures_dev(): the host checks (format, geometry, pointers and strides, the row-wise
 * overlap rule of destination and reference planes) and the launch of kernels/h264_inter_pic.hip on the caller's stream; and the
 * device-free faces: ffhip_h264_inter_plan_pictures_host(), the plan of every block by the function the kernel uses
 * (kernels/h264_inter_rules.h) on host arrays, and the record sizes.
 */
#include <string.h>

#include "kernels/common.h"
#include "kernels/h264_kernels.h"
#include "kernels/h264_inter_rules.h"
#include "kernels/picture_check.h"

extern "C" int ffhip_h264_inter_slice_record_size(void) { return (int)sizeof(FFHipH264InterSlice); }
extern "C" int ffhip_h264_inter_ref_record_size(void) { return (int)sizeof(FFHipH264InterRef); }
extern "C" int ffhip_h264_inter_pic_record_size(void) { return (int)sizeof(FFHipH264InterPic); }
extern "C" int ffhip_h264_inter_plan_record_size(void) { return (int)sizeof(FFHipH264InterBlockPlan); }
extern "C" int ffhip_h264_inter_plan_pic_record_size(void) { return (int)sizeof(FFHipH264InterPlanPic); }

namespace {
/* the arguments both faces share */
int check_common(const char *who, int mb_w, int mb_h, int npics, const void *pics)
{
    if (mb_w < 1 || mb_h < 1 || mb_w > 4096 || mb_h > 4096) {
        ffhip_set_error("%s: %d x %d macroblocks (1..4096 each)", who, mb_w, mb_h);
        return FFHIP_EINVAL;
    }
    return ffhip_check_count(who, npics, pics, "picture");
}
int check_maps(const char *who, int i, int mb_w, const void *mb, const void *mvf, const void *slices, int mvf_stride, int nslices, int nrefs)
{
    if (!mb || !mvf || !slices || ((uintptr_t)mvf & 3) || mvf_stride < 4 * mb_w || nslices < 1 || nrefs < 0 || nrefs > 32) {
        ffhip_set_error("%s: picture %d: a NULL mb, mvf or slices, an mvf that is not 4-byte aligned, mvf_stride %d (>= %d), nslices %d (>= 1) "
                        "or nrefs %d (0..32)", who, i, mvf_stride, 4 * mb_w, nslices, nrefs);
        return FFHIP_EINVAL;
    }
    return 0;
}

int check_dev(const char *who, int bit_depth, int chroma_format_idc, int mb_w, int mb_h, int npics, const FFHipH264InterPic *pics)
{
    if (chroma_format_idc == 2 || chroma_format_idc == 3) {
        ffhip_set_error("%s: chroma_format_idc %d: 4:2:2 and 4:4:4 are not implemented (0 or 1)", who, chroma_format_idc);
        return FFHIP_ENOSYS;
    }
    if ((bit_depth != 8 && bit_depth != 9 && bit_depth != 10 && bit_depth != 12 && bit_depth != 14) || chroma_format_idc < 0 || chroma_format_idc > 1) {
        ffhip_set_error("%s: bit depth %d (8, 9, 10, 12 or 14), chroma_format_idc %d (0 or 1)", who, bit_depth, chroma_format_idc);
        return FFHIP_EINVAL;
    }
    if (const int r = check_common(who, mb_w, mb_h, npics, pics))
        return r;
    const int ps = bit_depth > 8 ? 2 : 1;
    const unsigned amask = 4u * ps - 1;
    std::vector<FFHipRows> dst;
    dst.reserve((size_t)npics * 3);
    auto plane_rows = [&](const void *base, ptrdiff_t stride, int p) {
        return FFHipRows{ (uintptr_t)base, stride, (ptrdiff_t)(mb_w * (p ? 8 : 16)) * ps, mb_h * (p ? 8 : 16) };
    };
    for (int i = 0; i < npics; i++) {
        const FFHipH264InterPic &P = pics[i];
        const bool has_c = chroma_format_idc && (P.dst[1] || P.dst[2]);
        if (chroma_format_idc && !P.dst[1] != !P.dst[2]) {
            ffhip_set_error("%s: picture %d: one of Cb / Cr without the other", who, i);
            return FFHIP_EINVAL;
        }
        for (int p = 0; p < (has_c ? 3 : 1); p++) {
            if (!ffhip_plane_ok(P.dst[p], P.dst_stride[p], amask, (ptrdiff_t)(mb_w * (p ? 8 : 16)) * ps)) {
                ffhip_set_error("%s: picture %d: dst plane %d is NULL, its base or stride %td is not a multiple of 4 samples, or the stride "
                                "is below the plane's %d samples", who, i, p, P.dst_stride[p], mb_w * (p ? 8 : 16));
                return FFHIP_EINVAL;
            }
            dst.push_back(plane_rows(P.dst[p], P.dst_stride[p], p));
        }
        if (const int r = check_maps(who, i, mb_w, P.mb, P.mvf, P.slices, P.mvf_stride, P.nslices, P.nrefs))
            return r;
        for (int k = 0; k < P.nrefs; k++)
            for (int p = 0; p < (has_c ? 3 : 1); p++)
                if (!P.ref[k].base[p] || (((uintptr_t)P.ref[k].base[p] | (size_t)P.ref[k].stride[p]) & (ps - 1))) {
                    ffhip_set_error("%s: picture %d: reference %d: plane %d is NULL, or its base or stride %td is not a multiple of the "
                                    "sample size", who, i, k, p, P.ref[k].stride[p]);
                    return FFHIP_EINVAL;
                }
    }
    /* workgroups of every picture of the call read while others write: no destination row may share a byte with another destination
     * row or with a reference row of any picture; the span set sorts out the planes that cannot before the pairwise row rule */
    FFHipSpanSet out;
    if (ffhip_any_rows_share(dst, out)) {
        ffhip_set_error("%s: a destination plane overlaps another destination plane of the call", who);
        return FFHIP_EINVAL;
    }
    for (int i = 0; i < npics; i++) {
        const FFHipH264InterPic &P = pics[i];
        const bool has_c = chroma_format_idc && P.dst[1];
        for (int k = 0; k < P.nrefs; k++)
            for (int p = 0; p < (has_c ? 3 : 1); p++) {
                const FFHipRows r = plane_rows(P.ref[k].base[p], P.ref[k].stride[p], p);
                if (!out.hits(r.span()))
                    continue;
                for (const FFHipRows &d : dst)
                    if (ffhip_rows_share(d, r)) {
                        ffhip_set_error("%s: picture %d: reference %d: a row of plane %d overlaps a destination row of the call", who, i, k, p);
                        return FFHIP_EINVAL;
                    }
            }
        const ptrdiff_t nmb = (ptrdiff_t)mb_w * mb_h;
        const FFHipSpan in[3] = { ffhip_plane_span(P.mb, 0, nmb * (ptrdiff_t)sizeof(FFHipH264BsMb), 1),
                                  ffhip_map_span(P.mvf, P.mvf_stride, 4 * mb_w, 4 * mb_h, sizeof(FFHipH264MvField)),
                                  ffhip_plane_span(P.slices, 0, (ptrdiff_t)P.nslices * (ptrdiff_t)sizeof(FFHipH264InterSlice), 1) };
        for (int k = 0; k < 3; k++)
            if (out.hits(in[k])) {
                ffhip_set_error("%s: picture %d: an input table overlaps a destination plane of the call", who, i);
                return FFHIP_EINVAL;
            }
    }
    return 0;
}
} // namespace

extern "C" int ffhip_h264_inter_pictures_dev(int bit_depth, int chroma_format_idc, int mb_w, int mb_h, int npics, const FFHipH264InterPic *pics,
                                             void *stream)
{
    const int r = check_dev("ffhip_h264_inter_pictures_dev", bit_depth, chroma_format_idc, mb_w, mb_h, npics, pics);
    if (r < 0)
        return r;
    if (!ffhip_have_device())
        return FFHIP_ENOSYS;
    return ffhip_launch_h264_inter_pictures(bit_depth, chroma_format_idc, mb_w, mb_h, npics, pics, (hipStream_t)stream);
}

extern "C" int ffhip_h264_inter_plan_pictures_host(int mb_w, int mb_h, int npics, const FFHipH264InterPlanPic *pics)
{
    const char *who = "ffhip_h264_inter_plan_pictures_host";
    if (const int r = check_common(who, mb_w, mb_h, npics, pics))
        return r;
    const int w4 = 4 * mb_w, h4 = 4 * mb_h;
    const ptrdiff_t nmb = (ptrdiff_t)mb_w * mb_h;
    FFHipSpanSet out;
    out.reserve((size_t)npics);
    for (int i = 0; i < npics; i++) {
        const FFHipH264InterPlanPic &P = pics[i];
        if (const int r = check_maps(who, i, mb_w, P.mb, P.mvf, P.slices, P.mvf_stride, P.nslices, P.nrefs))
            return r;
        if (!P.plans) {
            ffhip_set_error("%s: picture %d: a NULL plans array", who, i);
            return FFHIP_EINVAL;
        }
        out.add(ffhip_plane_span(P.plans, 0, nmb * 16 * (ptrdiff_t)sizeof(FFHipH264InterBlockPlan), 1));
    }
    if (out.seal()) {
        ffhip_set_error("%s: a plans array overlaps another plans array of the call", who);
        return FFHIP_EINVAL;
    }
    for (int i = 0; i < npics; i++) {
        const FFHipH264InterPlanPic &P = pics[i];
        const FFHipSpan in[3] = { ffhip_plane_span(P.mb, 0, nmb * (ptrdiff_t)sizeof(FFHipH264BsMb), 1),
                                  ffhip_map_span(P.mvf, P.mvf_stride, w4, h4, sizeof(FFHipH264MvField)),
                                  ffhip_plane_span(P.slices, 0, (ptrdiff_t)P.nslices * (ptrdiff_t)sizeof(FFHipH264InterSlice), 1) };
        for (int k = 0; k < 3; k++)
            if (out.hits(in[k])) {
                ffhip_set_error("%s: picture %d: an input overlaps a plans array of the call", who, i);
                return FFHIP_EINVAL;
            }
    }
    for (int i = 0; i < npics; i++) {
        const FFHipH264InterPlanPic &P = pics[i];
        for (int by = 0; by < h4; by++)
            for (int bx = 0; bx < w4; bx++) {
                FFHipH264MvField f;
                memcpy(&f, P.mvf + (ptrdiff_t)by * P.mvf_stride + bx, sizeof(f));
                const FFHipH264InterBlockPlan p = h264inter_plan(P.mb + (ptrdiff_t)(by >> 2) * mb_w + (bx >> 2), &f, P.slices, P.nslices, P.nrefs);
                memcpy(P.plans + (ptrdiff_t)by * w4 + bx, &p, sizeof(p));
            }
    }
    return 0;
}
