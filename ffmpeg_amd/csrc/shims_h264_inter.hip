/*
 * shims_h264_inter.hip — ffhip_h264_inter_pictures_dev() and ffhip_h264_inter_pictures_fmt_dev(): the host checks (format, geometry,
 * pointers and strides, the row-wise overlap rule of destination and reference planes, with the planes sized by the chroma format)
 * and the launch of kernels/h264_inter_pic.hip on the caller's stream; and the device-free faces:
 * ffhip_h264_inter_plan_pictures_host(), the plan of every block by the function the kernel uses (kernels/h264_inter_rules.h) on
 * host arrays, ffhip_h264_inter_pictures_fmt_host(), the samples by the statements the kernel runs (h264_inter_rules.h,
 * h264_mc_rules.h) sample after sample, and the record sizes.
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

/* max_idc: 1 for the faces of 4:2:0 and monochrome, which name 2 and 3 in a refusal of their own; 3 for the _fmt faces */
int check_dev(const char *who, int max_idc, int bit_depth, int chroma_format_idc, int mb_w, int mb_h, int npics, const FFHipH264InterPic *pics)
{
    if (max_idc == 1 && (chroma_format_idc == 2 || chroma_format_idc == 3)) {
        ffhip_set_error("%s: chroma_format_idc %d: 4:2:2 and 4:4:4 are not implemented (0 or 1)", who, chroma_format_idc);
        return FFHIP_ENOSYS;
    }
    if ((bit_depth != 8 && bit_depth != 9 && bit_depth != 10 && bit_depth != 12 && bit_depth != 14) || chroma_format_idc < 0 ||
        chroma_format_idc > max_idc) {
        ffhip_set_error("%s: bit depth %d (8, 9, 10, 12 or 14), chroma_format_idc %d (%s)", who, bit_depth, chroma_format_idc,
                        max_idc == 1 ? "0 or 1" : "0..3");
        return FFHIP_EINVAL;
    }
    if (const int r = check_common(who, mb_w, mb_h, npics, pics))
        return r;
    /* the planes' sizes by format: 4:2:0 8 mb_w x 8 mb_h, 4:2:2 8 mb_w x 16 mb_h, 4:4:4 16 mb_w x 16 mb_h */
    const FFHipPlaneGeom g = FFHipPlaneGeom::hevc(bit_depth, chroma_format_idc, 16 * mb_w, 16 * mb_h);
    const int ps = g.ps;
    const unsigned amask = g.amask;
    std::vector<FFHipRows> dst;
    dst.reserve((size_t)npics * 3);
    auto plane_rows = [&](const void *base, ptrdiff_t stride, int p) {
        return FFHipRows{ (uintptr_t)base, stride, g.row_bytes(p), g.ph[p] };
    };
    for (int i = 0; i < npics; i++) {
        const FFHipH264InterPic &P = pics[i];
        const bool has_c = chroma_format_idc && (P.dst[1] || P.dst[2]);
        if (chroma_format_idc && !P.dst[1] != !P.dst[2]) {
            ffhip_set_error("%s: picture %d: one of Cb / Cr without the other", who, i);
            return FFHIP_EINVAL;
        }
        for (int p = 0; p < (has_c ? 3 : 1); p++) {
            if (!ffhip_plane_ok(P.dst[p], P.dst_stride[p], amask, g.row_bytes(p))) {
                ffhip_set_error("%s: picture %d: dst plane %d is NULL, its base or stride %td is not a multiple of 4 samples, or the stride "
                                "is below the plane's %d samples", who, i, p, P.dst_stride[p], g.pw[p]);
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
    const int r = check_dev("ffhip_h264_inter_pictures_dev", 1, bit_depth, chroma_format_idc, mb_w, mb_h, npics, pics);
    if (r < 0)
        return r;
    if (!ffhip_have_device())
        return FFHIP_ENOSYS;
    return ffhip_launch_h264_inter_pictures(bit_depth, chroma_format_idc, mb_w, mb_h, npics, pics, (hipStream_t)stream);
}

extern "C" int ffhip_h264_inter_pictures_fmt_dev(int bit_depth, int chroma_format_idc, int mb_w, int mb_h, int npics, const FFHipH264InterPic *pics,
                                                 void *stream)
{
    const int r = check_dev("ffhip_h264_inter_pictures_fmt_dev", 3, bit_depth, chroma_format_idc, mb_w, mb_h, npics, pics);
    if (r < 0)
        return r;
    if (!ffhip_have_device())
        return FFHIP_ENOSYS;
    return ffhip_launch_h264_inter_pictures(bit_depth, chroma_format_idc, mb_w, mb_h, npics, pics, (hipStream_t)stream);
}

namespace {
/* a sample of a host plane of w x h samples at clamped coordinates */
template <typename P>
struct HostSrc {
    const uint8_t *base;
    ptrdiff_t s;
    int x0, y0, w, h;
    int at(int dx, int dy) const
    {
        P v;
        memcpy(&v, base + (ptrdiff_t)std::min(std::max(y0 + dy, 0), h - 1) * s + (size_t)std::min(std::max(x0 + dx, 0), w - 1) * sizeof(P), sizeof(v));
        return (int)v;
    }
};
template <typename P>
void put(uint8_t *dst, ptrdiff_t stride, int x, int y, int v)
{
    const P px = (P)v;
    memcpy(dst + (ptrdiff_t)y * stride + (size_t)x * sizeof(P), &px, sizeof(px));
}

/* one 4x4 block: what the 16 lanes of a block do in k_h264_inter_pic, sample after sample */
template <typename P>
void inter_block(const FFHipH264InterPic &Pc, int fmt, bool has_c, int mb_w, int mb_h, int bx, int by, int bd)
{
    FFHipH264MvField f;
    memcpy(&f, Pc.mvf + (ptrdiff_t)by * Pc.mvf_stride + bx, sizeof(f));
    const FFHipH264InterBlockPlan plan = h264inter_plan(Pc.mb + (ptrdiff_t)(by >> 2) * mb_w + (bx >> 2), &f, Pc.slices, Pc.nslices, Pc.nrefs);
    if (plan.mode == FFHIP_H264_INTER_SKIP)
        return;
    const bool bi = plan.mode >= FFHIP_H264_INTER_BI_AVG;
    const int pw = 16 * mb_w, ph = 16 * mb_h, maxv = (1 << bd) - 1;
    for (int p = 0; p < (fmt == 3 && has_c ? 3 : 1); p++)       /* rule 3, and 4c on Cb / Cr */
        for (int y = 0; y < 4; y++)
            for (int x = 0; x < 4; x++) {
                int v[2] = { 0, 0 };
                for (int n = 0; n < (bi ? 2 : 1); n++) {
                    const int L = bi ? n : plan.list, mvx = f.mv[L][0], mvy = f.mv[L][1];
                    const FFHipH264InterRef &R = Pc.ref[plan.slot[n]];
                    const HostSrc<P> S = { R.base[p], R.stride[p], bx * 4 + x + (mvx >> 2), by * 4 + y + (mvy >> 2), pw, ph };
                    v[n] = h264mc_luma(S, mvx & 3, mvy & 3, maxv);
                }
                put<P>(Pc.dst[p], Pc.dst_stride[p], bx * 4 + x, by * 4 + y, h264inter_combine(&plan, p, v[0], v[1], bd));
            }
    if (!has_c || fmt == 3)
        return;
    for (int c = 0; c < 2; c++)                                  /* rules 4a / 4b */
        for (int n0 = 0; n0 < (fmt == 2 ? 8 : 4); n0++) {
            int v[2] = { 0, 0 }, x = n0 & 1, y = n0 >> 1;
            H264InterChroma C = {};
            for (int n = 0; n < (bi ? 2 : 1); n++) {
                const int L = bi ? n : plan.list;
                const FFHipH264InterRef &R = Pc.ref[plan.slot[n]];
                C = h264inter_chroma(fmt, bx, by, f.mv[L][0], f.mv[L][1], R.chroma_dy, mb_w, mb_h);
                const HostSrc<P> S = { R.base[1 + c], R.stride[1 + c], C.sx + x, C.sy + y, C.cw, C.ch };
                v[n] = h264mc_chroma(S, C.ax, C.ay);
            }
            put<P>(Pc.dst[1 + c], Pc.dst_stride[1 + c], C.x + x, C.y + y, h264inter_combine(&plan, 1 + c, v[0], v[1], bd));
        }
}
} // namespace

extern "C" int ffhip_h264_inter_pictures_fmt_host(int bit_depth, int chroma_format_idc, int mb_w, int mb_h, int npics, const FFHipH264InterPic *pics)
{
    const int r = check_dev("ffhip_h264_inter_pictures_fmt_host", 3, bit_depth, chroma_format_idc, mb_w, mb_h, npics, pics);
    if (r < 0)
        return r;
    for (int i = 0; i < npics; i++) {
        const bool has_c = chroma_format_idc && pics[i].dst[1];
        for (int by = 0; by < 4 * mb_h; by++)
            for (int bx = 0; bx < 4 * mb_w; bx++)
                if (bit_depth > 8)
                    inter_block<uint16_t>(pics[i], chroma_format_idc, has_c, mb_w, mb_h, bx, by, bit_depth);
                else
                    inter_block<uint8_t>(pics[i], chroma_format_idc, has_c, mb_w, mb_h, bx, by, bit_depth);
    }
    return 0;
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
