/*
 * shims_hevc_bs.hip — ffhip_hevc_boundary_strengths_pictures_dev(): the host checks (kernels/picture_check.h, map pointers and
 * strides, output / input overlap) and the launch of kernels/hevc_bs_pic.hip on the caller's stream; and the device-free faces:
 * ffhip_hevc_boundary_strengths_pictures_host(), the same checks and the same rules (kernels/hevc_bs_rules.h) on host arrays,
 * ffhip_hevc_bs_mark_tu() and the record sizes.
 */
#include <string.h>

#include "kernels/common.h"
#include "kernels/h264_kernels.h"
#include "kernels/hevc_bs_rules.h"
#include "kernels/picture_check.h"

extern "C" int ffhip_hevc_bs_mvf_record_size(void) { return (int)sizeof(FFHipHevcMvField); }
extern "C" int ffhip_hevc_bs_slice_record_size(void) { return (int)sizeof(FFHipHevcBsSlice); }

extern "C" void ffhip_hevc_bs_mark_tu(uint8_t *tu, int tu_stride, int x0, int y0, int log2_size, int cbf_luma)
{
    if (!tu || x0 < 0 || y0 < 0 || ((x0 | y0) & 3) || log2_size < 2 || log2_size > 5)
        return;
    const int n = 1 << (log2_size - 2);
    uint8_t *t = tu + (ptrdiff_t)(y0 >> 2) * tu_stride + (x0 >> 2);
    for (int y = 0; y < n; y++)
        for (int x = 0; x < n; x++)
            t[(ptrdiff_t)y * tu_stride + x] |= (uint8_t)((x == 0 ? 1 : 0) | (y == 0 ? 2 : 0) | (cbf_luma ? 4 : 0));
}

namespace {
/* the argument checks of both faces */
int check(const char *who, int width, int height, int log2_ctb_size, int npics, const FFHipHevcBsPic *pics)
{
    if (const int r = ffhip_check_hevc_geometry(who, log2_ctb_size, width, height, npics, pics))
        return r;
    const int w4 = width >> 2, h4 = height >> 2, C = 1 << log2_ctb_size, nctb = ((width + C - 1) / C) * ((height + C - 1) / C);
    for (int i = 0; i < npics; i++) {
        const FFHipHevcBsPic &P = pics[i];
        if (!P.mvf || !P.tu || !P.ctb_slice || !P.slices || !P.bs_ver || !P.bs_hor || ((uintptr_t)P.mvf & 3) || P.mvf_stride < w4 ||
            P.tu_stride < w4 || P.bs_stride < w4 || P.nslices < 1) {
            ffhip_set_error("%s: picture %d: a NULL map, an mvf that is not 4-byte aligned, mvf_stride %d, tu_stride %d or bs_stride %d (>= %d), "
                            "or nslices %d (>= 1)", who, i, P.mvf_stride, P.tu_stride, P.bs_stride, w4, P.nslices);
            return FFHIP_EINVAL;
        }
    }
    /* no output map of the call may overlap another one or an input map: workgroups of every picture read while others write */
    FFHipSpanSet out;
    out.reserve((size_t)npics * 2);
    for (int i = 0; i < npics; i++) {
        out.add(ffhip_map_span(pics[i].bs_ver, pics[i].bs_stride, w4, h4, 1));
        out.add(ffhip_map_span(pics[i].bs_hor, pics[i].bs_stride, w4, h4, 1));
    }
    if (out.seal()) {
        ffhip_set_error("%s: an output map overlaps another output map of the call", who);
        return FFHIP_EINVAL;
    }
    for (int i = 0; i < npics; i++) {
        const FFHipHevcBsPic &P = pics[i];
        const FFHipSpan in[5] = { ffhip_map_span(P.mvf, P.mvf_stride, w4, h4, sizeof(FFHipHevcMvField)), ffhip_map_span(P.tu, P.tu_stride, w4, h4, 1),
                                  ffhip_map_span(P.ctb_slice, nctb, nctb, 1, 2),
                                  ffhip_map_span(P.slices, P.nslices, P.nslices, 1, sizeof(FFHipHevcBsSlice)),
                                  ffhip_map_span(P.ctb_tile, nctb, nctb, 1, 2) };
        for (int k = 0; k < (P.ctb_tile ? 5 : 4); k++)
            if (out.hits(in[k])) {
                ffhip_set_error("%s: picture %d: an input map overlaps an output map of the call", who, i);
                return FFHIP_EINVAL;
            }
    }
    return 0;
}
} // namespace

extern "C" int ffhip_hevc_boundary_strengths_pictures_dev(int width, int height, int log2_ctb_size, int npics, const FFHipHevcBsPic *pics,
                                                          void *stream)
{
    const int r = check("ffhip_hevc_boundary_strengths_pictures_dev", width, height, log2_ctb_size, npics, pics);
    if (r < 0)
        return r;
    if (!ffhip_have_device())
        return FFHIP_ENOSYS;
    return ffhip_launch_hevc_boundary_strengths_pictures(width, height, log2_ctb_size, npics, pics, (hipStream_t)stream);
}

extern "C" int ffhip_hevc_boundary_strengths_pictures_host(int width, int height, int log2_ctb_size, int npics, const FFHipHevcBsPic *pics)
{
    const int r = check("ffhip_hevc_boundary_strengths_pictures_host", width, height, log2_ctb_size, npics, pics);
    if (r < 0)
        return r;
    const int w4 = width >> 2, h4 = height >> 2, lu = log2_ctb_size - 2, ctb_w = (w4 + (1 << lu) - 1) >> lu;
    std::vector<HbsUnit> rows((size_t)w4 * 2); /* the resolved units of the row above and of this row */
    std::vector<uint32_t> ctbs((size_t)w4 * 2); /* slice index | tile id << 16 of their CTBs */
    for (int i = 0; i < npics; i++) {
        const FFHipHevcBsPic &P = pics[i];
        const bool across = P.loop_filter_across_tiles != 0;
        for (int uy = 0; uy < h4; uy++) {
            HbsUnit *cur = rows.data() + (size_t)(uy & 1) * w4, *up = rows.data() + (size_t)(~uy & 1) * w4;
            uint32_t *ccur = ctbs.data() + (size_t)(uy & 1) * w4, *cup = ctbs.data() + (size_t)(~uy & 1) * w4;
            for (int ux = 0; ux < w4; ux++) {
                const int a = (uy >> lu) * ctb_w + (ux >> lu);
                uint32_t d[3];
                memcpy(d, P.mvf + (ptrdiff_t)uy * P.mvf_stride + ux, sizeof(d));
                ccur[ux] = (uint32_t)P.ctb_slice[a] | (P.ctb_tile ? (uint32_t)P.ctb_tile[a] << 16 : 0u);
                cur[ux] = hbs_resolve(d[0], d[1], d[2], P.tu[(ptrdiff_t)uy * P.tu_stride + ux], P.slices, P.nslices, ccur[ux] & 0xFFFF);
            }
            uint8_t *ver = P.bs_ver + (ptrdiff_t)uy * P.bs_stride, *hor = P.bs_hor + (ptrdiff_t)uy * P.bs_stride;
            for (int ux = 0; ux < w4; ux++) {
                const uint32_t cq = ccur[ux];
                int v = 0, h = 0;
                if (hbs_on_grid(ux)) {
                    const uint32_t cp = ccur[ux - 1];
                    v = hbs_segment(cur[ux - 1], cur[ux], 0, (cp & 0xFFFF) == (cq & 0xFFFF), cp >> 16 == cq >> 16, across);
                }
                if (hbs_on_grid(uy)) {
                    const uint32_t cp = cup[ux];
                    h = hbs_segment(up[ux], cur[ux], 1, (cp & 0xFFFF) == (cq & 0xFFFF), cp >> 16 == cq >> 16, across);
                }
                ver[ux] = (uint8_t)v;
                hor[ux] = (uint8_t)h;
            }
        }
    }
    return 0;
}
