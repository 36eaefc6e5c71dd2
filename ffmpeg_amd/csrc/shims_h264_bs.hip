/*
 * shims_h264_bs.hip — ffhip_h264_edge_params_pictures_dev() / _fmt_dev(): the host checks (geometry, pointers and strides, output /
 * input overlap through kernels/picture_check.h) and the launch of kernels/h264_bs_pic.hip on the caller's stream; the device-free
 * faces ffhip_h264_edge_params_pictures_host() / _fmt_host(), the same checks and the same rules (kernels/h264_bs_rules.h) on host
 * arrays; and the record sizes.  The faces without a format forward to the ones with it.  (The filter that takes the tables of every
 * format, ffhip_h264_deblock_pictures_fmt_dev(), is shims_h264_lf.hip.)
 */
#include <string.h>

#include <vector>

#include "kernels/common.h"
#include "kernels/h264_kernels.h"
#include "kernels/h264_bs_rules.h"
#include "kernels/picture_check.h"

extern "C" int ffhip_h264_bs_mb_record_size(void) { return (int)sizeof(FFHipH264BsMb); }
extern "C" int ffhip_h264_bs_mvf_record_size(void) { return (int)sizeof(FFHipH264MvField); }
extern "C" int ffhip_h264_bs_slice_record_size(void) { return (int)sizeof(FFHipH264BsSlice); }

namespace {
/* `n` records of `entry` bytes in a row */
FFHipSpan table_span(const void *base, ptrdiff_t n, size_t entry)
{
    return ffhip_plane_span(base, 0, n * (ptrdiff_t)entry, 1);
}

/* records of a macroblock in cb / cr */
int chroma_records(int fmt) { return fmt == 3 ? 8 : fmt == 2 ? 6 : 4; }

/* the argument checks of every edge-parameter face; fmt 0: chroma_qp / cb / cr are not looked at */
int check(const char *who, int fmt, int mb_w, int mb_h, int field, int qp_bd_offset, int npics, const FFHipH264BsPic *pics)
{
    if (fmt < 0 || fmt > 3) {
        ffhip_set_error("%s: chroma_format_idc %d (0..3)", who, fmt);
        return FFHIP_EINVAL;
    }
    if (mb_w < 1 || mb_h < 1 || mb_w > 4096 || mb_h > 4096) {
        ffhip_set_error("%s: %d x %d macroblocks (1..4096 each)", who, mb_w, mb_h);
        return FFHIP_EINVAL;
    }
    if ((qp_bd_offset != 0 && qp_bd_offset != 6 && qp_bd_offset != 12 && qp_bd_offset != 24 && qp_bd_offset != 36) || (field & ~1)) {
        ffhip_set_error("%s: qp_bd_offset %d (0, 6, 12, 24 or 36), field %d (0 or 1)", who, qp_bd_offset, field);
        return FFHIP_EINVAL;
    }
    if (const int r = ffhip_check_count(who, npics, pics, "picture"))
        return r;
    const int w4 = mb_w * 4, h4 = mb_h * 4;
    const ptrdiff_t nmb = (ptrdiff_t)mb_w * mb_h, nc = nmb * chroma_records(fmt);
    for (int i = 0; i < npics; i++) {
        const FFHipH264BsPic &P = pics[i];
        const bool chroma_bad = fmt && (!P.cb != !P.cr || (P.cb && !P.chroma_qp) || (((uintptr_t)P.cb | (uintptr_t)P.cr) & 3));
        if (!P.mb || !P.mvf || !P.slices || !P.luma || chroma_bad || (((uintptr_t)P.mvf | (uintptr_t)P.luma) & 3) || P.mvf_stride < w4 ||
            P.nslices < 1) {
            ffhip_set_error("%s: picture %d: a NULL mb, mvf, slices or luma, one of cb / cr without the other or without chroma_qp, an mvf or an "
                            "output table that is not 4-byte aligned, mvf_stride %d (>= %d) or nslices %d (>= 1)", who, i, P.mvf_stride, w4, P.nslices);
            return FFHIP_EINVAL;
        }
    }
    /* no output table of the call may overlap another one or an input: workgroups of every picture read while others write */
    FFHipSpanSet out;
    out.reserve((size_t)npics * 3);
    for (int i = 0; i < npics; i++) {
        out.add(table_span(pics[i].luma, nmb * 8, sizeof(FFHipH264Edge)));
        if (fmt && pics[i].cb) {
            out.add(table_span(pics[i].cb, nc, sizeof(FFHipH264Edge)));
            out.add(table_span(pics[i].cr, nc, sizeof(FFHipH264Edge)));
        }
    }
    if (out.seal()) {
        ffhip_set_error("%s: an output table overlaps another output table of the call", who);
        return FFHIP_EINVAL;
    }
    for (int i = 0; i < npics; i++) {
        const FFHipH264BsPic &P = pics[i];
        const FFHipSpan in[4] = { table_span(P.mb, nmb, sizeof(FFHipH264BsMb)), ffhip_map_span(P.mvf, P.mvf_stride, w4, h4, sizeof(FFHipH264MvField)),
                                  table_span(P.slices, P.nslices, sizeof(FFHipH264BsSlice)), table_span(P.chroma_qp, 2 * H264BS_QP_ENTRIES, 1) };
        for (int k = 0; k < (fmt && P.chroma_qp ? 4 : 3); k++)
            if (out.hits(in[k])) {
                ffhip_set_error("%s: picture %d: an input overlaps an output table of the call", who, i);
                return FFHIP_EINVAL;
            }
    }
    return 0;
}

/* the pictures as the kernel and the host loop take them: at format 0 without their chroma pointers, which are then neither read nor
 * written through */
const FFHipH264BsPic *luma_only(int fmt, int npics, const FFHipH264BsPic *pics, std::vector<FFHipH264BsPic> &copy)
{
    if (fmt)
        return pics;
    copy.assign(pics, pics + npics);
    for (FFHipH264BsPic &P : copy) {
        P.chroma_qp = nullptr;
        P.cb = P.cr = nullptr;
    }
    return copy.data();
}

int edge_params_dev(const char *who, int fmt, int mb_w, int mb_h, int field, int qp_bd_offset, int npics, const FFHipH264BsPic *pics, void *stream)
{
    const int r = check(who, fmt, mb_w, mb_h, field, qp_bd_offset, npics, pics);
    if (r < 0)
        return r;
    if (!ffhip_have_device())
        return FFHIP_ENOSYS;
    std::vector<FFHipH264BsPic> copy;
    pics = luma_only(fmt, npics, pics, copy);
    return ffhip_launch_h264_edge_params_pictures(fmt ? fmt : 1, mb_w, mb_h, field, qp_bd_offset, npics, pics, (hipStream_t)stream);
}

int edge_params_host(const char *who, int fmt, int mb_w, int mb_h, int field, int qp_bd_offset, int npics, const FFHipH264BsPic *pics)
{
    const int r = check(who, fmt, mb_w, mb_h, field, qp_bd_offset, npics, pics);
    if (r < 0)
        return r;
    std::vector<FFHipH264BsPic> copy;
    pics = luma_only(fmt, npics, pics, copy);
    const int w4 = mb_w * 4, per = chroma_records(fmt);
    std::vector<H264BsMb> mbs((size_t)mb_w * 2);        /* the resolved macroblocks of the row above and of this row */
    std::vector<H264BsBlk> blks((size_t)w4 * 5);        /* the resolved blocks of this row, behind the last block row of the row above */
    for (int i = 0; i < npics; i++) {
        const FFHipH264BsPic &P = pics[i];
        for (int my = 0; my < mb_h; my++) {
            H264BsMb *cur = mbs.data() + (size_t)(my & 1) * mb_w, *up = mbs.data() + (size_t)(~my & 1) * mb_w;
            if (my)
                memcpy(blks.data(), blks.data() + (size_t)w4 * 4, (size_t)w4 * sizeof(H264BsBlk));
            for (int mx = 0; mx < mb_w; mx++)
                cur[mx] = h264bs_resolve_mb(P.mb[(ptrdiff_t)my * mb_w + mx], P.slices, P.nslices);
            for (int y = 0; y < 4; y++)
                for (int ux = 0; ux < w4; ux++) {
                    uint32_t d[3];
                    memcpy(d, P.mvf + (ptrdiff_t)(my * 4 + y) * P.mvf_stride + ux, sizeof(d));
                    blks[(size_t)(y + 1) * w4 + ux] = h264bs_resolve_blk(d[0], d[1], d[2], cur[ux >> 2], P.slices);
                }
            for (int mx = 0; mx < mb_w; mx++) {
                const ptrdiff_t mb = (ptrdiff_t)my * mb_w + mx;
                const H264BsMb q = cur[mx];
                for (int dir = 0; dir < 2; dir++)
                    for (int e = 0; e < 4; e++) {
                        const bool border = dir ? my == 0 : mx == 0;
                        const H264BsMb p = e || border ? q : dir ? up[mx] : cur[mx - 1];
                        auto blk = [&](int x, int y) { return blks[(size_t)(y + 1) * w4 + mx * 4 + x]; };
                        uint32_t bs = h264bs_edge_bs(p, q, border, dir, e, field, blk);
                        uint32_t out[3];
                        h264bs_pack(false, dir, bs, bs ? h264bs_edge_qp(p, q, e, nullptr) : 0, q, qp_bd_offset, out);
                        memcpy(P.luma + (mb * 2 + dir) * 4 + e, out, sizeof(out));
                        if (!P.cb)
                            continue;
                        /* the record of this edge in cb / cr: 4:4:4 the luma layout; 4:2:2 the even vertical edges, then every
                         * horizontal one without the 8x8-transform skip; 4:2:0 the even edges */
                        int k = dir * 4 + e;
                        if (fmt == 2 && dir) {
                            k = 2 + e;
                            if (e & 1)
                                bs = h264bs_edge_bs(p, q, border, dir, e, field, blk, true);
                        } else if (fmt != 3) {
                            if (e & 1)
                                continue;
                            k = (fmt == 2 ? 0 : dir * 2) + (e >> 1);
                        }
                        for (int c = 0; c < 2; c++) {
                            h264bs_pack(fmt != 3, dir, bs, bs ? h264bs_edge_qp(p, q, e, P.chroma_qp + c * H264BS_QP_ENTRIES) : 0, q, qp_bd_offset, out);
                            memcpy((c ? P.cr : P.cb) + mb * per + k, out, sizeof(out));
                        }
                    }
            }
        }
    }
    return 0;
}
} // namespace

extern "C" int ffhip_h264_edge_params_pictures_fmt_dev(int chroma_format_idc, int mb_w, int mb_h, int field, int qp_bd_offset, int npics,
                                                       const FFHipH264BsPic *pics, void *stream)
{
    return edge_params_dev("ffhip_h264_edge_params_pictures_fmt_dev", chroma_format_idc, mb_w, mb_h, field, qp_bd_offset, npics, pics, stream);
}

extern "C" int ffhip_h264_edge_params_pictures_fmt_host(int chroma_format_idc, int mb_w, int mb_h, int field, int qp_bd_offset, int npics,
                                                        const FFHipH264BsPic *pics)
{
    return edge_params_host("ffhip_h264_edge_params_pictures_fmt_host", chroma_format_idc, mb_w, mb_h, field, qp_bd_offset, npics, pics);
}

/* the faces without a format: 4:2:0, where a picture with NULL cb / cr has no chroma tables */
extern "C" int ffhip_h264_edge_params_pictures_dev(int mb_w, int mb_h, int field, int qp_bd_offset, int npics, const FFHipH264BsPic *pics, void *stream)
{
    return edge_params_dev("ffhip_h264_edge_params_pictures_dev", 1, mb_w, mb_h, field, qp_bd_offset, npics, pics, stream);
}

extern "C" int ffhip_h264_edge_params_pictures_host(int mb_w, int mb_h, int field, int qp_bd_offset, int npics, const FFHipH264BsPic *pics)
{
    return edge_params_host("ffhip_h264_edge_params_pictures_host", 1, mb_w, mb_h, field, qp_bd_offset, npics, pics);
}
