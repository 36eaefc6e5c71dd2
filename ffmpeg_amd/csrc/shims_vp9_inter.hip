/*
 * shims_vp9_inter.hip — ffhip_vp9_inter_frames_dev(): the host checks (kernels/picture_check.h, references, reference / destination
 * overlap) and the launch of the inter reconstruction (kernels/vp9_inter_frame.hip) on the caller's stream.  The records themselves
 * are device data and are checked by the kernel.  Also ffhip_vp9_inter_block_preds(), the device-free expansion
 * of one decoded block into its prediction records (libavcodec/vp9_mc_template.h).  ffhip_vp9_inter_frames_scaled_dev() and
 * ffhip_vp9_inter_block_preds_scaled(): the same for frames with references of another size (the SCALED template).
 */
#include "kernels/common.h"
#include "kernels/h264_kernels.h"
#include "kernels/picture_check.h"

extern "C" int ffhip_vp9_inter_pred_record_size(void) { return (int)sizeof(FFHipVp9InterPred); }
extern "C" int ffhip_vp9_inter_tu_record_size(void) { return (int)sizeof(FFHipVp9InterTU); }

namespace {
/* ROUNDED_DIV (libavutil/common.h): half away from zero, then C division (towards zero) */
int rounded_div(int a, int b) { return (a >= 0 ? a + (b >> 1) : a - (b >> 1)) / b; }
struct Mv {
    int x, y;
};
Mv mv_of(const int16_t mv[4][2][2], int sub, int r) { return { mv[sub][r][0], mv[sub][r][1] }; }
Mv div2(Mv a, Mv b) { return { rounded_div(a.x + b.x, 2), rounded_div(a.y + b.y, 2) }; }
Mv div4(Mv a, Mv b, Mv c, Mv d) { return { rounded_div(a.x + b.x + c.x + d.x, 4), rounded_div(a.y + b.y + c.y + d.y, 4) }; }

/* the host checks of both faces: pic(i) is frame i's FFHipVp9InterPic and ref_size(i, r, p, &w, &h) gives the real size of plane p of
 * frame i's reference r, samples */
template <typename PIC, typename REFSIZE>
int check_frames(const char *who, int bit_depth, int ss_h, int ss_v, int width, int height, int npics, const void *pics, PIC pic,
                 REFSIZE ref_size)
{
    if (const int r = ffhip_check_vp9_frames(who, bit_depth, ss_h, ss_v, width, height, npics, pics))
        return r;
    const FFHipPlaneGeom G = FFHipPlaneGeom::vp9(bit_depth, ss_h, ss_v, width, height);
    for (int i = 0; i < npics; i++) {
        const FFHipVp9InterPic &P = pic(i);
        if (!P.preds || !P.pred_sb_start || P.nrefs < 1 || P.nrefs > 3) {
            ffhip_set_error("%s: frame %d: NULL prediction tables or nrefs = %d (1..3)", who, i, P.nrefs);
            return FFHIP_EINVAL;
        }
        for (int p = 0; p < 3; p++) {
            const FFHipVp9InterPlane &D = P.plane[p];
            if (!D.base || !D.tus || !D.tu_sb_start || !D.coeffs) {
                ffhip_set_error("%s: frame %d plane %d: a NULL pointer", who, i, p);
                return FFHIP_EINVAL;
            }
            if (!ffhip_plane_ok(D.base, D.stride, G.amask, G.row_bytes(p))) {
                ffhip_set_error("%s: frame %d plane %d: base and stride must be %u-byte aligned, the stride at least the decoded width", who,
                                i, p, G.amask + 1);
                return FFHIP_EINVAL;
            }
            for (int r = 0; r < P.nrefs; r++) {
                int rw, rh;
                ref_size(i, r, p, &rw, &rh);
                if (!ffhip_plane_ok(P.ref[r].base[p], P.ref[r].stride[p], G.ps - 1, (ptrdiff_t)rw * G.ps)) {
                    ffhip_set_error("%s: frame %d reference %d plane %d: NULL, misaligned or a stride below the width", who, i, r, p);
                    return FFHIP_EINVAL;
                }
            }
        }
    }
    /* no reference plane of the call may be a destination plane of the call: a launch's frames are predicted side by side
     * (destination planes that coincide are not refused) */
    FFHipSpanSet dst;
    dst.reserve((size_t)npics * 3);
    for (int i = 0; i < npics; i++)
        for (int p = 0; p < 3; p++)
            dst.add(G.span(pic(i).plane[p].base, pic(i).plane[p].stride, p));
    dst.seal();
    for (int j = 0; j < npics; j++)
        for (int r = 0; r < pic(j).nrefs; r++)
            for (int q = 0; q < 3; q++) {
                int rw, rh;
                ref_size(j, r, q, &rw, &rh);
                if (dst.hits(ffhip_plane_span(pic(j).ref[r].base[q], pic(j).ref[r].stride[q], (ptrdiff_t)rw * G.ps, rh))) {
                    ffhip_set_error("%s: frame %d reference %d plane %d overlaps a plane the call writes", who, j, r, q);
                    return FFHIP_EINVAL;
                }
            }
    return 0;
}
} // namespace

extern "C" int ffhip_vp9_inter_frames_dev(int bit_depth, int ss_h, int ss_v, int width, int height, int npics, const FFHipVp9InterPic *pics,
                                          void *stream)
{
    const int r = check_frames(
        "ffhip_vp9_inter_frames_dev", bit_depth, ss_h, ss_v, width, height, npics, pics,
        [&](int i) -> const FFHipVp9InterPic & { return pics[i]; },
        [&](int, int, int p, int *w, int *h) {
            *w = (width + (p ? ss_h : 0)) >> (p ? ss_h : 0);
            *h = (height + (p ? ss_v : 0)) >> (p ? ss_v : 0);
        });
    if (r < 0)
        return r;
    if (!ffhip_have_device())
        return FFHIP_ENOSYS;
    return ffhip_launch_vp9_inter_frames(bit_depth, ss_h, ss_v, width, height, npics, pics, (hipStream_t)stream);
}

extern "C" int ffhip_vp9_inter_frames_scaled_dev(int bit_depth, int ss_h, int ss_v, int width, int height, int npics,
                                                 const FFHipVp9InterPicScaled *pics, void *stream)
{
    static const char fn[] = "ffhip_vp9_inter_frames_scaled_dev";
    if (npics > 0 && pics && width > 0 && height > 0)
        for (int i = 0; i < npics; i++)
            for (int r = 0; r < pics[i].pic.nrefs && r < 3; r++) {
                const int rw = pics[i].ref_w[r], rh = pics[i].ref_h[r];
                const bool same = rw == width && rh == height; /* vp9.c: unscaled; otherwise the 2x / 16x limits */
                if (rw <= 0 || rh <= 0 || rw > 65535 || rh > 65535 ||
                    (!same && ((int64_t)2 * width < rw || (int64_t)2 * height < rh || width > (int64_t)16 * rw || height > (int64_t)16 * rh))) {
                    ffhip_set_error("%s: frame %d reference %d: size %d x %d for a %d x %d frame (1..65535, at most 2x larger, 16x smaller)",
                                    fn, i, r, rw, rh, width, height);
                    return FFHIP_EINVAL;
                }
            }
    const int r = check_frames(
        fn, bit_depth, ss_h, ss_v, width, height, npics, pics, [&](int i) -> const FFHipVp9InterPic & { return pics[i].pic; },
        [&](int i, int ref, int p, int *w, int *h) {
            *w = (pics[i].ref_w[ref] + (p ? ss_h : 0)) >> (p ? ss_h : 0);
            *h = (pics[i].ref_h[ref] + (p ? ss_v : 0)) >> (p ? ss_v : 0);
        });
    if (r < 0)
        return r;
    if (!ffhip_have_device())
        return FFHIP_ENOSYS;
    return ffhip_launch_vp9_inter_frames_scaled(bit_depth, ss_h, ss_v, width, height, npics, pics, (hipStream_t)stream);
}

extern "C" int ffhip_vp9_inter_block_preds(FFHipVp9InterPred *out, int bs, int row, int col, const int16_t mv[4][2][2], int comp,
                                           const uint8_t ref[2], int filter, int ss_h, int ss_v)
{
    if (!out || !mv || !ref || bs < 0 || bs > 12 || row < 0 || row > 8191 || col < 0 || col > 8191 || filter < 0 || filter > 3 ||
        (ss_h & ~1) || (ss_v & ~1)) {
        ffhip_set_error("ffhip_vp9_inter_block_preds: block size %d (0..12), row %d / col %d (0..8191), filter %d (0..3), subsampling %d, %d",
                        bs, row, col, filter, ss_h, ss_v);
        return FFHIP_EINVAL;
    }
    /* ff_vp9_bwh_tab[0] (libavcodec/vp9data.c) in samples: BS_64x64 .. BS_4x4 */
    static const uint8_t bw_tab[13] = { 64, 64, 32, 32, 32, 16, 16, 16, 8, 8, 8, 4, 4 };
    static const uint8_t bh_tab[13] = { 64, 32, 64, 32, 16, 32, 16, 8, 16, 8, 4, 8, 4 };
    int n = 0;
    const int nr = comp ? 2 : 1;
    /* one call: (x, y, w, h) in its plane, the MV of each reference from `pick` */
    auto emit = [&](bool chroma, int x, int y, int w, int h, auto pick) {
        FFHipVp9InterPred &R = out[n++];
        R = FFHipVp9InterPred();
        R.x = (uint16_t)x;
        R.y = (uint16_t)y;
        R.w = (uint8_t)w;
        R.h = (uint8_t)h;
        R.filter = (uint8_t)filter;
        R.flags = (uint8_t)((comp ? 1 : 0) | (chroma ? 2 : 0));
        for (int r = 0; r < nr; r++) {
            const Mv m = pick(r);
            R.ref[r] = ref[r];
            R.mv[r][0] = (int16_t)m.x;
            R.mv[r][1] = (int16_t)m.y;
        }
    };
    const int ly = row << 3, lx = col << 3, cy = row << (3 - ss_v), cx = col << (3 - ss_h);
    auto sub = [&](int s) { return [&, s](int r) { return mv_of(mv, s, r); }; };
    if (bs < 10) { /* at least 8 x 8 */
        const int w = bw_tab[bs], h = bh_tab[bs];
        emit(false, lx, ly, w, h, sub(0));
        emit(true, cx, cy, w >> ss_h, h >> ss_v, sub(0));
    } else if (bs == 10) { /* 8 x 4 */
        emit(false, lx, ly, 8, 4, sub(0));
        emit(false, lx, ly + 4, 8, 4, sub(2));
        auto d02 = [&](int r) { return div2(mv_of(mv, 0, r), mv_of(mv, 2, r)); };
        if (ss_v) {
            emit(true, cx, row << 2, 8 >> ss_h, 4, d02);
        } else {
            emit(true, cx, ly, 8 >> ss_h, 4, sub(0));
            /* libvpx takes the wrong block's MV for the bottom half in 4:2:2 (the reference emulates it) */
            if (ss_h)
                emit(true, cx, ly + 4, 4, 4, d02);
            else
                emit(true, cx, ly + 4, 8, 4, sub(2));
        }
    } else if (bs == 11) { /* 4 x 8 */
        emit(false, lx, ly, 4, 8, sub(0));
        emit(false, lx + 4, ly, 4, 8, sub(1));
        if (ss_h) {
            emit(true, col << 2, cy, 4, 8 >> ss_v, [&](int r) { return div2(mv_of(mv, 0, r), mv_of(mv, 1, r)); });
        } else {
            emit(true, lx, cy, 4, 8 >> ss_v, sub(0));
            emit(true, lx + 4, cy, 4, 8 >> ss_v, sub(1));
        }
    } else { /* 4 x 4 */
        emit(false, lx, ly, 4, 4, sub(0));
        emit(false, lx + 4, ly, 4, 4, sub(1));
        emit(false, lx, ly + 4, 4, 4, sub(2));
        emit(false, lx + 4, ly + 4, 4, 4, sub(3));
        auto d2 = [&](int a, int b) { return [&, a, b](int r) { return div2(mv_of(mv, a, r), mv_of(mv, b, r)); }; };
        if (ss_h && ss_v) {
            emit(true, col << 2, row << 2, 4, 4,
                 [&](int r) { return div4(mv_of(mv, 0, r), mv_of(mv, 1, r), mv_of(mv, 2, r), mv_of(mv, 3, r)); });
        } else if (ss_v) { /* 4:4:0 */
            emit(true, lx, row << 2, 4, 4, d2(0, 2));
            emit(true, lx + 4, row << 2, 4, 4, d2(1, 3));
        } else if (ss_h) { /* 4:2:2, the same libvpx quirk for the bottom block */
            emit(true, col << 2, ly, 4, 4, d2(0, 1));
            emit(true, col << 2, ly + 4, 4, 4, d2(1, 2));
        } else {
            emit(true, lx, ly, 4, 4, sub(0));
            emit(true, lx + 4, ly, 4, 4, sub(1));
            emit(true, lx, ly + 4, 4, 4, sub(2));
            emit(true, lx + 4, ly + 4, 4, 4, sub(3));
        }
    }
    return n;
}

extern "C" int ffhip_vp9_inter_block_preds_scaled(FFHipVp9InterPred *out, int bs, int row, int col, const int16_t mv[4][2][2], int comp,
                                                  const uint8_t ref[2], int filter, int ss_h, int ss_v)
{
    if (!out || !mv || !ref || bs < 0 || bs > 12 || row < 0 || row > 8191 || col < 0 || col > 8191 || filter < 0 || filter > 3 ||
        (ss_h & ~1) || (ss_v & ~1)) {
        ffhip_set_error("ffhip_vp9_inter_block_preds_scaled: block size %d (0..12), row %d / col %d (0..8191), filter %d (0..3), "
                        "subsampling %d, %d", bs, row, col, filter, ss_h, ss_v);
        return FFHIP_EINVAL;
    }
    static const uint8_t lw_tab[10] = { 6, 6, 5, 5, 5, 4, 4, 4, 3, 3 }; /* log2 of ff_vp9_bwh_tab[0] in samples, BS_64x64 .. BS_8x8 */
    static const uint8_t lh_tab[10] = { 6, 5, 6, 5, 4, 5, 4, 3, 4, 3 };
    int n = 0;
    const int nr = comp ? 2 : 1;
    /* one call of the SCALED template: (x, y, w, h) in its plane, its clip box (px, py, 1 << lpw, 1 << lph), the MV of each reference */
    auto emit = [&](bool chroma, int x, int y, int lw, int lh, int px, int py, int lpw, int lph, auto pick) {
        FFHipVp9InterPred &R = out[n++];
        R = FFHipVp9InterPred();
        R.x = (uint16_t)x;
        R.y = (uint16_t)y;
        R.w = (uint8_t)(1 << lw);
        R.h = (uint8_t)(1 << lh);
        R.filter = (uint8_t)filter;
        R.flags = (uint8_t)((comp ? 1 : 0) | (chroma ? 2 : 0) | FFHIP_VP9_PRED_SCALED);
        R.box[0] = (uint8_t)(px | py << 4);
        R.box[1] = (uint8_t)(lpw | lph << 4);
        for (int r = 0; r < nr; r++) {
            const Mv m = pick(r);
            R.ref[r] = ref[r];
            R.mv[r][0] = (int16_t)m.x;
            R.mv[r][1] = (int16_t)m.y;
        }
    };
    const int ly = row << 3, lx = col << 3, cy = row << (3 - ss_v), cx = col << (3 - ss_h);
    auto sub = [&](int s) { return [&, s](int r) { return mv_of(mv, s, r); }; };
    auto d2 = [&](int a, int b) { return [&, a, b](int r) { return div2(mv_of(mv, a, r), mv_of(mv, b, r)); }; };
    if (bs < 10) { /* at least 8 x 8: the whole block is the box */
        const int lw = lw_tab[bs], lh = lh_tab[bs];
        emit(false, lx, ly, lw, lh, 0, 0, lw, lh, sub(0));
        emit(true, cx, cy, lw - ss_h, lh - ss_v, 0, 0, lw - ss_h, lh - ss_v, sub(0));
        return n;
    }
    /* 8x4, 4x8 and 4x4: the 4x4 branch (vp9_mc_template.h keeps the 8x4 / 4x8 branches under SCALED == 0) */
    emit(false, lx, ly, 2, 2, 0, 0, 3, 3, sub(0));
    emit(false, lx + 4, ly, 2, 2, 4, 0, 3, 3, sub(1));
    emit(false, lx, ly + 4, 2, 2, 0, 4, 3, 3, sub(2));
    emit(false, lx + 4, ly + 4, 2, 2, 4, 4, 3, 3, sub(3));
    if (ss_h && ss_v) {
        emit(true, cx, cy, 2, 2, 0, 0, 2, 2, [&](int r) { return div4(mv_of(mv, 0, r), mv_of(mv, 1, r), mv_of(mv, 2, r), mv_of(mv, 3, r)); });
    } else if (ss_v) { /* 4:4:0: the chroma of the 8 x 8 area is 8 x 4 */
        emit(true, cx, cy, 2, 2, 0, 0, 3, 2, d2(0, 2));
        emit(true, cx + 4, cy, 2, 2, 4, 0, 3, 2, d2(1, 3));
    } else if (ss_h) { /* 4:2:2, 4 x 8, with libvpx's MV for the bottom block (webm issue 993) */
        emit(true, cx, cy, 2, 2, 0, 0, 2, 3, d2(0, 1));
        emit(true, cx, cy + 4, 2, 2, 0, 4, 2, 3, d2(1, 2));
    } else {
        emit(true, cx, cy, 2, 2, 0, 0, 3, 3, sub(0));
        emit(true, cx + 4, cy, 2, 2, 4, 0, 3, 3, sub(1));
        emit(true, cx, cy + 4, 2, 2, 0, 4, 3, 3, sub(2));
        emit(true, cx + 4, cy + 4, 2, 2, 4, 4, 3, 3, sub(3));
    }
    return n;
}
