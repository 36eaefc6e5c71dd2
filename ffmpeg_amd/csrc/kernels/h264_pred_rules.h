/*
 * h264_pred_rules.h — the sample arithmetic of H.264 intra prediction, once: the directional rules of pred4x4 / pred8x8l over a block's
 * edge line with the 8x8l low-pass filter, and the block rules of pred8x8 / pred8x16 / pred16x16 — which neighbours a mode reads, the
 * plane predictor, the DCs (libavcodec/h264pred_template.c, modes libavcodec/h264pred.h:35-82) — per output sample, on ints, through
 * callables, with the depth as the arguments mid = 1 << (bit_depth - 1) and maxv = (1 << bit_depth) - 1.
 *
 * Shared by the batch kernels of h264_pred.hip, the macroblock reconstruction of h264_intra_mb.h (the picture kernels of h264_intra.hip,
 * h264_c422.hip and h264_mbaff.hip, and the host emulation), the host faces of shims.hip (what to stage) and vp8_recon_frame.hip (the
 * whole-block DCs).  Loading, staging, who computes what and storing stay with the callers.  The table forms of h264_intra_mb.h
 * (imb_p4_entry, imb_p4_tab, imb_p8_edge_tab, imb_p8_tab) are hp_dir_sample_e and hp_filter8_e solved for another layout — three indices
 * and a weighting per sample, so that every lane runs one straight line — not copies of them: they stay there, and
 * tests/h264_pred_rules_check.cpp decodes them against these rules.  h264_pred_codec.inc holds the other codecs' forms.
 */
#ifndef FFHIP_H264_PRED_RULES_H
#define FFHIP_H264_PRED_RULES_H

#if defined(__HIPCC__)
#define HP_FN __host__ __device__ __forceinline__
#define HP_MEM __host__ __device__ __forceinline__
#else
#define HP_FN static inline
#define HP_MEM inline
#endif

/* ---- pred4x4 / pred8x8l: rules over the edge line e[]: left column bottom-up, corner, row above, top-right ---- */
HP_FN int hp_a2(int a, int b) { return (a + b + 1) >> 1; }
HP_FN int hp_a3(int a, int b, int c) { return (a + 2 * b + c + 2) >> 2; }

/* neighbours a pred4x4 / pred8x8l mode reads: bit0 left, bit1 top, bit2 corner, bit3 top-right (h264pred.h:35-48 order); pred8x8l's
 * edge filter also reads the corner when the block has one and the mode reads the left column or the row above */
HP_FN unsigned hp_need(int mode)
{
    /* 12 nibbles, mode 0 in the low one: V=2 H=1 DC=3 DDL=a DDR=7 VR=7 HD=7 VL=a HU=1 LEFT_DC=1 TOP_DC=2 DC_128=0 */
    return (unsigned)(0x0211a777a312ull >> (4 * mode)) & 15u;
}

/* the edge line as a callable e(k) (an array in LDS, or the tile read in place) */
struct HpArr {
    const int *p;
    HP_MEM int operator()(int k) const { return p[k]; }
};

template <int N, class E>
HP_FN int hp_dir_sample_e(int mode, const E &e, int x, int y, int dc)
{
    auto T = [&](int k) { return e(N + 1 + k); };
    switch (mode) {
    case 0: return T(x);
    case 1: return e(N - 1 - y);
    case 3: {
        const int i = x + y;
        return i < 2 * N - 2 ? hp_a3(T(i), T(i + 1), T(i + 2)) : (T(2 * N - 2) + 3 * T(2 * N - 1) + 2) >> 2;
    }
    case 4: {
        const int i = N - 1 - y + x;
        return hp_a3(e(i), e(i + 1), e(i + 2));
    }
    case 5: {
        const int d = 2 * x - y, h = d >> 1;
        if (d < 0)
            return hp_a3(e(N + d), e(N + d + 1), e(N + d + 2));
        return (d & 1) ? hp_a3(e(N + h), e(N + h + 1), e(N + h + 2)) : hp_a2(e(N + h), e(N + h + 1));
    }
    case 6: {
        const int d = 2 * y - x, h = d >> 1;
        if (d < 0)
            return hp_a3(e(N - d - 2), e(N - d - 1), e(N - d));
        return (d & 1) ? hp_a3(e(N - h), e(N - h - 1), e(N - h - 2)) : hp_a2(e(N - h), e(N - h - 1));
    }
    case 7: {
        const int i = (y >> 1) + x;
        return (y & 1) ? hp_a3(T(i), T(i + 1), T(i + 2)) : hp_a2(T(i), T(i + 1));
    }
    case 8: {
        const int i = 2 * y + x, j = N - 1 - (i >> 1);
        if (i >= 2 * N - 2)
            return e(0);
        if (i == 2 * N - 3)
            return (e(1) + 3 * e(0) + 2) >> 2;
        return (i & 1) ? hp_a3(e(j), e(j - 1), e(j - 2)) : hp_a2(e(j), e(j - 1));
    }
    default: return dc;
    }
}

template <int N>
HP_FN int hp_dir_sample(int mode, const int *e, int x, int y, int dc)
{
    return hp_dir_sample_e<N>(mode, HpArr{ e }, x, y, dc);
}

/* the DC of modes 2 (both sides), 9 (LEFT_DC), 10 (TOP_DC); 128 otherwise */
template <int N, class E>
HP_FN int hp_dir_dc_e(int mode, const E &e, int mid = 128 /* 1 << (bit_depth - 1) */)
{
    if (mode != 2 && mode != 9 && mode != 10)
        return mid;
    int sl = 0, st = 0;
    for (int i = 0; i < N; i++) {
        sl += mode != 10 ? e(i) : 0;
        st += mode != 9 ? e(N + 1 + i) : 0;
    }
    return mode == 2 ? (sl + st + N) >> (N == 8 ? 4 : 3) : ((mode == 9 ? sl : st) + N / 2) >> (N == 8 ? 3 : 2);
}

template <int N>
HP_FN int hp_dir_dc(int mode, const int *e)
{
    return hp_dir_dc_e<N>(mode, HpArr{ e });
}

/* PREDICT_8x8_LOAD_LEFT / _TOP / _TOPRIGHT / _TOPLEFT (h264pred_template.c:822-856): entry j of the low-pass filtered line from
 * the raw line w(0..24); entries the mode does not read are 0 */
template <class W>
HP_FN int hp_filter8_e(const W &w, int j, unsigned need, bool tl, bool tr)
{
    if (j < 8) {
        if (!(need & 1))
            return 0;
        return j == 7 ? hp_a3(tl ? w(8) : w(7), w(7), w(6)) : j == 0 ? (w(1) + 3 * w(0) + 2) >> 2 : hp_a3(w(j + 1), w(j), w(j - 1));
    }
    if (j == 8)
        return (need & 4) ? hp_a3(w(7), w(8), w(9)) : 0;
    if (j < 17) {
        if (!(need & 2))
            return 0;
        return j == 9 ? hp_a3(tl ? w(8) : w(9), w(9), w(10)) : j == 16 ? hp_a3(tr ? w(17) : w(16), w(16), w(15)) : hp_a3(w(j - 1), w(j), w(j + 1));
    }
    if (!(need & 8))
        return 0;
    return !tr ? w(16) : j == 24 ? (w(23) + 3 * w(24) + 2) >> 2 : hp_a3(w(j - 1), w(j), w(j + 1));
}

HP_FN int hp_filter8(const int *w, int j, unsigned need, bool tl, bool tr)
{
    return hp_filter8_e(HpArr{ w }, j, need, tl, tr);
}

/* ---- pred8x8 / pred8x16 (the pred8x8[] of 4:2:2) / pred16x16: modes 0 DC 1 HOR 2 VERT 3 PLANE 4 LEFT_DC 5 TOP_DC 6 DC_128, and for the
 *      8-wide blocks the one-sided "mad cow" DCs 7 L0T 8 0LT 9 L00 10 0L0 (h264pred.h:67-82) ---- */

/* neighbours a block mode reads: the left column, the row above, the corner (the plane alone); as a mask bit0, bit1, bit2 */
HP_FN bool hp_blk_left(int mode) { return mode == 0 || mode == 1 || mode == 3 || mode == 4 || mode >= 7; }
HP_FN bool hp_blk_top(int mode) { return mode == 0 || mode == 2 || mode == 3 || mode == 5 || mode == 7 || mode == 8; }
HP_FN bool hp_blk_corner(int mode) { return mode == 3; }
HP_FN unsigned hp_blk_need(int mode) { return (hp_blk_left(mode) ? 1u : 0u) | (hp_blk_top(mode) ? 2u : 0u) | (hp_blk_corner(mode) ? 4u : 0u); }
/* ... and how many rows of the left column, of a block h high: L0T is top_dc with pred4x4_dc on the first cell, four rows */
HP_FN int hp_blk_lrows(int mode, int h) { return mode == 7 ? 4 : h; }

/* the plane predictor of a W x H block (h264pred_template.c:410-455 16x16, :746-780 8x8, :781-817 8x16): a gradient fitted to the border,
 * TOP(i) / LEFT(i) the row above / the left column, i = -1 the corner.  A side of 8 weighs its gradient (17 g + 16) >> 5, one of 16
 * (5 g + 32) >> 6 */
struct HpPlane {
    int a, H, V;
};
template <int S>
HP_FN int hp_plane_grad(int g)
{
    return S == 16 ? (5 * g + 32) >> 6 : (17 * g + 16) >> 5;
}
template <int W, int H, class Top, class Left>
HP_FN HpPlane hp_plane(const Top &TOP, const Left &LEFT)
{
    int gh = 0, gv = 0;
    for (int i = 1; i <= W / 2; i++)
        gh += i * (TOP(W / 2 - 1 + i) - TOP(W / 2 - 1 - i));
    for (int i = 1; i <= H / 2; i++)
        gv += i * (LEFT(H / 2 - 1 + i) - LEFT(H / 2 - 1 - i));
    HpPlane P;
    P.H = hp_plane_grad<W>(gh);
    P.V = hp_plane_grad<H>(gv);
    P.a = 16 * (LEFT(H - 1) + TOP(W - 1) + 1) - (H / 2 - 1) * P.V - (W / 2 - 1) * P.H;
    return P;
}
/* sample (x, y) before the clip, and clipped to 0 .. maxv */
HP_FN int hp_plane_raw(const HpPlane &P, int x, int y) { return (P.a + y * P.V + x * P.H) >> 5; }
HP_FN int hp_plane_sample(const HpPlane &P, int x, int y, int maxv)
{
    const int v = hp_plane_raw(P, x, y);
    return v < 0 ? 0 : v > maxv ? maxv : v;
}

/* the DC over whole sides of an N x N block: (sum + n / 2) / n over the n samples of the sides taken, mid when none is.  pred16x16's
 * DC / LEFT_DC / TOP_DC / DC_128 (:389-455) and, for N = 8, RV40's pred8x8 DCs that VP8 installs (h264pred.c:184-229) */
template <int N>
HP_FN int hp_sides_dc(bool left, bool top, int sl, int st, int mid)
{
    constexpr int LG = N == 16 ? 4 : N == 8 ? 3 : 2;
    const int s = (left ? sl : 0) + (top ? st : 0);
    return left && top ? (s + N) >> (LG + 1) : left || top ? (s + N / 2) >> LG : mid;
}
/* pred16x16's DC family by mode, from the sums of the left column and of the row above */
HP_FN int hp_dc16(int mode, int sl, int st, int mid) { return hp_sides_dc<16>(mode == 0 || mode == 4, mode == 0 || mode == 5, sl, st, mid); }

/* the DC family of an 8-wide block, one value per 4x4 cell: cell row r (0..1 of pred8x8, 0..3 of pred8x16), cell column cx; t0 / t1 the
 * sums of the row above over columns 0..3 / 4..7, l0 the sum of left rows 0..3, lr that of the cell's own four rows (not looked at by
 * L0T).  pred8x8 is pred8x16 over its first two cell rows in every mode.  A switch over the mode, then selects: the tile readers run
 * it with a mode that is the same in every lane (as selects throughout, every lane holds all four sums at once: k_h264_intra_c422 then
 * takes 85 to 90 VGPRs for 79 and loses a wave of occupancy).  k_h264_pred_blk<8> and k_h264_pred_8x16, where ONE thread fills every
 * cell of a block under a mode of its own, keep this rule solved per mode in their own lines (h264_pred.hip says why) */
HP_FN int hp_cell_dc(int mode, int r, int cx, int t0, int t1, int l0, int lr, int mid)
{
    int v = mid;
    switch (mode) {
    case 0: case 8: /* pred8x16_dc (h264pred_template.c:650-695); 8 = mad_cow_dc_0lt: cell (0, 0) from the top alone */
        v = cx == 0 ? (r == 0 ? (mode == 0 ? (t0 + l0 + 4) >> 3 : (t0 + 2) >> 2) : (lr + 2) >> 2)
                    : (r == 0 ? (t1 + 2) >> 2 : (t1 + lr + 4) >> 3);
        break;
    case 4: case 9: case 10: /* left_dc (:567-571); 9 = _l00: the cells of rows 4..7 stay mid; 10 = _0l0: those of rows 0..3 (:725-749) */
        v = ((mode == 9 && r == 1) || (mode == 10 && r == 0)) ? mid : (lr + 2) >> 2;
        break;
    case 5: case 7: /* top_dc (:599-603); 7 = _l0t: cell (0, 0) is pred4x4_dc */
        v = cx == 0 ? (t0 + 2) >> 2 : (t1 + 2) >> 2;
        if (mode == 7 && (r | cx) == 0)
            v = (t0 + l0 + 4) >> 3;
        break;
    default: break; /* 6: DC_128 */
    }
    return v;
}
#endif
