/*
 * hevc_lf_rules.h — the per-line rules of HEVC deblocking (hevc_{h,v}_loop_filter_{luma,chroma}, libavcodec/hevc/dsp_template.c
 * with h2656_deblock_template.c) and the per-sample rules of SAO (sao_band_filter / sao_edge_filter / sao_edge_restore,
 * h26x/h2656_sao_template.c), shared by the batch kernels of hevc_idct.hip and the picture kernel (hevc_lf_pic.hip).
 *
 * A luma line is v[0..7] = p3 p2 p1 p0 q0 q1 q2 q3; beta and tc arrive scaled to the bit depth.  A 4-line group decides once, from
 * its lines 0 and 3, then every line of the group runs the strong or the weak rule.
 */
#ifndef FFHIP_HEVC_LF_RULES_H
#define FFHIP_HEVC_LF_RULES_H

#include <stdint.h>

#include "common.h"

__device__ __forceinline__ int hv_abs(int v) { return v < 0 ? -v : v; }

enum { HLF_NONE = 0, HLF_WEAK = 1, HLF_STRONG = 2 };

/* a luma group's decision from the second differences (dp, dq), flatness |p3 - p0| + |q3 - q0| and step |p0 - q0| of its lines 0
 * and 3; the weak filter's nd_p / nd_q (1 or 2 samples per side) come back through the references */
__device__ __forceinline__ int hevc_lf_decide(int dp0, int dq0, int dp3, int dq3, int flat0, int flat3, int step0, int step3, int beta,
                                              int tc, int &nd_p, int &nd_q)
{
    const int d0 = dp0 + dq0, d3 = dp3 + dq3;
    if (d0 + d3 >= beta)
        return HLF_NONE;
    const int beta_3 = beta >> 3, beta_2 = beta >> 2, tc25 = (tc * 5 + 1) >> 1;
    if (flat0 < beta_3 && step0 < tc25 && flat3 < beta_3 && step3 < tc25 && (d0 << 1) < beta_2 && (d3 << 1) < beta_2)
        return HLF_STRONG;
    const int side = (beta + (beta >> 1)) >> 3;
    nd_p = dp0 + dp3 < side ? 2 : 1;
    nd_q = dq0 + dq3 < side ? 2 : 1;
    return HLF_WEAK;
}

/* the strong filter on one line; returns the mask of changed entries (bit k: v[k]) */
__device__ __forceinline__ unsigned hevc_lf_strong(int (&v)[8], int tc, bool no_p, bool no_q)
{
    const int p3 = v[0], p2 = v[1], p1 = v[2], p0 = v[3], q0 = v[4], q1 = v[5], q2 = v[6], q3 = v[7];
    const int t = tc << 1;
    unsigned ch = 0;
    if (!no_p) {
        v[3] = p0 + clip3(((p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3) - p0, -t, t);
        v[2] = p1 + clip3(((p2 + p1 + p0 + q0 + 2) >> 2) - p1, -t, t);
        v[1] = p2 + clip3(((2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3) - p2, -t, t);
        ch |= 0x0E;
    }
    if (!no_q) {
        v[4] = q0 + clip3(((p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3) - q0, -t, t);
        v[5] = q1 + clip3(((p0 + q0 + q1 + q2 + 2) >> 2) - q1, -t, t);
        v[6] = q2 + clip3(((2 * q3 + 3 * q2 + q1 + q0 + p0 + 4) >> 3) - q2, -t, t);
        ch |= 0x70;
    }
    return ch;
}

/* the weak filter on one line (a no-op where |delta| >= 10 tc); returns the mask of changed entries */
__device__ __forceinline__ unsigned hevc_lf_weak(int (&v)[8], int tc, int nd_p, int nd_q, bool no_p, bool no_q, int maxv)
{
    const int p2 = v[1], p1 = v[2], p0 = v[3], q0 = v[4], q1 = v[5], q2 = v[6], tc_2 = tc >> 1;
    auto clipp = [&](int x) { return min(max(x, 0), maxv); };
    int delta = (9 * (q0 - p0) - 3 * (q1 - p1) + 8) >> 4;
    if (hv_abs(delta) >= 10 * tc)
        return 0;
    unsigned ch = 0;
    delta = clip3(delta, -tc, tc);
    if (!no_p) { v[3] = clipp(p0 + delta); ch |= 0x08; }
    if (!no_q) { v[4] = clipp(q0 - delta); ch |= 0x10; }
    if (!no_p && nd_p > 1) { v[2] = clipp(p1 + clip3((((p2 + p0 + 1) >> 1) - p1 + delta) >> 1, -tc_2, tc_2)); ch |= 0x04; }
    if (!no_q && nd_q > 1) { v[5] = clipp(q1 + clip3((((q2 + q0 + 1) >> 1) - q1 - delta) >> 1, -tc_2, tc_2)); ch |= 0x20; }
    return ch;
}

/* the chroma filter on one line p1 p0 | q0 q1 (tc > 0) */
__device__ __forceinline__ void hevc_lf_chroma(int p1, int &p0, int &q0, int q1, int tc, bool no_p, bool no_q, int maxv)
{
    const int delta = clip3((((q0 - p0) * 4) + p1 - q1 + 4) >> 3, -tc, tc);
    const int P0 = p0, Q0 = q0;
    if (!no_p) p0 = min(max(P0 + delta, 0), maxv);
    if (!no_q) q0 = min(max(Q0 - delta, 0), maxv);
}

/* SAO: the offset sao_edge_filter adds to c between neighbours na and nb (edge_idx = { 1, 2, 0, 3, 4 } of the sign sum + 2) */
__device__ __forceinline__ int hevc_sao_edge_off(int c, int na, int nb, int o0, int o1, int o2, int o3, int o4)
{
    const int sel = 2 + (c > na) - (c < na) + (c > nb) - (c < nb);
    return sel == 0 ? o1 : sel == 1 ? o2 : sel == 2 ? o0 : sel == 3 ? o3 : o4;
}

/* SAO: the offset sao_band_filter adds to c (band = c >> (bd - 5); the four bands from left_class get o1..o4) */
__device__ __forceinline__ int hevc_sao_band_off(int c, int shift, int left_class, int o1, int o2, int o3, int o4)
{
    const int band = ((c >> shift) - left_class) & 31;
    return band == 0 ? o1 : band == 1 ? o2 : band == 2 ? o3 : band == 3 ? o4 : 0;
}

/* sao_edge_restore[variant] at sample (x, y) of a W x H block: 0 keeps the edge filter's output, 1 writes src + offset_val[0], 2
 * writes src.  The reference is a sequence of short loops whose later writes win; this evaluates that sequence for one sample.
 * borders: bit i = borders[i] (left, top, right, bottom); ve / he / de: vert_edge / horiz_edge / diag_edge bits. */
__device__ __forceinline__ int hevc_sao_restore_kind(int x, int y, int W, int H, int eo, unsigned borders, unsigned ve, unsigned he,
                                                     unsigned de, bool variant)
{
    enum { HORIZ = 0, VERT = 1, D135 = 2, D45 = 3 };
    const bool b0 = borders & 1, b1 = borders & 2, b2 = borders & 4, b3 = borders & 8;
    const bool ve0 = ve & 1, ve1 = ve & 2, he0 = he & 1, he1 = he & 2;
    const bool de0 = de & 1, de1 = de & 2, de2 = de & 4, de3 = de & 8;
    /* the running state of the reference after its border loops */
    const int init_x = (eo != VERT && b0) ? 1 : 0, w = W - ((eo != VERT && b2) ? 1 : 0);
    const int init_y = (eo != HORIZ && b1) ? 1 : 0, h = H - ((eo != HORIZ && b3) ? 1 : 0);
    const int s_ul = !de0 && eo == D135 && !b0 && !b1, s_ur = !de1 && eo == D45 && !b1 && !b2;
    const int s_lr = !de2 && eo == D135 && !b2 && !b3, s_ll = !de3 && eo == D45 && !b0 && !b3;
    int kind = 0;
    if (eo != VERT) {
        if (b0 && x == 0) kind = 1;
        if (b2 && x == W - 1) kind = 1;
    }
    if (eo != HORIZ) {
        if (b1 && y == 0 && x >= init_x && x < w) kind = 1;
        if (b3 && y == H - 1 && x >= init_x && x < w) kind = 1;
    }
    if (variant) {
        if (ve0 && eo != VERT && x == 0 && y >= init_y + s_ul && y < h - s_ll) kind = 2;
        if (ve1 && eo != VERT && x == w - 1 && y >= init_y + s_ur && y < h - s_lr) kind = 2;
        if (he0 && eo != HORIZ && y == 0 && x >= init_x + s_ul && x < w - s_ur) kind = 2;
        if (he1 && eo != HORIZ && y == h - 1 && x >= init_x + s_ll && x < w - s_lr) kind = 2;
        if (de0 && eo == D135 && x == 0 && y == 0) kind = 2;
        if (de1 && eo == D45 && x == w - 1 && y == 0) kind = 2;
        if (de2 && eo == D135 && x == w - 1 && y == h - 1) kind = 2;
        if (de3 && eo == D45 && x == 0 && y == h - 1) kind = 2;
    }
    return kind;
}

#endif
