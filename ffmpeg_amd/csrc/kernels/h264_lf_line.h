/*
 * h264_lf_line.h — the H.264 in-loop filter rule (h264_{v,h}_loop_filter_{luma,chroma}[_intra]_<depth>_c,
 * libavcodec/h264dsp_template.c:104-330): the only place in the device code where it is written.
 *
 * The rule exists in exactly TWO forms, because two kinds of kernel want opposite things from it:
 *   lf_line   the readable one: branches as the reference branches, returns the mask of the taps it changed.  A lane that fails the
 *             alpha / beta test is done after three compares, and a caller stores only what changed — which the batch faces need
 *             (they promise only that the WRITTEN pixels of a launch's edges are disjoint).  With its wrappers lf_apply (one line
 *             through any sample pointer) and lf_apply_dwords (eight contiguous 8-bit samples as two dwords):
 *             k_h264_loop_filter, k_h264_loop_filter_hbd, the row kernel k_h264_deblock_frame, k_h264_deblock_c422 and both
 *             MBAFF kernels of h264_mbaff.hip.
 *   db_edge   the register one: no per-lane control flow, every decision a sign, one wave-uniform branch for bS = 4.  A wave that
 *             walks a picture in decoder order is a chain of dependent edges with its lines in registers, and its time is the
 *             instructions it issues: k_h264_deblock_skew (the product path, every depth) and k_h264_deblock_band (8 bits).
 * Both take alpha, beta and tc0 scaled to the depth by lf_depth (db_edge scales inside, from a record's 8-bit fields), and
 * maxv = (1 << depth) - 1.
 */
#ifndef FFHIP_H264_LF_LINE_H
#define FFHIP_H264_LF_LINE_H
#include "common.h"

struct LfLine { int p3, p2, p1, p0, q0, q1, q2, q3; };

/* Filters one sample line in place; returns the mask of changed taps: bit0 p2, bit1 p1, bit2 p0, bit3 q0,
 * bit4 q1, bit5 q2.  cls: 0 luma, 1 chroma, 2 luma intra, 3 chroma intra. */
__device__ __forceinline__ int lf_line(LfLine &v, int cls, int alpha, int beta, int tc0, int maxv = 255)
{
    const int p0 = v.p0, p1 = v.p1, p2 = v.p2, q0 = v.q0, q1 = v.q1, q2 = v.q2;
    if (abs(p0 - q0) >= alpha || abs(p1 - p0) >= beta || abs(q1 - q0) >= beta)
        return 0;
    if (cls == 0) {
        if (tc0 < 0)
            return 0;
        int tc = tc0, m = 4 | 8;
        if (abs(p2 - p0) < beta) {
            if (tc0) {
                v.p1 = p1 + clip3(((p2 + ((p0 + q0 + 1) >> 1)) >> 1) - p1, -tc0, tc0);
                m |= 2;
            }
            tc++;
        }
        if (abs(q2 - q0) < beta) {
            if (tc0) {
                v.q1 = q1 + clip3(((q2 + ((p0 + q0 + 1) >> 1)) >> 1) - q1, -tc0, tc0);
                m |= 16;
            }
            tc++;
        }
        const int delta = clip3((((q0 - p0) * 4) + (p1 - q1) + 4) >> 3, -tc, tc);
        v.p0 = min(max(p0 + delta, 0), maxv);
        v.q0 = min(max(q0 - delta, 0), maxv);
        return m;
    }
    if (cls == 1) {
        if (tc0 <= 0)
            return 0;
        const int delta = clip3((((q0 - p0) * 4) + (p1 - q1) + 4) >> 3, -tc0, tc0);
        v.p0 = min(max(p0 + delta, 0), maxv);
        v.q0 = min(max(q0 - delta, 0), maxv);
        return 4 | 8;
    }
    if (cls == 3) {
        v.p0 = (2 * p1 + p0 + q1 + 2) >> 2;
        v.q0 = (2 * q1 + q0 + p1 + 2) >> 2;
        return 4 | 8;
    }
    /* luma intra */
    int m = 4 | 8;
    if (abs(p0 - q0) < ((alpha >> 2) + 2)) {
        if (abs(p2 - p0) < beta) {
            v.p0 = (p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3;
            v.p1 = (p2 + p1 + p0 + q0 + 2) >> 2;
            v.p2 = (2 * v.p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3;
            m |= 1 | 2;
        } else {
            v.p0 = (2 * p1 + p0 + q1 + 2) >> 2;
        }
        if (abs(q2 - q0) < beta) {
            v.q0 = (p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3;
            v.q1 = (p0 + q0 + q1 + q2 + 2) >> 2;
            v.q2 = (2 * v.q3 + 3 * q2 + q1 + q0 + p0 + 4) >> 3;
            m |= 16 | 32;
        } else {
            v.q0 = (2 * q1 + q0 + p1 + 2) >> 2;
        }
    } else {
        v.p0 = (2 * p1 + p0 + q1 + 2) >> 2;
        v.q0 = (2 * q1 + q0 + p1 + 2) >> 2;
    }
    return m;
}

/* alpha, beta and tc0 in 8-bit units (the decoder's tables, an edge record's bytes) scaled to depth 8 + sh as the reference scales
 * them: alpha << sh, beta << sh, luma tc0 * (1 << sh), chroma ((tc0 - 1) << sh) + 1.  The shifts are unsigned: the host faces hand
 * checkasm's alpha / beta through, ints far outside the tables' range.  The intra classes have no tc0 (pass 0). */
struct LfDepth { int alpha, beta, tc0; };
__device__ __forceinline__ int lf_depth_ab(int ab8, int sh) { return (int)((unsigned)ab8 << sh); }
__device__ __forceinline__ int lf_depth_tc0(int cls, int tc0_8, int sh)
{
    return (cls & 1) ? (int)(((unsigned)tc0_8 - 1U) << sh) + 1 : tc0_8 * (1 << sh);
}
__device__ __forceinline__ LfDepth lf_depth(int cls, int alpha8, int beta8, int tc0_8, int sh)
{
    return { lf_depth_ab(alpha8, sh), lf_depth_ab(beta8, sh), lf_depth_tc0(cls, tc0_8, sh) };
}

/* load / filter / store one line through a sample pointer; xs = step across the edge.  Reads p1 .. q1, for the luma classes p2 and
 * q2, for luma intra p3 and q3 (never beyond 4 samples from the edge for luma, 2 for chroma); stores the taps lf_line changed.
 * GATE_FIRST: lf_line's first test runs ahead of the outer taps' loads, so a line that fails it costs four loads and not six or
 * eight - measured worth it where every lane's loads touch cache lines of their own (k_h264_loop_filter_hbd on column edges: 0.052 ms
 * against 0.067 ms) and on the MBAFF kernels' serial chain of calls (2 - 3 %); docs/EXPERIMENTS.md. */
template <typename P, bool GATE_FIRST = false>
__device__ __forceinline__ void lf_apply(P *pix, ptrdiff_t xs, int cls, int alpha, int beta, int tc0, int maxv = 255)
{
    LfLine v;
    const bool luma = !(cls & 1);
    v.p1 = pix[-2 * xs]; v.p0 = pix[-xs]; v.q0 = pix[0]; v.q1 = pix[xs];
    if (GATE_FIRST && (abs(v.p0 - v.q0) >= alpha || abs(v.p1 - v.p0) >= beta || abs(v.q1 - v.q0) >= beta))
        return;
    v.p2 = luma ? pix[-3 * xs] : 0; v.q2 = luma ? pix[2 * xs] : 0;
    v.p3 = cls == 2 ? pix[-4 * xs] : 0; v.q3 = cls == 2 ? pix[3 * xs] : 0;
    const int m = lf_line(v, cls, alpha, beta, tc0, maxv);
    if (m & 1)  pix[-3 * xs] = (P)v.p2;
    if (m & 2)  pix[-2 * xs] = (P)v.p1;
    if (m & 4)  pix[-xs] = (P)v.p0;
    if (m & 8)  pix[0] = (P)v.q0;
    if (m & 16) pix[xs] = (P)v.q1;
    if (m & 32) pix[2 * xs] = (P)v.q2;
}

/* the same for a line of eight contiguous 8-bit samples p3 .. q3 at a dword-aligned address: two dwords in, the dwords that changed
 * out (the sample-wise form costs up to 8 byte loads and 6 byte stores per lane) */
__device__ __forceinline__ void lf_apply_dwords(uint32_t *w, int cls, int alpha, int beta, int tc0)
{
    const uint32_t a = w[0], b = w[1];
    LfLine v = { (int)(a & 255), (int)((a >> 8) & 255), (int)((a >> 16) & 255), (int)(a >> 24),
                 (int)(b & 255), (int)((b >> 8) & 255), (int)((b >> 16) & 255), (int)(b >> 24) };
    const int m = lf_line(v, cls, alpha, beta, tc0);
    if (m & 7)
        w[0] = (uint32_t)v.p3 | (uint32_t)v.p2 << 8 | (uint32_t)v.p1 << 16 | (uint32_t)v.p0 << 24;
    if (m & 56)
        w[1] = (uint32_t)v.q0 | (uint32_t)v.q1 << 8 | (uint32_t)v.q2 << 16 | (uint32_t)v.q3 << 24;
}

/* ---- the register form -----------------------------------------------------------------------------
 * A wave that is alone on its SIMD issues ONE instruction every four cycles, scalar or vector, and a step of the wavefront is eight
 * DEPENDENT edges: the filter is written for the fewest instructions, not for the fewest operations.
 *   - every comparison of h264dsp_template.c:104-330 is a sign: |a - b| < t  <=>  v_sad_u32(a, b, -t) < 0, and a conjunction is the
 *     sign of a maximum (v_max3_i32) — no compare / s_and chains, no exec-mask control flow;
 *   - alpha == 0 or beta == 0 (a bS = 0 edge) disables itself: |a - b| - 0 is never negative;
 *   - clips are v_med3_i32 (lanes whose range is empty, tc0 < 0, are deselected anyway); `if (tc0) p1 += clip(..., -tc0, tc0)` is the
 *     unconditional form because the clip range is empty when tc0 == 0;
 *   - the bS = 4 filter runs behind one wave-uniform branch and overrides the lanes it owns from the ORIGINAL samples.
 * v[0..7] = p3 p2 p1 p0 q0 q1 q2 q3 of one line; rec = {bS, alpha, beta, -} bytes, tcw = the edge's four tc0 bytes. */
__device__ __forceinline__ int db_sad3(int a, int b, int c)
{
    int d;
    asm("v_sad_u32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}
__device__ __forceinline__ int db_med3(int a, int lo, int hi)
{
    int d;
    asm("v_med3_i32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(lo), "v"(hi));
    return d;
}
__device__ __forceinline__ int db_clip255(int a)
{
    int d;
    asm("v_med3_i32 %0, %1, 0, %2" : "=v"(d) : "v"(a), "s"(255));
    return d;
}
__device__ __forceinline__ int db_max3(int a, int b, int c)
{
    int d;
    asm("v_max3_i32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}

/* sh = bit depth - 8: alpha, beta and tc0 arrive in 8-bit units and are scaled by lf_depth; maxv = 2^depth - 1 */
template <bool CHROMA>
__device__ __forceinline__ void db_edge(int (&v)[8], uint32_t rec, uint32_t tcw, int tcsh, bool skip, int sh = 0, int maxv = 255)
{
    const int p3 = v[0], p2 = v[1], p1 = v[2], p0 = v[3], q0 = v[4], q1 = v[5], q2 = v[6], q3 = v[7];
    const int alpha = lf_depth_ab((int)((rec >> 8) & 255), sh), negb = -lf_depth_ab((int)((rec >> 16) & 255), sh);
    const int nega = skip ? 0 : -alpha;                       /* a picture edge: never filtered */
    const int tc0 = lf_depth_tc0(CHROMA ? 1 : 0, __builtin_amdgcn_sbfe(tcw, tcsh, 8), sh);
    const bool is4 = (rec & 255) >= 4;
    /* m < 0: |p0 - q0| < alpha && |p1 - p0| < beta && |q1 - q0| < beta */
    const int m = db_max3(db_sad3(p0, q0, nega), db_sad3(p1, p0, negb), db_sad3(q1, q0, negb));
    const int mn = max(m, CHROMA ? -tc0 : ~tc0);              /* ... && tc0 > 0 (chroma) / tc0 >= 0 (luma): the bS < 4 filter's lanes */
    {   /* the bS < 4 filter, every lane (four macroblocks of different rows share an instruction: they are rarely all bS = 0, and a
         * wave-uniform skip costs register copies on both paths) */
        const int x4 = ((q0 - p0) << 2) + (p1 - q1) + 4;
        if (CHROMA) {
            const int delta = (mn >> 31) & db_med3(x4 >> 3, -tc0, tc0);
            v[3] = db_med3(p0 + delta, 0, maxv);
            v[4] = db_med3(q0 - delta, 0, maxv);
        } else {
            const int dap = db_sad3(p2, p0, negb), daq = db_sad3(q2, q0, negb);     /* < 0: |p2 - p0| < beta */
            const int avg = (p0 + q0 + 1) >> 1, ntc0 = -tc0;
            const int dp = db_med3(((p2 + avg) >> 1) - p1, ntc0, tc0), dq = db_med3(((q2 + avg) >> 1) - q1, ntc0, tc0);
            const int tc = tc0 + (int)((uint32_t)dap >> 31) + (int)((uint32_t)daq >> 31);
            const int delta = (mn >> 31) & db_med3(x4 >> 3, -tc, tc);
            v[2] = p1 + (dp & (max(mn, dap) >> 31));
            v[5] = q1 + (dq & (max(mn, daq) >> 31));
            v[3] = db_med3(p0 + delta, 0, maxv);
            v[4] = db_med3(q0 - delta, 0, maxv);
        }
    }
    const int mi = is4 ? m : 0;                               /* < 0: a bS = 4 line that passes the alpha / beta test */
    if (__builtin_amdgcn_ballot_w64(mi < 0)) {
        const int wp0 = (2 * p1 + p0 + q1 + 2) >> 2, wq0 = (2 * q1 + q0 + p1 + 2) >> 2;   /* the weak forms */
        if (CHROMA) {
            v[3] = mi < 0 ? wp0 : v[3];
            v[4] = mi < 0 ? wq0 : v[4];
        } else {
            const int ds = db_sad3(p0, q0, -((alpha >> 2) + 2));                        /* < 0: the strong filter */
            const int msp = db_max3(mi, ds, db_sad3(p2, p0, negb)), msq = db_max3(mi, ds, db_sad3(q2, q0, negb));
            const int s4 = p0 + q0, ep = p1 + s4, eq = q1 + s4;
            int sp0 = (2 * ep + p2 + q1 + 4) >> 3, sp1 = (p2 + ep + 2) >> 2, sp2 = (2 * (p3 + p2) + p2 + ep + 4) >> 3;
            int sq0 = (2 * eq + q2 + p1 + 4) >> 3, sq1 = (q2 + eq + 2) >> 2, sq2 = (2 * (q3 + q2) + q2 + eq + 4) >> 3;
            int w0 = mi < 0 ? wp0 : v[3], w1 = mi < 0 ? wq0 : v[4], w2 = mi < 0 ? p1 : v[2], w3 = mi < 0 ? q1 : v[5];
            /* every candidate first, opaque: with the arithmetic visible behind the selects the compiler sinks it into divergent
             * branches (exec-mask bookkeeping around three-instruction blocks) instead of emitting v_cndmask */
            asm("" : "+v"(sp0), "+v"(sp1), "+v"(sp2), "+v"(sq0), "+v"(sq1), "+v"(sq2), "+v"(w0), "+v"(w1), "+v"(w2), "+v"(w3));
            v[3] = msp < 0 ? sp0 : w0;
            v[2] = msp < 0 ? sp1 : w2;
            v[1] = msp < 0 ? sp2 : p2;
            v[4] = msq < 0 ? sq0 : w1;
            v[5] = msq < 0 ? sq1 : w3;
            v[6] = msq < 0 ? sq2 : q2;
        }
    }
}

#endif
