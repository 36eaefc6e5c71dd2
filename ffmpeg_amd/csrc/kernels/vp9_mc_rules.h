/*
 * vp9_mc_rules.h — the sample arithmetic of VP9 motion compensation, once: the three 8-tap filter sets (ff_vp9_subpel_filters,
 * libavcodec/vp9dsp.c:32-86), one pass of VP9DSPContext.mc[size][filter][avg][!!mx][!!my] for one sample — 8 taps, clip((sum + 64) >> 7),
 * or the bilinear a + ((m (b - a) + 8) >> 4) (libavcodec/vp9dsp_template.c:1966-2293) —, the walk of the scaled form smc[size][filter][avg]
 * (vp9dsp_template.c:2362-2540: output i of a pass sits at m + i d sixteenths, reads around its whole part with the taps of its
 * fraction) and the output stage (put, or avg (dst + v + 1) >> 1), on ints, with the largest sample value as an argument.
 *
 * Shared by the sample-per-lane kernels k_vp9_smc (vp9_mc.hip) and k_vp9_inter_frame (vp9_inter_frame.hip): the taps, the pass, the
 * walk, the output stage; and by the 8-bit kernels k_vp9_mc and k_vp9_mc_m (vp9_mc.hip): the taps, the bilinear, the output stage.
 * A caller hands a pass its samples as at(k), the sample k steps along the pass from the output sample (k = -3 .. 4; bilinear 0, 1).
 *
 * What stays with the kernels: fetching, the clamping of coordinates (vif_ref), the tile, the coverage mask and the stores; the origin
 * arithmetic of mc_luma_scaled / mc_chroma_scaled with vif_scale_mv (stated once, in vp9_inter_frame.hip).  vp9_mc.hip's packed forms
 * (vm_hrow4 on -128-biased bytes with v_dot4_i32_i8, the v_dot2_i32_i16 pass over row pairs) and k_vp9_mc_m's matrix-core products
 * (the banded tap operands, the 128 * 128 + 64 seeds, the identity band) are statements of the same filter for other data layouts,
 * not copies of this one: they stay there, with their operand tables generated from the taps below.
 */
#ifndef FFHIP_VP9_MC_RULES_H
#define FFHIP_VP9_MC_RULES_H

#include <stdint.h>

#if defined(__HIPCC__)
#include "common.h"
#define VP9MC_FN __host__ __device__ __forceinline__
#else
#define VP9MC_FN static inline
#endif

/* ---- the taps ------------------------------------------------------------------------------------------------------------------- */

/* tap t of filter 0 smooth / 1 regular / 2 sharp (enum FilterMode; 3, bilinear, has no row here) at fraction m in sixteenths; 0
 * outside the filter.  Row m = 0 is zeros, not the reference's { 0, 0, 0, 128, .. } (128 is no int8): a zero fraction is a copy, and
 * every caller handles it before it asks for taps.  Every other row sums to 128 */
VP9MC_FN constexpr int vp9mc_tap(int filter, int m, int t)
{
    constexpr int8_t taps[3][16][8] = {
        { { 0 }, { -3, -1, 32, 64, 38, 1, -3, 0 }, { -2, -2, 29, 63, 41, 2, -3, 0 }, { -2, -2, 26, 63, 43, 4, -4, 0 },
          { -2, -3, 24, 62, 46, 5, -4, 0 }, { -2, -3, 21, 60, 49, 7, -4, 0 }, { -1, -4, 18, 59, 51, 9, -4, 0 }, { -1, -4, 16, 57, 53, 12, -4, -1 },
          { -1, -4, 14, 55, 55, 14, -4, -1 }, { -1, -4, 12, 53, 57, 16, -4, -1 }, { 0, -4, 9, 51, 59, 18, -4, -1 }, { 0, -4, 7, 49, 60, 21, -3, -2 },
          { 0, -4, 5, 46, 62, 24, -3, -2 }, { 0, -4, 4, 43, 63, 26, -2, -2 }, { 0, -3, 2, 41, 63, 29, -2, -2 }, { 0, -3, 1, 38, 64, 32, -1, -3 } },
        { { 0 }, { 0, 1, -5, 126, 8, -3, 1, 0 }, { -1, 3, -10, 122, 18, -6, 2, 0 }, { -1, 4, -13, 118, 27, -9, 3, -1 },
          { -1, 4, -16, 112, 37, -11, 4, -1 }, { -1, 5, -18, 105, 48, -14, 4, -1 }, { -1, 5, -19, 97, 58, -16, 5, -1 }, { -1, 6, -19, 88, 68, -18, 5, -1 },
          { -1, 6, -19, 78, 78, -19, 6, -1 }, { -1, 5, -18, 68, 88, -19, 6, -1 }, { -1, 5, -16, 58, 97, -19, 5, -1 }, { -1, 4, -14, 48, 105, -18, 5, -1 },
          { -1, 4, -11, 37, 112, -16, 4, -1 }, { -1, 3, -9, 27, 118, -13, 4, -1 }, { 0, 2, -6, 18, 122, -10, 3, -1 }, { 0, 1, -3, 8, 126, -5, 1, 0 } },
        { { 0 }, { -1, 3, -7, 127, 8, -3, 1, 0 }, { -2, 5, -13, 125, 17, -6, 3, -1 }, { -3, 7, -17, 121, 27, -10, 5, -2 },
          { -4, 9, -20, 115, 37, -13, 6, -2 }, { -4, 10, -23, 108, 48, -16, 8, -3 }, { -4, 10, -24, 100, 59, -19, 9, -3 }, { -4, 11, -24, 90, 70, -21, 10, -4 },
          { -4, 11, -23, 80, 80, -23, 11, -4 }, { -4, 10, -21, 70, 90, -24, 11, -4 }, { -3, 9, -19, 59, 100, -24, 10, -4 }, { -3, 8, -16, 48, 108, -23, 10, -4 },
          { -2, 6, -13, 37, 115, -20, 9, -4 }, { -2, 5, -10, 27, 121, -17, 7, -3 }, { -1, 3, -6, 17, 125, -13, 5, -2 }, { 0, 1, -3, 8, 127, -7, 3, -1 } },
    };
    return (t < 0 || t >= 8) ? 0 : taps[filter][m][t];
}

/* a table as a value, so that a constexpr function can make it; rows are [filter * 16 + m] */
template <int C>
struct Vp9McTab { uint32_t v[48][C]; };

/* the 8 taps of a row as two dwords of int8, tap 0 the lowest byte: v_dot4_i32_i8 operands, k_vp9_mc_m's 64-bit tap row and, read as
 * bytes, the int8 [48][8] view of the per-sample pass */
constexpr Vp9McTab<2> vp9mc_tap_dwords()
{
    Vp9McTab<2> r{};
    for (int f = 0; f < 3; f++)
        for (int m = 0; m < 16; m++)
            for (int t = 0; t < 8; t++)
                r.v[f * 16 + m][t >> 2] |= ((uint32_t)vp9mc_tap(f, m, t) & 0xffu) << (8 * (t & 3));
    return r;
}

/* the taps as v_dot2_i32_i16 operands over pairs of vertically adjacent rows, pk(a, b) = a | b << 16 multiplying rows (2q, 2q + 1).
 * Five pairs cover an output whichever parity its first row has:
 *   [..][0 .. 4]  first row even: (c0, c1) (c2, c3) (c4, c5) (c6, c7) (0, 0)
 *   [..][5 .. 9]  first row odd:  (0, c0) (c1, c2) (c3, c4) (c5, c6) (c7, 0)       — the same taps one row down
 * and two words of zeros pad the row to 16 bytes' multiple */
constexpr Vp9McTab<12> vp9mc_dot2_rows()
{
    Vp9McTab<12> r{};
    for (int f = 0; f < 3; f++)
        for (int m = 0; m < 16; m++)
            for (int odd = 0; odd < 2; odd++)
                for (int q = 0; q < 5; q++) {
                    const int t = 2 * q - odd; /* the tap on the pair's first row */
                    r.v[f * 16 + m][odd * 5 + q] = ((uint32_t)vp9mc_tap(f, m, t) & 0xffffu) | ((uint32_t)vp9mc_tap(f, m, t + 1) << 16);
                }
    return r;
}

#if defined(__HIPCC__)
/* the tables of the kernels.  16-byte aligned: a uniform fraction's row is read with scalar loads.  static: every file that includes
 * this has its own copy (one symbol for all would need relocatable device code); a file that reads none drops it */
static __constant__ __attribute__((aligned(16))) Vp9McTab<2> vp9_h8 = vp9mc_tap_dwords();
static __constant__ __attribute__((aligned(16))) Vp9McTab<12> vp9_v2 = vp9mc_dot2_rows();
/* vp9mc_tap() for a kernel: vp9_h8 read as bytes, where m may differ from lane to lane.  __device__ alone: a table that a function
 * of the host's side names is made a global symbol and read through a pointer */
__device__ __forceinline__ int vp9mc_tap_c(int filter, int m, int t) { return reinterpret_cast<const int8_t (*)[16][8]>(vp9_h8.v)[filter][m][t]; }
#define VP9MC_TAP vp9mc_tap_c
#else
#define VP9MC_TAP vp9mc_tap
#endif

/* ---- one pass for one sample ------------------------------------------------------------------------------------------------------ */

/* the bilinear of filter 3 between a and its neighbour b along the pass; equal to ((16 - m) a + m b + 8) >> 4 */
VP9MC_FN int vp9mc_bilin(int m, int a, int b) { return a + ((m * (b - a) + 8) >> 4); }

/* one pass of mc[][filter][][!!mx][!!my] at fraction m (not 0) for one sample, at(k) the sample k steps along the pass: FILTER_8TAP's
 * av_clip_pixel((sum + 64) >> 7) over k = -3 .. 4, or FILTER_BILIN over k = 0, 1.  maxv: (1 << BIT_DEPTH) - 1 */
template <class At>
VP9MC_FN int vp9mc_pass(int filter, int m, int maxv, At at)
{
    if (filter == 3) {
        const int a = at(0);
        return vp9mc_bilin(m, a, at(1));
    }
    int sum = 64;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int t = 0; t < 8; t++)
        sum += VP9MC_TAP(filter, m, t) * at(t - 3);
    sum >>= 7;
    sum = sum < 0 ? 0 : sum;
    return sum > maxv ? maxv : sum;
}
/* the same where the fraction may be 0 — the scaled form, and an unscaled axis without a fraction: fraction 0 is the sample itself */
template <class At>
VP9MC_FN int vp9mc_pass0(int filter, int m, int maxv, At at)
{
    return m ? vp9mc_pass(filter, m, maxv, at) : at(0);
}

/* ---- the scaled walk -------------------------------------------------------------------------------------------------------------- */

/* output i of a pass that starts at fraction m and steps d sixteenths (16: unscaled, 32: 2x down, 1: 16x up) sits at vp9mc_pos():
 * it reads around sample vp9mc_whole() of the pass's source with the taps of fraction vp9mc_frac() */
VP9MC_FN constexpr int vp9mc_pos(int m, int i, int d) { return m + i * d; }
VP9MC_FN constexpr int vp9mc_whole(int pos) { return pos >> 4; }
VP9MC_FN constexpr int vp9mc_frac(int pos) { return pos & 15; }
/* rows of the source above the first output row that the vertical pass reads, and rows it reads beyond the last output's whole part
 * counted from the first (the filter's length) */
VP9MC_FN constexpr int vp9mc_before(int filter) { return filter == 3 ? 0 : 3; }
VP9MC_FN constexpr int vp9mc_extra(int filter) { return filter == 3 ? 2 : 8; }
/* the rows the horizontal pass makes for n output rows from fraction m0 at step d, the first of them vp9mc_before() above the first
 * output's whole part: smc's ((h - 1) dy + my) >> 4 plus the filter's length.  134 for 64 rows at 2x down */
VP9MC_FN constexpr int vp9mc_rows(int filter, int m0, int n, int d) { return vp9mc_whole(vp9mc_pos(m0, n - 1, d)) + vp9mc_extra(filter); }

/* ---- the output stage ------------------------------------------------------------------------------------------------------------- */

/* avg: (dst + v + 1) >> 1, and the same on the four bytes of a dword */
VP9MC_FN int vp9mc_avg(int d, int v) { return (d + v + 1) >> 1; }
VP9MC_FN uint32_t vp9mc_avg4(uint32_t a, uint32_t b) { return (a | b) - (((a ^ b) & 0xfefefefeu) >> 1); }

#endif /* FFHIP_VP9_MC_RULES_H */
