/*
 * hevc_mc_rules.h — the sample arithmetic of HEVC motion compensation, once: the 8-tap luma and 4-tap chroma filters (H.265 Tables
 * 8-11 and 8-12: ff_hevc_qpel_filters / ff_hevc_epel_filters), the integer steps that make the 14-bit intermediate of
 * put_hevc_{qpel,epel}_{pixels,h,v,hv} (libavcodec/h26x/h2656_inter_template.c:29-58,97-245,342-485) and the five output stages
 * put, _uni, _uni_w, _bi, _bi_w (h2656_inter_template.c:60-88,247-340,487-578; libavcodec/hevc/dsp_template.c:368-815), per output
 * sample, on ints, with the depth as an argument.
 *
 * Shared by the sample-per-lane kernels k_hevc_mc_s (hevc_mc.hip) and k_hevc_inter_pic (hevc_inter_pic.hip): the taps, every integer
 * step, the positions without a second pass, the output stages; and by the 8-bit kernels k_hevc_mc (hevc_mc.hip) and k_hevc_qpel_m
 * (hevc_qpel_m.hip): the taps, the output stages, the row-piece load and the int16 pack.  Fetching, clamping of coordinates and storing
 * stay with the callers: a caller hands the statements a source, anything with `int at(int dx, int dy) const` that returns the
 * reference sample (dx, dy) away from the output sample (the convention of h264_mc_rules.h).
 *
 * Departure: the two loops over a block (first-pass plane, then every sample) stay in the bodies of k_hevc_mc_s and of hip_predict,
 * written over the pieces here.  As one sweep in this header, over functors for the source, the item split and the store,
 * k_hevc_inter_pic took 90 VGPRs for 87 and k_hevc_mc_s<uint16_t, luma, bi> 30 for 28.
 *
 * hevc_mc.hip's packed forms (mc_hrow4 on -128-biased bytes with v_dot4_i32_i8, the v_dot2_i32_i16 pass over row pairs) and
 * hevc_qpel_m.hip's matrix-core products (the banded tap matrices of HqTab, the 8192 / 128 accumulator seeds, the low / high byte
 * split) are statements of the same filter for other data layouts, not copies of this one: they stay there, with their operand
 * tables generated from the taps below.
 */
#ifndef FFHIP_HEVC_MC_RULES_H
#define FFHIP_HEVC_MC_RULES_H

#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#if defined(__HIPCC__)
#include "common.h"
#define HEVCMC_FN __host__ __device__ __forceinline__
#else
#define HEVCMC_FN static inline
#endif

/* ---- the taps ------------------------------------------------------------------------------------------------------------------- */

/* tap t of the filter of fraction f; 0 outside the filter.  TAPS 8: luma, f in quarters; TAPS 4: chroma, f in eighths.  Row 0 is
 * zeros as in the reference's tables: an integer position takes no filter */
template <int TAPS>
HEVCMC_FN constexpr int hevcmc_tap(int f, int t)
{
    constexpr int8_t luma[4][8] = { { 0 }, { -1, 4, -10, 58, 17, -5, 1, 0 }, { -1, 4, -11, 40, 40, -11, 4, -1 }, { 0, 1, -5, 17, 58, -10, 4, -1 } };
    constexpr int8_t chroma[8][4] = { { 0 }, { -2, 58, 10, -2 }, { -4, 54, 16, -2 }, { -6, 46, 28, -4 }, { -4, 36, 36, -4 },
                                      { -4, 28, 46, -6 }, { -2, 16, 54, -4 }, { -2, 10, 58, -2 } };
    static_assert(TAPS == 8 || TAPS == 4, "luma or chroma");
    return (t < 0 || t >= TAPS) ? 0 : TAPS == 8 ? luma[f][t] : chroma[f][t];
}
/* samples before the output sample under the filter: QPEL_EXTRA_BEFORE 3, EPEL_EXTRA_BEFORE 1 */
template <int TAPS>
HEVCMC_FN constexpr int hevcmc_before() { return TAPS / 2 - 1; }

/* a table as a value, so that a constexpr function can make it */
template <class T, int R, int C>
struct HevcMcTab { T v[R][C]; };

/* the taps as bytes, [fraction][tap]: what a kernel keeps in __constant__ memory */
template <int TAPS>
constexpr HevcMcTab<int8_t, 32 / TAPS, TAPS> hevcmc_tap_bytes()
{
    HevcMcTab<int8_t, 32 / TAPS, TAPS> r{};
    for (int f = 0; f < 32 / TAPS; f++)
        for (int t = 0; t < TAPS; t++)
            r.v[f][t] = (int8_t)hevcmc_tap<TAPS>(f, t);
    return r;
}

#if defined(__HIPCC__)
/* the byte tables of the kernels.  16-byte aligned: k_hevc_mc reads a row of taps as one or two dwords (scalar loads).  static: every
 * file that includes this has its own copy (one symbol for all would need relocatable device code); a file that reads none drops it */
static __constant__ __attribute__((aligned(16))) HevcMcTab<int8_t, 4, 8> hevc_lf8 = hevcmc_tap_bytes<8>();
static __constant__ __attribute__((aligned(16))) HevcMcTab<int8_t, 8, 4> hevc_cf4 = hevcmc_tap_bytes<4>();
/* hevcmc_taps() for a kernel: the same values out of the byte tables (scalar loads where the fraction is uniform) */
template <int TAPS>
__device__ __forceinline__ void hevcmc_taps_c(int mx, int my, int (&hf)[TAPS], int (&vf)[TAPS])
{
#pragma unroll
    for (int t = 0; t < TAPS; t++) {
        if constexpr (TAPS == 4) {
            hf[t] = hevc_cf4.v[mx][t]; vf[t] = hevc_cf4.v[my][t];
        } else {
            hf[t] = hevc_lf8.v[mx][t]; vf[t] = hevc_lf8.v[my][t];
        }
    }
}
#endif

/* the taps as v_dot2_i32_i16 operands over pairs of vertically adjacent rows, pk(a, b) = a | b << 16 multiplying rows (2q, 2q + 1).
 * NP = TAPS / 2 + 1 pairs cover an output whichever parity its first row has:
 *   [f][0 .. NP-1]    first row even: (c0, c1) (c2, c3) .. (0, 0)
 *   [f][NP .. 2NP-1]  first row odd:  (0, c0) (c1, c2) .. (c_last, 0)      — the same taps one row down
 * and two words of zeros pad the row to 16 bytes' multiple */
template <int TAPS>
constexpr HevcMcTab<uint32_t, 32 / TAPS, TAPS + 4> hevcmc_dot2_rows()
{
    constexpr int NP = TAPS / 2 + 1;
    HevcMcTab<uint32_t, 32 / TAPS, TAPS + 4> r{};
    for (int f = 0; f < 32 / TAPS; f++)
        for (int odd = 0; odd < 2; odd++)
            for (int q = 0; q < NP; q++) {
                const int t = 2 * q - odd; /* the tap on the pair's first row */
                r.v[f][odd * NP + q] = ((uint32_t)hevcmc_tap<TAPS>(f, t) & 0xffffu) | ((uint32_t)hevcmc_tap<TAPS>(f, t + 1) << 16);
            }
    return r;
}

/* ---- the interpolation: the 14-bit intermediate ---------------------------------------------------------------------------------- */

/* the FIR sum over TAPS samples, s(t) the sample under tap t (QPEL_FILTER / EPEL_FILTER) */
template <int TAPS, class Smp>
HEVCMC_FN int hevcmc_fir(const int (&c)[TAPS], Smp s)
{
    int acc = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int t = 0; t < TAPS; t++)
        acc += c[t] * s(t);
    return acc;
}
/* a sum over samples drops BIT_DEPTH - 8 bits (the only pass of _h and _v, the first of _hv: h2656_inter_template.c:113,131,160) */
HEVCMC_FN int hevcmc_first(int sum, int bd) { return sum >> (bd - 8); }
/* the second pass of _hv sums first-pass values and drops 6 (:168) */
HEVCMC_FN int hevcmc_second(int sum) { return sum >> 6; }
/* an integer position gains 14 - BIT_DEPTH (put_pixels, :29-42) */
HEVCMC_FN int hevcmc_full(int sample, int bd) { return sample << (14 - bd); }

/* the taps of the two fractions of a block, as ints */
template <int TAPS>
HEVCMC_FN void hevcmc_taps(int mx, int my, int (&hf)[TAPS], int (&vf)[TAPS])
{
    for (int t = 0; t < TAPS; t++) {
        hf[t] = hevcmc_tap<TAPS>(mx, t);
        vf[t] = hevcmc_tap<TAPS>(my, t);
    }
}

/* the positions that need no second pass, for one sample: h, v, or the integer position */
template <int TAPS, class Src>
HEVCMC_FN int hevcmc_direct(const Src &S, const int (&hf)[TAPS], const int (&vf)[TAPS], int mx, int my, int bd)
{
    constexpr int B = hevcmc_before<TAPS>();
    if (mx)
        return hevcmc_first(hevcmc_fir<TAPS>(hf, [&](int t) { return S.at(t - B, 0); }), bd);
    if (my)
        return hevcmc_first(hevcmc_fir<TAPS>(vf, [&](int t) { return S.at(0, t - B); }), bd);
    return hevcmc_full(S.at(0, 0), bd);
}

/* put_hevc_{qpel,epel}_{pixels,h,v,hv} for one sample: the intermediate at the fraction (mx, my); hv without a plane — the TAPS
 * first-pass values of the sample's column, each an int16 as in the reference's tmp_array */
template <int TAPS, class Src>
HEVCMC_FN int hevcmc_sample_taps(const Src &S, int mx, int my, int bd)
{
    constexpr int B = hevcmc_before<TAPS>();
    int hf[TAPS], vf[TAPS], col[TAPS];
    hevcmc_taps<TAPS>(mx, my, hf, vf);
    if (!(mx && my))
        return hevcmc_direct<TAPS>(S, hf, vf, mx, my, bd);
    for (int r = 0; r < TAPS; r++)
        col[r] = (int16_t)hevcmc_first(hevcmc_fir<TAPS>(hf, [&](int t) { return S.at(t - B, r - B); }), bd);
    return hevcmc_second(hevcmc_fir<TAPS>(vf, [&](int t) { return col[t]; }));
}
template <class Src>
HEVCMC_FN int hevcmc_sample(const Src &S, bool chroma, int mx, int my, int bd)
{
    return chroma ? hevcmc_sample_taps<4>(S, mx, my, bd) : hevcmc_sample_taps<8>(S, mx, my, bd);
}

/* ---- the output stages ----------------------------------------------------------------------------------------------------------- */

enum { HEVCMC_PUT = 0, HEVCMC_UNI = 1, HEVCMC_UNI_W = 2, HEVCMC_BI = 3, HEVCMC_BI_W = 4 };

/* the per-block parts.  The weight shift: `shift` of _uni_w, log2Wd of _bi_w — denom + 14 - BIT_DEPTH */
HEVCMC_FN int hevcmc_wshift(int denom, int bd) { return denom + 14 - bd; }
/* a slice-header offset in the units of the depth: ox * (1 << (BIT_DEPTH - 8)) */
HEVCMC_FN int hevcmc_offset(int ox, int bd) { return ox * (1 << (bd - 8)); }
/* what _uni_w adds before its shift, and _bi_w before its: (ox0 + ox1 + 1) << log2Wd in the reference's multiply form — the summed
 * offset may be negative */
HEVCMC_FN int hevcmc_uniw_round(int wsh) { return 1 << (wsh - 1); }
HEVCMC_FN int hevcmc_biw_offset(int ox, int wsh) { return (ox + 1) * (1 << wsh); }
/* av_clip_pixel */
HEVCMC_FN int hevcmc_clip(int v, int bd)
{
    const int maxv = (1 << bd) - 1;
    v = v < 0 ? 0 : v;
    return v > maxv ? maxv : v;
}

/* what a stage makes of the intermediate v — and, bi / bi_w, of the other list's v2, which goes with wx0 as in the reference
 * (src2 * wx0 + src * wx1) — before the clip.  ox: hevcmc_offset()'s, for bi_w the two lists' sum; wsh: hevcmc_wshift()'s.  HEVCMC_PUT
 * hands the intermediate through.  With mode and bd constants the shifts fold: 6 and 7 at 8 bits.  The 8-bit kernels that pack four
 * samples into a dword clip with common.h's clip_u8(), which keeps the compiler from a packed clip; everyone else calls hevcmc_out() */
HEVCMC_FN int hevcmc_stage(int mode, int v, int v2, int wx0, int wx1, int ox, int wsh, int bd)
{
    const int shu = 14 - bd;
    if (mode == HEVCMC_UNI)
        return (v + (1 << (shu - 1))) >> shu;
    if (mode == HEVCMC_UNI_W)
        return ((v * wx0 + hevcmc_uniw_round(wsh)) >> wsh) + ox;
    if (mode == HEVCMC_BI)
        return (v + v2 + (1 << shu)) >> (shu + 1);
    if (mode == HEVCMC_BI_W)
        return (v * wx1 + v2 * wx0 + hevcmc_biw_offset(ox, wsh)) >> (wsh + 1);
    return v;
}
/* the sample: the stage, clipped (the put stage leaves its int16 alone) */
HEVCMC_FN int hevcmc_out(int mode, int v, int v2, int wx0, int wx1, int ox, int wsh, int bd)
{
    const int o = hevcmc_stage(mode, v, v2, wx0, wx1, ox, wsh, bd);
    return mode == HEVCMC_PUT ? o : hevcmc_clip(o, bd);
}

/* ---- launching: the mode as a compile-time constant ------------------------------------------------------------------------------ */

/* f(std::integral_constant<int, mode>()); anything above 4 is bi_w, as the switches this replaces had it */
template <class F>
static inline void hevcmc_with_mode(int mode, F &&f)
{
    switch (mode) {
    case HEVCMC_PUT:   f(std::integral_constant<int, HEVCMC_PUT>()); break;
    case HEVCMC_UNI:   f(std::integral_constant<int, HEVCMC_UNI>()); break;
    case HEVCMC_UNI_W: f(std::integral_constant<int, HEVCMC_UNI_W>()); break;
    case HEVCMC_BI:    f(std::integral_constant<int, HEVCMC_BI>()); break;
    default:           f(std::integral_constant<int, HEVCMC_BI_W>()); break;
    }
}

#if defined(__HIPCC__)
/* ---- device only ----------------------------------------------------------------------------------------------------------------- */

/* two int16 in a dword, and a row piece of four int16 (the other list's intermediates; rows are MAX_PB_SIZE = 64 apart): one 8-byte
 * load where the piece is aligned */
__device__ __forceinline__ uint32_t hevcmc_pk16(int lo, int hi) { return ((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16); }
__device__ __forceinline__ void hevcmc_ld4(const int16_t *q, bool aligned, int (&o)[4])
{
    if (aligned) {
        const uint2 v = *reinterpret_cast<const uint2 *>(q);
        o[0] = (int16_t)(v.x & 0xffff); o[1] = (int)v.x >> 16; o[2] = (int16_t)(v.y & 0xffff); o[3] = (int)v.y >> 16;
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
            o[j] = q[j];
    }
}

#endif /* __HIPCC__ */

#endif /* FFHIP_HEVC_MC_RULES_H */
