/*
 * me_search_cost.h — how the motion-search kernels (me_search.hip, me_search_pred.hip) compute a block cost: one wave, eight lanes per
 * candidate; lane = 8 * i + r evaluates candidate i, rows r and (16x16) r + 8 of the block, one 16-byte (8x8: 8-byte) load per row at
 * the candidate's byte-exact address in `ref`, against the current block's rows in registers.  SAD: v_sad_u8 over the dwords.  SATD: the
 * horizontal 8-point transform of a row's differences in the lane, the vertical one across the eight lanes of the candidate, then the
 * absolute sum.  The eight partial sums are added with DPP moves, the butterfly across lanes r and r ^ 4 is a ds_swizzle: no LDS.
 * With it what else the kernels share: the load of the current block, the wave minimum of a step's keys, and the launchers' choice of
 * a (block size, metric) instantiation; and, for the predictive kernels (me_search_pred.hip, me_search_seq.hip), the bilateral cost
 * mes_cost_bilat() and the cost policies they are instantiated with.  For the kernel files only.
 */
#ifndef FFHIP_ME_SEARCH_COST_H
#define FFHIP_ME_SEARCH_COST_H

#include <stdlib.h>

#include <type_traits>

#include "common.h"
#include "me_kernels.h"
#include "me_search_bilat_rules.h"

#define MES_DPP_XOR1 0xB1           /* quad_perm:[1,0,3,2] */
#define MES_DPP_XOR2 0x4E           /* quad_perm:[2,3,0,1] */
#define MES_DPP_HALF_MIRROR 0x141   /* lane r of an 8-lane half row reads lane 7 - r */
#define MES_DPP_ROR8 0x128          /* row_ror:8: lane l of a 16-lane row reads lane l ^ 8 */
#define MES_SWIZZLE_XOR4 0x101F     /* bit mode: and 0x1F, or 0, xor 4 */

template <int CTRL>
__device__ __forceinline__ int mes_dpp(int v)
{
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false);
}

/* the sum of v over the eight lanes of a candidate, in every one of them (all 64 lanes take part) */
__device__ __forceinline__ uint32_t mes_sum8(uint32_t v)
{
    v += (uint32_t)mes_dpp<MES_DPP_XOR1>((int)v);
    v += (uint32_t)mes_dpp<MES_DPP_XOR2>((int)v);
    v += (uint32_t)mes_dpp<MES_DPP_HALF_MIRROR>((int)v);   /* the quads are uniform by now: the other quad's sum */
    return v;
}

/* one row of eight differences a - b (two dwords each) of an 8x8 block whose row r lives in lane r of the candidate's eight: the
 * lane's share of sum |H8 (a - b) H8^T|.  The transform is the un-normalised Walsh-Hadamard one in any row order and sign, which
 * the absolute sum does not see. */
__device__ __forceinline__ uint32_t mes_satd_row(uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1, int lane)
{
    int d[8];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        d[i] = (int)((a0 >> (8 * i)) & 255u) - (int)((b0 >> (8 * i)) & 255u);
        d[4 + i] = (int)((a1 >> (8 * i)) & 255u) - (int)((b1 >> (8 * i)) & 255u);
    }
#pragma unroll
    for (int span = 1; span < 8; span <<= 1)
#pragma unroll
        for (int i = 0; i < 8; i++)
            if (!(i & span)) {
                const int p = d[i], q = d[i + span];
                d[i] = p + q;
                d[i + span] = p - q;
            }
    uint32_t sum = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        int v = d[i], o;
        o = mes_dpp<MES_DPP_XOR1>(v);
        v = (lane & 1) ? o - v : o + v;
        o = mes_dpp<MES_DPP_XOR2>(v);
        v = (lane & 2) ? o - v : o + v;
        o = __builtin_amdgcn_ds_swizzle(v, MES_SWIZZLE_XOR4);
        v = (lane & 4) ? o - v : o + v;
        sum += (uint32_t)abs(v);
    }
    return sum;
}

/* cost(x, y) of the lane's candidate, summed over its eight lanes.  c: the lane's rows of the current block; rf: the reference
 * frame.  Every lane of the wave calls it; valid (uniform over a candidate's eight lanes) false: no load, the result means nothing. */
template <int MB, int KIND>
__device__ __forceinline__ uint32_t mes_cost(const uint32_t (&c)[MB / 8][MB / 4], const uint8_t *rf, ptrdiff_t stride, bool valid, int x, int y,
                                             int lane)
{
    constexpr int NR = MB / 8, ND = MB / 4;
    uint32_t v[NR][ND];
#pragma unroll
    for (int k = 0; k < NR; k++)
#pragma unroll
        for (int j = 0; j < ND; j++)
            v[k][j] = 0;
    if (valid) {
        const uint8_t *p = rf + (ptrdiff_t)(y + (lane & 7)) * stride + x;
#pragma unroll
        for (int k = 0; k < NR; k++)
            __builtin_memcpy(v[k], p + (ptrdiff_t)(8 * k) * stride, MB);
    }
    uint32_t part = 0;
#pragma unroll
    for (int k = 0; k < NR; k++) {
        if (KIND == FFHIP_ME_SAD) {
#pragma unroll
            for (int j = 0; j < ND; j++)
                part = __builtin_amdgcn_sad_u8(c[k][j], v[k][j], part);
        } else {
#pragma unroll
            for (int j = 0; j < ND; j += 2)
                part += mes_satd_row(c[k][j], c[k][j + 1], v[k][j], v[k][j + 1], lane);
        }
    }
    return mes_sum8(part);
}

/* The bilateral cost's sum (me_search_bilat_rules.h: the filter's get_sbad_ob) of the lane's candidate, summed over its eight lanes:
 * |A - B| over the two windows of 2 MB x 2 MB samples whose top-left samples `at` names.  Lane l & 7 takes rows l & 7, + 8, ... of the
 * windows (4 at MB 16, 2 at MB 8), each 2 MB bytes of A and of B at their byte-exact addresses, loaded as mes_cost() loads; a row's
 * dwords go through v_sad_u8 before the next row's are needed, so only the rows in flight hold registers.  valid false: no load. */
template <int MB>
__device__ __forceinline__ uint32_t mes_cost_bilat(const uint8_t *a, const uint8_t *b, ptrdiff_t stride, bool valid, const MesbPlace &at, int lane)
{
    constexpr int NR = MB / 4, ND = MB / 2;
    uint32_t part = 0;
    if (valid) {
        const uint8_t *pa = a + (ptrdiff_t)(at.ay + (lane & 7)) * stride + at.ax;
        const uint8_t *pb = b + (ptrdiff_t)(at.by + (lane & 7)) * stride + at.bx;
#pragma unroll
        for (int k = 0; k < NR; k++) {
            uint32_t va[ND], vb[ND];
            __builtin_memcpy(va, pa + (ptrdiff_t)(8 * k) * stride, 2 * MB);
            __builtin_memcpy(vb, pb + (ptrdiff_t)(8 * k) * stride, 2 * MB);
#pragma unroll
            for (int j = 0; j < ND; j++)
                part = __builtin_amdgcn_sad_u8(va[j], vb[j], part);
        }
    }
    return mes_sum8(part);
}

/* the lane's rows of the current block at (x_mb, y_mb) of the frame `cf`: what mes_cost() takes as c */
template <int MB>
__device__ __forceinline__ void mes_load_cur(uint32_t (&c)[MB / 8][MB / 4], const uint8_t *cf, ptrdiff_t stride, int x_mb, int y_mb, int lane)
{
    const uint8_t *p = cf + (ptrdiff_t)(y_mb + (lane & 7)) * stride + x_mb;
#pragma unroll
    for (int k = 0; k < MB / 8; k++)
        __builtin_memcpy(c[k], p + (ptrdiff_t)(8 * k) * stride, MB);
}

/* ---- a block's cost as the predictive kernels (me_search_pred.hip, me_search_seq.hip) take it: a policy per (MB, KIND) --------------
 * load(): what the block needs before its first cost, issued with the block's other loads; set_window(): the block's window.  sum(): the part of cost(x, y) that needs
 * nothing of the row above, over the candidate's eight lanes.  penalty(): the part that needs the block's median predictor (set_pred),
 * added by the kernel once the row above has arrived; zero for the two block metrics, whose cost is sum() alone. */
template <int MB, int KIND>
struct MesCostPolicy {
    uint32_t c[MB / 8][MB / 4];
    const uint8_t *rf;
    ptrdiff_t stride;
    __device__ __forceinline__ void load(const uint8_t *cf, const uint8_t *ref, ptrdiff_t st, int x_mb, int y_mb, int lane)
    {
        rf = ref;
        stride = st;
        uint32_t t[MB / 8][MB / 4];
        mes_load_cur<MB>(t, cf, st, x_mb, y_mb, lane);
#pragma unroll
        for (int k = 0; k < MB / 8; k++)
#pragma unroll
            for (int j = 0; j < MB / 4; j++)
                c[k][j] = t[k][j];
    }
    __device__ __forceinline__ void set_window(const MesWindow &) {}
    __device__ __forceinline__ void set_pred(int, int) {}
    __device__ __forceinline__ uint32_t sum(bool valid, int x, int y, int lane) const { return mes_cost<MB, KIND>(c, rf, stride, valid, x, y, lane); }
    __device__ __forceinline__ uint32_t penalty(int, int) const { return 0; }
};

template <int MB>
struct MesCostPolicy<MB, MES_COST_BILAT> {
    const uint8_t *a, *b;
    ptrdiff_t stride;
    int x_mb, y_mb, pred_x, pred_y;
    MesWindow w;
    __device__ __forceinline__ void load(const uint8_t *cf, const uint8_t *ref, ptrdiff_t st, int x, int y, int)
    {
        a = cf;
        b = ref;
        stride = st;
        x_mb = x;
        y_mb = y;
    }
    /* the block's window: the placement clamps against it */
    __device__ __forceinline__ void set_window(const MesWindow &win) { w = win; }
    /* the block's median predictor */
    __device__ __forceinline__ void set_pred(int px, int py)
    {
        pred_x = px;
        pred_y = py;
    }
    __device__ __forceinline__ uint32_t sum(bool valid, int x, int y, int lane) const
    {
        return mes_cost_bilat<MB>(a, b, stride, valid, mesb_place(w, x_mb, y_mb, MB, x, y), lane);
    }
    __device__ __forceinline__ uint32_t penalty(int x, int y) const { return mesb_penalty(x, y, x_mb, y_mb, pred_x, pred_y); }
};

/* the minimum of a key that is uniform over each candidate's eight lanes, in scalar registers: one DPP row rotate, four v_readlane */
__device__ __forceinline__ uint32_t mes_wave_min(uint32_t key)
{
    key = min(key, (uint32_t)mes_dpp<MES_DPP_ROR8>((int)key));
    const uint32_t k0 = (uint32_t)__builtin_amdgcn_readlane((int)key, 0), k1 = (uint32_t)__builtin_amdgcn_readlane((int)key, 16);
    const uint32_t k2 = (uint32_t)__builtin_amdgcn_readlane((int)key, 32), k3 = (uint32_t)__builtin_amdgcn_readlane((int)key, 48);
    return min(min(k0, k1), min(k2, k3));
}

/* the launchers' choice of an instantiation: launch(mb, kind) with std::integral_constants of mb_size (16, else 8) and cost_kind */
template <class Launch>
static inline void mes_dispatch(int mb_size, int cost_kind, Launch launch)
{
    using Sad = std::integral_constant<int, FFHIP_ME_SAD>;
    using Satd = std::integral_constant<int, FFHIP_ME_SATD>;
    using Mb16 = std::integral_constant<int, 16>;
    using Mb8 = std::integral_constant<int, 8>;
    if (cost_kind == FFHIP_ME_SAD) {
        if (mb_size == 16) launch(Mb16(), Sad()); else launch(Mb8(), Sad());
    } else {
        if (mb_size == 16) launch(Mb16(), Satd()); else launch(Mb8(), Satd());
    }
}

/* the same for the predictive kernels, which have the bilateral cost as a third kind */
template <class Launch>
static inline void mes_dispatch_pred(int mb_size, int cost_kind, Launch launch)
{
    using Bilat = std::integral_constant<int, MES_COST_BILAT>;
    if (cost_kind != MES_COST_BILAT)
        mes_dispatch(mb_size, cost_kind, launch);
    else if (mb_size == 16)
        launch(std::integral_constant<int, 16>(), Bilat());
    else
        launch(std::integral_constant<int, 8>(), Bilat());
}

#endif
