/*
 * vp9_itxfm_tile.h — one VP9 inverse transform added to an LDS tile of 16-bit samples by one wave: itxfm_add[tx][txtp]
 * (libavcodec/vp9dsp_template.c) through the butterfly network of vp9_itxfm.hip (vp9_itxfm_net.inc; 32-bit arithmetic at 8 bits,
 * 64-bit above), the dc-only shortcut of DCT_DCT included.  Shared by the whole-frame faces: k_vp9_inter_frame (vp9_inter_frame.hip)
 * and k_vp9_intra_frame (vp9_intra_frame.hip).
 */
#ifndef FFHIP_VP9_ITXFM_TILE_H
#define FFHIP_VP9_ITXFM_TILE_H

#include <type_traits>

#include "common.h"

namespace {
namespace vq32 {
#define VP_ST int
#define VP_UT uint32_t
#include "vp9_itxfm_net.inc"
#undef VP_ST
#undef VP_UT
} // namespace vq32
namespace vq64 {
#define VP_ST long long
#define VP_UT unsigned long long
#include "vp9_itxfm_net.inc"
#undef VP_ST
#undef VP_UT
} // namespace vq64

/* one TU of N = 4 << LOG2-2 samples (WHT: the lossless 4x4) added to the tile at (lx, ly) (row pitch PITCH samples), clipped to
 * 0 .. maxv; MASKED: only to the samples whose bit is set in cov[row] (bit = column).  Lanes 0 .. N - 1 take a column each.  The order of the batch kernel (vp9_itxfm.hip): column i through the first pass into `mine` (wave-private
 * LDS, as the reference's dctcoef tmp[]), row i of that through the second; its outputs are picture column i. */
template <int LOG2, bool WHT, bool HBD, int PITCH, bool MASKED>
__device__ __forceinline__ void vif_tu(uint16_t *tile, const unsigned long long *cov, void *mine_, const void *coeffs_, int txtp, bool dc,
                                       int lx, int ly, int maxv, int lane)
{
    using COEF = typename std::conditional<HBD, int32_t, int16_t>::type;
    using ST = typename std::conditional<HBD, long long, int>::type;
    using UT = typename std::conditional<HBD, unsigned long long, uint32_t>::type;
    constexpr int N = 1 << LOG2, BITS = WHT ? 0 : LOG2 == 2 ? 4 : LOG2 == 3 ? 5 : 6;
    const COEF *coeffs = static_cast<const COEF *>(coeffs_);
    COEF *mine = static_cast<COEF *>(mine_);
    const int i = lane;
    const bool adst1 = !WHT && LOG2 < 5 && (txtp == 1 || txtp == 3), adst2 = !WHT && LOG2 < 5 && (txtp == 2 || txtp == 3);
    const bool dc_only = !WHT && dc && !adst1 && !adst2;
    auto r14 = [](UT x) { return (ST)(x + ((UT)1 << 13)) >> 14; };
    ST x[N], o[N];
    auto run = [&](bool adst, bool first) {
        if constexpr (HBD) {
            if constexpr (WHT) vq64::vp_iwht(x, o, first);
            else if (adst) vq64::vp_iadst(x, o);
            else vq64::vp_idct<N>(x, o);
        } else {
            if constexpr (WHT) vq32::vp_iwht(x, o, first);
            else if (adst) vq32::vp_iadst(x, o);
            else vq32::vp_idct<N>(x, o);
        }
    };
    if (dc_only) {
        const int dcv = (int)r14((UT)r14((UT)(ST)coeffs[0] * 11585u) * 11585u);
#pragma unroll
        for (int k = 0; k < N; k++)
            o[k] = (COEF)dcv;
    } else {
        if (i < N) {
#pragma unroll
            for (int k = 0; k < N; k++)
                x[k] = coeffs[k * N + i];
            run(adst1, true);
#pragma unroll
            for (int k = 0; k < N; k++)
                mine[k * N + i] = (COEF)o[k];
        }
        ffhip_wave_sync();
        if (i < N) {
#pragma unroll
            for (int k = 0; k < N; k++)
                x[k] = mine[i * N + k];
            run(adst2, false);
        }
        ffhip_wave_sync(); /* `mine` is reused by the wave's next TU */
    }
    if (i < N) {
        const int xx = lx + i;
#pragma unroll
        for (int k = 0; k < N; k++) {
            const int r = (int)(COEF)o[k];
            const int z = BITS ? (int)((uint32_t)r + (1u << (BITS ? BITS - 1 : 0))) >> BITS : r;
            if (!MASKED || (cov[ly + k] >> xx & 1)) {
                uint16_t &d = tile[(ly + k) * PITCH + xx];
                d = (uint16_t)min(max((int)d + z, 0), maxv);
            }
        }
    }
}
} // namespace

#endif
