/*
 * me_search.hip — the filter's per-block fast motion searches (TSS, TDLS, NTSS, FSS, DS, HEXBS) of whole frame pairs in one launch.
 *
 * The rules — pattern tables, window, the candidates of a step and the state transition — are kernels/me_search_rules.h, the same code
 * ffhip_me_search_frames_host() runs on the CPU; how a cost is computed is kernels/me_search_cost.h, shared with me_search_pred.hip.
 *
 * The search of one block is a short chain of dependent steps of at most 8 independent candidates, so the parallelism is candidates x
 * pixels inside a step and blocks across the grid:
 *   - one wave per block, eight lanes per candidate: lane = 8 * i + r evaluates candidate i of the step, rows r and (16x16) r + 8 of
 *     the block: one 16-byte (8x8: 8-byte) load per row at the candidate's byte-exact address in `ref`.  The current block's rows
 *     stay in registers for the whole search.  A candidate outside the window issues no load; the 4- and 6-candidate patterns leave
 *     lane groups idle (the next step depends on this one's result, so nothing can be packed in).
 *   - SAD: v_sad_u8 over the dwords.  SATD: the horizontal 8-point transform of a row's differences in the lane, the vertical one
 *     across the eight lanes of the candidate (rows r and r + 8 belong to different 8x8 blocks), then the absolute sum.
 *   - the eight partial sums of a candidate are added with DPP moves (quad_perm, quad_perm, row_half_mirror), no LDS; the Hadamard
 *     butterfly across lanes r and r ^ 4 is a ds_swizzle (the crossbar, no LDS memory).
 *   - the ordered minimum of cost << 3 | index over the in-window candidates (rules header) is one DPP row rotate, four v_readlane and
 *     scalar minima; the state (method, step, first, centre, cost_min) is wave-uniform and lives in scalar registers.
 *   - a grid-stride loop over blocks x frames: a 4K pair and a 64x48 one run the same code.
 * No LDS, no scratch; every loop is bounded by the rules header's step bound.
 */
#include <stdlib.h>

#include "common.h"
#include "me_kernels.h"
#include "me_search_cost.h"
#include "me_search_rules.h"

#define MES_WAVES 4                 /* blocks (waves) per workgroup */

template <int MB, int KIND>
__global__ __launch_bounds__(64 * MES_WAVES) void k_me_search(int method, const uint8_t *cur, const uint8_t *ref, int width, int height,
                                                              ptrdiff_t stride, size_t frame_pitch, uint32_t nblocks, int R, int16_t *mv_out,
                                                              uint32_t *cost_out)
{
    constexpr int LOG2 = MB == 16 ? 4 : 3, NR = MB / 8;
    const int bw = width >> LOG2, bh = height >> LOG2;
    const uint32_t per = (uint32_t)bw * (uint32_t)bh;                    /* blocks of a frame */
    const int lane = threadIdx.x & 63, cand = lane >> 3;
    const uint32_t wave = blockIdx.x * MES_WAVES + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t nwaves = gridDim.x * MES_WAVES;
    for (uint32_t b = wave; b < nblocks; b += nwaves) {
        const uint32_t f = b / per, rem = b - f * per;
        const int by = (int)(rem / (uint32_t)bw), bx = (int)(rem - (uint32_t)by * (uint32_t)bw);
        const int x_mb = bx << LOG2, y_mb = by << LOG2;
        const uint8_t *cf = cur + (size_t)f * frame_pitch, *rf = ref + (size_t)f * frame_pitch;
        uint32_t c[NR][MB / 4];
        mes_load_cur<MB>(c, cf, stride, x_mb, y_mb, lane);
        const MesWindow w = mes_window(x_mb, y_mb, R, bw, bh, LOG2);
        /* the start: every candidate group evaluates the centre */
        const uint32_t cost0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)mes_cost<MB, KIND>(c, rf, stride, true, x_mb, y_mb, lane));
        MesState s = mes_start(method, x_mb, y_mb, R, cost0);
        /* the text of mes_run(), not a call: through the call the compiler joins the loop's two exit tests differently and emits one
         * conditional branch more per instantiation (docs/KERNELS.md 5.7b), and a block's time here is its chain of scalar steps */
        const uint32_t bound = mes_step_bound(w);
        for (uint32_t n = 0; !s.done && n < bound; n++) {
            const MesStep st = mes_step(s);
            int x, y;
            const bool valid = mes_candidate(s, st, w, cand, x, y) && cand < st.n;
            const uint32_t cost = mes_cost<MB, KIND>(c, rf, stride, valid, x, y, lane);
            mes_advance(s, st, w, mes_wave_min(valid ? mes_key(cost, cand) : MES_NO_KEY));
        }
        if (lane == 0) {
            mv_out[2 * (size_t)b] = (int16_t)s.mvx;
            mv_out[2 * (size_t)b + 1] = (int16_t)s.mvy;
            cost_out[b] = s.cost_min;
        }
    }
}

int ffhip_launch_me_search(int method, const uint8_t *cur, const uint8_t *ref, int width, int height, ptrdiff_t stride, size_t frame_pitch,
                           int nframes, int mb_size, int R, int cost_kind, int16_t *mv_out, uint32_t *cost_out, hipStream_t stream)
{
    const int lg = mb_size == 16 ? 4 : 3;
    const int64_t nblocks = (int64_t)(width >> lg) * (height >> lg) * nframes;
    if (nblocks <= 0)
        return 0;
    /* as many workgroups as stay resident at 8 waves per SIMD; the rest of the blocks are the waves' next rounds.
     * FFHIP_ME_SEARCH_WGS (measurement build) fixes the number, so that a small picture takes several rounds */
    int64_t wgs = knob_int("FFHIP_ME_SEARCH_WGS", ffhip_cu_count() * (32 / MES_WAVES));
    if (wgs > (nblocks + MES_WAVES - 1) / MES_WAVES)
        wgs = (nblocks + MES_WAVES - 1) / MES_WAVES;
    mes_dispatch(mb_size, cost_kind, [&](auto mb, auto kind) {
        hipLaunchKernelGGL((k_me_search<decltype(mb)::value, decltype(kind)::value>), dim3((unsigned)wgs), dim3(64 * MES_WAVES), 0, stream, method,
                           cur, ref, width, height, stride, frame_pitch, (uint32_t)nblocks, R, mv_out, cost_out);
    });
    LAUNCH_CHECK();
    return 0;
}
