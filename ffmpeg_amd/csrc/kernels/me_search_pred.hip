/*
 * me_search_pred.hip — the filter's two predictive motion searches (EPZS, UMH) of whole frame pairs in one launch.
 *
 * The rules — predictor list, phases, the candidates of a step and the state transition — are kernels/me_search_pred_rules.h, the same
 * code ffhip_me_search_pred_frames_host() runs on the CPU; a cost is computed as in me_search.hip (kernels/me_search_cost.h: eight lanes
 * per candidate, the current block in registers, DPP sums, no LDS).  What this file owns is the order between blocks: a block takes the
 * vectors of its left, top and top-right (UMH, last column: top-left) neighbours of the SAME pair, so
 *   - one wave per block row of a pair, claimed with ffhip_row_ticket(); tickets number the rows outermost and the pairs interleaved
 *     (as k_vp8_lf_frame), so the row a wave waits for holds a smaller ticket and belongs to a wave that runs: the grid is
 *     min(units, resident capacity) and a small grid simply takes more rounds;
 *   - one counter per row and pair (plus the ticket) in a progress-pool slot.  The wave walks its row left to right; before block bx it
 *     waits until the row above has published min(bx + 2, b_w); the left vector stays in the wave's scalar state, the vectors of the row
 *     above are read from mv_out as one dword each with ffhip_row_ld, the block's own is stored with ffhip_row_st and then published
 *     (row_handoff.h).  cost_out and the prev fields use plain accesses: nobody else touches them in the launch.
 *   - the critical path of a picture is about b_w + 2 * b_h blocks, each the whole loop body of a wave, so a block's chain of dependent
 *     memory round trips is what counts (fetching the current block and the prev vectors one block ahead was measured and did not
 *     pay: docs/EXPERIMENTS.md).  EPZS: the costs of (0,0), the left vector, the collocated vector, the accelerator and prev1's four
 *     neighbours — eight candidates, one pass — are evaluated BEFORE the wait, with the current block's loads; the median, top and
 *     top-right follow the wait in a second pass, and the ordered minimum over both carries the list position (the rules header's
 *     mesp_advance_list).  Running the list in order behind the wait, two steps, was measured 14 to 19 % slower and taken out.
 *   - the cost is a policy (MesCostPolicy<MB, KIND>, me_search_cost.h): the two block metrics, and KIND MES_COST_BILAT, the bilateral
 *     cost of ffhip_me_search_bilat_batch_dev() (cur = picture A, ref = picture B).  Its penalty needs the block's median predictor,
 *     hence the row above: the early pass computes its candidates' sums before the wait and their penalties join the keys after it.
 * A lost hand-off sets the slot's fail word and the kernel leaves (ffhip_progress_check reports it).  No LDS, no scratch; every loop is
 * bounded by the rules header's step bound and the hand-off's spin limit.
 */
#include <stdlib.h>

#include "common.h"
#include "me_kernels.h"
#include "me_search_cost.h"
#include "me_search_pred_rules.h"
#include "progress_pool.h"
#include "row_handoff.h"

#define MESP_PER_CU 8   /* resident waves per CU the grid counts on */

namespace {
/* block (bx, by)'s relative vector of a prev field (NULL: zero vectors); nobody writes the field in the launch */
__device__ __forceinline__ MespVec mesp_prev_rel(const int16_t *field, size_t b, int bx, int by, int log2mb)
{
    MespVec v;
    v.x = v.y = 0;
    if (field)
        v = mesp_rel(field[2 * b], field[2 * b + 1], bx, by, log2mb);
    v.x = __builtin_amdgcn_readfirstlane(v.x);
    v.y = __builtin_amdgcn_readfirstlane(v.y);
    return v;
}

/* the same of mv_out, which the row above wrote in this launch */
__device__ __forceinline__ MespVec mesp_row_rel(const int16_t *mv_out, size_t b, int bx, int by, int log2mb)
{
    const uint32_t d = (uint32_t)__builtin_amdgcn_readfirstlane((int)ffhip_row_ld<uint32_t>(reinterpret_cast<const uint8_t *>(mv_out + 2 * b)));
    return mesp_rel((int16_t)(d & 0xFFFFu), (int16_t)(d >> 16), bx, by, log2mb);
}
} // namespace

template <int MB, int KIND, bool EARLY = true>
__global__ __launch_bounds__(64) void k_me_search_pred(int method, const uint8_t *cur, const uint8_t *ref, int width, int height, ptrdiff_t stride,
                                                       size_t frame_pitch, int npairs, int R, const int16_t *prev1, const int16_t *prev2,
                                                       int16_t *mv_out, uint32_t *cost_out, int *progress_all, int *fail)
{
    constexpr int LOG2 = MB == 16 ? 4 : 3;
    const int bw = width >> LOG2, bh = height >> LOG2;
    const size_t per = (size_t)bw * (size_t)bh;                          /* blocks of a frame */
    const int lane = (int)threadIdx.x, cand = lane >> 3;
    const int units = npairs * bh;
    int *const ticket = progress_all + units;
    const bool epzs = method == FFHIP_ME_METHOD_EPZS;
    const MespVec zero = { 0, 0 };

    for (;;) {
        const int t = __builtin_amdgcn_readfirstlane(ffhip_row_ticket(ticket, lane));
        if (t >= units)
            return;
        const int row = t / npairs, f = t - row * npairs;
        const uint8_t *cf = cur + (size_t)f * frame_pitch, *rf = ref + (size_t)f * frame_pitch;
        const size_t fb = (size_t)f * per, rb = fb + (size_t)row * (size_t)bw;     /* the pair's, the row's first block */
        int *const progress = progress_all + f * bh + row;                         /* [0]: this row's counter, [-1]: the row above's */
        const bool publish = row + 1 < bh;
        const int y_mb = row << LOG2;
        int known = 0;
        MespVec left = zero;

        for (int bx = 0; bx < bw; bx++) {
            const int x_mb = bx << LOG2;
            const size_t b = rb + (size_t)bx;
            const MespNeigh N = mesp_neighbours(method, bx, row, bw, bh);
            /* ---- what needs nothing of the row above: the current block, the prev fields ---- */
            MesCostPolicy<MB, KIND> cost;
            cost.load(cf, rf, stride, x_mb, y_mb, lane);
            MespNear v = {};
            v.left = left;
            mesp_fetch_prev(v, N, [&](int which, int dbx, int dby) {
                return mesp_prev_rel(which == 1 ? prev1 : prev2, b + (ptrdiff_t)dby * bw + dbx, bx + dbx, row + dby, LOG2);
            });
            const MesWindow w = mes_window(x_mb, y_mb, R, bw, bh, LOG2);
            cost.set_window(w);
            MespState s = mesp_start(method, x_mb, y_mb, R);
            uint32_t key_early = MES_NO_KEY;
            int x_early = 0, y_early = 0;                     /* the early candidate of the lane's group */
            if (epzs && EARLY) {
                /* list positions zero, left, collocated, accelerator, prev1's left, top, right, bottom: one per candidate group */
                const int k = (int)(0xA9876521u >> (4 * cand)) & 15;
                const MespPred P = mesp_predictors(N, v);
                int x, y;
                const bool valid = mesp_candidate(s, w, P, k, x, y);
                const uint32_t c = cost.sum(valid, x, y, lane);
                key_early = valid ? mesp_list_key(c, k) : MES_NO_KEY;
                x_early = x;
                y_early = y;
            }
            /* ---- the row above has published min(bx + 2, b_w) blocks: its vectors ---- */
            if (mesp_has(N, MESP_TOP)) {
                const int want = min(bx + 2, bw);
                if (!ffhip_row_wait(&progress[-1], want, known, fail, lane))
                    return;
                mesp_fetch_above(v, N, [&](int dbx) { return mesp_row_rel(mv_out, b - (size_t)bw + dbx, bx + dbx, row - 1, LOG2); });
            }
            const MespPred P = mesp_predictors(N, v);
            cost.set_pred(P.median.x, P.median.y);
            if (epzs && EARLY) {
                /* the median, top, top-right: the rest of the list */
                const int k = cand == 0 ? MESP_MEDIAN : cand == 1 ? MESP_TOP : cand == 2 ? MESP_DIAG : -1;
                int x, y;
                const bool valid = mesp_candidate(s, w, P, k, x, y);
                const uint32_t c = cost.sum(valid, x, y, lane) + cost.penalty(x, y);
                const uint32_t key = valid ? mesp_list_key(c, k) : MES_NO_KEY;
                /* the early pass's sums take their penalty now that the median is known */
                key_early = mesp_list_key_add(key_early, cost.penalty(x_early, y_early));
                mesp_advance_list(s, w, P, mes_wave_min(min(key, key_early)));
            }
            /* EARLY false (a measured variant): the whole list in order behind the wait, two steps of mesp_run() below */
            mesp_run(s, w, P, [&](const MespState &s) {
                int x, y;
                const bool valid = mesp_candidate(s, w, P, s.pos + cand, x, y);
                const uint32_t c = cost.sum(valid, x, y, lane) + cost.penalty(x, y);
                return mes_wave_min(valid ? mes_key(c, cand) : MES_NO_KEY);
            });
            /* ---- the block's vector: to the row below, and to the next block of this row ---- */
            if (lane == 0) {
                ffhip_row_st<uint32_t>(reinterpret_cast<uint8_t *>(mv_out + 2 * b), (uint32_t)(uint16_t)s.mvx | (uint32_t)(uint16_t)s.mvy << 16);
                cost_out[b] = s.cost_min;
            }
            left = mesp_rel(s.mvx, s.mvy, bx, row, LOG2);
            if (publish)
                ffhip_row_publish(&progress[0], bx + 1, lane);
        }
    }
}

int ffhip_launch_me_search_pred(int method, const uint8_t *cur, const uint8_t *ref, int width, int height, ptrdiff_t stride, size_t frame_pitch,
                                int nframes, int mb_size, int R, int cost_kind, const int16_t *prev1, const int16_t *prev2, int16_t *mv_out,
                                uint32_t *cost_out, hipStream_t stream)
{
    const int lg = mb_size == 16 ? 4 : 3, bw = width >> lg, bh = height >> lg;
    if (bw <= 0 || bh <= 0 || nframes <= 0)
        return 0;
    /* a launch's counters (one per block row and pair) and its ticket fit one progress slot: larger calls are split by pairs */
    const int per = (FFHIP_PROGRESS_SLOT_INTS - 1) / bh;
    const bool bilat = cost_kind == MES_COST_BILAT;
    const char *const who = bilat ? "ffhip_me_search_bilat_batch_dev" : "ffhip_me_search_pred_batch_dev";
    const char *const what = bilat ? "ffhip_me_search_bilat_batch_dev: kernel launch" : "ffhip_me_search_pred_batch_dev: kernel launch";
    if (per < 1) {
        ffhip_set_error("%s: %d block rows exceed a progress-pool slot", who, bh);
        return FFHIP_EINVAL;
    }
    /* FFHIP_ME_PRED_WGS (measurement build) fixes the number of workgroups, so that a small picture takes several ticket rounds */
    const int cap = knob_int("FFHIP_ME_PRED_WGS", ffhip_cu_count() * MESP_PER_CU);
    const size_t blocks = (size_t)bw * (size_t)bh;
    for (int p0 = 0; p0 < nframes; p0 += per) {
        const int n = nframes - p0 < per ? nframes - p0 : per, units = n * bh;
        const uint8_t *c0 = cur + (size_t)p0 * frame_pitch, *r0 = ref + (size_t)p0 * frame_pitch;
        const int16_t *q1 = prev1 ? prev1 + 2 * blocks * (size_t)p0 : nullptr, *q2 = prev2 ? prev2 + 2 * blocks * (size_t)p0 : nullptr;
        int16_t *mv0 = mv_out + 2 * blocks * (size_t)p0;
        uint32_t *k0 = cost_out + blocks * (size_t)p0;
        const int r = ffhip_progress_launch(units + 1, stream, what, [&](const FFHipProgressSlot &ps) {
            const int grid = units < cap ? units : cap;
            mes_dispatch_pred(mb_size, cost_kind, [&](auto mb, auto kind) {
                hipLaunchKernelGGL((k_me_search_pred<decltype(mb)::value, decltype(kind)::value>), dim3((unsigned)grid), dim3(64), 0, stream, method,
                                   c0, r0, width, height, stride, frame_pitch, n, R, q1, q2, mv0, k0, ps.prog, ps.fail);
            });
            return hipGetLastError();
        });
        if (r < 0)
            return r;
    }
    return 0;
}
