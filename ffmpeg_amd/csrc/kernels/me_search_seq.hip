/*
 * me_search_seq.hip — EPZS and UMH of whole sequences in one launch: ffhip_me_search_pred_sequence_dev().
 *
 * k_me_search_pred (me_search_pred.hip) searches the independent pairs of a call; pair k of a sequence, though, reads the vector fields
 * of pairs k - 1 and k - 2 (EPZS's collocated vector, accelerator and prev1's four neighbours), so a caller of that face pays one
 * launch, and the whole chain of about b_w + 2 * b_h dependent blocks, per picture.  This kernel is the same skeleton — the rules of
 * kernels/me_search_pred_rules.h, the costs of kernels/me_search_cost.h, one wave per block row, the hand-off of row_handoff.h — with a
 * second dependency, so that a sequence is a wavefront over (pair, row):
 *   - a unit is one block row of one pair of one sequence, one wave per unit, claimed with ffhip_row_ticket().  Tickets number the
 *     pairs outermost, then the rows, the sequences interleaved innermost: unit (k, r) awaits (k, r - 1) and (k - 1, r + 1) — (k - 1, r)
 *     on the last row — and both hold smaller tickets, so the awaited wave runs; the grid is min(units, resident capacity).
 *   - one counter per unit (plus the ticket) in a progress-pool slot.  Block (bx, r) of pair k reads of pair k - 1 the collocated block
 *     and its left, top, right and bottom neighbours (mesp_fetch_prev): before block bx the wave waits until row r + 1 of pair k - 1
 *     has published bx + 1 — that block needed (bx + 1, r) of its own pair — or, on the last row, until row r has published
 *     min(bx + 2, b_w).  So the last row of a pair publishes too.  This wait stands before the early predictor pass, which evaluates
 *     prev1's vectors; the wait on the row above stays behind it.  Pair k - 2's collocated block was read by pair k - 1 long before.
 *   - a field written in this launch (prev1 of the launch's second pair on, prev2 of its third on) is read with ffhip_row_ld, every
 *     vector is stored with ffhip_row_st before the publish; init1 / init2 and the fields of an earlier launch are read plainly.  Which
 *     it is is decided per unit in scalar code.
 * UMH reads no prev field: its pairs are independent and run unchained in the same launches.
 * The cost is k_me_search_pred's policy; with KIND MES_COST_BILAT and direction 1 this is ffhip_me_search_bilat_sequence_dev().
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

/* Waves per CU the grid counts on.  Every instantiation keeps 20 or more resident (5 per SIMD for <16, SATD>, 7 for the others).  A pair
 * runs three block steps behind the one before it, so far more units are ready than k_me_search_pred's 8 per CU hold: 16 measured 24 to
 * 28 % below 8 per pair at 61 pictures, 24 another 4 to 6 % (docs/EXPERIMENTS.md).  Not a matter of correctness: a wave that holds a
 * ticket runs, and only smaller tickets are awaited.  FFHIP_ME_SEQ_PER_CU (measurement build) sets it. */
#define MESQ_PER_CU 16

namespace {
/* block n's relative vector of a field of absolute positions, block (bx, by) of its picture.  NULL: zero vectors; live: a wave of
 * this launch wrote it (the wait before made it visible), otherwise nobody writes it in the launch */
__device__ __forceinline__ MespVec mesq_field_rel(const int16_t *field, bool live, size_t n, int bx, int by, int log2mb)
{
    MespVec v;
    v.x = v.y = 0;
    if (!field)
        return v;
    if (live) {
        const uint32_t d = (uint32_t)__builtin_amdgcn_readfirstlane((int)ffhip_row_ld<uint32_t>(reinterpret_cast<const uint8_t *>(field + 2 * n)));
        return mesp_rel((int16_t)(d & 0xFFFFu), (int16_t)(d >> 16), bx, by, log2mb);
    }
    v = mesp_rel(field[2 * n], field[2 * n + 1], bx, by, log2mb);
    v.x = __builtin_amdgcn_readfirstlane(v.x);
    v.y = __builtin_amdgcn_readfirstlane(v.y);
    return v;
}
} // namespace

/* pairs k0 .. k0 + nk - 1 of the sequences s0 .. s0 + ns - 1 of a call over nseq sequences; `frames`, `init1`, `init2`, `mv_out` and
 * `cost_out` are the call's */
template <int MB, int KIND, bool EARLY = true>
__global__ __launch_bounds__(64) void k_me_search_seq(int method, const uint8_t *frames, int width, int height, ptrdiff_t stride, size_t frame_pitch,
                                                      size_t seq_pitch, int direction, int R, int k0, int nk, int s0, int ns, int nseq,
                                                      const int16_t *init1, const int16_t *init2, int16_t *mv_out, uint32_t *cost_out,
                                                      int *progress_all, int *fail)
{
    constexpr int LOG2 = MB == 16 ? 4 : 3;
    const int bw = width >> LOG2, bh = height >> LOG2;
    const size_t per = (size_t)bw * (size_t)bh;                          /* blocks of a field */
    const int lane = (int)threadIdx.x, cand = lane >> 3;
    const int step = bh * ns, units = nk * step;                         /* the units of one pair of every sequence, of the launch */
    int *const ticket = progress_all + units;
    const bool epzs = method == FFHIP_ME_METHOD_EPZS;
    const MespVec zero = { 0, 0 };

    for (;;) {
        const int t = __builtin_amdgcn_readfirstlane(ffhip_row_ticket(ticket, lane));
        if (t >= units)
            return;
        const int kl = t / step, rest = t - kl * step, row = rest / ns, sl = rest - row * ns;
        const int k = k0 + kl, s = s0 + sl;
        const uint8_t *lo = frames + (size_t)s * seq_pitch + (size_t)k * frame_pitch;      /* pictures k and k + 1 */
        const uint8_t *cf = direction ? lo : lo + frame_pitch, *rf = direction ? lo + frame_pitch : lo;
        const size_t fb = ((size_t)k * (size_t)nseq + (size_t)s) * per, back = (size_t)nseq * per;    /* the field's first block; one step */
        int16_t *const mv = mv_out + 2 * fb;
        uint32_t *const cost_row = cost_out + fb;
        const int16_t *const i1 = init1 ? init1 + 2 * per * (size_t)s : nullptr, *const i2 = init2 ? init2 + 2 * per * (size_t)s : nullptr;
        const int16_t *const p1 = k >= 1 ? mv - 2 * back : i1, *const p2 = k >= 2 ? mv - 4 * back : k == 1 ? i1 : i2;
        const bool live1 = kl >= 1, live2 = kl >= 2, chained = epzs && live1;
        const bool last = row + 1 == bh;
        int *const progress = progress_all + (kl * ns + sl) * bh + row;    /* [0]: this row's counter, [-1]: the row above's */
        const int *const before = chained ? progress - step + (last ? 0 : 1) : progress;   /* of pair k - 1: the row below's, on the last row this row's */
        const bool publish = !last || (epzs && kl + 1 < nk);
        const int y_mb = row << LOG2;
        const size_t rb = (size_t)row * (size_t)bw;                        /* the row's first block of the field */
        int known = 0, known_before = 0;
        MespVec left = zero;

        for (int bx = 0; bx < bw; bx++) {
            const int x_mb = bx << LOG2;
            const size_t b = rb + (size_t)bx;
            const MespNeigh N = mesp_neighbours(method, bx, row, bw, bh);
            MesCostPolicy<MB, KIND> cost;
            cost.load(cf, rf, stride, x_mb, y_mb, lane);
            /* ---- pair k - 1 has searched what this block reads of it ---- */
            if (chained) {
                const int want = last ? min(bx + 2, bw) : bx + 1;
                if (!ffhip_row_wait(before, want, known_before, fail, lane))
                    return;
            }
            MespNear v = {};
            v.left = left;
            mesp_fetch_prev(v, N, [&](int which, int dbx, int dby) {
                return mesq_field_rel(which == 1 ? p1 : p2, which == 1 ? live1 : live2, b + (ptrdiff_t)dby * bw + dbx, bx + dbx, row + dby, LOG2);
            });
            const MesWindow w = mes_window(x_mb, y_mb, R, bw, bh, LOG2);
            cost.set_window(w);
            MespState st = mesp_start(method, x_mb, y_mb, R);
            uint32_t key_early = MES_NO_KEY;
            int x_early = 0, y_early = 0;                     /* the early candidate of the lane's group */
            if (epzs && EARLY) {
                /* list positions zero, left, collocated, accelerator, prev1's left, top, right, bottom: one per candidate group */
                const int pos = (int)(0xA9876521u >> (4 * cand)) & 15;
                const MespPred P = mesp_predictors(N, v);
                int x, y;
                const bool valid = mesp_candidate(st, w, P, pos, x, y);
                const uint32_t c = cost.sum(valid, x, y, lane);
                key_early = valid ? mesp_list_key(c, pos) : MES_NO_KEY;
                x_early = x;
                y_early = y;
            }
            /* ---- the row above has published min(bx + 2, b_w) blocks: its vectors ---- */
            if (mesp_has(N, MESP_TOP)) {
                const int want = min(bx + 2, bw);
                if (!ffhip_row_wait(&progress[-1], want, known, fail, lane))
                    return;
                mesp_fetch_above(v, N, [&](int dbx) { return mesq_field_rel(mv, true, b - (size_t)bw + dbx, bx + dbx, row - 1, LOG2); });
            }
            const MespPred P = mesp_predictors(N, v);
            cost.set_pred(P.median.x, P.median.y);
            if (epzs && EARLY) {
                /* the median, top, top-right: the rest of the list */
                const int pos = cand == 0 ? MESP_MEDIAN : cand == 1 ? MESP_TOP : cand == 2 ? MESP_DIAG : -1;
                int x, y;
                const bool valid = mesp_candidate(st, w, P, pos, x, y);
                const uint32_t c = cost.sum(valid, x, y, lane) + cost.penalty(x, y);
                const uint32_t key = valid ? mesp_list_key(c, pos) : MES_NO_KEY;
                /* the early pass's sums take their penalty now that the median is known */
                key_early = mesp_list_key_add(key_early, cost.penalty(x_early, y_early));
                mesp_advance_list(st, w, P, mes_wave_min(min(key, key_early)));
            }
            /* EARLY false (a measured variant): the whole list in order behind the wait, two steps of mesp_run() below */
            mesp_run(st, w, P, [&](const MespState &st) {
                int x, y;
                const bool valid = mesp_candidate(st, w, P, st.pos + cand, x, y);
                const uint32_t c = cost.sum(valid, x, y, lane) + cost.penalty(x, y);
                return mes_wave_min(valid ? mes_key(c, cand) : MES_NO_KEY);
            });
            /* ---- the block's vector: to the row below, to the next pair, and to the next block of this row ---- */
            if (lane == 0) {
                ffhip_row_st<uint32_t>(reinterpret_cast<uint8_t *>(mv + 2 * b), (uint32_t)(uint16_t)st.mvx | (uint32_t)(uint16_t)st.mvy << 16);
                cost_row[b] = st.cost_min;
            }
            left = mesp_rel(st.mvx, st.mvy, bx, row, LOG2);
            if (publish)
                ffhip_row_publish(&progress[0], bx + 1, lane);
        }
    }
}

int ffhip_launch_me_search_seq(int method, const uint8_t *frames, int width, int height, ptrdiff_t stride, size_t frame_pitch, int nframes,
                               size_t seq_pitch, int nseq, int direction, int mb_size, int R, int cost_kind, const int16_t *init1,
                               const int16_t *init2, int16_t *mv_out, uint32_t *cost_out, hipStream_t stream)
{
    const int lg = mb_size == 16 ? 4 : 3, bw = width >> lg, bh = height >> lg, np = nframes - 1;
    if (bw <= 0 || bh <= 0 || np <= 0 || nseq <= 0)
        return 0;
    /* a launch's counters (one per block row, pair and sequence) and its ticket fit one progress slot: a larger call is split at pair
     * boundaries, all sequences together, and by sequences as well when one step alone does not fit.  Stream order carries the
     * dependency between the launches; the kernel reads the fields of an earlier launch plainly */
    const int room = FFHIP_PROGRESS_SLOT_INTS - 1;
    const bool bilat = cost_kind == MES_COST_BILAT;
    const char *const who = bilat ? "ffhip_me_search_bilat_sequence_dev" : "ffhip_me_search_pred_sequence_dev";
    const char *const what = bilat ? "ffhip_me_search_bilat_sequence_dev: kernel launch" : "ffhip_me_search_pred_sequence_dev: kernel launch";
    if (bh > room) {
        ffhip_set_error("%s: %d block rows exceed a progress-pool slot", who, bh);
        return FFHIP_EINVAL;
    }
    const int seqs = nseq < room / bh ? nseq : room / bh;
    const int pairs = seqs == nseq ? room / (bh * nseq) : 1;
    /* FFHIP_ME_PRED_WGS (measurement build) fixes the number of workgroups, so that a small sequence takes several ticket rounds */
    const int cap = knob_int("FFHIP_ME_PRED_WGS", ffhip_cu_count() * knob_int("FFHIP_ME_SEQ_PER_CU", MESQ_PER_CU));
    for (int k0 = 0; k0 < np; k0 += pairs)
        for (int s0 = 0; s0 < nseq; s0 += seqs) {
            const int nk = np - k0 < pairs ? np - k0 : pairs, ns = nseq - s0 < seqs ? nseq - s0 : seqs, units = nk * ns * bh;
            const int r = ffhip_progress_launch(units + 1, stream, what, [&](const FFHipProgressSlot &ps) {
                const int grid = units < cap ? units : cap;
#ifdef FFHIP_MEASURE
                /* FFHIP_ME_BILAT_NO_EARLY (measurement build): the bilateral instances without the early predictor pass (docs/EXPERIMENTS.md) */
                if (bilat && knob_int("FFHIP_ME_BILAT_NO_EARLY", 0)) {
                    if (mb_size == 16)
                        hipLaunchKernelGGL((k_me_search_seq<16, MES_COST_BILAT, false>), dim3((unsigned)grid), dim3(64), 0, stream, method, frames, width,
                                           height, stride, frame_pitch, seq_pitch, direction, R, k0, nk, s0, ns, nseq, init1, init2, mv_out, cost_out,
                                           ps.prog, ps.fail);
                    else
                        hipLaunchKernelGGL((k_me_search_seq<8, MES_COST_BILAT, false>), dim3((unsigned)grid), dim3(64), 0, stream, method, frames, width,
                                           height, stride, frame_pitch, seq_pitch, direction, R, k0, nk, s0, ns, nseq, init1, init2, mv_out, cost_out,
                                           ps.prog, ps.fail);
                    return hipGetLastError();
                }
#endif
                mes_dispatch_pred(mb_size, cost_kind, [&](auto mb, auto kind) {
                    hipLaunchKernelGGL((k_me_search_seq<decltype(mb)::value, decltype(kind)::value>), dim3((unsigned)grid), dim3(64), 0, stream, method,
                                       frames, width, height, stride, frame_pitch, seq_pitch, direction, R, k0, nk, s0, ns, nseq, init1, init2, mv_out,
                                       cost_out, ps.prog, ps.fail);
                });
                return hipGetLastError();
            });
            if (r < 0)
                return r;
        }
    return 0;
}
