/*
 * me_api.hip — C-ABI entry points of the me_cmp / motion-search part of libffhip (include/ffhip.h).
 */
#include <limits.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "kernels/common.h"
#include "kernels/me_interp_rules.h"
#include "kernels/me_kernels.h"
#include "kernels/me_scene_rules.h"
#include "kernels/me_search_bilat_rules.h"
#include "kernels/me_search_pred_rules.h"
#include "kernels/me_search_rules.h"
#include "kernels/picture_check.h"

extern "C" int ffhip_me_cmp_batch_dev(int kind, int width, int h, const uint8_t *blk1, const int32_t *off1,
                                      const uint8_t *blk2, const int32_t *off2, ptrdiff_t stride, int32_t *out, int n,
                                      void *stream)
{
    if (!blk1 || !blk2 || !off1 || !off2 || !out || n < 0 || (width != 16 && width != 8) || h <= 0 ||
        kind < FFHIP_ME_SAD || kind > FFHIP_ME_NSSE)
        return FFHIP_EINVAL;
    if (kind == FFHIP_ME_SATD && h != 8 && h != 16) /* hadamard8_diff16_c handles h 8|16 only (me_cmp.c:933-950) */
        return FFHIP_EINVAL;
    if (!ffhip_have_device())
        return FFHIP_ENOSYS;
    return ffhip_launch_me_cmp(kind, width, h, blk1, off1, blk2, off2, stride, out, n, (hipStream_t)stream);
}

extern "C" int ffhip_me_esa_batch_dev(const uint8_t *cur, const uint8_t *ref, int width, int height, ptrdiff_t stride,
                                      size_t frame_pitch, int nframes, int mb_size, int search_param, int cost_kind,
                                      int16_t *mv_out, uint32_t *cost_out, void *stream)
{
    if (!cur || !ref || !mv_out || !cost_out || width <= 0 || height <= 0 || nframes < 0 || search_param < 0 ||
        (mb_size != 16 && mb_size != 8) || (cost_kind != FFHIP_ME_SAD && cost_kind != FFHIP_ME_SATD))
        return FFHIP_EINVAL;
    if (!ffhip_have_device())
        return FFHIP_ENOSYS;
    return ffhip_launch_me_esa(cur, ref, width, height, stride, frame_pitch, nframes, mb_size, search_param, cost_kind,
                               mv_out, cost_out, (hipStream_t)stream);
}

/* ---- the filter's per-block searches (kernels/me_search_rules.h) ----------------------------------------------------------------- */
/* what the per-block and the predictive faces check alike, the method apart: 0 or FFHIP_EINVAL, no text */
static int me_search_check_args(const uint8_t *cur, const uint8_t *ref, int width, int height, ptrdiff_t stride, size_t frame_pitch, int nframes,
                                int mb_size, int search_param, int cost_kind, const int16_t *mv_out, const uint32_t *cost_out)
{
    if (!cur || !ref || !mv_out || !cost_out || width < 0 || height < 0 || nframes < 0 || search_param < 0 || (mb_size != 16 && mb_size != 8) ||
        (cost_kind != FFHIP_ME_SAD && cost_kind != FFHIP_ME_SATD) || stride < width)
        return FFHIP_EINVAL;
    if (nframes > 1 && height && frame_pitch / (size_t)height < (size_t)stride)     /* frame_pitch < stride * height, without the product */
        return FFHIP_EINVAL;
    const int lg = mb_size == 16 ? 4 : 3;
    if ((int64_t)(width >> lg) * (height >> lg) * nframes > INT_MAX)
        return FFHIP_EINVAL;
    return 0;
}

/* the per-block faces: 0, FFHIP_EINVAL, or FFHIP_ENOSYS with a text for the two methods that are not functions of one block */
static int me_search_check(int method, const uint8_t *cur, const uint8_t *ref, int width, int height, ptrdiff_t stride, size_t frame_pitch,
                           int nframes, int mb_size, int search_param, int cost_kind, const int16_t *mv_out, const uint32_t *cost_out)
{
    if (method < FFHIP_ME_METHOD_ESA || method > FFHIP_ME_METHOD_UMH ||
        me_search_check_args(cur, ref, width, height, stride, frame_pitch, nframes, mb_size, search_param, cost_kind, mv_out, cost_out))
        return FFHIP_EINVAL;
    if (method >= FFHIP_ME_METHOD_EPZS) {
        ffhip_set_error("motion search method %d (%s) needs the neighbouring blocks' vectors of the current and the previous frame: "
                        "it is not a function of one block and stays on the CPU", method, method == FFHIP_ME_METHOD_EPZS ? "EPZS" : "UMH");
        return FFHIP_ENOSYS;
    }
    return 0;
}

extern "C" int ffhip_me_search_batch_dev(int method, const uint8_t *cur, const uint8_t *ref, int width, int height, ptrdiff_t stride,
                                         size_t frame_pitch, int nframes, int mb_size, int search_param, int cost_kind,
                                         int16_t *mv_out, uint32_t *cost_out, void *stream)
{
    const int r = me_search_check(method, cur, ref, width, height, stride, frame_pitch, nframes, mb_size, search_param, cost_kind, mv_out,
                                  cost_out);
    if (r)
        return r;
    if (!ffhip_have_device())
        return FFHIP_ENOSYS;
    if (method == FFHIP_ME_METHOD_ESA)
        return ffhip_launch_me_esa(cur, ref, width, height, stride, frame_pitch, nframes, mb_size, search_param, cost_kind, mv_out,
                                   cost_out, (hipStream_t)stream);
    return ffhip_launch_me_search(method, cur, ref, width, height, stride, frame_pitch, nframes, mb_size, search_param, cost_kind, mv_out,
                                  cost_out, (hipStream_t)stream);
}

/* the two metrics on the CPU: cur = blk1 (the current block), ref = blk2 */
static uint32_t host_sad(const uint8_t *a, const uint8_t *b, ptrdiff_t stride, int mb)
{
    uint32_t s = 0;
    for (int y = 0; y < mb; y++, a += stride, b += stride)
        for (int x = 0; x < mb; x++)
            s += (uint32_t)abs((int)a[x] - (int)b[x]);
    return s;
}

static uint32_t host_satd8x8(const uint8_t *a, const uint8_t *b, ptrdiff_t stride)
{
    int t[64];
    for (int y = 0; y < 8; y++)
        for (int x = 0; x < 8; x++)
            t[8 * y + x] = (int)a[y * stride + x] - (int)b[y * stride + x];
    for (int pass = 0; pass < 2; pass++) {              /* rows, then columns */
        const int st = pass ? 8 : 1, line = pass ? 1 : 8;
        for (int l = 0; l < 8; l++)
            for (int span = 1; span < 8; span <<= 1)
                for (int i = 0; i < 8; i++)
                    if (!(i & span)) {
                        int *p = t + l * line + i * st, *q = p + span * st;
                        const int u = *p, v = *q;
                        *p = u + v;
                        *q = u - v;
                    }
    }
    uint32_t s = 0;
    for (int i = 0; i < 64; i++)
        s += (uint32_t)abs(t[i]);
    return s;
}

struct HostCost {
    const uint8_t *cur_blk, *ref;   /* the current block's first sample, the reference plane */
    ptrdiff_t stride;
    int mb, kind;
    uint64_t n;
    uint32_t operator()(int x, int y)
    {
        const uint8_t *b = ref + (ptrdiff_t)y * stride + x;
        n++;
        if (kind == FFHIP_ME_SAD)
            return host_sad(cur_blk, b, stride, mb);
        uint32_t s = 0;
        for (int by = 0; by < mb; by += 8)
            for (int bx = 0; bx < mb; bx += 8)
                s += host_satd8x8(cur_blk + by * stride + bx, b + by * stride + bx, stride);
        return s;
    }
};

static thread_local uint64_t t_host_blocks, t_host_costs;

extern "C" void ffhip_me_search_host_counts(uint64_t *blocks, uint64_t *costs)
{
    if (blocks)
        *blocks = t_host_blocks;
    if (costs)
        *costs = t_host_costs;
}

struct HostBest {
    int mvx, mvy;
    uint32_t cost_min;
};

/* The driver of every host face: every block of every frame in raster order.  make_cost(f, x_mb, y_mb, w) gives the block's cost
 * (a callable cost(x, y) that counts its calls in .n); search_block(bx, by, b, w, cost) -> HostBest searches block (bx, by) of a frame,
 * the b-th of the call, in the window w with it. */
template <class MakeCost, class SearchBlock>
static void me_search_host_with(int width, int height, int nframes, int mb_size, int search_param, int16_t *mv_out, uint32_t *cost_out,
                                MakeCost make_cost, SearchBlock search_block)
{
    const int lg = mb_size == 16 ? 4 : 3, bw = width >> lg, bh = height >> lg;
    uint64_t blocks = 0, costs = 0;
    for (int f = 0; f < nframes; f++)
        for (int by = 0; by < bh; by++)
            for (int bx = 0; bx < bw; bx++) {
                const int x_mb = bx << lg, y_mb = by << lg;
                const size_t b = ((size_t)f * bh + by) * bw + bx;
                const MesWindow w = mes_window(x_mb, y_mb, search_param, bw, bh, lg);
                auto cost = make_cost(f, x_mb, y_mb, w);
                const HostBest best = search_block(bx, by, b, w, cost);
                mv_out[2 * b] = (int16_t)best.mvx;
                mv_out[2 * b + 1] = (int16_t)best.mvy;
                cost_out[b] = best.cost_min;
                blocks++;
                costs += cost.n;
            }
    t_host_blocks = blocks;
    t_host_costs = costs;
}

/* the driver with the block metrics: cost(x, y) is HostCost's */
template <class SearchBlock>
static void me_search_host(const uint8_t *cur, const uint8_t *ref, int width, int height, ptrdiff_t stride, size_t frame_pitch, int nframes,
                           int mb_size, int search_param, int cost_kind, int16_t *mv_out, uint32_t *cost_out, SearchBlock search_block)
{
    me_search_host_with(width, height, nframes, mb_size, search_param, mv_out, cost_out,
                        [&](int f, int x_mb, int y_mb, const MesWindow &) {
                            return HostCost{ cur + (size_t)f * frame_pitch + (ptrdiff_t)y_mb * stride + x_mb, ref + (size_t)f * frame_pitch, stride, mb_size,
                                             cost_kind, 0 };
                        },
                        search_block);
}

/* a step's ordered minimum on the CPU: the n candidates one by one.  candidate(i, x, y) -> bool */
template <class Cost, class Candidate>
static uint32_t host_step_key(Cost &cost, int n, Candidate candidate)
{
    uint32_t key = MES_NO_KEY;
    for (int i = 0; i < n; i++) {
        int x, y;
        if (candidate(i, x, y)) {
            const uint32_t k = mes_key(cost(x, y), i);
            key = k < key ? k : key;
        }
    }
    return key;
}

extern "C" int ffhip_me_search_frames_host(int method, const uint8_t *cur, const uint8_t *ref, int width, int height, ptrdiff_t stride,
                                           size_t frame_pitch, int nframes, int mb_size, int search_param, int cost_kind,
                                           int16_t *mv_out, uint32_t *cost_out)
{
    const int r = me_search_check(method, cur, ref, width, height, stride, frame_pitch, nframes, mb_size, search_param, cost_kind, mv_out,
                                  cost_out);
    if (r)
        return r;
    const int lg = mb_size == 16 ? 4 : 3;
    me_search_host(cur, ref, width, height, stride, frame_pitch, nframes, mb_size, search_param, cost_kind, mv_out, cost_out,
                   [&](int bx, int by, size_t, const MesWindow &w, HostCost &cost) {
                       const int x_mb = bx << lg, y_mb = by << lg;
                       if (method == FFHIP_ME_METHOD_ESA) {
                           HostBest best;
                           mes_search_esa(x_mb, y_mb, w, cost, best.mvx, best.mvy, best.cost_min);
                           return best;
                       }
                       MesState s = mes_start(method, x_mb, y_mb, search_param, cost(x_mb, y_mb));
                       mes_run(s, w, [&](const MesState &s, const MesStep &st) {
                           return host_step_key(cost, st.n, [&](int i, int &x, int &y) { return mes_candidate(s, st, w, i, x, y); });
                       });
                       return HostBest{ s.mvx, s.mvy, s.cost_min };
                   });
    return 0;
}

/* ---- the predictive searches, EPZS and UMH (kernels/me_search_pred_rules.h) ------------------------------------------------------- */
#define MESP_WHO "ffhip_me_search_pred_batch_dev / _frames_host"
/* what every predictive face checks of the method, the size of the picture and the vector field it writes */
static int me_search_pred_check_field(const char *who, int method, int width, int height, const int16_t *mv_out)
{
    if (method != FFHIP_ME_METHOD_EPZS && method != FFHIP_ME_METHOD_UMH) {
        ffhip_set_error("%s: method %d is neither EPZS (8) nor UMH (9); the per-block methods 1 to 7 are ffhip_me_search_batch_dev's", who, method);
        return FFHIP_EINVAL;
    }
    if (width > 32768 || height > 32768) {
        ffhip_set_error("%s: %d x %d: positions of a picture above 32768 do not fit the int16 vector fields", who, width, height);
        return FFHIP_EINVAL;
    }
    if ((uintptr_t)mv_out & 3) {
        ffhip_set_error("%s: mv_out is not 4-byte aligned (a block's vector travels as one dword)", who);
        return FFHIP_EINVAL;
    }
    return 0;
}

static int me_search_pred_check(const char *who, int method, const uint8_t *cur, const uint8_t *ref, int width, int height, ptrdiff_t stride, size_t frame_pitch,
                                int nframes, int mb_size, int search_param, int cost_kind, const int16_t *prev1, const int16_t *prev2,
                                const int16_t *mv_out, const uint32_t *cost_out)
{
    if (me_search_check_args(cur, ref, width, height, stride, frame_pitch, nframes, mb_size, search_param, cost_kind, mv_out, cost_out)) {
        ffhip_set_error("%s: a NULL cur, ref, mv_out or cost_out, mb_size %d (16 or 8), cost_kind %d (0 or 1), a negative width, height, "
                        "nframes or search_param, stride < width, frame_pitch < stride * height, or more than 2^31 - 1 blocks", who, mb_size, cost_kind);
        return FFHIP_EINVAL;
    }
    if (me_search_pred_check_field(who, method, width, height, mv_out))
        return FFHIP_EINVAL;
    /* mv_out is read back while it is written: it shares no byte with anything else the call reads or writes */
    const int lg = mb_size == 16 ? 4 : 3;
    const ptrdiff_t field = (ptrdiff_t)(width >> lg) * (height >> lg) * nframes * 4;
    const ptrdiff_t planes = nframes && height ? (ptrdiff_t)(nframes - 1) * (ptrdiff_t)frame_pitch + (ptrdiff_t)(height - 1) * stride + width : 0;
    FFHipSpanSet others;
    others.add(ffhip_plane_span(cur, 0, field ? planes : 0, 1));
    others.add(ffhip_plane_span(ref, 0, field ? planes : 0, 1));
    others.add(ffhip_plane_span(cost_out, 0, field, 1));
    if (prev1)
        others.add(ffhip_plane_span(prev1, 0, field, 1));
    if (prev2)
        others.add(ffhip_plane_span(prev2, 0, field, 1));
    others.seal();
    if (others.hits(ffhip_plane_span(mv_out, 0, field, 1))) {
        ffhip_set_error("%s: mv_out overlaps prev1, prev2, cur, ref or cost_out", who);
        return FFHIP_EINVAL;
    }
    return 0;
}

extern "C" int ffhip_me_search_pred_batch_dev(int method, const uint8_t *cur, const uint8_t *ref, int width, int height, ptrdiff_t stride,
                                              size_t frame_pitch, int nframes, int mb_size, int search_param, int cost_kind,
                                              const int16_t *prev1, const int16_t *prev2, int16_t *mv_out, uint32_t *cost_out, void *stream)
{
    const int r = me_search_pred_check(MESP_WHO, method, cur, ref, width, height, stride, frame_pitch, nframes, mb_size, search_param, cost_kind, prev1,
                                       prev2, mv_out, cost_out);
    if (r)
        return r;
    if (!ffhip_have_device())
        return FFHIP_ENOSYS;
    return ffhip_launch_me_search_pred(method, cur, ref, width, height, stride, frame_pitch, nframes, mb_size, search_param, cost_kind, prev1,
                                       prev2, mv_out, cost_out, (hipStream_t)stream);
}

/* one block of a predictive search on the CPU: its neighbours' vectors, the list, the run.  Raster order: the neighbours of the current
 * frame are in mv_out already.  before_run(P) sees the list before the first cost (the bilateral cost takes its median). */
template <class Cost, class BeforeRun>
static HostBest me_search_pred_block(int method, int bx, int by, size_t b, int bw, int bh, int lg, int search_param, const MesWindow &w,
                                     const int16_t *prev1, const int16_t *prev2, const int16_t *mv_out, Cost &cost, BeforeRun before_run)
{
    /* block (bx + dbx, by + dby)'s relative vector of a field of absolute positions; NULL: a field of zero vectors */
    auto rel = [&](const int16_t *field, int dbx, int dby) {
        const size_t n = b + (ptrdiff_t)dby * bw + dbx;
        const MespVec zero = { 0, 0 };
        return field ? mesp_rel(field[2 * n], field[2 * n + 1], bx + dbx, by + dby, lg) : zero;
    };
    const MespNeigh N = mesp_neighbours(method, bx, by, bw, bh);
    MespNear v = {};
    if (mesp_has(N, MESP_LEFT))
        v.left = rel(mv_out, -1, 0);
    mesp_fetch_prev(v, N, [&](int which, int dbx, int dby) { return rel(which == 1 ? prev1 : prev2, dbx, dby); });
    mesp_fetch_above(v, N, [&](int dbx) { return rel(mv_out, dbx, -1); });
    const MespPred P = mesp_predictors(N, v);
    before_run(P);
    MespState s = mesp_start(method, bx << lg, by << lg, search_param);
    mesp_run(s, w, P, [&](const MespState &s) {
        return host_step_key(cost, 8, [&](int i, int &x, int &y) { return mesp_candidate(s, w, P, s.pos + i, x, y); });
    });
    return HostBest{ s.mvx, s.mvy, s.cost_min };
}

/* the predictive searches of nframes independent pairs on the CPU, arguments checked: the body of the host faces */
static void me_search_pred_host(int method, const uint8_t *cur, const uint8_t *ref, int width, int height, ptrdiff_t stride, size_t frame_pitch,
                                int nframes, int mb_size, int search_param, int cost_kind, const int16_t *prev1, const int16_t *prev2,
                                int16_t *mv_out, uint32_t *cost_out)
{
    const int lg = mb_size == 16 ? 4 : 3, bw = width >> lg, bh = height >> lg;
    me_search_host(cur, ref, width, height, stride, frame_pitch, nframes, mb_size, search_param, cost_kind, mv_out, cost_out,
                   [&](int bx, int by, size_t b, const MesWindow &w, HostCost &cost) {
                       return me_search_pred_block(method, bx, by, b, bw, bh, lg, search_param, w, prev1, prev2, mv_out, cost, [](const MespPred &) {});
                   });
}

extern "C" int ffhip_me_search_pred_frames_host(int method, const uint8_t *cur, const uint8_t *ref, int width, int height, ptrdiff_t stride,
                                                size_t frame_pitch, int nframes, int mb_size, int search_param, int cost_kind,
                                                const int16_t *prev1, const int16_t *prev2, int16_t *mv_out, uint32_t *cost_out)
{
    const int r = me_search_pred_check(MESP_WHO, method, cur, ref, width, height, stride, frame_pitch, nframes, mb_size, search_param, cost_kind, prev1,
                                       prev2, mv_out, cost_out);
    if (r)
        return r;
    me_search_pred_host(method, cur, ref, width, height, stride, frame_pitch, nframes, mb_size, search_param, cost_kind, prev1, prev2, mv_out,
                        cost_out);
    return 0;
}

/* ---- the predictive searches of whole sequences: pair k chained to the fields of pairs k - 1 and k - 2 ----------------------------- */
#define MESQ_WHO "ffhip_me_search_pred_sequence_dev / _host"
static int me_search_seq_check(const char *who, int method, const uint8_t *frames, int width, int height, ptrdiff_t stride, size_t frame_pitch, int nframes,
                               size_t seq_pitch, int nseq, int direction, int mb_size, int search_param, int cost_kind, const int16_t *init1,
                               const int16_t *init2, const int16_t *mv_out, const uint32_t *cost_out)
{
    /* what the pair face refuses, applied to the pictures; the blocks are counted below, over all pairs and sequences */
    if (me_search_check_args(frames, frames, width, height, stride, frame_pitch, nframes < 2 ? nframes : 2, mb_size, search_param, cost_kind, mv_out,
                             cost_out)) {
        ffhip_set_error("%s: a NULL frames, mv_out or cost_out, mb_size %d (16 or 8), cost_kind %d (0 or 1), a negative width, height, "
                        "nframes or search_param, stride < width, or frame_pitch < stride * height", who, mb_size, cost_kind);
        return FFHIP_EINVAL;
    }
    if (me_search_pred_check_field(who, method, width, height, mv_out))
        return FFHIP_EINVAL;
    if (direction < 0 || direction > 1) {
        ffhip_set_error("%s: direction %d is neither 0 (cur = picture k + 1, ref = picture k) nor 1 (cur = picture k, ref = picture k + 1)", who,
                        direction);
        return FFHIP_EINVAL;
    }
    if (nseq < 0) {
        ffhip_set_error("%s: a negative nseq (%d)", who, nseq);
        return FFHIP_EINVAL;
    }
    if (nseq > 1 && nframes > 0) {
        /* a sequence's pictures end (nframes - 1) * frame_pitch + stride * height bytes behind its first */
        size_t gap, need;
        if (__builtin_mul_overflow((size_t)(nframes - 1), frame_pitch, &gap) ||
            __builtin_add_overflow(gap, (size_t)stride * (size_t)height, &need) || seq_pitch < need) {
            ffhip_set_error("%s: seq_pitch %zu < (nframes - 1) * frame_pitch + stride * height: the pictures of two sequences would share bytes", who,
                            seq_pitch);
            return FFHIP_EINVAL;
        }
    }
    const int lg = mb_size == 16 ? 4 : 3, np = nframes > 1 ? nframes - 1 : 0;
    const int64_t per = (int64_t)(width >> lg) * (height >> lg);          /* at most 2^24 */
    if (per * nseq > INT_MAX || per * nseq * np > INT_MAX) {
        ffhip_set_error("%s: %d pairs of %d sequences of %lld blocks each are more than 2^31 - 1 blocks", who, np, nseq, (long long)per);
        return FFHIP_EINVAL;
    }
    /* mv_out is read back while it is written: it shares no byte with anything else the call reads or writes */
    const ptrdiff_t step = (ptrdiff_t)per * nseq * 4, field = step * np;
    const ptrdiff_t planes = field ? (ptrdiff_t)(nseq - 1) * (ptrdiff_t)seq_pitch + (ptrdiff_t)(nframes - 1) * (ptrdiff_t)frame_pitch +
                                     (ptrdiff_t)(height - 1) * stride + width : 0;
    FFHipSpanSet others;
    others.add(ffhip_plane_span(frames, 0, planes, 1));
    others.add(ffhip_plane_span(cost_out, 0, field, 1));
    if (init1)
        others.add(ffhip_plane_span(init1, 0, field ? step : 0, 1));
    if (init2)
        others.add(ffhip_plane_span(init2, 0, field ? step : 0, 1));
    others.seal();
    if (others.hits(ffhip_plane_span(mv_out, 0, field, 1))) {
        ffhip_set_error("%s: mv_out overlaps init1, init2, frames or cost_out", who);
        return FFHIP_EINVAL;
    }
    return 0;
}

extern "C" int ffhip_me_search_pred_sequence_dev(int method, const uint8_t *frames, int width, int height, ptrdiff_t stride, size_t frame_pitch,
                                                 int nframes, size_t seq_pitch, int nseq, int direction, int mb_size, int search_param,
                                                 int cost_kind, const int16_t *init1, const int16_t *init2, int16_t *mv_out, uint32_t *cost_out,
                                                 void *stream)
{
    const int r = me_search_seq_check(MESQ_WHO, method, frames, width, height, stride, frame_pitch, nframes, seq_pitch, nseq, direction, mb_size, search_param,
                                      cost_kind, init1, init2, mv_out, cost_out);
    if (r)
        return r;
    if (!ffhip_have_device())
        return FFHIP_ENOSYS;
    return ffhip_launch_me_search_seq(method, frames, width, height, stride, frame_pitch, nframes, seq_pitch, nseq, direction, mb_size,
                                      search_param, cost_kind, init1, init2, mv_out, cost_out, (hipStream_t)stream);
}

extern "C" int ffhip_me_search_pred_sequence_host(int method, const uint8_t *frames, int width, int height, ptrdiff_t stride, size_t frame_pitch,
                                                  int nframes, size_t seq_pitch, int nseq, int direction, int mb_size, int search_param,
                                                  int cost_kind, const int16_t *init1, const int16_t *init2, int16_t *mv_out, uint32_t *cost_out)
{
    const int r = me_search_seq_check(MESQ_WHO, method, frames, width, height, stride, frame_pitch, nframes, seq_pitch, nseq, direction, mb_size, search_param,
                                      cost_kind, init1, init2, mv_out, cost_out);
    if (r)
        return r;
    /* the definition: step k is the pair face over the nseq pairs (picture k, picture k + 1), its prev fields the two steps before */
    const int lg = mb_size == 16 ? 4 : 3;
    const size_t step = (size_t)(width >> lg) * (size_t)(height >> lg) * (size_t)nseq;    /* blocks of a step */
    uint64_t blocks = 0, costs = 0;
    for (int k = 0; k + 1 < nframes; k++) {
        const uint8_t *lo = frames + (size_t)k * frame_pitch, *hi = lo + frame_pitch;
        int16_t *mv = mv_out + 2 * step * (size_t)k;
        const int16_t *prev1 = k >= 1 ? mv - 2 * step : init1, *prev2 = k >= 2 ? mv - 4 * step : k == 1 ? init1 : init2;
        me_search_pred_host(method, direction ? lo : hi, direction ? hi : lo, width, height, stride, seq_pitch, nseq, mb_size, search_param,
                            cost_kind, prev1, prev2, mv, cost_out + step * (size_t)k);
        blocks += t_host_blocks;
        costs += t_host_costs;
    }
    t_host_blocks = blocks;
    t_host_costs = costs;
    return 0;
}

/* ---- the bilateral searches: EPZS and UMH under the cost of kernels/me_search_bilat_rules.h ----------------------------------------- */
#define MESB_WHO "ffhip_me_search_bilat_batch_dev / _frames_host"
#define MESBQ_WHO "ffhip_me_search_bilat_sequence_dev / _host"
/* what the bilateral faces refuse beyond the predictive faces' checks, which ran with `method` replaced by EPZS for 1..7: the
 * per-block methods, and the geometry for which the cost's two windows could leave the plane.  searching: the call has a block */
static int me_search_bilat_check(const char *who, int method, int width, int height, int mb_size, int search_param, bool searching)
{
    if (method >= FFHIP_ME_METHOD_ESA && method <= FFHIP_ME_METHOD_HEXBS) {
        static const char *const name[] = { "ESA", "TSS", "TDLS", "NTSS", "FSS", "DS", "HEXBS" };
        ffhip_set_error("%s: motion search method %d (%s) is not offered under the bilateral cost: EPZS (8) and UMH (9) are", who, method,
                        name[method - FFHIP_ME_METHOD_ESA]);
        return FFHIP_ENOSYS;
    }
    if (search_param < mb_size) {
        ffhip_set_error("%s: search_param %d below mb_size %d: the overlapped windows of the bilateral cost would leave the picture", who, search_param,
                        mb_size);
        return FFHIP_EINVAL;
    }
    const int lg = mb_size == 16 ? 4 : 3, bw = width >> lg, bh = height >> lg;
    if (searching && bw > 0 && bh > 0 && (bw < 2 || bh < 2)) {
        ffhip_set_error("%s: %d x %d is %d x %d blocks: the bilateral cost needs two block columns and two block rows", who, width, height, bw, bh);
        return FFHIP_EINVAL;
    }
    return 0;
}

static int me_search_bilat_pair_check(int method, const uint8_t *cur, const uint8_t *ref, int width, int height, ptrdiff_t stride, size_t frame_pitch,
                                      int nframes, int mb_size, int search_param, const int16_t *prev1, const int16_t *prev2, const int16_t *mv_out,
                                      const uint32_t *cost_out)
{
    /* the order of the refusals: the arguments every method shares (this text, the faces have no cost_kind), then what the predictive
     * faces refuse of the field and of overlaps with the per-block methods standing in as EPZS, then the method, then the geometry */
    if (me_search_check_args(cur, ref, width, height, stride, frame_pitch, nframes, mb_size, search_param, FFHIP_ME_SAD, mv_out, cost_out)) {
        ffhip_set_error(MESB_WHO ": a NULL cur, ref, mv_out or cost_out, mb_size %d (16 or 8), a negative width, height, nframes or search_param, "
                        "stride < width, frame_pitch < stride * height, or more than 2^31 - 1 blocks", mb_size);
        return FFHIP_EINVAL;
    }
    const bool per_block = method >= FFHIP_ME_METHOD_ESA && method <= FFHIP_ME_METHOD_HEXBS;
    const int r = me_search_pred_check(MESB_WHO, per_block ? FFHIP_ME_METHOD_EPZS : method, cur, ref, width, height, stride, frame_pitch, nframes, mb_size,
                                       search_param, FFHIP_ME_SAD, prev1, prev2, mv_out, cost_out);
    return r ? r : me_search_bilat_check(MESB_WHO, method, width, height, mb_size, search_param, nframes > 0);
}

static int me_search_bilat_seq_check(int method, const uint8_t *frames, int width, int height, ptrdiff_t stride, size_t frame_pitch, int nframes,
                                     size_t seq_pitch, int nseq, int mb_size, int search_param, const int16_t *init1, const int16_t *init2,
                                     const int16_t *mv_out, const uint32_t *cost_out)
{
    /* the order of the pair face's refusals */
    if (me_search_check_args(frames, frames, width, height, stride, frame_pitch, nframes < 2 ? nframes : 2, mb_size, search_param, FFHIP_ME_SAD, mv_out,
                             cost_out)) {
        ffhip_set_error(MESBQ_WHO ": a NULL frames, mv_out or cost_out, mb_size %d (16 or 8), a negative width, height, nframes or search_param, "
                        "stride < width, or frame_pitch < stride * height", mb_size);
        return FFHIP_EINVAL;
    }
    const bool per_block = method >= FFHIP_ME_METHOD_ESA && method <= FFHIP_ME_METHOD_HEXBS;
    const int r = me_search_seq_check(MESBQ_WHO, per_block ? FFHIP_ME_METHOD_EPZS : method, frames, width, height, stride, frame_pitch, nframes, seq_pitch,
                                      nseq, 1, mb_size, search_param, FFHIP_ME_SAD, init1, init2, mv_out, cost_out);
    return r ? r : me_search_bilat_check(MESBQ_WHO, method, width, height, mb_size, search_param, nframes > 1 && nseq > 0);
}

/* cost(X, Y) of the block at (x_mb, y_mb) on the CPU: the sum over the two windows mesb_place() names, and the penalty round `pred` */
struct HostBilatCost {
    const uint8_t *a, *b;           /* pictures A and B */
    ptrdiff_t stride;
    int mb, x_mb, y_mb;
    MesWindow w;
    MespVec pred;
    uint64_t n;
    uint32_t operator()(int X, int Y)
    {
        const MesbPlace at = mesb_place(w, x_mb, y_mb, mb, X, Y);
        const uint8_t *pa = a + (ptrdiff_t)at.ay * stride + at.ax, *pb = b + (ptrdiff_t)at.by * stride + at.bx;
        uint32_t s = 0;
        n++;
        for (int j = 0; j < 2 * mb; j++, pa += stride, pb += stride)
            for (int i = 0; i < 2 * mb; i++)
                s += (uint32_t)abs((int)pa[i] - (int)pb[i]);
        return s + mesb_penalty(X, Y, x_mb, y_mb, pred.x, pred.y);
    }
};

/* the bilateral searches of nframes independent pairs on the CPU, arguments checked: the body of the host faces */
static void me_search_bilat_host(int method, const uint8_t *cur, const uint8_t *ref, int width, int height, ptrdiff_t stride, size_t frame_pitch,
                                 int nframes, int mb_size, int search_param, const int16_t *prev1, const int16_t *prev2, int16_t *mv_out,
                                 uint32_t *cost_out)
{
    const int lg = mb_size == 16 ? 4 : 3, bw = width >> lg, bh = height >> lg;
    me_search_host_with(width, height, nframes, mb_size, search_param, mv_out, cost_out,
                        [&](int f, int x_mb, int y_mb, const MesWindow &w) {
                            const MespVec zero = { 0, 0 };
                            return HostBilatCost{ cur + (size_t)f * frame_pitch, ref + (size_t)f * frame_pitch, stride, mb_size, x_mb, y_mb, w, zero, 0 };
                        },
                        [&](int bx, int by, size_t b, const MesWindow &w, HostBilatCost &cost) {
                            return me_search_pred_block(method, bx, by, b, bw, bh, lg, search_param, w, prev1, prev2, mv_out, cost,
                                                        [&](const MespPred &P) { cost.pred = P.median; });
                        });
}

extern "C" int ffhip_me_search_bilat_cost_host(const uint8_t *cur, const uint8_t *ref, int width, int height, ptrdiff_t stride, int mb_size,
                                               int search_param, int bx, int by, int x, int y, int pred_x, int pred_y, uint32_t *cost)
{
    static const char who[] = "ffhip_me_search_bilat_cost_host";
    if (!cur || !ref || !cost || width < 0 || height < 0 || width > 32768 || height > 32768 || stride < width || (mb_size != 16 && mb_size != 8) ||
        search_param < 0) {
        ffhip_set_error("%s: a NULL cur, ref or cost, mb_size %d (16 or 8), a width or height outside 0..32768, stride < width or a negative search_param",
                        who, mb_size);
        return FFHIP_EINVAL;
    }
    /* the geometry the pair face refuses: the cost's two windows could leave the plane */
    const int r = me_search_bilat_check(who, FFHIP_ME_METHOD_EPZS, width, height, mb_size, search_param, true);
    if (r)
        return r;
    const int lg = mb_size == 16 ? 4 : 3, bw = width >> lg, bh = height >> lg;
    if (bx < 0 || bx >= bw || by < 0 || by >= bh || pred_x < -32768 || pred_x > 32768 || pred_y < -32768 || pred_y > 32768) {
        ffhip_set_error("%s: block (%d, %d) outside %d x %d blocks, or a predictor (%d, %d) beyond +-32768", who, bx, by, bw, bh, pred_x, pred_y);
        return FFHIP_EINVAL;
    }
    const MesWindow w = mes_window(bx << lg, by << lg, search_param, bw, bh, lg);
    if (x < w.x_min || x > w.x_max || y < w.y_min || y > w.y_max) {
        ffhip_set_error("%s: (%d, %d) lies outside the block's window %d..%d x %d..%d", who, x, y, w.x_min, w.x_max, w.y_min, w.y_max);
        return FFHIP_EINVAL;
    }
    HostBilatCost c = { cur, ref, stride, mb_size, bx << lg, by << lg, w, MespVec{ pred_x, pred_y }, 0 };
    *cost = c(x, y);
    return 0;
}

extern "C" int ffhip_me_search_bilat_batch_dev(int method, const uint8_t *cur, const uint8_t *ref, int width, int height, ptrdiff_t stride,
                                               size_t frame_pitch, int nframes, int mb_size, int search_param, const int16_t *prev1,
                                               const int16_t *prev2, int16_t *mv_out, uint32_t *cost_out, void *stream)
{
    const int r = me_search_bilat_pair_check(method, cur, ref, width, height, stride, frame_pitch, nframes, mb_size, search_param, prev1, prev2, mv_out,
                                             cost_out);
    if (r)
        return r;
    if (!ffhip_have_device())
        return FFHIP_ENOSYS;
    return ffhip_launch_me_search_pred(method, cur, ref, width, height, stride, frame_pitch, nframes, mb_size, search_param, MES_COST_BILAT, prev1,
                                       prev2, mv_out, cost_out, (hipStream_t)stream);
}

extern "C" int ffhip_me_search_bilat_frames_host(int method, const uint8_t *cur, const uint8_t *ref, int width, int height, ptrdiff_t stride,
                                                 size_t frame_pitch, int nframes, int mb_size, int search_param, const int16_t *prev1,
                                                 const int16_t *prev2, int16_t *mv_out, uint32_t *cost_out)
{
    const int r = me_search_bilat_pair_check(method, cur, ref, width, height, stride, frame_pitch, nframes, mb_size, search_param, prev1, prev2, mv_out,
                                             cost_out);
    if (r)
        return r;
    me_search_bilat_host(method, cur, ref, width, height, stride, frame_pitch, nframes, mb_size, search_param, prev1, prev2, mv_out, cost_out);
    return 0;
}

extern "C" int ffhip_me_search_bilat_sequence_dev(int method, const uint8_t *frames, int width, int height, ptrdiff_t stride, size_t frame_pitch,
                                                  int nframes, size_t seq_pitch, int nseq, int mb_size, int search_param, const int16_t *init1,
                                                  const int16_t *init2, int16_t *mv_out, uint32_t *cost_out, void *stream)
{
    const int r = me_search_bilat_seq_check(method, frames, width, height, stride, frame_pitch, nframes, seq_pitch, nseq, mb_size, search_param, init1,
                                            init2, mv_out, cost_out);
    if (r)
        return r;
    if (!ffhip_have_device())
        return FFHIP_ENOSYS;
    /* picture A is picture k, picture B picture k + 1: the sequence kernel's direction 1 */
    return ffhip_launch_me_search_seq(method, frames, width, height, stride, frame_pitch, nframes, seq_pitch, nseq, 1, mb_size, search_param,
                                      MES_COST_BILAT, init1, init2, mv_out, cost_out, (hipStream_t)stream);
}

extern "C" int ffhip_me_search_bilat_sequence_host(int method, const uint8_t *frames, int width, int height, ptrdiff_t stride, size_t frame_pitch,
                                                   int nframes, size_t seq_pitch, int nseq, int mb_size, int search_param, const int16_t *init1,
                                                   const int16_t *init2, int16_t *mv_out, uint32_t *cost_out)
{
    const int r = me_search_bilat_seq_check(method, frames, width, height, stride, frame_pitch, nframes, seq_pitch, nseq, mb_size, search_param, init1,
                                            init2, mv_out, cost_out);
    if (r)
        return r;
    /* the definition: step k is the pair face over the nseq pairs (picture k, picture k + 1), its prev fields the two steps before */
    const int lg = mb_size == 16 ? 4 : 3;
    const size_t step = (size_t)(width >> lg) * (size_t)(height >> lg) * (size_t)nseq;    /* blocks of a step */
    uint64_t blocks = 0, costs = 0;
    for (int k = 0; k + 1 < nframes; k++) {
        const uint8_t *lo = frames + (size_t)k * frame_pitch;
        int16_t *mv = mv_out + 2 * step * (size_t)k;
        const int16_t *prev1 = k >= 1 ? mv - 2 * step : init1, *prev2 = k >= 2 ? mv - 4 * step : k == 1 ? init1 : init2;
        me_search_bilat_host(method, lo, lo + frame_pitch, width, height, stride, seq_pitch, nseq, mb_size, search_param, prev1, prev2, mv,
                             cost_out + step * (size_t)k);
        blocks += t_host_blocks;
        costs += t_host_costs;
    }
    t_host_blocks = blocks;
    t_host_costs = costs;
    return 0;
}

/* ---- vf_minterpolate's compensation of whole sequences (kernels/me_interp_rules.h) -------------------------------------------------- */
#define MEI_WHO "ffhip_me_interp_sequence_dev / _host"
extern "C" int ffhip_me_interp_job_size(void) { return (int)sizeof(FFHipMeInterpJob); }
static_assert(sizeof(FFHipMeInterpJob) == 16, "the job record of include/ffhip.h");

/* the faces the texts of me_interp_refuse() name: the bilateral faces put their own here for the length of their checks */
static const char mei_who_default[] = MEI_WHO;
static thread_local const char *t_mei_who = mei_who_default;
struct MeiWho {
    const char *before;
    explicit MeiWho(const char *who) : before(t_mei_who) { t_mei_who = who; }
    ~MeiWho() { t_mei_who = before; }
};

static int me_interp_refuse(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
static int me_interp_refuse(const char *fmt, ...)
{
    char text[400];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(text, sizeof text, fmt, ap);
    va_end(ap);
    ffhip_set_error("%s: %s", t_mei_who, text);
    return FFHIP_EINVAL;
}

/* plane i's size */
static int mei_pw(int i, int width, int sw) { return i ? (width + (1 << sw) - 1) >> sw : width; }
static int mei_ph(int i, int height, int sh) { return i ? (height + (1 << sh) - 1) >> sh : height; }

static int me_interp_check(const FFHipMePlanes *src, const FFHipMePlanes *dst, int nplanes, int sw, int sh, int width, int height, int nframes,
                           int nseq, int mb_size, int mv_range, const uint8_t *window, const int16_t *mv_fwd, const int16_t *mv_bwd,
                           const FFHipMeInterpJob *jobs, int njobs)
{
    if (!src || !dst || !window || !jobs)
        return me_interp_refuse("a NULL src, dst, window or jobs");
    if (nplanes != 1 && nplanes != 3)
        return me_interp_refuse("nplanes %d is neither 1 nor 3", nplanes);
    for (int i = 0; i < nplanes; i++)
        if (!src->base[i] || !dst->base[i])
            return me_interp_refuse("plane %d of %s is NULL", i, !src->base[i] ? "src" : "dst");
    if (sw < 0 || sw > 1 || sh < 0 || sh > 1)
        return me_interp_refuse("chroma shifts %d, %d (0 or 1 each)", sw, sh);
    if (mb_size != 16 && mb_size != 8)
        return me_interp_refuse("mb_size %d (16 or 8)", mb_size);
    if (mv_range < 0 || mv_range > MEI_MAX_RANGE)
        return me_interp_refuse("mv_range %d outside 0..%d", mv_range, MEI_MAX_RANGE);
    if (width < 0 || height < 0 || nframes < 0 || nseq < 0 || njobs < 0)
        return me_interp_refuse("a negative width, height, nframes, nseq or njobs (%d, %d, %d, %d, %d)", width, height, nframes, nseq, njobs);
    if (width > 32768 || height > 32768)
        return me_interp_refuse("%d x %d: positions of a picture above 32768 do not fit the int16 vector fields", width, height);
    for (int i = 0; i < nplanes; i++) {
        const int pw = mei_pw(i, width, sw), ph = mei_ph(i, height, sh);
        if (src->stride[i] < pw || dst->stride[i] < pw)
            return me_interp_refuse("plane %d: a stride (src %td, dst %td) below the plane's width %d", i, src->stride[i], dst->stride[i], pw);
        /* the sequence face's rule per plane: a picture is stride * height bytes, a sequence ends that far behind its last picture */
        const size_t pic = (size_t)src->stride[i] * (size_t)ph, dpic = (size_t)dst->stride[i] * (size_t)ph;
        if (nframes > 1 && src->frame_pitch[i] < pic)
            return me_interp_refuse("plane %d: src frame_pitch %zu < stride * height %zu", i, src->frame_pitch[i], pic);
        if (nseq > 1 && nframes > 0) {
            size_t gap, need;
            if (__builtin_mul_overflow((size_t)(nframes - 1), src->frame_pitch[i], &gap) || __builtin_add_overflow(gap, pic, &need) ||
                src->seq_pitch[i] < need)
                return me_interp_refuse("plane %d: src seq_pitch %zu < (nframes - 1) * frame_pitch + stride * height: the pictures of two sequences "
                                        "would share bytes", i, src->seq_pitch[i]);
        }
        if (njobs > 1 && dst->frame_pitch[i] < dpic)
            return me_interp_refuse("plane %d: dst frame_pitch %zu < stride * height %zu", i, dst->frame_pitch[i], dpic);
    }
    bool mci = false;
    for (int j = 0; j < njobs; j++) {
        const FFHipMeInterpJob &J = jobs[j];
        if (J.seq < 0 || J.seq >= nseq || J.pair < 0 || J.pair > nframes - 2 || J.alpha < 0 || J.alpha > 1024 ||
            (J.mode != FFHIP_ME_INTERP_MCI && J.mode != FFHIP_ME_INTERP_BLEND))
            return me_interp_refuse("job %d: seq %d (0..%d), pair %d (0..%d), alpha %d (0..1024), mode %d (0 or 1)", j, J.seq, nseq - 1, J.pair,
                                    nframes - 2, J.alpha, J.mode);
        mci |= J.mode == FFHIP_ME_INTERP_MCI;
    }
    const bool one_field = mv_fwd == mv_bwd && t_mei_who != mei_who_default;      /* the bilateral faces pass their one field twice */
    if (mci && (!mv_fwd || !mv_bwd))
        return me_interp_refuse("a NULL %s with an MCI job", one_field ? "mv" : "mv_fwd or mv_bwd");
    /* what the call writes shares no byte with what it reads */
    const bool any = njobs > 0 && width > 0 && height > 0;
    const int lg = mb_size == 16 ? 4 : 3;
    const ptrdiff_t field = any && mci ? (ptrdiff_t)(width >> lg) * (height >> lg) * nseq * (nframes - 1) * 4 : 0;
    FFHipSpanSet reads;
    std::vector<FFHipSpan> writes;
    for (int i = 0; i < nplanes && any; i++) {
        const int pw = mei_pw(i, width, sw), ph = mei_ph(i, height, sh);
        reads.add(ffhip_plane_span(src->base[i], 0, (ptrdiff_t)(nseq - 1) * (ptrdiff_t)src->seq_pitch[i] + (ptrdiff_t)(nframes - 1) * (ptrdiff_t)src->frame_pitch[i] +
                                                        (ptrdiff_t)(ph - 1) * src->stride[i] + pw, 1));
        writes.push_back(ffhip_plane_span(dst->base[i], 0, (ptrdiff_t)(njobs - 1) * (ptrdiff_t)dst->frame_pitch[i] + (ptrdiff_t)(ph - 1) * dst->stride[i] + pw, 1));
    }
    if (mv_fwd)
        reads.add(ffhip_plane_span(mv_fwd, 0, field, 1));
    if (mv_bwd)
        reads.add(ffhip_plane_span(mv_bwd, 0, field, 1));
    reads.seal();
    for (const FFHipSpan &w : writes)
        if (reads.hits(w))
            return me_interp_refuse("dst overlaps src, %s", one_field ? "or mv" : "mv_fwd or mv_bwd");
    return 0;
}

extern "C" int ffhip_me_interp_sequence_dev(const FFHipMePlanes *src, const FFHipMePlanes *dst, int nplanes, int log2_chroma_w, int log2_chroma_h,
                                            int width, int height, int nframes, int nseq, int mb_size, int mv_range, const uint8_t *window,
                                            const int16_t *mv_fwd, const int16_t *mv_bwd, const FFHipMeInterpJob *jobs, int njobs, void *stream)
{
    const int r = me_interp_check(src, dst, nplanes, log2_chroma_w, log2_chroma_h, width, height, nframes, nseq, mb_size, mv_range, window, mv_fwd,
                                  mv_bwd, jobs, njobs);
    if (r)
        return r;
    if (!njobs)
        return 0;
    if (!ffhip_have_device())
        return FFHIP_ENOSYS;
    return ffhip_launch_me_interp(src, dst, nplanes, log2_chroma_w, log2_chroma_h, width, height, nseq, mb_size, mv_range, window, mv_fwd, mv_bwd,
                                  jobs, njobs, (hipStream_t)stream);
}

static thread_local uint64_t t_interp_counts[MEI_NCOUNTS];
static_assert(MEI_NCOUNTS == 8, "ffhip_me_interp_host_counts() reports eight");

extern "C" void ffhip_me_interp_host_counts(uint64_t counts[8])
{
    if (counts)
        memcpy(counts, t_interp_counts, sizeof t_interp_counts);
}

/* the host face after the checks; scene: NULL or the pair-major flags of ffhip_me_interp_sequence_scd_host() */
template <bool BILAT = false>
static int me_interp_host(const FFHipMePlanes *src, const FFHipMePlanes *dst, int nplanes, int log2_chroma_w, int log2_chroma_h, int width, int height,
                          int nseq, int mb_size, int mv_range, const uint8_t *window, const int16_t *mv_fwd, const int16_t *mv_bwd,
                          const FFHipMeInterpJob *jobs, int njobs, const uint8_t *scene, int scene_action)
{
    const MeiGeom g = mei_geom(width, height, mb_size, mv_range);
    const size_t per = (size_t)g.bw * g.bh;
    uint64_t cnt[MEI_NCOUNTS] = {};
    std::vector<MeiBlock> blocks(2 * per);      /* a job's windows, formed once; a malformed block's is empty */
    for (int j = 0; j < njobs; j++) {
        const FFHipMeInterpJob &J = jobs[j];
        const int alpha = J.alpha;
        /* an MCI job whose pair is flagged runs the scene action, sample by sample like the blend */
        const bool cut = scene && J.mode == FFHIP_ME_INTERP_MCI && scene[(size_t)J.pair * nseq + J.seq];
        const bool blend = J.mode == FFHIP_ME_INTERP_BLEND || cut;
        const int wb = mei_scene_alpha(cut, scene_action, alpha);
        const uint8_t *A[3] = {}, *B[3] = {};
        uint8_t *D[3] = {};
        for (int i = 0; i < nplanes; i++) {
            A[i] = src->base[i] + (size_t)J.seq * src->seq_pitch[i] + (size_t)J.pair * src->frame_pitch[i];
            B[i] = A[i] + src->frame_pitch[i];
            D[i] = dst->base[i] + (size_t)j * dst->frame_pitch[i];
        }
        if (!blend)
            for (int dir = 0; dir < (BILAT ? 1 : 2); dir++) {         /* BILAT: mv_fwd is the one field of half-vectors */
                const int16_t *f = (dir ? mv_bwd : mv_fwd) + 2 * per * ((size_t)J.pair * nseq + J.seq);
                for (int by = 0; by < g.bh; by++)
                    for (int bx = 0; bx < g.bw; bx++) {
                        const size_t b = (size_t)by * g.bw + bx;
                        int vx, vy;
                        const bool ok = mei_vector(g, bx, by, f[2 * b], f[2 * b + 1], vx, vy);
                        cnt[MEI_N_MALFORMED] += !ok;
                        blocks[dir * per + b] = !ok ? mei_no_block() : BILAT ? mei_block_bilat(g, bx, by, vx, vy) : mei_block(g, alpha, dir, bx, by, vx, vy);
                    }
            }
        auto block = [&](int dir, int bx, int by) -> const MeiBlock & { return blocks[dir * per + (size_t)by * g.bw + bx]; };
        for (int i = 0; i < nplanes; i++) {
            const int sw = i ? log2_chroma_w : 0, sh = i ? log2_chroma_h : 0, pw = mei_pw(i, width, sw), ph = mei_ph(i, height, sh);
            const ptrdiff_t ss = src->stride[i];
            for (int cy = 0; cy < ph; cy++)
                for (int cx = 0; cx < pw; cx++) {
                    uint8_t *d = D[i] + (ptrdiff_t)cy * dst->stride[i] + cx;
                    cnt[MEI_N_SAMPLES]++;
                    if (blend) {
                        *d = (uint8_t)mei_blend(A[i][cy * ss + cx], B[i][cy * ss + cx], wb);
                        cnt[MEI_N_BLEND]++;
                        continue;
                    }
                    /* the luma pixel whose list the sample uses: itself, or the last writer of the reference's walk */
                    const int x = std::min(((cx + 1) << sw) - 1, width - 1), y = std::min(((cy + 1) << sh) - 1, height - 1);
                    uint64_t S = 0, Wt = 0;
                    auto take = [&](int wa, int dxa, int dya, int wb, int dxb, int dyb) {
                        S += (uint64_t)wa * A[i][((y >> sh) + mei_tshift(dya, sh)) * ss + (x >> sw) + mei_tshift(dxa, sw)] +
                             (uint64_t)wb * B[i][((y >> sh) + mei_tshift(dyb, sh)) * ss + (x >> sw) + mei_tshift(dxb, sw)];
                        Wt += (uint64_t)(wa + wb);
                    };
                    if (BILAT)
                        mei_walk_bilat(g, alpha, x, y, window, [&](int bx, int by) -> const MeiBlock & { return block(0, bx, by); }, take, i ? nullptr : cnt);
                    else
                        mei_walk(g, alpha, x, y, window, block, take, i ? nullptr : cnt);
                    *d = (uint8_t)((S + (Wt >> 1)) / Wt);
                }
        }
    }
    memcpy(t_interp_counts, cnt, sizeof cnt);
    return 0;
}

extern "C" int ffhip_me_interp_sequence_host(const FFHipMePlanes *src, const FFHipMePlanes *dst, int nplanes, int log2_chroma_w, int log2_chroma_h,
                                             int width, int height, int nframes, int nseq, int mb_size, int mv_range, const uint8_t *window,
                                             const int16_t *mv_fwd, const int16_t *mv_bwd, const FFHipMeInterpJob *jobs, int njobs)
{
    const int r = me_interp_check(src, dst, nplanes, log2_chroma_w, log2_chroma_h, width, height, nframes, nseq, mb_size, mv_range, window, mv_fwd,
                                  mv_bwd, jobs, njobs);
    if (r)
        return r;
    return me_interp_host(src, dst, nplanes, log2_chroma_w, log2_chroma_h, width, height, nseq, mb_size, mv_range, window, mv_fwd, mv_bwd, jobs, njobs,
                          nullptr, FFHIP_ME_SCENE_BLEND);
}

/* ---- the interpolation that takes its MCI-or-fallback choice from scene flags ------------------------------------------------------ */
/* what the scd faces check beyond me_interp_check() */
static int me_interp_scd_check(const FFHipMePlanes *dst, int nplanes, int sw, int sh, int width, int height, int nframes, int nseq, int njobs,
                               const uint8_t *scene, int scene_action)
{
    if (scene_action != FFHIP_ME_SCENE_BLEND && scene_action != FFHIP_ME_SCENE_DUP) {
        ffhip_set_error("%s: scene_action %d (1: blend, 2: duplicate)", t_mei_who != mei_who_default ? t_mei_who : "ffhip_me_interp_sequence_scd_dev / _host",
                        scene_action);
        return FFHIP_EINVAL;
    }
    if (!scene || njobs <= 0 || width <= 0 || height <= 0 || nframes < 2 || nseq < 1)
        return 0;
    FFHipSpanSet reads;
    reads.add(ffhip_plane_span(scene, 0, (ptrdiff_t)(nframes - 1) * nseq, 1));
    reads.seal();
    for (int i = 0; i < nplanes; i++) {
        const int pw = mei_pw(i, width, sw), ph = mei_ph(i, height, sh);
        if (reads.hits(ffhip_plane_span(dst->base[i], 0, (ptrdiff_t)(njobs - 1) * (ptrdiff_t)dst->frame_pitch[i] + (ptrdiff_t)(ph - 1) * dst->stride[i] + pw, 1))) {
            ffhip_set_error("%s: dst overlaps scene", t_mei_who != mei_who_default ? t_mei_who : "ffhip_me_interp_sequence_scd_dev / _host");
            return FFHIP_EINVAL;
        }
    }
    return 0;
}

extern "C" int ffhip_me_interp_sequence_scd_dev(const FFHipMePlanes *src, const FFHipMePlanes *dst, int nplanes, int log2_chroma_w, int log2_chroma_h,
                                                int width, int height, int nframes, int nseq, int mb_size, int mv_range, const uint8_t *window,
                                                const int16_t *mv_fwd, const int16_t *mv_bwd, const FFHipMeInterpJob *jobs, int njobs,
                                                const uint8_t *scene, int scene_action, void *stream)
{
    int r = me_interp_check(src, dst, nplanes, log2_chroma_w, log2_chroma_h, width, height, nframes, nseq, mb_size, mv_range, window, mv_fwd, mv_bwd,
                            jobs, njobs);
    if (!r)
        r = me_interp_scd_check(dst, nplanes, log2_chroma_w, log2_chroma_h, width, height, nframes, nseq, njobs, scene, scene_action);
    if (r)
        return r;
    if (!njobs)
        return 0;
    if (!ffhip_have_device())
        return FFHIP_ENOSYS;
    return ffhip_launch_me_interp_scd(src, dst, nplanes, log2_chroma_w, log2_chroma_h, width, height, nseq, mb_size, mv_range, window, mv_fwd, mv_bwd,
                                      jobs, njobs, scene, scene_action, (hipStream_t)stream);
}

extern "C" int ffhip_me_interp_sequence_scd_host(const FFHipMePlanes *src, const FFHipMePlanes *dst, int nplanes, int log2_chroma_w, int log2_chroma_h,
                                                 int width, int height, int nframes, int nseq, int mb_size, int mv_range, const uint8_t *window,
                                                 const int16_t *mv_fwd, const int16_t *mv_bwd, const FFHipMeInterpJob *jobs, int njobs,
                                                 const uint8_t *scene, int scene_action)
{
    int r = me_interp_check(src, dst, nplanes, log2_chroma_w, log2_chroma_h, width, height, nframes, nseq, mb_size, mv_range, window, mv_fwd, mv_bwd,
                            jobs, njobs);
    if (!r)
        r = me_interp_scd_check(dst, nplanes, log2_chroma_w, log2_chroma_h, width, height, nframes, nseq, njobs, scene, scene_action);
    if (r)
        return r;
    return me_interp_host(src, dst, nplanes, log2_chroma_w, log2_chroma_h, width, height, nseq, mb_size, mv_range, window, mv_fwd, mv_bwd, jobs, njobs,
                          scene, scene_action);
}

/* ---- the bilateral compensation: one field of half-vectors (kernels/me_interp_rules.h: mei_block_bilat, mei_walk_bilat) ------------- */
#define MEIB_WHO "ffhip_me_interp_bilat_sequence_dev / _host"
static int me_interp_bilat_check(const FFHipMePlanes *src, const FFHipMePlanes *dst, int nplanes, int sw, int sh, int width, int height, int nframes,
                                 int nseq, int mb_size, int mv_range, const uint8_t *window, const int16_t *mv, const FFHipMeInterpJob *jobs, int njobs,
                                 const uint8_t *scene, int scene_action)
{
    const MeiWho who(MEIB_WHO);
    const int r = me_interp_check(src, dst, nplanes, sw, sh, width, height, nframes, nseq, mb_size, mv_range, window, mv, mv, jobs, njobs);
    return r ? r : me_interp_scd_check(dst, nplanes, sw, sh, width, height, nframes, nseq, njobs, scene, scene_action);
}

extern "C" int ffhip_me_interp_bilat_sequence_dev(const FFHipMePlanes *src, const FFHipMePlanes *dst, int nplanes, int log2_chroma_w, int log2_chroma_h,
                                                  int width, int height, int nframes, int nseq, int mb_size, int mv_range, const uint8_t *window,
                                                  const int16_t *mv, const FFHipMeInterpJob *jobs, int njobs, const uint8_t *scene, int scene_action,
                                                  void *stream)
{
    const int r = me_interp_bilat_check(src, dst, nplanes, log2_chroma_w, log2_chroma_h, width, height, nframes, nseq, mb_size, mv_range, window, mv, jobs,
                                        njobs, scene, scene_action);
    if (r)
        return r;
    if (!njobs)
        return 0;
    if (!ffhip_have_device())
        return FFHIP_ENOSYS;
    return ffhip_launch_me_interp_bilat(src, dst, nplanes, log2_chroma_w, log2_chroma_h, width, height, nseq, mb_size, mv_range, window, mv, jobs, njobs,
                                        scene, scene_action, (hipStream_t)stream);
}

extern "C" int ffhip_me_interp_bilat_sequence_host(const FFHipMePlanes *src, const FFHipMePlanes *dst, int nplanes, int log2_chroma_w, int log2_chroma_h,
                                                   int width, int height, int nframes, int nseq, int mb_size, int mv_range, const uint8_t *window,
                                                   const int16_t *mv, const FFHipMeInterpJob *jobs, int njobs, const uint8_t *scene, int scene_action)
{
    const int r = me_interp_bilat_check(src, dst, nplanes, log2_chroma_w, log2_chroma_h, width, height, nframes, nseq, mb_size, mv_range, window, mv, jobs,
                                        njobs, scene, scene_action);
    if (r)
        return r;
    return me_interp_host<true>(src, dst, nplanes, log2_chroma_w, log2_chroma_h, width, height, nseq, mb_size, mv_range, window, mv, mv, jobs, njobs, scene,
                                scene_action);
}

/* ---- vf_minterpolate's scene-change detection of whole sequences (kernels/me_scene_rules.h) ------------------------------------------ */
static int me_scene_refuse(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
static int me_scene_refuse(const char *fmt, ...)
{
    char text[400];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(text, sizeof text, fmt, ap);
    va_end(ap);
    ffhip_set_error("ffhip_me_scene_sequence_dev / _host: %s", text);
    return FFHIP_EINVAL;
}

static int me_scene_check(const uint8_t *frames, int depth, int width, int height, ptrdiff_t stride, size_t frame_pitch, int nframes, size_t seq_pitch,
                          int nseq, double threshold, const double *mafd_in, double *mafd_out, uint64_t *sad_out, float *score_out, uint8_t *flags_out)
{
    if (!frames || (!sad_out && !score_out && !flags_out))
        return me_scene_refuse("a NULL frames, or sad_out, score_out and flags_out all NULL");
    if (depth < 8 || depth > 16)
        return me_scene_refuse("depth %d outside 8..16", depth);
    if (width < 1 || width > 32768 || height < 1 || height > 32768)
        return me_scene_refuse("%d x %d: width and height are 1..32768", width, height);
    if (nframes < 0 || nseq < 0)
        return me_scene_refuse("a negative nframes or nseq (%d, %d)", nframes, nseq);
    const int px = depth > 8 ? 2 : 1;
    const ptrdiff_t row = (ptrdiff_t)width * px;
    if (stride < row)
        return me_scene_refuse("stride %td below the row's %td bytes", stride, row);
    if (px == 2 && (((uintptr_t)frames | (uintptr_t)stride | frame_pitch | seq_pitch) & 1))
        return me_scene_refuse("above 8 bits samples are uint16_t: an odd frames address, stride, frame_pitch or seq_pitch (%p, %td, %zu, %zu)",
                               (const void *)frames, stride, frame_pitch, seq_pitch);
    const size_t pic = (size_t)stride * (size_t)height;
    if (nframes > 1 && frame_pitch < pic)
        return me_scene_refuse("frame_pitch %zu < stride * height %zu", frame_pitch, pic);
    size_t seq_end = pic;           /* a sequence ends stride * height behind the start of its last picture */
    if (nframes > 1 && (__builtin_mul_overflow((size_t)(nframes - 1), frame_pitch, &seq_end) || __builtin_add_overflow(seq_end, pic, &seq_end)))
        return me_scene_refuse("(nframes - 1) * frame_pitch + stride * height does not fit size_t");
    if (nseq > 1 && nframes > 0 && seq_pitch < seq_end)
        return me_scene_refuse("seq_pitch %zu < (nframes - 1) * frame_pitch + stride * height %zu: the pictures of two sequences would share bytes",
                               seq_pitch, seq_end);
    if (!(threshold >= 0.0 && threshold <= 100.0))
        return me_scene_refuse("threshold %g is not a number in 0..100", threshold);
    const int64_t npairs = nframes > 1 ? (int64_t)(nframes - 1) * nseq : 0;
    if (npairs > INT_MAX)
        return me_scene_refuse("%lld pairs: more than 2^31 - 1", (long long)npairs);
    /* what the call writes shares no byte with what it reads or with another output */
    FFHipSpanSet reads, writes;
    if (nframes > 0 && nseq > 0)
        reads.add(ffhip_plane_span(frames, 0, (ptrdiff_t)(nseq - 1) * (ptrdiff_t)seq_pitch + (ptrdiff_t)(nframes - 1) * (ptrdiff_t)frame_pitch +
                                                  (ptrdiff_t)(height - 1) * stride + row, 1));
    if (mafd_in)
        reads.add(ffhip_plane_span(mafd_in, 0, (ptrdiff_t)nseq * 8, 1));
    reads.seal();
    const FFHipSpan out[4] = { ffhip_plane_span(mafd_out, 0, mafd_out ? (ptrdiff_t)nseq * 8 : 0, 1), ffhip_plane_span(sad_out, 0, sad_out ? (ptrdiff_t)npairs * 8 : 0, 1),
                               ffhip_plane_span(score_out, 0, score_out ? (ptrdiff_t)npairs * 4 : 0, 1),
                               ffhip_plane_span(flags_out, 0, flags_out ? (ptrdiff_t)npairs : 0, 1) };
    bool shared = false;
    for (const FFHipSpan &o : out) {
        shared |= reads.hits(o);
        writes.add(o);
    }
    if (writes.seal() || shared)
        return me_scene_refuse("an output (mafd_out, sad_out, score_out, flags_out) overlaps frames, mafd_in or another output");
    return 0;
}

extern "C" int ffhip_me_scene_sequence_dev(const uint8_t *frames, int depth, int width, int height, ptrdiff_t stride, size_t frame_pitch, int nframes,
                                           size_t seq_pitch, int nseq, double threshold, const double *mafd_in, double *mafd_out, uint64_t *sad_out,
                                           float *score_out, uint8_t *flags_out, void *stream)
{
    const int r = me_scene_check(frames, depth, width, height, stride, frame_pitch, nframes, seq_pitch, nseq, threshold, mafd_in, mafd_out, sad_out,
                                 score_out, flags_out);
    if (r)
        return r;
    if (!nseq || (nframes <= 1 && !mafd_out))
        return 0;
    if (!ffhip_have_device())
        return FFHIP_ENOSYS;
    return ffhip_launch_me_scene(frames, depth, width, height, stride, frame_pitch, nframes, seq_pitch, nseq, threshold, mafd_in, mafd_out, sad_out,
                                 score_out, flags_out, (hipStream_t)stream);
}

extern "C" int ffhip_me_scene_sequence_host(const uint8_t *frames, int depth, int width, int height, ptrdiff_t stride, size_t frame_pitch, int nframes,
                                            size_t seq_pitch, int nseq, double threshold, const double *mafd_in, double *mafd_out, uint64_t *sad_out,
                                            float *score_out, uint8_t *flags_out)
{
    const int r = me_scene_check(frames, depth, width, height, stride, frame_pitch, nframes, seq_pitch, nseq, threshold, mafd_in, mafd_out, sad_out,
                                 score_out, flags_out);
    if (r)
        return r;
    const int steps = nframes > 1 ? nframes - 1 : 0;
    for (int s = 0; s < nseq; s++) {
        const uint8_t *const S = frames + (size_t)s * seq_pitch;
        const double prev = mes_scene_walk(steps, width, height, depth, threshold, mafd_in ? mafd_in[s] : 0.0,
            [&](int k) {
                const uint8_t *const A = S + (size_t)k * frame_pitch, *const B = A + frame_pitch;
                uint64_t sad = 0;
                for (int y = 0; y < height; y++)
                    sad += depth > 8 ? mes_scene_sad_row(reinterpret_cast<const uint16_t *>(A + (ptrdiff_t)y * stride),
                                                         reinterpret_cast<const uint16_t *>(B + (ptrdiff_t)y * stride), width)
                                     : mes_scene_sad_row(A + (ptrdiff_t)y * stride, B + (ptrdiff_t)y * stride, width);
                return sad;
            },
            [&](int k, uint64_t sad, float score, int flag) {
                const size_t o = (size_t)k * nseq + s;
                if (sad_out)
                    sad_out[o] = sad;
                if (score_out)
                    score_out[o] = score;
                if (flags_out)
                    flags_out[o] = (uint8_t)flag;
            });
        if (mafd_out)
            mafd_out[s] = prev;
    }
    return 0;
}
