/*
 * me_search_rules.h — the per-block fast motion searches of the filter (the methods libavfilter/motion_estimation.c offers to
 * vf_mestimate and vf_minterpolate beside the exhaustive one): TSS, TDLS, NTSS, FSS, DS and HEXBS, as include/ffhip.h states them for
 * ffhip_me_search_batch_dev().  RESTATED, NOT CHECKED AGAINST THE SOURCE: the rules were written down without the reference's source at
 * hand; the statement in include/ffhip.h is the definition the tests pin.
 *
 * The header owns the pattern tables, the window, per method the ordered candidate list of an evaluation step and the state
 * transition given that step's result, and the loop over the steps, mes_run().  It does not own how a cost is computed: the kernel
 * of me_search.hip (one wave per block, eight lanes per candidate) and ffhip_me_search_frames_host() (me_api.hip, plain loops on the
 * CPU) both run mes_run() on the state of mes_start() (the kernel as its text, for the reason given there) and differ in step_key
 * alone: the minimum of mes_key(cost(x, y), i) over the i < st.n with mes_candidate(s, st, w, i, x, y), MES_NO_KEY if there is none.
 *
 * A step holds at most 8 candidates, all round one centre, so they are independent of each
 * other; applying them in table order with a strict comparison (COST_MV) equals taking the minimum of cost << 3 | index and
 * comparing its cost strictly with cost_min: on equal costs the lowest index wins, and an equal cost never displaces the centre.
 * NTSS's first iteration has 16 candidates round one centre (the large ring, then the unit ring): it is two steps.
 */
#ifndef FFHIP_ME_SEARCH_RULES_H
#define FFHIP_ME_SEARCH_RULES_H

#include <stdint.h>

#include "ffhip.h"

#if defined(__HIPCC__)
#define MES_FN __host__ __device__ __forceinline__
#else
#define MES_FN static inline
#endif

/* ---- the pattern tables: (dx, dy) of entry i in nibble i, biased by 2 ------------------------------------------------------- */
#define MES_NIB(v, i) ((uint32_t)((v) + 2) << (4 * (i)))
#define MES_TAB(a, b, c, d, e, f, g, h) \
    (MES_NIB(a, 0) | MES_NIB(b, 1) | MES_NIB(c, 2) | MES_NIB(d, 3) | MES_NIB(e, 4) | MES_NIB(f, 5) | MES_NIB(g, 6) | MES_NIB(h, 7))
enum { MES_SQR1 = 0, MES_DIA1 = 1, MES_DIA2 = 2, MES_HEX2 = 3 };
/* sqr1 = (0,-1) (0,1) (-1,0) (1,0) (-1,-1) (-1,1) (1,-1) (1,1) */
#define MES_SQR1_DX MES_TAB(0, 0, -1, 1, -1, -1, 1, 1)
#define MES_SQR1_DY MES_TAB(-1, 1, 0, 0, -1, 1, -1, 1)
/* dia1 = (-1,0) (0,-1) (1,0) (0,1) */
#define MES_DIA1_DX MES_TAB(-1, 0, 1, 0, 0, 0, 0, 0)
#define MES_DIA1_DY MES_TAB(0, -1, 0, 1, 0, 0, 0, 0)
/* dia2 = (-2,0) (-1,-1) (0,-2) (1,-1) (2,0) (1,1) (0,2) (-1,1) */
#define MES_DIA2_DX MES_TAB(-2, -1, 0, 1, 2, 1, 0, -1)
#define MES_DIA2_DY MES_TAB(0, -1, -2, -1, 0, 1, 2, 1)
/* hex2 = (-2,0) (-1,-2) (-1,2) (1,-2) (1,2) (2,0) */
#define MES_HEX2_DX MES_TAB(-2, -1, -1, 1, 1, 2, 0, 0)
#define MES_HEX2_DY MES_TAB(0, -2, 2, -2, 2, 0, 0, 0)

MES_FN int mes_pattern_n(int pattern) { return pattern == MES_DIA1 ? 4 : pattern == MES_HEX2 ? 6 : 8; }
MES_FN int mes_pattern_dx(int pattern, int i)
{
    const uint32_t t = pattern == MES_SQR1 ? MES_SQR1_DX : pattern == MES_DIA1 ? MES_DIA1_DX : pattern == MES_DIA2 ? MES_DIA2_DX : MES_HEX2_DX;
    return (int)((t >> (4 * i)) & 15u) - 2;
}
MES_FN int mes_pattern_dy(int pattern, int i)
{
    const uint32_t t = pattern == MES_SQR1 ? MES_SQR1_DY : pattern == MES_DIA1 ? MES_DIA1_DY : pattern == MES_DIA2 ? MES_DIA2_DY : MES_HEX2_DY;
    return (int)((t >> (4 * i)) & 15u) - 2;
}

/* ---- the window: [x_mb - R, x_mb + R] cut to [0, (b_w - 1) << log2mb], the same for y ---------------------------------------- */
struct MesWindow {
    int x_min, x_max, y_min, y_max;
};

MES_FN int mes_clip64(int64_t v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : (int)v; }

/* the block at (x_mb, y_mb) of a picture with b_w x b_h whole blocks; R >= 0 of any size */
MES_FN MesWindow mes_window(int x_mb, int y_mb, int R, int b_w, int b_h, int log2mb)
{
    const int lim_x = (b_w - 1) << log2mb, lim_y = (b_h - 1) << log2mb;
    MesWindow w;
    w.x_min = mes_clip64((int64_t)x_mb - R, 0, lim_x);
    w.x_max = mes_clip64((int64_t)x_mb + R, 0, lim_x);
    w.y_min = mes_clip64((int64_t)y_mb - R, 0, lim_y);
    w.y_max = mes_clip64((int64_t)y_mb + R, 0, lim_y);
    return w;
}

/* ---- the state of one block's search ------------------------------------------------------------------------------------------ */
enum {
    MES_PHASE_MAIN = 0,       /* the method's pattern round the centre, scaled by `step` in the four step methods */
    MES_PHASE_NTSS_UNIT = 1,  /* NTSS, first iteration: the unit ring round the same centre */
    MES_PHASE_LAST = 2        /* the closing pattern (NTSS: the unit ring round the new centre; DS, HEXBS: dia1), then the end */
};

struct MesState {
    int method, phase, step, first, done;
    int x, y;           /* the centre of the step: mv as it was at the top of the iteration */
    int mvx, mvy;       /* mv: the best position so far */
    uint32_t cost_min;  /* its cost */
};

struct MesStep {
    int pattern, n, scale;
};

/* the common start: mv = (x_mb, y_mb), cost_min = its cost; a cost of 0 ends the search at once */
MES_FN MesState mes_start(int method, int x_mb, int y_mb, int R, uint32_t cost0)
{
    MesState s;
    s.method = method;
    s.phase = MES_PHASE_MAIN;
    s.step = method == FFHIP_ME_METHOD_FSS ? 2 : (R >> 1) + (R & 1);   /* (R + 1) >> 1 without the overflow */
    s.first = 1;
    s.done = cost0 == 0;
    s.x = s.mvx = x_mb;
    s.y = s.mvy = y_mb;
    s.cost_min = cost0;
    return s;
}

/* what the step evaluates */
MES_FN MesStep mes_step(const MesState &s)
{
    MesStep st;
    st.scale = 1;
    if (s.phase == MES_PHASE_NTSS_UNIT) {
        st.pattern = MES_SQR1;
    } else if (s.phase == MES_PHASE_LAST) {
        st.pattern = s.method == FFHIP_ME_METHOD_NTSS ? MES_SQR1 : MES_DIA1;
    } else if (s.method == FFHIP_ME_METHOD_DS) {
        st.pattern = MES_DIA2;
    } else if (s.method == FFHIP_ME_METHOD_HEXBS) {
        st.pattern = MES_HEX2;
    } else {
        st.pattern = s.method == FFHIP_ME_METHOD_TDLS ? MES_DIA1 : MES_SQR1;
        st.scale = s.step;
    }
    st.n = mes_pattern_n(st.pattern);
    return st;
}

/* candidate i < st.n of the step: COST_P_MV's test.  false: outside the window, nothing is evaluated.  Inside the window the block
 * read lies inside the width x height plane, whatever R and the step are (the sum is taken in 64 bits). */
MES_FN bool mes_candidate(const MesState &s, const MesStep &st, const MesWindow &w, int i, int &x, int &y)
{
    const int64_t cx = (int64_t)s.x + (int64_t)mes_pattern_dx(st.pattern, i) * st.scale;
    const int64_t cy = (int64_t)s.y + (int64_t)mes_pattern_dy(st.pattern, i) * st.scale;
    x = (int)cx;
    y = (int)cy;
    return cx >= w.x_min && cx <= w.x_max && cy >= w.y_min && cy <= w.y_max;
}

/* the ordered minimum: a cost is below 2^29 (the largest, a 16x16 SATD, is below 2^20) */
#define MES_NO_KEY 0xFFFFFFFFu
MES_FN uint32_t mes_key(uint32_t cost, int i) { return cost << 3 | (uint32_t)i; }

/* every step but the closing ones either moves mv to a position of the window it never held (cost_min falls strictly), halves
 * `step` (at most 31 times) or changes the phase (at most twice): no search takes more steps than this, and none waits for
 * anything outside its own block */
MES_FN uint32_t mes_step_bound(const MesWindow &w)
{
    const uint64_t n = (uint64_t)(w.x_max - w.x_min + 1) * (uint64_t)(w.y_max - w.y_min + 1);
    return (uint32_t)(n < (1u << 30) ? n : (1u << 30)) + 40u;
}

/* the transition: `key` is the step's ordered minimum (MES_NO_KEY when every candidate was refused) */
MES_FN void mes_advance(MesState &s, const MesStep &st, const MesWindow &w, uint32_t key)
{
    if ((key >> 3) < s.cost_min) {
        s.cost_min = key >> 3;
        mes_candidate(s, st, w, (int)(key & 7u), s.mvx, s.mvy);
    }
    const bool moved = s.mvx != s.x || s.mvy != s.y;
    if (s.phase == MES_PHASE_LAST) {
        s.done = 1;
        return;
    }
    if (s.phase == MES_PHASE_NTSS_UNIT) {
        if (!moved) {                                   /* the centre is the minimum of both rings */
            s.done = 1;
            return;
        }
        const int ax = s.x > s.mvx ? s.x - s.mvx : s.mvx - s.x, ay = s.y > s.mvy ? s.y - s.mvy : s.mvy - s.y;
        s.x = s.mvx;
        s.y = s.mvy;
        if (ax <= 1 && ay <= 1) {                       /* the minimum lies on the unit ring: one more unit ring round it */
            s.phase = MES_PHASE_LAST;
            return;
        }
        s.first = 0;                                    /* on the large ring: go on as TSS does */
        s.phase = MES_PHASE_MAIN;
        s.step >>= 1;
        s.done = s.step <= 0;
        return;
    }
    switch (s.method) {
    case FFHIP_ME_METHOD_DS:
    case FFHIP_ME_METHOD_HEXBS:
        if (!moved)
            s.phase = MES_PHASE_LAST;                   /* dia1 round the last centre */
        break;
    case FFHIP_ME_METHOD_NTSS:
        if (s.first) {
            s.phase = MES_PHASE_NTSS_UNIT;              /* round the same (x, y), not round the updated mv */
            return;
        }
        s.step >>= 1;
        s.done = s.step <= 0;
        break;
    case FFHIP_ME_METHOD_TSS:
        s.step >>= 1;
        s.done = s.step <= 0;
        break;
    default:                                            /* TDLS, FSS: halve only when the centre was kept */
        if (!moved)
            s.step >>= 1;
        s.done = s.step <= 0;
        break;
    }
    s.x = s.mvx;
    s.y = s.mvy;
}

/* the search of one block from the state mes_start() gave.  step_key(s, st) -> uint32_t: the step's ordered minimum, or MES_NO_KEY. */
template <class StepKey>
MES_FN void mes_run(MesState &s, const MesWindow &w, StepKey step_key)
{
    const uint32_t bound = mes_step_bound(w);
    for (uint32_t n = 0; !s.done && n < bound; n++) {
        const MesStep st = mes_step(s);
        mes_advance(s, st, w, step_key(s, st));
    }
}

/* ESA through the same two macros: the start, then the raster scan of the window with COST_MV.  cost(x, y) -> uint32_t. */
template <class Cost>
MES_FN void mes_search_esa(int x_mb, int y_mb, const MesWindow &w, Cost &cost, int &mvx, int &mvy, uint32_t &cost_min)
{
    mvx = x_mb;
    mvy = y_mb;
    cost_min = cost(x_mb, y_mb);
    if (!cost_min)
        return;
    for (int y = w.y_min; y <= w.y_max; y++)
        for (int x = w.x_min; x <= w.x_max; x++) {
            const uint32_t c = cost(x, y);
            if (c < cost_min) {
                cost_min = c;
                mvx = x;
                mvy = y;
            }
        }
}

#endif
