/*
 * me_search_pred_rules.h — the two predictive motion searches of the filter, EPZS and UMH (ff_me_search_epzs / ff_me_search_umh as
 * vf_mestimate drives them), as include/ffhip.h states them for ffhip_me_search_pred_batch_dev().  RESTATED, NOT CHECKED AGAINST THE
 * SOURCE: the rules were written down without the reference's source at hand; the statement in include/ffhip.h is the definition the
 * tests pin.  Tables, window and key are me_search_rules.h's.
 *
 * The header owns which neighbours a block has (mesp_neighbours) and which of their vectors are fetched (mesp_fetch_prev,
 * mesp_fetch_above), the predictor list made of them, the step machine of the phases and the loop over the steps, mesp_run().  It does
 * not own how a cost is computed or how a neighbour's vector arrives: k_me_search_pred (me_search_pred.hip, one wave per block row,
 * hand-off between the rows) and ffhip_me_search_pred_frames_host() (me_api.hip, raster order on the CPU) both fetch through the two
 * functions, call mesp_predictors(), mesp_start() and mesp_run(), and differ in the callbacks they hand them alone: how a block's
 * vector is read, and step_key, the minimum of mes_key(cost(x, y), i) over the i < 8 with mesp_candidate(s, w, P, s.pos + i, x, y),
 * MES_NO_KEY if there is none.
 *
 * Every phase is an ordered list of candidates round a centre that is fixed during the phase (the predictors round the block's origin;
 * the cross, the 5 x 5 raster, all rings together, one turn of a closing loop round the mv the phase found at its start).  Cutting
 * such a list into steps of at most 8 and taking, per step, the minimum of cost << 3 | index with a strict comparison against cost_min
 * equals applying COST_MV / COST_P_MV one by one — the argument me_search_rules.h makes for NTSS's 16 candidates.  The same argument
 * allows the costs of one list to be computed in ANY order as long as the minimum carries the list position: mesp_advance_list() takes
 * the minimum of mesp_list_key() (cost << 4 | position) over a whole predictor list, which the kernel evaluates in two passes, the
 * candidates that need nothing of the row above first.
 *
 * The d loops of UMH's cross and rings stop at the first d beyond which every candidate lies outside the window; the candidates left
 * out are all refused by COST_P_MV, so vectors, costs and cost counts are what the full loops give, for any search_param >= 0.
 */
#ifndef FFHIP_ME_SEARCH_PRED_RULES_H
#define FFHIP_ME_SEARCH_PRED_RULES_H

#include "me_search_rules.h"

/* hex4 = (-4,-2) (-4,-1) (-4,0) (-4,1) (-4,2) (4,-2) (4,-1) (4,0) (4,1) (4,2) (-2,3) (0,4) (2,3) (-2,-3) (0,-4) (2,-3); entry i in
 * nibble i, biased by 4 */
#define MESP_NIB(v, i) ((uint64_t)((v) + 4) << (4 * (i)))
#define MESP_TAB16(a, b, c, d, e, f, g, h, i, j, k, l, m, n, o, p)                                                                      \
    (MESP_NIB(a, 0) | MESP_NIB(b, 1) | MESP_NIB(c, 2) | MESP_NIB(d, 3) | MESP_NIB(e, 4) | MESP_NIB(f, 5) | MESP_NIB(g, 6) | MESP_NIB(h, 7) | \
     MESP_NIB(i, 8) | MESP_NIB(j, 9) | MESP_NIB(k, 10) | MESP_NIB(l, 11) | MESP_NIB(m, 12) | MESP_NIB(n, 13) | MESP_NIB(o, 14) | MESP_NIB(p, 15))
#define MESP_HEX4_DX MESP_TAB16(-4, -4, -4, -4, -4, 4, 4, 4, 4, 4, -2, 0, 2, -2, 0, 2)
#define MESP_HEX4_DY MESP_TAB16(-2, -1, 0, 1, 2, -2, -1, 0, 1, 2, 3, 4, 3, -3, -4, -3)
MES_FN int mesp_hex4_dx(int i) { return (int)((MESP_HEX4_DX >> (4 * i)) & 15u) - 4; }
MES_FN int mesp_hex4_dy(int i) { return (int)((MESP_HEX4_DY >> (4 * i)) & 15u) - 4; }

/* ---- the predictor list of a block ------------------------------------------------------------------------------------------------ */
/* the positions of the list, in the order the candidates are evaluated: the median, then P0 as appended, then P1 as appended.  An
 * entry the block does not have (no such neighbour) keeps its position and is never evaluated; duplicates stay. */
enum {
    MESP_MEDIAN = 0,
    MESP_ZERO = 1,      /* P0: (0, 0) */
    MESP_LEFT = 2,      /* P0: the left block of the current frame */
    MESP_TOP = 3,       /* P0: the top block */
    MESP_DIAG = 4,      /* P0: the top-right block; UMH in the last column: the top-left block */
    MESP_COLLOC = 5,    /* P0, EPZS: rel1(b), appended after the median was taken */
    MESP_ACCEL = 6,     /* P1, EPZS: 2 * rel1(b) - rel2(b) */
    MESP_PLEFT = 7,     /* P1: rel1 of the left, top, right, bottom neighbour */
    MESP_PTOP = 8,
    MESP_PRIGHT = 9,
    MESP_PBOTTOM = 10,
    MESP_NPRED = 11
};

struct MespVec {
    int x, y;
};

/* relative vectors, one per list position, and which positions exist */
struct MespPred {
    uint32_t have;
    MespVec median, left, top, diag, colloc, accel, pleft, ptop, pright, pbottom;
};

MES_FN int mesp_mid(int a, int b, int c)
{
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    return c < lo ? lo : c > hi ? hi : c;
}

/* a block's relative vector from the absolute position a field holds for it: position minus block origin, in 32 bits */
MES_FN MespVec mesp_rel(int px, int py, int bx, int by, int log2mb)
{
    MespVec v;
    v.x = px - (bx << log2mb);
    v.y = py - (by << log2mb);
    return v;
}

/* The neighbour rule: which list positions block (bx, by) of b_w x b_h has, and where its "diag" neighbour stands.  This is the one
 * place that looks at the block's position; whoever fetches a vector or builds the list tests a bit of `have`. */
struct MespNeigh {
    uint32_t have;      /* bit k: list position k exists */
    int diag_dx;        /* the diag neighbour is block (bx + diag_dx, by - 1): the top-right one, or, for UMH in the last column, the top-left */
};

MES_FN MespNeigh mesp_neighbours(int method, int bx, int by, int b_w, int b_h)
{
    const bool epzs = method == FFHIP_ME_METHOD_EPZS;
    const bool hl = bx > 0, ht = by > 0, hr = bx + 1 < b_w, hb = by + 1 < b_h;
    const bool hd = ht && (hr || (!epzs && hl));   /* the top-right block; UMH falls back on the top-left one */
    MespNeigh N;
    N.diag_dx = hr ? 1 : -1;
    N.have = 1u << MESP_MEDIAN | 1u << MESP_ZERO | (uint32_t)hl << MESP_LEFT | (uint32_t)ht << MESP_TOP | (uint32_t)hd << MESP_DIAG;
    if (epzs)                                       /* UMH takes nothing of the prev fields */
        N.have |= 1u << MESP_COLLOC | 1u << MESP_ACCEL | (uint32_t)hl << MESP_PLEFT | (uint32_t)ht << MESP_PTOP |
                  (uint32_t)hr << MESP_PRIGHT | (uint32_t)hb << MESP_PBOTTOM;
    return N;
}

MES_FN bool mesp_has(const MespNeigh &N, int k) { return N.have >> k & 1u; }

/* The vectors a block takes of its neighbours, all relative ones of the block they belong to; one of a neighbour the block does not
 * have stays zero and is not looked at. */
struct MespNear {
    MespVec left, top, diag;    /* of the current frame */
    MespVec c1, c2;             /* the collocated block's of prev1 and prev2 */
    MespVec pl, pt, pr, pb;     /* prev1's of the left, top, right, bottom neighbour */
};

/* The two fetch points: the prev fields, which nothing of the current frame writes, and the row above of the current frame (the
 * kernel waits for it in between).  prev(which, dbx, dby), above(dbx) -> MespVec: block (bx + dbx, by + dby)'s relative vector of
 * prev`which`, block (bx + dbx, by - 1)'s of the current frame.  `left` is the caller's: the block it searched last, if MESP_LEFT. */
template <class Prev>
MES_FN void mesp_fetch_prev(MespNear &v, const MespNeigh &N, Prev prev)
{
    if (mesp_has(N, MESP_COLLOC))
        v.c1 = prev(1, 0, 0);
    if (mesp_has(N, MESP_ACCEL))
        v.c2 = prev(2, 0, 0);
    if (mesp_has(N, MESP_PLEFT))
        v.pl = prev(1, -1, 0);
    if (mesp_has(N, MESP_PTOP))
        v.pt = prev(1, 0, -1);
    if (mesp_has(N, MESP_PRIGHT))
        v.pr = prev(1, 1, 0);
    if (mesp_has(N, MESP_PBOTTOM))
        v.pb = prev(1, 0, 1);
}

template <class Above>
MES_FN void mesp_fetch_above(MespNear &v, const MespNeigh &N, Above above)
{
    if (mesp_has(N, MESP_TOP))
        v.top = above(0);
    if (mesp_has(N, MESP_DIAG))
        v.diag = above(N.diag_dx);
}

/* the list of a block from its neighbours' vectors */
MES_FN MespPred mesp_predictors(const MespNeigh &N, const MespNear &v)
{
    const bool hl = mesp_has(N, MESP_LEFT), ht = mesp_has(N, MESP_TOP), hd = mesp_has(N, MESP_DIAG);
    MespPred P;
    P.have = N.have;
    P.left = v.left;
    P.top = v.top;
    P.diag = v.diag;
    /* the median of P0 as it stands: (0, 0) and what of left, top, diag the block has, in that order */
    const int n = 1 + hl + ht + hd;
    MespVec a, b;                                   /* P0[1], P0[2] */
    a = hl ? v.left : v.top;                        /* without left, top comes first (a diag implies a top) */
    b = hl ? (ht ? v.top : v.left) : v.diag;
    if (n == 4) {
        P.median.x = mesp_mid(v.left.x, v.top.x, v.diag.x);
        P.median.y = mesp_mid(v.left.y, v.top.y, v.diag.y);
    } else if (n == 3) {
        P.median.x = mesp_mid(0, a.x, b.x);
        P.median.y = mesp_mid(0, a.y, b.y);
    } else if (n == 2) {
        P.median = a;
    } else {
        P.median.x = P.median.y = 0;
    }
    P.colloc = v.c1;
    P.accel.x = 2 * v.c1.x - v.c2.x;
    P.accel.y = 2 * v.c1.y - v.c2.y;
    P.pleft = v.pl;
    P.ptop = v.pt;
    P.pright = v.pr;
    P.pbottom = v.pb;
    return P;
}

/* the relative vector at list position k < MESP_NPRED (a chain of selects: k may differ from lane to lane) */
MES_FN MespVec mesp_pred_vec(const MespPred &P, int k)
{
    MespVec v;
    v.x = v.y = 0;                                  /* MESP_ZERO */
    v = k == MESP_MEDIAN ? P.median : v;
    v = k == MESP_LEFT ? P.left : v;
    v = k == MESP_TOP ? P.top : v;
    v = k == MESP_DIAG ? P.diag : v;
    v = k == MESP_COLLOC ? P.colloc : v;
    v = k == MESP_ACCEL ? P.accel : v;
    v = k == MESP_PLEFT ? P.pleft : v;
    v = k == MESP_PTOP ? P.ptop : v;
    v = k == MESP_PRIGHT ? P.pright : v;
    v = k == MESP_PBOTTOM ? P.pbottom : v;
    return v;
}

/* ---- the state of one block's search ------------------------------------------------------------------------------------------- */
enum {
    MESP_PHASE_PRED = 0,      /* the median, P0, P1 round the block's origin */
    MESP_PHASE_DIA_LOOP = 1,  /* EPZS: do { dia1 round mv } while (mv moved) */
    MESP_PHASE_CROSS = 2,     /* UMH: the cross round mv */
    MESP_PHASE_RASTER = 3,    /* UMH: the 5 x 5 raster round mv as it is after the cross */
    MESP_PHASE_RINGS = 4,     /* UMH: hex4[1 .. 15] * d, d = 1 .. R / 4, all round one mv */
    MESP_PHASE_HEX_LOOP = 5,  /* UMH: do { hex2 round mv } while (mv moved) */
    MESP_PHASE_LAST = 6,      /* UMH: dia1 round the last centre */
    MESP_PHASE_END = 7
};

#define MESP_NO_COST 0xFFFFFFFFu    /* cost_min "none yet": every cost is below it */

struct MespState {
    int method, phase, done, R;
    int pos, n;         /* the list position of the step's first candidate, the length of the phase's list */
    int x, y;           /* the centre of the phase */
    int mvx, mvy;       /* mv: the best position so far */
    uint32_t cost_min;  /* its cost */
};

/* the largest distance from the centre to a side of the window; the centre lies in the window */
MES_FN int mesp_extent(const MespState &s, const MesWindow &w)
{
    const int ex = s.x - w.x_min > w.x_max - s.x ? s.x - w.x_min : w.x_max - s.x;
    const int ey = s.y - w.y_min > w.y_max - s.y ? s.y - w.y_min : w.y_max - s.y;
    return ex > ey ? ex : ey;
}

/* enters `phase`, or the first one after it whose list is not empty, round the current mv */
MES_FN void mesp_enter(MespState &s, const MesWindow &w, int phase)
{
    s.pos = 0;
    s.x = s.mvx;
    s.y = s.mvy;
    for (;; phase++) {
        const int ext = mesp_extent(s, w);
        int n;
        switch (phase) {
        case MESP_PHASE_DIA_LOOP:
        case MESP_PHASE_LAST:
            n = 4;
            break;
        case MESP_PHASE_CROSS:                      /* d = 1, 3, .. <= R; beyond the extent every arm has left the window */
            n = 4 * (((s.R < ext ? s.R : ext) + 1) >> 1);
            break;
        case MESP_PHASE_RASTER:
            n = 25;
            break;
        case MESP_PHASE_RINGS:                      /* every entry of hex4 has a component of at least 3 */
            n = 15 * ((s.R >> 2) < ext / 3 ? (s.R >> 2) : ext / 3);
            break;
        case MESP_PHASE_HEX_LOOP:
            n = 6;
            break;
        default:
            n = 0;
            break;
        }
        if (n > 0 || phase >= MESP_PHASE_END) {
            s.phase = phase;
            s.n = n;
            s.done = phase >= MESP_PHASE_END;
            return;
        }
    }
}

/* the common start: mv = (x_mb, y_mb), no cost yet, the predictors first */
MES_FN MespState mesp_start(int method, int x_mb, int y_mb, int R)
{
    MespState s;
    s.method = method;
    s.phase = MESP_PHASE_PRED;
    s.done = 0;
    s.R = R;
    s.pos = 0;
    s.n = method == FFHIP_ME_METHOD_EPZS ? MESP_NPRED : MESP_COLLOC;
    s.x = s.mvx = x_mb;
    s.y = s.mvy = y_mb;
    s.cost_min = MESP_NO_COST;
    return s;
}

/* entry k of the phase's list: COST_P_MV's test.  false: no such entry, or outside the window; nothing is evaluated. */
MES_FN bool mesp_candidate(const MespState &s, const MesWindow &w, const MespPred &P, int k, int &x, int &y)
{
    int dx = 0, dy = 0;
    bool have = k >= 0 && k < s.n;
    k = have ? k : 0;
    switch (s.phase) {
    case MESP_PHASE_PRED: {
        const MespVec v = mesp_pred_vec(P, k);
        have = have && (P.have >> k & 1u);
        dx = v.x;
        dy = v.y;
        break;
    }
    case MESP_PHASE_DIA_LOOP:
    case MESP_PHASE_LAST:
        dx = mes_pattern_dx(MES_DIA1, k);
        dy = mes_pattern_dy(MES_DIA1, k);
        break;
    case MESP_PHASE_HEX_LOOP:
        dx = mes_pattern_dx(MES_HEX2, k);
        dy = mes_pattern_dy(MES_HEX2, k);
        break;
    case MESP_PHASE_CROSS: {                        /* (x - d, y) (x + d, y), and while d <= R / 2: (x, y - d) (x, y + d) */
        const int d = 1 + 2 * (k >> 2), j = k & 3;
        have = have && (j < 2 || d <= (s.R >> 1));
        dx = j == 0 ? -d : j == 1 ? d : 0;
        dy = j == 2 ? -d : j == 3 ? d : 0;
        break;
    }
    case MESP_PHASE_RASTER:
        dy = k / 5 - 2;
        dx = k - 5 * (k / 5) - 2;
        break;
    case MESP_PHASE_RINGS: {
        const int d = 1 + k / 15, e = 1 + (k - 15 * (k / 15));
        dx = mesp_hex4_dx(e) * d;
        dy = mesp_hex4_dy(e) * d;
        break;
    }
    default:
        have = false;
        break;
    }
    x = s.x + dx;
    y = s.y + dy;
    return have && x >= w.x_min && x <= w.x_max && y >= w.y_min && y <= w.y_max;
}

/* the predictors take at most 2 steps, the cross at most 2^13 (an extent below 2^15), the raster 4, the rings at most 15 * 2^15 / 24;
 * a turn of a closing loop either ends it or moves mv to a position of the window it never held (cost_min falls strictly) */
MES_FN uint32_t mesp_step_bound(const MesWindow &w) { return mes_step_bound(w) + (1u << 13) + (1u << 15); }

/* the end of a phase's list */
MES_FN void mesp_phase_end(MespState &s, const MesWindow &w)
{
    const bool moved = s.mvx != s.x || s.mvy != s.y;
    switch (s.phase) {
    case MESP_PHASE_PRED:
        mesp_enter(s, w, s.method == FFHIP_ME_METHOD_EPZS ? MESP_PHASE_DIA_LOOP : MESP_PHASE_CROSS);
        break;
    case MESP_PHASE_DIA_LOOP:
        mesp_enter(s, w, moved ? MESP_PHASE_DIA_LOOP : MESP_PHASE_END);
        break;
    case MESP_PHASE_HEX_LOOP:
        mesp_enter(s, w, moved ? MESP_PHASE_HEX_LOOP : MESP_PHASE_LAST);
        break;
    case MESP_PHASE_LAST:
        mesp_enter(s, w, MESP_PHASE_END);
        break;
    default:                                        /* cross -> raster -> rings -> the hex2 loop */
        mesp_enter(s, w, s.phase + 1);
        break;
    }
}

/* the transition: `key` is the ordered minimum of the step's 8 list entries from s.pos on (MES_NO_KEY when all were refused) */
MES_FN void mesp_advance(MespState &s, const MesWindow &w, const MespPred &P, uint32_t key)
{
    if (key != MES_NO_KEY && (key >> 3) < s.cost_min) {
        s.cost_min = key >> 3;
        mesp_candidate(s, w, P, s.pos + (int)(key & 7u), s.mvx, s.mvy);
    }
    s.pos += 8;
    if (s.pos >= s.n)
        mesp_phase_end(s, w);
}

/* the search of one block from the state it is given: mesp_start()'s, or what mesp_advance_list() made of it.  step_key(s) ->
 * uint32_t: the ordered minimum of the step's 8 list entries from s.pos on, or MES_NO_KEY. */
template <class StepKey>
MES_FN void mesp_run(MespState &s, const MesWindow &w, const MespPred &P, StepKey step_key)
{
    const uint32_t bound = mesp_step_bound(w);
    for (uint32_t n = 0; !s.done && n < bound; n++)
        mesp_advance(s, w, P, step_key(s));
}

/* A whole list of at most 16 entries at once (the predictors): the minimum of mesp_list_key(cost, k) over the entries k evaluated,
 * in any order.  Equals the steps of 8 in order. */
MES_FN uint32_t mesp_list_key(uint32_t cost, int k) { return cost << 4 | (uint32_t)k; }
/* the key of cost + extra from the key of cost, for a cost whose second part is known later; MES_NO_KEY stays */
MES_FN uint32_t mesp_list_key_add(uint32_t key, uint32_t extra) { return key == MES_NO_KEY ? key : key + (extra << 4); }
MES_FN void mesp_advance_list(MespState &s, const MesWindow &w, const MespPred &P, uint32_t key)
{
    if (key != MES_NO_KEY && (key >> 4) < s.cost_min) {
        s.cost_min = key >> 4;
        mesp_candidate(s, w, P, (int)(key & 15u), s.mvx, s.mvy);
    }
    mesp_phase_end(s, w);
}

#endif
