/*
 * me_interp_rules.h — the motion-compensated interpolation of vf_minterpolate (mi_mode=mci, me_mode=bidir, mc_mode=obmc: the
 * overlapped-block accumulation of bidirectional_obmc() and the per-pixel weighted average of set_frame_data()), as include/ffhip.h
 * states it for ffhip_me_interp_sequence_dev().  RESTATED FROM MEMORY, NOT CHECKED AGAINST THE SOURCE: libavfilter/vf_minterpolate.c
 * was not at hand; the statement in include/ffhip.h is the definition the tests pin.
 *
 * The reference scatters: every block adds itself to the pixels its displaced window covers, in (direction, block row, block column)
 * order, and a pixel stops taking contributions at MEI_CAP.  This header is the same rule as a gather: a pixel walks, in that order,
 * the blocks that can reach it and keeps S, Wt and the count in registers; no list is stored.  It owns
 *   - mei_vector(), mei_block(): a block's relative vector, whether it is well formed, and its displaced, clipped window (steps 1 - 3);
 *   - mei_candidates(): the block rectangle that can reach a pixel rectangle under mv_range;
 *   - mei_contribute(): what one block adds to one pixel (steps 3 - 5), and mei_walk(), the ordered walk of one pixel with the
 *     empty-list fallback.
 *   - mei_block_bilat(), mei_walk_bilat(): the same for the bilateral compensation of ffhip_me_interp_bilat_sequence_dev(), whose one
 *     field of half-vectors does not shift the windows: at most four blocks at computed indices reach a pixel.
 * It does not own where a sample comes from: take(wa, dxa, dya, wb, dxb, dyb) is the caller's and receives one contribution, the
 * weight and the clipped displacement of its entry in picture A and of its entry in picture B.  ffhip_me_interp_sequence_host()
 * (me_api.hip) is mei_walk() in a plain loop over samples; k_me_interp (me_interp.hip) sorts the candidates of a wave out with a
 * ballot and calls mei_contribute() for the survivors, in the same order.
 */
#ifndef FFHIP_ME_INTERP_RULES_H
#define FFHIP_ME_INTERP_RULES_H

#include "me_search_rules.h"

#define MEI_CAP 16          /* contributions a pixel takes: the reference's nb + 1 >= NB_PIXEL_MVS with two entries per contribution */
#define MEI_MAX_RANGE 256   /* the largest mv_range a face accepts */

/* the slots of ffhip_me_interp_host_counts() */
enum { MEI_N_TAKEN, MEI_N_ZERO_WEIGHT, MEI_N_CAPPED, MEI_N_MALFORMED, MEI_N_FALLBACK, MEI_N_CLIPPED, MEI_N_SAMPLES, MEI_N_BLEND, MEI_NCOUNTS };

struct MeiGeom {
    int W, H;       /* luma size */
    int lg, mb;     /* log2 of the block size, the block size */
    int bw, bh;     /* blocks of a field */
    int range;      /* mv_range */
};

MES_FN MeiGeom mei_geom(int width, int height, int mb_size, int mv_range)
{
    MeiGeom g;
    g.W = width;
    g.H = height;
    g.lg = mb_size == 16 ? 4 : 3;
    g.mb = mb_size;
    g.bw = width >> g.lg;
    g.bh = height >> g.lg;
    g.range = mv_range;
    return g;
}

MES_FN int mei_tdiv(int n) { return n / 1024; }                                           /* C division: towards zero */
MES_FN int mei_tshift(int d, int s) { return (d + ((d >> 31) & ((1 << s) - 1))) >> s; }  /* d / (1 << s), towards zero */
MES_FN int mei_clip(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

/* is luma column (row) x the site of a chroma column (row) under shift s, the last writer of the reference's walk?  The column is
 * then x >> s. */
MES_FN bool mei_site(int x, int s, int size) { return !((x + 1) & ((1 << s) - 1)) || x == size - 1; }

/* step 1: the relative vector of block (bx, by) whose field entry is the absolute position (X, Y); false: malformed */
MES_FN bool mei_vector(const MeiGeom &g, int bx, int by, int X, int Y, int &vx, int &vy)
{
    vx = X - (bx << g.lg);
    vy = Y - (by << g.lg);
    return vx >= -g.range && vx <= g.range && vy >= -g.range && vy <= g.range;
}

/* a block's window: origin (sx, sy) of the 2 mb x 2 mb table, the pixels [x0, x1) x [y0, y1) it covers, and its vector */
struct MeiBlock {
    int sx, sy, x0, x1, y0, y1, vx, vy;
};
MES_FN MeiBlock mei_no_block(void)
{
    const MeiBlock b = { 0, 0, 0, 0, 0, 0, 0, 0 };
    return b;
}
/* steps 2 and 3 for a well-formed vector.  Column W - 1 and row H - 1 are never covered: that is the reference's clip */
MES_FN MeiBlock mei_block(const MeiGeom &g, int alpha, int dir, int bx, int by, int vx, int vy)
{
    const int a = dir ? alpha : 1024 - alpha;
    MeiBlock b;
    b.sx = (bx << g.lg) - g.mb / 2 + mei_tdiv(vx * a);
    b.sy = (by << g.lg) - g.mb / 2 + mei_tdiv(vy * a);
    b.x0 = mei_clip(b.sx, 0, g.W - 1);
    b.x1 = mei_clip(b.sx + 2 * g.mb, 0, g.W - 1);
    b.y0 = mei_clip(b.sy, 0, g.H - 1);
    b.y1 = mei_clip(b.sy + 2 * g.mb, 0, g.H - 1);
    b.vx = vx;
    b.vy = vy;
    return b;
}

/* The bilateral compensation (me_mode=bilat: the filter's bilateral_obmc, as include/ffhip.h states it for
 * ffhip_me_interp_bilat_sequence_dev()) takes ONE field of half-vectors.  A well-formed block's window is not shifted by its vector,
 * and its contribution is step 5 of the rule above read with m = 2 * v: the block is given to mei_contribute() as a direction-0 block
 * whose vector is m.  Windows of 2 mb stand mb apart, so at most two blocks per axis, four in all, reach a pixel — mei_bilat_first()
 * and the one after it per axis — and the cap of MEI_CAP never binds. */
MES_FN MeiBlock mei_block_bilat(const MeiGeom &g, int bx, int by, int vx, int vy)
{
    MeiBlock b = mei_block(g, 0, 0, bx, by, 0, 0);      /* no displacement: sx = (bx << lg) - mb / 2 */
    b.vx = 2 * vx;
    b.vy = 2 * vy;
    return b;
}
/* the first of the two block columns (rows) whose unshifted window [b * mb - mb / 2, b * mb + 3 * mb / 2) holds column (row) x; it
 * may be -1, and the second may be b_w (b_h): neither is a block then */
MES_FN int mei_bilat_first(const MeiGeom &g, int x) { return ((x + g.mb / 2) >> g.lg) - 1; }

/* The blocks [bx0, bx1) x [by0, by1) that can reach a pixel of [px0, px1) x [py0, py1).  |tdiv(v * a)| <= mv_range, so block bx covers
 * only columns of [bx * mb - mb / 2 - range, bx * mb + 3 * mb / 2 + range): it reaches the rectangle only if
 * bx * mb <= px1 - 1 + mb / 2 + range and bx * mb > px0 - 3 * mb / 2 - range.  (>> of a negative int floors.) */
struct MeiRange {
    int bx0, bx1, by0, by1;
};
MES_FN MeiRange mei_candidates(const MeiGeom &g, int px0, int px1, int py0, int py1)
{
    MeiRange r;
    r.bx0 = mei_clip(((px0 - 3 * g.mb / 2 - g.range) >> g.lg) + 1, 0, g.bw);
    r.bx1 = mei_clip(((px1 - 1 + g.mb / 2 + g.range) >> g.lg) + 1, r.bx0, g.bw);
    r.by0 = mei_clip(((py0 - 3 * g.mb / 2 - g.range) >> g.lg) + 1, 0, g.bh);
    r.by1 = mei_clip(((py1 - 1 + g.mb / 2 + g.range) >> g.lg) + 1, r.by0, g.bh);
    return r;
}
/* the most blocks per axis mei_candidates() returns for a rectangle `span` pixels long: floor(a / mb) - floor(b / mb) is at most
 * (a - b) / mb + 1, and a - b = span - 1 + 2 * mb + 2 * range */
MES_FN int mei_max_candidates(const MeiGeom &g, int span) { return (span - 1 + 2 * g.mb + 2 * g.range) / g.mb + 1; }

/* steps 3 to 5: what block `b` of direction `dir` adds to luma pixel (x, y), which holds n contributions so far.  cnt: the host
 * face's counters, or NULL */
template <class Take>
MES_FN void mei_contribute(const MeiGeom &g, int alpha, const MeiBlock &b, int dir, int x, int y, const uint8_t *window, int &n, Take &&take,
                           uint64_t *cnt)
{
    if (x < b.x0 || x >= b.x1 || y < b.y0 || y >= b.y1)
        return;
    const int w = window[(x - b.sx) + ((y - b.sy) << (g.lg + 1))];
    if (!w) {
        if (cnt)
            cnt[MEI_N_ZERO_WEIGHT]++;
        return;
    }
    if (n >= MEI_CAP) {
        if (cnt)
            cnt[MEI_N_CAPPED]++;
        return;
    }
    n++;
    const int mx = dir ? -b.vx : b.vx, my = dir ? -b.vy : b.vy;
    const int ax = mei_tdiv(mx * alpha), ay = mei_tdiv(my * alpha);
    const int ex = mei_tdiv(-mx * (1024 - alpha)), ey = mei_tdiv(-my * (1024 - alpha));
    const int dxa = mei_clip(ax, -x, g.W - 1 - x), dya = mei_clip(ay, -y, g.H - 1 - y);
    const int dxb = mei_clip(ex, -x, g.W - 1 - x), dyb = mei_clip(ey, -y, g.H - 1 - y);
    if (cnt) {
        cnt[MEI_N_TAKEN]++;
        cnt[MEI_N_CLIPPED] += (uint64_t)(dxa != ax || dya != ay) + (uint64_t)(dxb != ex || dyb != ey);
    }
    take(w * (1024 - alpha), dxa, dya, w * alpha, dxb, dyb);
}

/* The walk of luma pixel (x, y): the candidates in (dir, by, bx) order, then the fallback for an empty list.  block(dir, bx, by) gives
 * the block's window, mei_no_block() for a malformed one.  Returns the contributions taken. */
template <class Block, class Take>
MES_FN int mei_walk(const MeiGeom &g, int alpha, int x, int y, const uint8_t *window, Block &&block, Take &&take, uint64_t *cnt)
{
    const MeiRange r = mei_candidates(g, x, x + 1, y, y + 1);
    int n = 0;
    for (int dir = 0; dir < 2; dir++)
        for (int by = r.by0; by < r.by1; by++)
            for (int bx = r.bx0; bx < r.bx1; bx++)
                mei_contribute(g, alpha, block(dir, bx, by), dir, x, y, window, n, take, cnt);
    if (!n) {
        if (cnt)
            cnt[MEI_N_FALLBACK]++;
        take(1024 - alpha, 0, 0, alpha, 0, 0);
    }
    return n;
}

/* The bilateral walk of luma pixel (x, y): the at most four blocks in (by, bx) order, then the fallback.  block(bx, by) gives the
 * block's window (mei_block_bilat()), mei_no_block() for a malformed one. */
template <class Block, class Take>
MES_FN int mei_walk_bilat(const MeiGeom &g, int alpha, int x, int y, const uint8_t *window, Block &&block, Take &&take, uint64_t *cnt)
{
    const int bx0 = mei_bilat_first(g, x), by0 = mei_bilat_first(g, y);
    int n = 0;
    for (int by = by0; by < by0 + 2; by++)
        for (int bx = bx0; bx < bx0 + 2; bx++)
            if (bx >= 0 && bx < g.bw && by >= 0 && by < g.bh)
                mei_contribute(g, alpha, block(bx, by), 0, x, y, window, n, take, cnt);
    if (!n) {
        if (cnt)
            cnt[MEI_N_FALLBACK]++;
        take(1024 - alpha, 0, 0, alpha, 0, 0);
    }
    return n;
}

/* A sample from its sums.  Wt = 1024 * (the sum of the window weights taken), at most 1024 * 16 * 255 < 2^22, or 1024 on the
 * fallback: never 0.  S <= 255 * Wt < 2^30.  The definition says 64 bits; 32 hold every value, S + (Wt >> 1) included. */
MES_FN uint32_t mei_sample(uint32_t S, uint32_t Wt) { return (S + (Wt >> 1)) / Wt; }
MES_FN uint32_t mei_blend(int a, int b, int alpha) { return (uint32_t)(alpha * b + (1024 - alpha) * a + 512) >> 10; }

/* ffhip_me_interp_sequence_scd_dev(): the weight of picture B in the streaming pass of a job.  A flagged pair (`cut`) under
 * FFHIP_ME_SCENE_DUP copies picture A when alpha <= 512 and picture B otherwise: mei_blend() at 0 is A and at 1024 is B, exactly */
MES_FN int mei_scene_alpha(bool cut, int scene_action, int alpha) { return cut && scene_action == FFHIP_ME_SCENE_DUP ? (alpha <= 512 ? 0 : 1024) : alpha; }

#endif
