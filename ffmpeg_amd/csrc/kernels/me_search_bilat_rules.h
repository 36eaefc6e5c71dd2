/*
 * me_search_bilat_rules.h — the cost of the filter's bilateral motion estimation (vf_minterpolate's me_mode=bilat, get_sbad_ob), as
 * include/ffhip.h states it for ffhip_me_search_bilat_batch_dev().  RESTATED FROM MEMORY, NOT CHECKED against
 * libavfilter/vf_minterpolate.c, which was not at hand; the statement in include/ffhip.h is the definition the tests pin.
 *
 * The search itself — predictor lists, median, phases, window, COST_MV / COST_P_MV — is me_search_pred_rules.h's, unchanged.  This
 * header owns what differs: where a candidate (X, Y) of the block at (x_mb, y_mb) places the two overlapped windows of 2 mb x 2 mb
 * samples (mesb_place), and the penalty round the block's median predictor (mesb_penalty).  It does not own how the sum of absolute
 * differences over the two windows is computed: mes_cost_bilat() (me_search_cost.h, eight lanes per candidate) and the host faces of
 * me_api.hip (plain loops) both call the two functions.
 *
 * Reads stay inside the plane: with lo = min + h <= hi = max - h the centre c lies in [lo, hi] and |d| <= r = min(c - lo, hi - c), so
 * both c + d - h >= min >= 0 and c + d + 3 h - 1 <= max + mb - 1 <= ((b - 1) << log2mb) + mb - 1, the last sample of the last whole
 * block.  lo <= hi is max - min >= mb, which the window gives every block when search_param >= mb_size and the picture has two block
 * columns and two block rows; the faces refuse everything else, so no caller of these functions can make the inequality fail.
 */
#ifndef FFHIP_ME_SEARCH_BILAT_RULES_H
#define FFHIP_ME_SEARCH_BILAT_RULES_H

#include "me_search_rules.h"

MES_FN int mesb_clip(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

/* one axis: the block's origin o, the candidate's position p, the window [w_min, w_max], h = mb / 2.  -> the first sample of picture
 * A's window (c + d - h) and of picture B's (c - d - h) */
MES_FN void mesb_place_axis(int o, int p, int w_min, int w_max, int h, int &a0, int &b0)
{
    const int lo = w_min + h, hi = w_max - h;
    const int c = mesb_clip(o, lo, hi);
    const int r = c - lo < hi - c ? c - lo : hi - c;
    const int d = mesb_clip(p - c, -r, r);
    a0 = c + d - h;
    b0 = c - d - h;
}

/* the top-left samples of the two 2 mb x 2 mb windows of candidate (X, Y): A is sampled at +v, B at -v */
struct MesbPlace {
    int ax, ay, bx, by;
};

MES_FN MesbPlace mesb_place(const MesWindow &w, int x_mb, int y_mb, int mb, int X, int Y)
{
    MesbPlace p;
    mesb_place_axis(x_mb, X, w.x_min, w.x_max, mb >> 1, p.ax, p.bx);
    mesb_place_axis(y_mb, Y, w.y_min, w.y_max, mb >> 1, p.ay, p.by);
    return p;
}

/* 64 * (|X - x_mb - pred.x| + |Y - y_mb - pred.y|): below 2^24 for positions and predictors of a picture of at most 32768, so
 * sbad (below 2^18) + penalty leaves the ordered minimum's 4 index bits free */
MES_FN uint32_t mesb_penalty(int X, int Y, int x_mb, int y_mb, int pred_x, int pred_y)
{
    const int ex = X - x_mb - pred_x, ey = Y - y_mb - pred_y;
    return 64u * ((uint32_t)(ex < 0 ? -ex : ex) + (uint32_t)(ey < 0 ? -ey : ey));
}

#endif
