/*
 * me_scene_rules.h — the scene-change score of vf_minterpolate's detect_scene_change() (scd=fdiff), as include/ffhip.h states it for
 * ffhip_me_scene_sequence_dev(): the whole-picture SAD of ff_scene_sad_get_fn(), the mean absolute frame difference, its difference to
 * the previous pair's, the clipped float score and the threshold.  RESTATED FROM MEMORY, NOT CHECKED AGAINST THE SOURCE:
 * libavfilter/vf_minterpolate.c and scene_sad.c were not at hand; the statement in include/ffhip.h is the definition the tests pin.
 *
 * One implementation for host and device.  It owns
 *   - mes_scene_sad_row(): the exact sum of |A - B| over one row of samples (the host face's loop; the kernel sums dwords instead and
 *     must give the same integer);
 *   - mes_scene_mafd(), mes_scene_score(), mes_scene_flag(): the arithmetic from the sum to the flag, every operation in the order of
 *     the rule text.  The library is built with -ffp-contract=off and without fast-math: +, *, / and the conversions of doubles and
 *     floats are IEEE operations on both sides, so the results are bit-identical;
 *   - mes_scene_walk(): the pairs of one sequence in order with the carried double.
 */
#ifndef FFHIP_ME_SCENE_RULES_H
#define FFHIP_ME_SCENE_RULES_H

#include "me_search_rules.h"

/* sum of |a - b| over n samples of T (uint8_t at depth 8, uint16_t holding the full 16-bit value above) */
template <class T>
MES_FN uint64_t mes_scene_sad_row(const T *a, const T *b, int n)
{
    uint64_t s = 0;
    for (int i = 0; i < n; i++)
        s += (uint64_t)(a[i] > b[i] ? a[i] - b[i] : b[i] - a[i]);
    return s;
}

/* mafd = (double)sad * 100.0 / (height * width) / (1 << depth): the int product, then the two divisions, in that order */
MES_FN double mes_scene_mafd(uint64_t sad, int width, int height, int depth)
{
    const double scaled = (double)sad * 100.0;
    const double per_sample = scaled / (double)(height * width);
    return per_sample / (double)(1 << depth);
}

/* score = av_clipf((float)FFMIN(mafd, diff), 0, 100) with diff = fabs(mafd - prev); the conversion to float is part of the rule */
MES_FN float mes_scene_score(double mafd, double prev)
{
    double diff = mafd - prev;
    if (diff < 0.0)
        diff = -diff;
    const float v = (float)(mafd > diff ? diff : mafd);
    return v < 0.0f ? 0.0f : v > 100.0f ? 100.0f : v;
}

MES_FN int mes_scene_flag(float score, double threshold) { return (double)score >= threshold; }

/* the `n` pairs of one sequence in order: sad(j) is pair j's sum, out(j, sad, score, flag) takes its results; returns the carry */
template <class Sad, class Out>
MES_FN double mes_scene_walk(int n, int width, int height, int depth, double threshold, double prev, Sad &&sad, Out &&out)
{
    for (int j = 0; j < n; j++) {
        const uint64_t s = sad(j);
        const double mafd = mes_scene_mafd(s, width, height, depth);
        const float score = mes_scene_score(mafd, prev);
        out(j, s, score, mes_scene_flag(score, threshold));
        prev = mafd;
    }
    return prev;
}

#endif
