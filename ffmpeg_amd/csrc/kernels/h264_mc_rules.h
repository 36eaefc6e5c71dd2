/*
 * h264_mc_rules.h — the sample arithmetic of H.264 motion compensation, once: the 6-tap lowpass and the quarter-pel positions of
 * libavcodec/h264qpel_template.c, the 1/8-pel bilinear of h264chroma_template.c and weight / biweight_h264_pixels of
 * h264dsp_template.c:30-100, per output sample, on ints, with the depth as an argument.
 *
 * Shared by the depth-generic batch kernels of h264_hbd.hip and the whole-picture kernel of h264_inter_pic.hip (all of it), by the
 * 8-bit kernels of h264_qpel.hip (the scalar tap, the position table, the packed average) and of h264_chroma.hip (the bilinear weights,
 * the packed average, weight / biweight).  Fetching, clamping of coordinates and storing stay with the callers: a caller hands the
 * statements a source, anything with `int at(int dx, int dy) const` that returns the reference sample (dx, dy) away from the output
 * sample.  h264_qpel.hip's packed and matrix-core forms (qp_tap6 on int16 pairs, the s23 * 20 - s14 * 5 + s05 lines of qp_block, the
 * 4096 + 512 accumulators of qm_block) are statements of the same filter for other data layouts, not copies of this one: they stay there.
 */
#ifndef FFHIP_H264_MC_RULES_H
#define FFHIP_H264_MC_RULES_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define H264MC_FN __host__ __device__ __forceinline__
#else
#define H264MC_FN static inline
#endif

/* the 6-tap lowpass (1, -5, 20, 20, -5, 1) of h264qpel_template.c:77-305, unrounded */
H264MC_FN int h264mc_tap6(int a, int b, int c, int d, int e, int f) { return (c + d) * 20 - (b + e) * 5 + (a + f); }
/* av_clip_pixel: maxv = (1 << bit_depth) - 1 */
H264MC_FN int h264mc_clip(int v, int maxv)
{
    v = v < 0 ? 0 : v;
    return v > maxv ? maxv : v;
}
/* rnd_avg: what a quarter position makes of its two planes, and what avg_ makes of the result and dst (op_avg, :461) */
H264MC_FN int h264mc_avg(int a, int b) { return (a + b + 1) >> 1; }
/* four 8-bit (a + b + 1) >> 1 at once: rnd_avg32 of libavcodec/rnd_avg.h */
H264MC_FN uint32_t h264mc_avg4(uint32_t a, uint32_t b) { return (a | b) - (((a ^ b) & 0xFEFEFEFEu) >> 1); }

/*
 * Which planes position (fx, fy), mcxy = fx + 4 * fy, combines (h264qpel_template.c:313-459): F the full sample, H / V the horizontal /
 * vertical half sample clip((tap6 + 16) >> 5), J the centre clip((tap6 along y of the UNROUNDED horizontal sums + 512) >> 10).  A
 * position is one plane or the rnd_avg of two:
 *      mcxy  0 1 2 3 | 4 5 6 7 | 8 9 10 11 | 12 13 14 15
 *      F     F F . F | F . . . | . . .  .  | F  .  .  .       one column right at 3 (fdx), one row down at 12 (fdy)
 *      H     . H H H | . H H H | . . .  .  | .  H  H  H       of the row below where fy == 3 (hrow1)
 *      V     . . . . | V V . V | V V .  V  | V  V  .  V       of the column to the right where fx == 3 (vcol1)
 *      J     . . . . | . . J . | . J J  J  | .  .  J  .
 */
struct H264McPos { bool useF, useH, useV, useJ, hrow1, vcol1; int fdx, fdy; };
H264MC_FN H264McPos h264mc_pos(int fx, int fy)
{
    const int mcxy = fx + 4 * fy;
    H264McPos p;
    p.useJ = (fx == 2 && fy != 0) || (fy == 2 && fx != 0);
    p.useV = fx != 2 && fy != 0;
    p.useH = fy != 2 && fx != 0;
    p.useF = (fx == 0 || fy == 0) && fx != 2 && fy != 2;
    p.hrow1 = fy == 3;
    p.vcol1 = fx == 3;
    p.fdx = mcxy == 3;
    p.fdy = mcxy == 12;
    return p;
}

/* the unrounded 6-tap sums along x / along y at (dx, dy) */
template <class Src>
H264MC_FN int h264mc_hsum(const Src &S, int dx, int dy)
{
    return h264mc_tap6(S.at(dx - 2, dy), S.at(dx - 1, dy), S.at(dx, dy), S.at(dx + 1, dy), S.at(dx + 2, dy), S.at(dx + 3, dy));
}
template <class Src>
H264MC_FN int h264mc_vsum(const Src &S, int dx, int dy)
{
    return h264mc_tap6(S.at(dx, dy - 2), S.at(dx, dy - 1), S.at(dx, dy), S.at(dx, dy + 1), S.at(dx, dy + 2), S.at(dx, dy + 3));
}

/* the planes of position p but J, which the caller hands over as j, and what the position makes of them */
template <class Src>
H264MC_FN int h264mc_planes(const Src &S, const H264McPos p, int j, int maxv)
{
    int sum = p.useJ ? j : 0;    /* of the one or two planes */
    if (p.useF)
        sum += S.at(p.fdx, p.fdy);
    if (p.useH)
        sum += h264mc_clip((h264mc_hsum(S, 0, p.hrow1) + 16) >> 5, maxv);
    if (p.useV)
        sum += h264mc_clip((h264mc_vsum(S, p.vcol1, 0) + 16) >> 5, maxv);
    return p.useF + p.useH + p.useV + p.useJ == 2 ? (sum + 1) >> 1 : sum;
}

/* put_h264_qpel*_mcXY for one sample, v = ...: J where the position has it, then the position's row of the table as a constant in
 * each of 16 cases, so that a lane's offsets into its source fold into its addresses.  (Taken from the table at run time they stay
 * live across the J plane: k_h264_inter_pic goes from 64 to 70 VGPRs, an occupancy step, and k_h264_qpel_hbd takes 8 % longer.)
 * A macro, because the kernels need the statement in their own bodies: behind a call, inlined or not, the compiler schedules the J plane
 * of k_h264_inter_pic into 69 VGPRs and k_h264_qpel_hbd takes 2.5 % longer than with its own switch.  h264mc_luma() below is this macro
 * and nothing more, for host code */
#define H264MC_POS(n) case n: v_ = h264mc_planes(S_, h264mc_pos(n & 3, n >> 2), j_, maxv_); break
#define H264MC_LUMA(v, S, fx, fy, maxv)                                                                                              \
    do {                                                                                                                             \
        const auto &S_ = (S);                                                                                                        \
        const int fx_ = (fx), fy_ = (fy), maxv_ = (maxv);                                                                            \
        int j_ = 0, v_ = 0;                                                                                                          \
        if (h264mc_pos(fx_, fy_).useJ) {   /* the vertical 6-tap over the unrounded horizontal sums of rows -2 .. 3 */               \
            int t_[6];                                                                                                               \
            _Pragma("unroll")                                                                                                        \
            for (int k_ = 0; k_ < 6; k_++)                                                                                           \
                t_[k_] = h264mc_hsum(S_, 0, k_ - 2);                                                                                 \
            j_ = h264mc_clip((h264mc_tap6(t_[0], t_[1], t_[2], t_[3], t_[4], t_[5]) + 512) >> 10, maxv_);                            \
        }                                                                                                                            \
        switch (fx_ + 4 * fy_) {                                                                                                     \
        H264MC_POS(0); H264MC_POS(1); H264MC_POS(2); H264MC_POS(3); H264MC_POS(4); H264MC_POS(5); H264MC_POS(6); H264MC_POS(7);      \
        H264MC_POS(8); H264MC_POS(9); H264MC_POS(10); H264MC_POS(11); H264MC_POS(12); H264MC_POS(13); H264MC_POS(14); H264MC_POS(15);\
        }                                                                                                                            \
        v = v_;                                                                                                                      \
    } while (0)
template <class Src>
H264MC_FN int h264mc_luma(const Src &S, int fx, int fy, int maxv)
{
    int v;
    H264MC_LUMA(v, S, fx, fy, maxv);
    return v;
}

/* the weights A, B, C, D of the bilinear (h264chroma_template.c:28-172) on the sample, its right neighbour, the one below, the one
 * below right; they sum to 64 */
struct H264McBilin { int a, b, c, d; };
H264MC_FN H264McBilin h264mc_chroma_weights(int ax, int ay)
{
    const H264McBilin w = { (8 - ax) * (8 - ay), ax * (8 - ay), (8 - ax) * ay, ax * ay };
    return w;
}
/* put_h264_chroma_mc* for one sample at the fraction (ax, ay) in eighths */
template <class Src>
H264MC_FN int h264mc_chroma(const Src &S, int ax, int ay)
{
    const H264McBilin w = h264mc_chroma_weights(ax, ay);
    int v = w.a * S.at(0, 0);
    if (w.b) v += w.b * S.at(1, 0);        /* the template never reads a neighbour whose weight is zero */
    if (w.c) v += w.c * S.at(0, 1);
    if (w.d) v += w.d * S.at(1, 1);
    return (v + 32) >> 6;
}

/* weight_h264_pixels / biweight_h264_pixels for one sample at depth bd (h264dsp_template.c:30-100); the offset o in 8-bit units.  The
 * *_offset helpers are the part that does not depend on the sample, for a caller that weights a row with one record */
H264MC_FN int h264mc_weight_offset(int bd, int ld, int o)
{
    int offset = (int)((unsigned)o << (ld + (bd - 8)));
    if (ld)
        offset += 1 << (ld - 1);
    return offset;
}
H264MC_FN int h264mc_biweight_offset(int bd, int ld, int o)
{
    const int offset = (int)((unsigned)o << (bd - 8));
    return (int)((unsigned)((offset + 1) | 1) << ld);
}
H264MC_FN int h264mc_weight(int p, int bd, int ld, int w, int o)
{
    return h264mc_clip((p * w + h264mc_weight_offset(bd, ld, o)) >> ld, (1 << bd) - 1);
}
H264MC_FN int h264mc_biweight(int p0, int p1, int bd, int ld, int w0, int w1, int o)
{
    return h264mc_clip((p1 * w1 + p0 * w0 + h264mc_biweight_offset(bd, ld, o)) >> (ld + 1), (1 << bd) - 1);
}

#endif /* FFHIP_H264_MC_RULES_H */
