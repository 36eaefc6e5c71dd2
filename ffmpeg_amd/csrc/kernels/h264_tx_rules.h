/*
 * h264_tx_rules.h — the arithmetic of the H.264 residual, once: the 4x4 and 8x8 inverse transforms, the *_dc_add value and the luma,
 * chroma and 4:2:2 chroma DC dequantisers of libavcodec/h264idct_template.c, on values held as ints.  The coefficient type CF
 * (int16_t at 8 bits, int32_t above: dctcoef of bit_depth_template.c) is the type the reference stores its intermediates in:
 * block[0] += 32 and the results of a first pass wrap to CF, all sums are modulo 2^32, shifts are arithmetic.
 *
 * Shared by the batch and dispatcher kernels of h264_idct.hip and h264_hbd.hip, the residual pictures (h264_res_rules.h: kernel and
 * host face) and the intra wavefronts (h264_intra_mb.h: kernels and host emulation).  Reading, clearing, dispatching and the add to
 * the samples stay with the callers; where a caller spreads one block over lanes it keeps a per-lane form written over the pieces here.
 */
#ifndef FFHIP_H264_TX_RULES_H
#define FFHIP_H264_TX_RULES_H

#include <stdint.h>

#if defined(__HIPCC__)
#define H264TX_FN __host__ __device__ __forceinline__
#else
#define H264TX_FN static inline
#endif

/* dctcoef for samples of type PIX */
template <typename PIX> struct H264Coef { typedef int16_t T; };
template <> struct H264Coef<uint16_t> { typedef int32_t T; };

/* av_clip_pixel: maxv = (1 << bit_depth) - 1 */
H264TX_FN int h264tx_clip(int v, int maxv) { return v < 0 ? 0 : v > maxv ? maxv : v; }

/* what *_dc_add puts on every sample of a block (h264idct_template.c:145-175).  The sum is an int's, where the transforms add the 32
 * in CF: at 8 bits a DC of 32736 .. 32767 wraps there and not here, the one place where the reference's two forms differ */
H264TX_FN int h264tx_dc(int c0) { return (int)((uint32_t)c0 + 32u) >> 6; }

/* is a block nothing but its DC?  (A block of zeros is flat too: both forms add 0.) */
template <int N>
H264TX_FN bool h264tx_flat(const int (&v)[N])
{
    int ac = 0;
#pragma unroll
    for (int i = 1; i < N; i++)
        ac |= v[i];
    return !ac;
}

/* the 4-point butterfly of idct_add (h264idct_template.c:39-64) on in[0], in[S], in[2 * S], in[3 * S]:
 * o[] = { e0 + o1, e1 + o0, e1 - o0, e0 - o1 } >> SH */
template <int S, int SH>
H264TX_FN void h264tx_bfly4(const int *in, int (&o)[4])
{
    const uint32_t e0 = (uint32_t)in[0] + (uint32_t)in[2 * S], e1 = (uint32_t)in[0] - (uint32_t)in[2 * S];
    const uint32_t o0 = (uint32_t)(in[S] >> 1) - (uint32_t)in[3 * S], o1 = (uint32_t)in[S] + (uint32_t)(in[3 * S] >> 1);
    o[0] = (int)(e0 + o1) >> SH;
    o[1] = (int)(e1 + o0) >> SH;
    o[2] = (int)(e1 - o0) >> SH;
    o[3] = (int)(e0 - o1) >> SH;
}
/* its output k alone, for a lane that keeps one (the column-per-lane forms of h264_intra_mb.h).  The four sums are said again rather
 * than picked out of o[]: picked, all four are summed ahead of the selects, and the intra wavefronts spill two more scalar registers.
 * The two forms state one rule: a change to either is a change to both */
H264TX_FN int h264tx_bfly4(int k, int s0, int s1, int s2, int s3)
{
    const uint32_t e0 = (uint32_t)s0 + (uint32_t)s2, e1 = (uint32_t)s0 - (uint32_t)s2;
    const uint32_t o0 = (uint32_t)(s1 >> 1) - (uint32_t)s3, o1 = (uint32_t)s1 + (uint32_t)(s3 >> 1);
    return (int)(k == 0 ? e0 + o1 : k == 1 ? e1 + o0 : k == 2 ? e1 - o0 : e0 - o1);
}

/* idct_add (h264idct_template.c:33-67) on v[] = block[0 .. 15]: on return v[4 * i + k] is what is added to the sample of row k, column i */
template <class CF>
H264TX_FN void h264tx_idct4(int (&v)[16])
{
    v[0] = (CF)((uint32_t)v[0] + 32u);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        int o[4];
        h264tx_bfly4<4, 0>(v + i, o);
#pragma unroll
        for (int k = 0; k < 4; k++)
            v[i + 4 * k] = (CF)o[k];
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        int o[4];
        h264tx_bfly4<1, 6>(v + 4 * i, o);
#pragma unroll
        for (int k = 0; k < 4; k++)
            v[4 * i + k] = o[k];
    }
}

/* one 8-point pass of idct8_add (h264idct_template.c:69-143) on in[0], in[S], .. in[7 * S]; the results modulo 2^32 */
template <int S>
H264TX_FN void h264tx_idct8_1d(const int *in, uint32_t (&out)[8])
{
    const uint32_t a0 = (uint32_t)in[0] + (uint32_t)in[4 * S], a2 = (uint32_t)in[0] - (uint32_t)in[4 * S];
    const uint32_t a4 = (uint32_t)(in[2 * S] >> 1) - (uint32_t)in[6 * S], a6 = (uint32_t)(in[6 * S] >> 1) + (uint32_t)in[2 * S];
    const uint32_t b0 = a0 + a6, b2 = a2 + a4, b4 = a2 - a4, b6 = a0 - a6;
    const int a1 = (int)(-(uint32_t)in[3 * S] + (uint32_t)in[5 * S] - (uint32_t)in[7 * S] - (uint32_t)(in[7 * S] >> 1));
    const int a3 = (int)((uint32_t)in[S] + (uint32_t)in[7 * S] - (uint32_t)in[3 * S] - (uint32_t)(in[3 * S] >> 1));
    const int a5 = (int)(-(uint32_t)in[S] + (uint32_t)in[7 * S] + (uint32_t)in[5 * S] + (uint32_t)(in[5 * S] >> 1));
    const int a7 = (int)((uint32_t)in[3 * S] + (uint32_t)in[5 * S] + (uint32_t)in[S] + (uint32_t)(in[S] >> 1));
    const uint32_t b1 = (uint32_t)(a7 >> 2) + (uint32_t)a1, b3 = (uint32_t)a3 + (uint32_t)(a5 >> 2);
    const uint32_t b5 = (uint32_t)(a3 >> 2) - (uint32_t)a5, b7 = (uint32_t)a7 - (uint32_t)(a1 >> 2);
    out[0] = b0 + b7; out[7] = b0 - b7; out[1] = b2 + b5; out[6] = b2 - b5;
    out[2] = b4 + b3; out[5] = b4 - b3; out[3] = b6 + b1; out[4] = b6 - b1;
}

/* the first half of idct8_add on v[] = block[0 .. 63]: block[0] += 32 and the first pass, both stored as CF.  h264tx_idct8_1d<1> on
 * v + 8 * i, >> 6, is then column i: a caller that adds the columns to the samples as they come need not hold all 64 results */
template <class CF>
H264TX_FN void h264tx_idct8_first(int (&v)[64])
{
    v[0] = (CF)((uint32_t)v[0] + 32u);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint32_t o[8];
        h264tx_idct8_1d<8>(v + i, o);
#pragma unroll
        for (int k = 0; k < 8; k++)
            v[i + 8 * k] = (CF)o[k];
    }
}

/* idct8_add on v[] = block[0 .. 63]: on return v[8 * i + k] is what is added to the sample of row k, column i */
template <class CF>
H264TX_FN void h264tx_idct8(int (&v)[64])
{
    h264tx_idct8_first<CF>(v);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint32_t o[8];
        h264tx_idct8_1d<1>(v + 8 * i, o);
#pragma unroll
        for (int k = 0; k < 8; k++)
            v[8 * i + k] = (int)o[k] >> 6;
    }
}

/* luma_dc_dequant_idct (h264idct_template.c:259-293) on dc[] = input[0 .. 15]: on return dc[4 * i + k] is the value of
 * output[16 * {0, 1, 4, 5}[k] + x_offset[i]], x_offset = { 0, 32, 128, 160 }: of luma block {0, 1, 4, 5}[k] + {0, 2, 8, 10}[i] */
template <class CF>
H264TX_FN void h264tx_luma_dc(int (&dc)[16], int32_t qmul)
{
    const uint32_t q = (uint32_t)qmul;
    uint32_t t[16];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t z0 = (uint32_t)dc[4 * i] + (uint32_t)dc[4 * i + 1], z1 = (uint32_t)dc[4 * i] - (uint32_t)dc[4 * i + 1];
        const uint32_t z2 = (uint32_t)dc[4 * i + 2] - (uint32_t)dc[4 * i + 3], z3 = (uint32_t)dc[4 * i + 2] + (uint32_t)dc[4 * i + 3];
        t[4 * i] = z0 + z3; t[4 * i + 1] = z0 - z3; t[4 * i + 2] = z1 - z2; t[4 * i + 3] = z1 + z2;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t z0 = t[i] + t[8 + i], z1 = t[i] - t[8 + i], z2 = t[4 + i] - t[12 + i], z3 = t[4 + i] + t[12 + i];
        dc[4 * i] = (CF)((int)((z0 + z3) * q + 128u) >> 8);
        dc[4 * i + 1] = (CF)((int)((z1 + z2) * q + 128u) >> 8);
        dc[4 * i + 2] = (CF)((int)((z1 - z2) * q + 128u) >> 8);
        dc[4 * i + 3] = (CF)((int)((z0 - z3) * q + 128u) >> 8);
    }
}

/* chroma_dc_dequant_idct (h264idct_template.c:323-345) on the first coefficients dc[j] of a plane's four blocks, as the reference
 * stores them back */
template <class CF>
H264TX_FN void h264tx_chroma_dc(int (&dc)[4], int32_t qmul)
{
    const uint32_t q = (uint32_t)qmul;
    uint32_t a = (uint32_t)dc[0], b = (uint32_t)dc[1], c = (uint32_t)dc[2], d = (uint32_t)dc[3];
    const uint32_t e = a - b;
    a = a + b;
    b = c - d;
    c = c + d;
    dc[0] = (CF)((int)((a + c) * q) >> 7);
    dc[1] = (CF)((int)((e + b) * q) >> 7);
    dc[2] = (CF)((int)((a - c) * q) >> 7);
    dc[3] = (CF)((int)((e - b) * q) >> 7);
}

/* chroma422_dc_dequant_idct (h264idct_template.c:295-321) on the first coefficients dc[j] of a plane's eight blocks (block j = row
 * j >> 1, column j & 1 of the 4 x 2 DC array), as the reference stores them back */
template <class CF>
H264TX_FN void h264tx_chroma422_dc(int (&dc)[8], int32_t qmul)
{
    const uint32_t q = (uint32_t)qmul;
    uint32_t t[8];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        t[2 * i] = (uint32_t)dc[2 * i] + (uint32_t)dc[2 * i + 1];
        t[2 * i + 1] = (uint32_t)dc[2 * i] - (uint32_t)dc[2 * i + 1];
    }
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const uint32_t z0 = t[i] + t[4 + i], z1 = t[i] - t[4 + i], z2 = t[2 + i] - t[6 + i], z3 = t[2 + i] + t[6 + i];
        dc[i] = (CF)((int)((z0 + z3) * q + 128u) >> 8);
        dc[2 + i] = (CF)((int)((z1 + z2) * q + 128u) >> 8);
        dc[4 + i] = (CF)((int)((z1 - z2) * q + 128u) >> 8);
        dc[6 + i] = (CF)((int)((z0 - z3) * q + 128u) >> 8);
    }
}

#endif
