/*
 * h264_res_rules.h — the residual of one H.264 inter macroblock (rules 1 to 9 of ffhip_h264_residual_pictures_dev as include/ffhip.h
 * states them), once: what a macroblock's records ask for (h264res_plan) and the arithmetic of one block, shared by the kernel of
 * h264_res_pic.hip and by ffhip_h264_residual_pictures_host() (shims_h264_res.hip), which runs it on the CPU.
 *
 * The arithmetic is the one of h264_idct.hip / h264_hbd.hip (h264idct_template.c:33-175, 323-345) on values held as ints, with the
 * coefficient type CF (int16_t at 8 bits, int32_t above) as the type the reference stores its intermediates in: block[0] += 32 and
 * the results of the first pass wrap to CF, all sums are modulo 2^32, shifts are arithmetic.  Those kernels read, clear and dispatch
 * by lists; here the coefficients are never written, so the transforms are restated on registers rather than shared with them.
 */
#ifndef FFHIP_H264_RES_RULES_H
#define FFHIP_H264_RES_RULES_H

#include <stdint.h>

#include "ffhip.h"

#if defined(__HIPCC__)
#define H264RES_FN __host__ __device__ __forceinline__
#else
#define H264RES_FN static inline
#endif

/* what macroblock m asks for (rules 1 to 3): need 0 = nothing is read or written */
struct H264ResPlan {
    int32_t need;       /* 0, 256 (luma alone) or 768 coefficients from `off` */
    int32_t off;        /* coeff_offset, valid when need != 0 */
    uint16_t nnz;       /* the macroblock's luma bits, bit (x4 + 4 * y4) */
    uint8_t t8;         /* the 8x8 transform */
    uint8_t chroma;     /* bit j: Cb block j, bit 4 + j: Cr block j; 0 without chroma planes */
    uint8_t chroma_dc;  /* bit c: plane c's DC is coded; 0 without chroma planes */
};

H264RES_FN H264ResPlan h264res_plan(const FFHipH264BsMb &m, const FFHipH264ResMb &r, bool has_chroma, int64_t ncoeffs)
{
    H264ResPlan p = {};
    if (m.flags & 1)                                                        /* rule 1 */
        return p;
    const bool c = has_chroma && (r.chroma | r.chroma_dc);
    const int need = c ? 768 : m.nnz ? 256 : 0;                             /* rule 2 */
    if (!need || r.coeff_offset < 0 || (r.coeff_offset & 15) || (int64_t)r.coeff_offset + need > ncoeffs)   /* rule 3 */
        return p;
    p.need = need;
    p.off = r.coeff_offset;
    p.nnz = m.nnz;
    p.t8 = (m.flags >> 1) & 1;
    p.chroma = c ? r.chroma : 0;
    p.chroma_dc = c ? r.chroma_dc & 3 : 0;
    return p;
}

/* luma block i of the decoder's order sits at (x4, y4) in 4x4 units of the macroblock; its coefficients at 16 * i */
H264RES_FN int h264res_x4(int i) { return (i & 1) + 2 * ((i >> 2) & 1); }
H264RES_FN int h264res_y4(int i) { return ((i >> 1) & 1) + 2 * (i >> 3); }
/* rule 4: 4x4 block i is transformed; rule 5: 8x8 block k (blocks 4k .. 4k + 3) is, by the bit of its top-left 4x4 block */
H264RES_FN bool h264res_luma4_on(const H264ResPlan &p, int i) { return !p.t8 && ((p.nnz >> (h264res_x4(i) + 4 * h264res_y4(i))) & 1); }
H264RES_FN bool h264res_luma8_on(const H264ResPlan &p, int k) { return p.t8 && ((p.nnz >> (2 * (k & 1) + 8 * (k >> 1))) & 1); }

/* rule 9: what *_dc_add puts on every sample of a block.  The sum is an int's, where the transforms add the 32 in CF: at 8 bits a
 * DC of 32736 .. 32767 wraps there and not here, the one place where the reference's two forms differ */
H264RES_FN int h264res_dc(int c0) { return (int)((uint32_t)c0 + 32u) >> 6; }

/* idct_add on v[] = block[0 .. 15]: on return v[4 * i + k] is what is added to the sample of row k, column i */
template <class CF>
H264RES_FN void h264res_idct4(int (&v)[16])
{
    v[0] = (CF)((uint32_t)v[0] + 32u);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t z0 = (uint32_t)v[i] + (uint32_t)v[i + 8], z1 = (uint32_t)v[i] - (uint32_t)v[i + 8];
        const uint32_t z2 = (uint32_t)(v[i + 4] >> 1) - (uint32_t)v[i + 12], z3 = (uint32_t)v[i + 4] + (uint32_t)(v[i + 12] >> 1);
        v[i] = (CF)(z0 + z3);
        v[i + 4] = (CF)(z1 + z2);
        v[i + 8] = (CF)(z1 - z2);
        v[i + 12] = (CF)(z0 - z3);
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t z0 = (uint32_t)v[4 * i] + (uint32_t)v[4 * i + 2], z1 = (uint32_t)v[4 * i] - (uint32_t)v[4 * i + 2];
        const uint32_t z2 = (uint32_t)(v[4 * i + 1] >> 1) - (uint32_t)v[4 * i + 3], z3 = (uint32_t)v[4 * i + 1] + (uint32_t)(v[4 * i + 3] >> 1);
        v[4 * i] = (int)(z0 + z3) >> 6;
        v[4 * i + 1] = (int)(z1 + z2) >> 6;
        v[4 * i + 2] = (int)(z1 - z2) >> 6;
        v[4 * i + 3] = (int)(z0 - z3) >> 6;
    }
}

/* one 8-point pass of the 8x8 transform on in[0], in[s], .. in[7 * s], in place; the results modulo 2^32 */
template <int S>
H264RES_FN void h264res_idct8_1d(int *in, uint32_t (&out)[8])
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

/* idct8_add on v[] = block[0 .. 63]: on return v[8 * i + k] is what is added to the sample of row k, column i */
template <class CF>
H264RES_FN void h264res_idct8(int (&v)[64])
{
    v[0] = (CF)((uint32_t)v[0] + 32u);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint32_t o[8];
        h264res_idct8_1d<8>(v + i, o);
#pragma unroll
        for (int k = 0; k < 8; k++)
            v[i + 8 * k] = (CF)o[k];
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint32_t o[8];
        h264res_idct8_1d<1>(v + 8 * i, o);
#pragma unroll
        for (int k = 0; k < 8; k++)
            v[8 * i + k] = (int)o[k] >> 6;
    }
}

/* rules 4, 5 and 9: is a luma block nothing but its DC?  idct_add16 / idct8_add4 take *_dc_add for a count of 1 with block[0] set, which
 * in a decoder's data is the block whose other coefficients are all zero: seen here from the coefficients, the face has no counts.
 * (A block of zeros is flat too: both forms add 0.) */
template <int N>
H264RES_FN bool h264res_flat(const int (&v)[N])
{
    int ac = 0;
#pragma unroll
    for (int i = 1; i < N; i++)
        ac |= v[i];
    return !ac;
}
/* a luma block of N coefficients by those rules, v[] in and out as the transforms above have it */
template <class CF, int N>
H264RES_FN void h264res_luma(int (&v)[N])
{
    if (h264res_flat(v)) {
        const int dc = h264res_dc(v[0]);
#pragma unroll
        for (int i = 0; i < N; i++)
            v[i] = dc;
    } else if constexpr (N == 16) {
        h264res_idct4<CF>(v);
    } else {
        h264res_idct8<CF>(v);
    }
}

/* rule 6: chroma_dc_dequant_idct on the first coefficients dc[j] of a plane's four blocks, as the reference stores them back */
template <class CF>
H264RES_FN void h264res_chroma_dc(int (&dc)[4], int32_t qmul)
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

/* rule 11 */
H264RES_FN int h264res_clip(int v, int maxv) { return v < 0 ? 0 : v > maxv ? maxv : v; }

#endif
