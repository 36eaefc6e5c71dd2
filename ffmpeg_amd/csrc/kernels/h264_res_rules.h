/*
 * h264_res_rules.h — the residual of one H.264 inter macroblock (rules 1 to 9 of ffhip_h264_residual_pictures_dev and 13 to 15 of its
 * _fmt face as include/ffhip.h states them), once: what a macroblock's records ask for at a chroma format (h264res_plan), where its
 * blocks sit, which bits switch them on at each format and which of the two forms a luma block takes (h264res_luma), shared by the
 * kernel of h264_res_pic.hip and by ffhip_h264_residual_pictures_host() / _fmt_host() (shims_h264_res.hip), which run it on the CPU.
 * The DC transforms of a chroma plane (2x2, and 2x4 at 4:2:2) are h264_tx_rules.h's h264tx_chroma_dc / h264tx_chroma422_dc.
 *
 * The arithmetic of a block is h264_tx_rules.h's, the one the batch kernels of h264_idct.hip / h264_hbd.hip run: those read, clear and
 * dispatch by lists, here the coefficients are never written.
 */
#ifndef FFHIP_H264_RES_RULES_H
#define FFHIP_H264_RES_RULES_H

#include <stdint.h>

#include "ffhip.h"
#include "h264_tx_rules.h"

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
    uint8_t chroma;     /* bit j: Cb block j, bit 4 + j: Cr block j; 0 without chroma planes and at 4:4:4 */
    uint8_t chroma_dc;  /* bit c: plane c's DC is coded; 0 without chroma planes and at 4:4:4 */
    uint8_t chroma_lo;  /* 4:2:2: bit j - 4: Cb block j = 4 .. 7, bit 4 + (j - 4): Cr block j; 0 at every other format */
    uint16_t nnz444[2]; /* 4:4:4: the bits of Cb and Cr in nnz's layout; 0 at every other format and without chroma planes */
};

/* fmt: chroma_format_idc, 0 .. 3 (has_chroma is false at 0) */
H264RES_FN H264ResPlan h264res_plan(const FFHipH264BsMb &m, const FFHipH264ResMb &r, bool has_chroma, int64_t ncoeffs, int fmt)
{
    H264ResPlan p = {};
    if (m.flags & 1)                                                        /* rule 1 */
        return p;
    const bool c = has_chroma && (fmt == 3 ? ((r.nnz444[0] | r.nnz444[1]) & 0xFFFF) != 0         /* rule 15 */
                                           : (r.chroma | r.chroma_dc | (fmt == 2 ? r.chroma_lo422 : 0)) != 0);   /* rules 2, 13, 14 */
    const int need = c ? 768 : m.nnz ? 256 : 0;                             /* rule 2 */
    if (!need || r.coeff_offset < 0 || (r.coeff_offset & 15) || (int64_t)r.coeff_offset + need > ncoeffs)   /* rule 3 */
        return p;
    p.need = need;
    p.off = r.coeff_offset;
    p.nnz = m.nnz;
    p.t8 = (m.flags >> 1) & 1;
    if (fmt == 3) {
        p.nnz444[0] = c ? (uint16_t)r.nnz444[0] : 0;
        p.nnz444[1] = c ? (uint16_t)r.nnz444[1] : 0;
        return p;
    }
    p.chroma = c ? r.chroma : 0;
    p.chroma_dc = c ? r.chroma_dc & 3 : 0;
    p.chroma_lo = c && fmt == 2 ? r.chroma_lo422 : 0;
    return p;
}

/* luma block i of the decoder's order sits at (x4, y4) in 4x4 units of the macroblock; its coefficients at 16 * i */
H264RES_FN int h264res_x4(int i) { return (i & 1) + 2 * ((i >> 2) & 1); }
H264RES_FN int h264res_y4(int i) { return ((i >> 1) & 1) + 2 * (i >> 3); }
/* the bits of plane pl in nnz's layout: the luma plane's, and at 4:4:4 (rule 15) those of Cb and Cr */
/* (a shift, not a choice among the three fields: a kernel that walks the planes keeps the plan in registers then) */
H264RES_FN int h264res_plane_nnz(const H264ResPlan &p, int pl)
{
    return (int)((((uint64_t)p.nnz444[1] << 32) | ((uint64_t)p.nnz444[0] << 16) | p.nnz) >> (16 * pl)) & 0xFFFF;
}
/* rule 4: 4x4 block i of plane pl is transformed; rule 5: 8x8 block k (blocks 4k .. 4k + 3) is, by the bit of its top-left 4x4 block */
H264RES_FN bool h264res_luma4_on(const H264ResPlan &p, int i, int pl = 0)
{
    return !p.t8 && ((h264res_plane_nnz(p, pl) >> (h264res_x4(i) + 4 * h264res_y4(i))) & 1);
}
H264RES_FN bool h264res_luma8_on(const H264ResPlan &p, int k, int pl = 0)
{
    return p.t8 && ((h264res_plane_nnz(p, pl) >> (2 * (k & 1) + 8 * (k >> 1))) & 1);
}
/* 4:2:0 and 4:2:2: block j = x + 2 * y of chroma plane c (0 Cb, 1 Cr) has its bit; 4 blocks a plane at 4:2:0, 8 at 4:2:2 (rule 14), at
 * (4 x, 4 y) of the macroblock's chroma, its coefficients at 256 * (1 + c) + 16 * j */
H264RES_FN int h264res_chroma_blocks(int fmt) { return fmt == 2 ? 8 : 4; }
H264RES_FN bool h264res_chroma_on(const H264ResPlan &p, int c, int j)
{
    return ((j < 4 ? p.chroma >> (4 * c + j) : p.chroma_lo >> (4 * c + j - 4)) & 1) != 0;
}

/* rules 4, 5 and 9: a luma block of N coefficients, v[] in and out as h264tx_idct4 / h264tx_idct8 have it.  idct_add16 / idct8_add4 take
 * *_dc_add for a count of 1 with block[0] set, which in a decoder's data is the block whose other coefficients are all zero: seen here
 * from the coefficients (h264tx_flat), the face has no counts. */
template <class CF, int N>
H264RES_FN void h264res_luma(int (&v)[N])
{
    if (h264tx_flat(v)) {
        const int dc = h264tx_dc(v[0]);
#pragma unroll
        for (int i = 0; i < N; i++)
            v[i] = dc;
    } else if constexpr (N == 16) {
        h264tx_idct4<CF>(v);
    } else {
        h264tx_idct8<CF>(v);
    }
}

#endif
