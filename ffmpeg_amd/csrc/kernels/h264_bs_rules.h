/*
 * h264_bs_rules.h — the H.264 deblocking edge parameters (bS, then alpha / beta / tc0 per edge: H.264 8.7.2.1 / 8.7.2.2 as
 * include/ffhip.h states them for ffhip_h264_edge_params_pictures_dev), once: shared by the kernel of h264_bs_pic.hip and by the
 * device-free face ffhip_h264_edge_params_pictures_host() (shims_h264_bs.hip), which runs them on the host.  Restated from the
 * standard and the behaviour of the reference's h264_loopfilter.c, not checked against its source.  Plain functions of resolved
 * macroblocks and blocks; nothing here touches a map but through the pointers it is handed.  The three tables live here and nowhere
 * else.
 *
 * A macroblock and a 4x4 block are resolved once: the macroblock to two words with everything of its slice an edge needs, the block
 * to its two motion vectors as the dwords the record holds (x in the low half, y in the high half; the records are read as three
 * little-endian dwords) and one word with the picture each list refers to.
 */
#ifndef FFHIP_H264_BS_RULES_H
#define FFHIP_H264_BS_RULES_H

#include <stdint.h>

#include "ffhip.h"

#if defined(__HIPCC__)
#define H264BS_FN __host__ __device__ __forceinline__
#else
#define H264BS_FN static inline
#endif

/* Tables 8-16 (alpha', beta') and 8-17 (tc0' for bS 1, 2, 3) by indexA / indexB */
static constexpr uint8_t h264bs_alpha[52] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 4, 4, 5, 6, 7, 8, 9, 10, 12, 13,
                                              15, 17, 20, 22, 25, 28, 32, 36, 40, 45, 50, 56, 63, 71, 80, 90, 101, 113, 127, 144,
                                              162, 182, 203, 226, 255, 255 };
static constexpr uint8_t h264bs_beta[52] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4,
                                             6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13, 14, 14, 15, 15,
                                             16, 16, 17, 17, 18, 18 };
static constexpr uint8_t h264bs_tc0[52][3] = {
    { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 },
    { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 },
    { 0, 0, 1 }, { 0, 0, 1 }, { 0, 0, 1 }, { 0, 0, 1 }, { 0, 1, 1 }, { 0, 1, 1 }, { 1, 1, 1 }, { 1, 1, 1 }, { 1, 1, 1 },
    { 1, 1, 1 }, { 1, 1, 2 }, { 1, 1, 2 }, { 1, 1, 2 }, { 1, 1, 2 }, { 1, 2, 3 }, { 1, 2, 3 }, { 2, 2, 3 }, { 2, 2, 4 },
    { 2, 3, 4 }, { 2, 3, 4 }, { 3, 3, 5 }, { 3, 4, 6 }, { 3, 4, 6 }, { 4, 5, 7 }, { 4, 5, 8 }, { 4, 6, 9 }, { 5, 7, 10 },
    { 6, 8, 11 }, { 6, 8, 13 }, { 7, 10, 14 }, { 8, 11, 16 }, { 9, 12, 18 }, { 10, 13, 20 }, { 11, 15, 23 }, { 13, 17, 25 } };

/* H264BsMb.b: bits 0..7 qp, 8 intra, 9 the 8x8 transform, 10 the slice index is below nslices, 11..12 the slice's idc (1 and 2 as
 * they are, anything else 0), 13 B slice, 16..23 alpha_c0_offset, 24..31 beta_offset (both int8_t) */
#define H264BS_INTRA    (1u << 8)
#define H264BS_T8X8     (1u << 9)
#define H264BS_SLICE_OK (1u << 10)
#define H264BS_IDC_SHIFT 11
#define H264BS_BSLICE   (1u << 13)
/* a block's reference of a list: the slice's byte; UNUSED (ref_idx < 0): equal to every other unused one; BAD (an index outside the
 * slice's list, or no slice): equal to nothing, itself included */
#define H264BS_REF_UNUSED 0x100u
#define H264BS_REF_BAD    0x200u
#define H264BS_QP_ENTRIES 88 /* chroma_qp[2][88]: QP'Y 0 .. 51 + 36 */

struct H264BsMb {
    uint32_t a; /* slice | nnz << 16 */
    uint32_t b;
};
struct H264BsBlk {
    uint32_t mv[2];
    uint32_t refs; /* list 0 | list 1 << 16 */
};

H264BS_FN H264BsMb h264bs_resolve_mb(const FFHipH264BsMb &m, const FFHipH264BsSlice *slices, int nslices)
{
    H264BsMb r;
    r.a = (uint32_t)m.slice | (uint32_t)m.nnz << 16;
    r.b = (uint32_t)m.qp | (uint32_t)(m.flags & 3u) << 8;
    if ((int)m.slice < nslices) {
        const FFHipH264BsSlice &S = slices[m.slice];
        r.b |= H264BS_SLICE_OK | (S.idc == 1 || S.idc == 2 ? (uint32_t)S.idc << H264BS_IDC_SHIFT : 0u) | (S.flags & 1u ? H264BS_BSLICE : 0u) |
               (uint32_t)(uint8_t)S.alpha_c0_offset << 16 | (uint32_t)(uint8_t)S.beta_offset << 24;
    }
    return r;
}

/* one block from the dwords of its FFHipH264MvField and its resolved macroblock */
H264BS_FN H264BsBlk h264bs_resolve_blk(uint32_t mv0, uint32_t mv1, uint32_t rest, const H264BsMb &mb, const FFHipH264BsSlice *slices)
{
    H264BsBlk u;
    u.mv[0] = mv0;
    u.mv[1] = mv1;
    u.refs = 0;
    for (int l = 0; l < 2; l++) {
        const int ri = (int8_t)(rest >> (8 * l));
        uint32_t code;
        if (ri < 0)
            code = H264BS_REF_UNUSED;
        else if (!(mb.b & H264BS_SLICE_OK) || ri >= 32 || ri >= (int)slices[mb.a & 0xFFFF].num_ref[l])
            code = H264BS_REF_BAD;
        else
            code = slices[mb.a & 0xFFFF].ref[l][ri];
        if (code > 0xFF)
            u.mv[l] = 0;
        u.refs |= code << (16 * l);
    }
    return u;
}

H264BS_FN bool h264bs_ref_differ(const H264BsBlk &a, int la, const H264BsBlk &b, int lb)
{
    const uint32_t ra = (a.refs >> (16 * la)) & 0xFFFF, rb = (b.refs >> (16 * lb)) & 0xFFFF;
    return ra != rb || ra == H264BS_REF_BAD;
}

/* x at least 4 quarter samples apart, or y at least mvy_limit (4 in a frame, 2 in a field picture) */
H264BS_FN bool h264bs_mv_differ(uint32_t a, uint32_t b, int mvy_limit)
{
    const int dx = (int16_t)(a & 0xFFFF) - (int16_t)(b & 0xFFFF), dy = (int16_t)(a >> 16) - (int16_t)(b >> 16);
    return (dx < 0 ? -dx : dx) >= 4 || (dy < 0 ? -dy : dy) >= mvy_limit;
}

/* the reference's check_mv order: 1 or 0 */
H264BS_FN int h264bs_check_mv(const H264BsBlk &p, const H264BsBlk &q, bool two_lists, int mvy_limit)
{
    bool v = h264bs_ref_differ(p, 0, q, 0) || h264bs_mv_differ(p.mv[0], q.mv[0], mvy_limit);
    if (!two_lists)
        return v;
    if (!v)
        v = h264bs_ref_differ(p, 1, q, 1) || h264bs_mv_differ(p.mv[1], q.mv[1], mvy_limit);
    if (!v)
        return 0;
    if (h264bs_ref_differ(p, 0, q, 1) || h264bs_ref_differ(p, 1, q, 0))
        return 1;
    return h264bs_mv_differ(p.mv[0], q.mv[1], mvy_limit) || h264bs_mv_differ(p.mv[1], q.mv[0], mvy_limit);
}

/* Rules 1 and 2 of edge e of direction dir of macroblock q: the bS of group g in byte g, 0 for a skipped edge.  p: the macroblock
 * across edge 0 (anything at the border), q itself otherwise.  blk(x, y): the resolved block x, y of q in 4x4 blocks, -1 being the
 * last column / row of the macroblock to the left / above; called for blocks inside the picture only.
 * c422h: the edge is a chroma edge of the horizontal direction of a 4:2:2 picture (rule 6): the 8x8-transform clause of rule 1 does
 * not hold for it, everything else does. */
template <class Blk>
H264BS_FN uint32_t h264bs_edge_bs(const H264BsMb &p, const H264BsMb &q, bool border, int dir, int e, int field, Blk &&blk, bool c422h = false)
{
    if (!(q.b & H264BS_SLICE_OK))
        return 0;
    const unsigned idc = (q.b >> H264BS_IDC_SHIFT) & 3;
    if (idc == 1 || (!c422h && (e & 1) && (q.b & H264BS_T8X8)))
        return 0;
    if (!e && (border || (idc == 2 && (p.a & 0xFFFF) != (q.a & 0xFFFF))))
        return 0;
    if ((p.b | q.b) & H264BS_INTRA)
        return (!e && (!field || !dir) ? 4u : 3u) * 0x01010101u;
    const bool two = (q.b & H264BS_BSLICE) != 0;
    const int lim = field ? 2 : 4;
    uint32_t bs = 0;
    for (int g = 0; g < 4; g++) {
        const int qx = dir ? g : e, qy = dir ? e : g, px = dir ? g : e - 1, py = dir ? e - 1 : g;
        const unsigned pbit = ((e ? q.a : p.a) >> (16 + (px & 3) + 4 * (py & 3))) & 1, qbit = (q.a >> (16 + qx + 4 * qy)) & 1;
        const uint32_t v = pbit | qbit ? 2u : (uint32_t)h264bs_check_mv(blk(px, py), blk(qx, qy), two, lim);
        bs |= v << (8 * g);
    }
    return bs;
}

/* rule 3 / 4: the qp of the edge; tab: NULL for luma, else the plane's 88 entries of chroma_qp */
H264BS_FN int h264bs_edge_qp(const H264BsMb &p, const H264BsMb &q, int e, const uint8_t *tab)
{
    int qq = (int)(q.b & 0xFF), qp = (int)(p.b & 0xFF);
    if (tab) {
        qq = tab[qq < H264BS_QP_ENTRIES ? qq : H264BS_QP_ENTRIES - 1];
        qp = tab[qp < H264BS_QP_ENTRIES ? qp : H264BS_QP_ENTRIES - 1];
    }
    return e ? qq : (qp + qq + 1) >> 1;
}

H264BS_FN int h264bs_clip51(int v) { return v < 0 ? 0 : v > 51 ? 51 : v; }

/* rules 3 .. 5: the record of an edge as three little-endian dwords (offset; kind, alpha, beta, pad; tc0[4]).  chroma chooses the
 * kinds and the tc0 convention, not the plane: true for the Cb / Cr records of 4:2:0 and 4:2:2 (*_CHROMA kinds, tc0' + 1, 0 at bS 0),
 * false for luma and for the Cb / Cr records of 4:4:4 (rule 7: the luma kinds, tc0', -1 at bS 0), whose qp is the plane's all the same. */
H264BS_FN void h264bs_pack(bool chroma, int dir, uint32_t bs, int qp, const H264BsMb &q, int qp_bd_offset, uint32_t out[3])
{
    const uint32_t kind = (chroma ? FFHIP_H264_LF_V_CHROMA : FFHIP_H264_LF_V_LUMA) + (dir ? 0 : 1);
    out[0] = 0;
    if (!bs) {
        out[1] = kind;
        out[2] = chroma ? 0u : 0xFFFFFFFFu;
        return;
    }
    const int ia = h264bs_clip51(qp - qp_bd_offset + (int8_t)(q.b >> 16)), ib = h264bs_clip51(qp - qp_bd_offset + (int8_t)(q.b >> 24));
    const uint32_t ab = (uint32_t)h264bs_alpha[ia] << 8 | (uint32_t)h264bs_beta[ib] << 16;
    if ((bs & 0xFF) == 4) {
        out[1] = (kind + 4) | ab;
        out[2] = 0;
        return;
    }
    uint32_t tc = 0;
    for (int g = 0; g < 4; g++) {
        const unsigned b = (bs >> (8 * g)) & 0xFF;
        const int t = b ? h264bs_tc0[ia][b - 1] + (chroma ? 1 : 0) : (chroma ? 0 : -1);
        tc |= (uint32_t)(uint8_t)t << (8 * g);
    }
    out[1] = kind | ab;
    out[2] = tc;
}

#endif /* FFHIP_H264_BS_RULES_H */
