/*
 * hevc_bs_rules.h — the HEVC deblocking boundary-strength rule (H.265 8.7.2.3 / 8.7.2.4 as include/ffhip.h states it for
 * ffhip_hevc_boundary_strengths_pictures_dev), once: shared by the kernel of hevc_bs_pic.hip and by the device-free face
 * ffhip_hevc_boundary_strengths_pictures_host() (shims_hevc_bs.hip), which runs it on the host.  Restated from the standard, not
 * checked against the reference's source.  Plain functions of resolved units; nothing here touches a map.
 *
 * A unit is resolved once: its two motion vectors as the dwords the record holds (x in the low half, y in the high half; the
 * records are read as three little-endian dwords), and one word of everything else a comparison needs.
 */
#ifndef FFHIP_HEVC_BS_RULES_H
#define FFHIP_HEVC_BS_RULES_H

#include <stdint.h>

#include "ffhip.h"

#if defined(__HIPCC__)
#define HBS_FN __host__ __device__ __forceinline__
#else
#define HBS_FN static inline
#endif

/* HbsUnit.info: bits 0..7 / 8..15 the DPB slot of list 0 / 1, 16..17 pred_flag (0 intra), 18 / 19 that list's slot is a resolved
 * reference, 20..22 the unit's tu byte, 23 its CTB's slice index is below nslices, 24..25 that slice's flags */
#define HBS_PRED_SHIFT  16
#define HBS_VALID_SHIFT 18
#define HBS_TU_SHIFT    20
#define HBS_SLICE_OK    (1u << 23)
#define HBS_FLAGS_SHIFT 24

struct HbsUnit {
    uint32_t mv[2];
    uint32_t info;
};

/* one unit from the dwords of its FFHipHevcMvField, its tu byte and the slice index of its CTB */
HBS_FN HbsUnit hbs_resolve(uint32_t mv0, uint32_t mv1, uint32_t rest, unsigned tu, const FFHipHevcBsSlice *slices, int nslices, unsigned slice)
{
    HbsUnit u;
    u.mv[0] = mv0;
    u.mv[1] = mv1;
    unsigned pred = (rest >> 16) & 0xFF;
    if (pred > 3)
        pred = 0;
    uint32_t info = pred << HBS_PRED_SHIFT | (tu & 7u) << HBS_TU_SHIFT;
    if (slice < (unsigned)nslices) {
        const FFHipHevcBsSlice &S = slices[slice];
        info |= HBS_SLICE_OK | (uint32_t)(S.flags & 3u) << HBS_FLAGS_SHIFT;
        for (int l = 0; l < 2; l++) {
            const unsigned ri = (rest >> (8 * l)) & 0xFF; /* int8_t ref_idx: a negative one is above 15 here */
            const unsigned n = S.num_ref[l];
            if ((pred >> l & 1) && n <= 16 && ri < n)
                info |= (uint32_t)S.ref[l][ri] << (8 * l) | 1u << (HBS_VALID_SHIFT + l);
        }
    }
    u.info = info;
    return u;
}

/* x or y at least 4 quarter samples apart */
HBS_FN bool hbs_mv_differ(uint32_t a, uint32_t b)
{
    const int dx = (int16_t)(a & 0xFFFF) - (int16_t)(b & 0xFFFF), dy = (int16_t)(a >> 16) - (int16_t)(b >> 16);
    return (dx < 0 ? -dx : dx) >= 4 || (dy < 0 ? -dy : dy) >= 4;
}

/* list la of a and list lb of b name the same picture: both resolved, equal slots */
HBS_FN bool hbs_same_pic(const HbsUnit &a, int la, const HbsUnit &b, int lb)
{
    return (a.info >> (HBS_VALID_SHIFT + la) & 1) && (b.info >> (HBS_VALID_SHIFT + lb) & 1) &&
           ((a.info >> (8 * la)) & 0xFF) == ((b.info >> (8 * lb)) & 0xFF);
}

/* rule 6 */
HBS_FN int hbs_motion(const HbsUnit &p, const HbsUnit &q)
{
    const unsigned pp = (p.info >> HBS_PRED_SHIFT) & 3, pq = (q.info >> HBS_PRED_SHIFT) & 3;
    if (!pp || !pq)
        return pp || pq ? 2 : 0; /* two intra units meet only on a TU edge, which rule 4 has taken; inside a TU: nothing to filter */
    if (pp == 3 && pq == 3) {
        const bool d00 = hbs_mv_differ(p.mv[0], q.mv[0]), d11 = hbs_mv_differ(p.mv[1], q.mv[1]);
        const bool d10 = hbs_mv_differ(p.mv[1], q.mv[0]), d01 = hbs_mv_differ(p.mv[0], q.mv[1]);
        const bool straight = hbs_same_pic(q, 0, p, 0) && hbs_same_pic(q, 1, p, 1);
        const bool crossed = hbs_same_pic(q, 0, p, 1) && hbs_same_pic(q, 1, p, 0);
        if (hbs_same_pic(q, 0, p, 0) && hbs_same_pic(q, 0, q, 1) && hbs_same_pic(p, 0, p, 1))
            return (d00 || d11) && (d10 || d01);
        if (straight)
            return d00 || d11;
        if (crossed)
            return d10 || d01;
        return 1;
    }
    if (pp == 3 || pq == 3)
        return 1;
    const int lp = pp == 2, lq = pq == 2;
    if (!hbs_same_pic(p, lp, q, lq))
        return 1;
    return hbs_mv_differ(p.mv[lp], q.mv[lq]);
}

/* rules 2..6 of the segment between p and q on q's left (dir 0) or top (dir 1) side; rule 1 (the grid and the picture border) is
 * the caller's */
HBS_FN int hbs_segment(const HbsUnit &p, const HbsUnit &q, int dir, bool same_slice, bool same_tile, bool across_tiles)
{
    if (!(q.info & HBS_SLICE_OK) || (q.info >> HBS_FLAGS_SHIFT & 1))
        return 0;
    if (!same_slice && !(q.info >> (HBS_FLAGS_SHIFT + 1) & 1))
        return 0;
    if (!same_tile && !across_tiles)
        return 0;
    if (q.info >> (HBS_TU_SHIFT + dir) & 1) {
        if (!((p.info >> HBS_PRED_SHIFT) & 3) || !((q.info >> HBS_PRED_SHIFT) & 3))
            return 2;
        if ((p.info | q.info) >> (HBS_TU_SHIFT + 2) & 1)
            return 1;
    }
    return hbs_motion(p, q);
}

/* rule 1: a unit coordinate across the edge direction that carries a segment */
HBS_FN bool hbs_on_grid(int u) { return u > 0 && !(u & 1); }

#endif /* FFHIP_HEVC_BS_RULES_H */
