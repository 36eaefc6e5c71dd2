/*
 * h264_inter_rules.h — how the lists of one 4x4 block combine in H.264 inter prediction (rules 1, 2 and 5 to 8 of
 * ffhip_h264_inter_pictures_dev as include/ffhip.h states them), where a block's chroma samples lie and come from at each chroma
 * format (rule 4, 4a / 4b of the _fmt faces: h264inter_chroma) and what a mode makes of the lists' samples on a plane
 * (h264inter_combine), once: shared by the kernel of h264_inter_pic.hip and by the device-free faces
 * ffhip_h264_inter_plan_pictures_host() and ffhip_h264_inter_pictures_fmt_host() (shims_h264_inter.hip), which run it on the host.  Restated from memory of
 * the reference's h264_mb.c (mc_part and what it calls) and from H.264 8.4.2.2 / 8.4.2.3, not checked against its source.  One plain
 * function of the macroblock record, the block's motion record and the slice table; it reads nothing else.  What a mode does to the
 * samples (weight / biweight_h264_pixels) is h264_mc_rules.h's.
 */
#ifndef FFHIP_H264_INTER_RULES_H
#define FFHIP_H264_INTER_RULES_H

#include <stdint.h>

#include "ffhip.h"
#include "h264_mc_rules.h"

#if defined(__HIPCC__)
#define H264INTER_FN __host__ __device__ __forceinline__
#else
#define H264INTER_FN static inline
#endif

/* the plan of the block whose motion record is f, in macroblock m; every field the mode does not use is 0 */
H264INTER_FN FFHipH264InterBlockPlan h264inter_plan(const FFHipH264BsMb *m, const FFHipH264MvField *f, const FFHipH264InterSlice *slices,
                                                    int nslices, int nrefs)
{
    FFHipH264InterBlockPlan p = {};
    if ((m->flags & 1) || (int)m->slice >= nslices)                         /* rule 1; rule 2: no slice */
        return p;
    const FFHipH264InterSlice *S = slices + m->slice;
    if (S->luma_log2_denom > 7 || S->chroma_log2_denom > 7 || S->use_weight > 2)
        return p;
    const int r0 = f->ref_idx[0], r1 = f->ref_idx[1];
    const int nlists = (r0 >= 0) + (r1 >= 0);
    if (!nlists)
        return p;
    int slot[2] = { 0, 0 };
    for (int l = 0; l < 2; l++) {
        const int r = l ? r1 : r0;
        if (r < 0)
            continue;
        if (r >= 32 || S->num_ref[l] > 32 || r >= (int)S->num_ref[l] || (int)S->ref[l][r] >= nrefs)
            return p;
        slot[l] = S->ref[l][r];
    }
    if (nlists == 2) {
        p.slot[0] = (uint8_t)slot[0];
        p.slot[1] = (uint8_t)slot[1];
        if (S->use_weight == 2 && S->implicit_weight[r0][r1] != 32) {      /* rule 7, implicit */
            const int w0 = S->implicit_weight[r0][r1];
            p.mode = FFHIP_H264_INTER_BI_W;
            p.chroma_weighted = 1;
            p.luma_log2_denom = p.chroma_log2_denom = 5;
            p.luma_weight[0] = (int16_t)w0;
            p.luma_weight[1] = (int16_t)(64 - w0);
            for (int c = 0; c < 2; c++) {
                p.chroma_weight[c][0] = (int16_t)w0;
                p.chroma_weight[c][1] = (int16_t)(64 - w0);
            }
        } else if (S->use_weight == 1) {                                     /* rule 7, explicit */
            p.mode = FFHIP_H264_INTER_BI_W;
            p.chroma_weighted = 1;
            p.luma_log2_denom = S->luma_log2_denom;
            p.chroma_log2_denom = S->chroma_log2_denom;
            p.luma_weight[0] = S->luma_weight[r0][0][0];
            p.luma_weight[1] = S->luma_weight[r1][1][0];
            p.luma_offset = (int16_t)(S->luma_weight[r0][0][1] + S->luma_weight[r1][1][1]);
            for (int c = 0; c < 2; c++) {
                p.chroma_weight[c][0] = S->chroma_weight[r0][0][c][0];
                p.chroma_weight[c][1] = S->chroma_weight[r1][1][c][0];
                p.chroma_offset[c] = (int16_t)(S->chroma_weight[r0][0][c][1] + S->chroma_weight[r1][1][c][1]);
            }
        } else {
            p.mode = FFHIP_H264_INTER_BI_AVG;                                /* rule 6 */
        }
        return p;
    }
    const int L = r0 >= 0 ? 0 : 1, r = L ? r1 : r0;
    p.list = (uint8_t)L;
    p.slot[0] = (uint8_t)slot[L];
    if (S->use_weight != 1) {
        p.mode = FFHIP_H264_INTER_UNI;                                       /* rule 6; implicit weights need two lists */
        return p;
    }
    p.mode = FFHIP_H264_INTER_UNI_W;                                         /* rule 8 */
    p.luma_log2_denom = S->luma_log2_denom;
    p.luma_weight[0] = S->luma_weight[r][L][0];
    p.luma_offset = S->luma_weight[r][L][1];
    if (S->use_weight_chroma) {
        p.chroma_weighted = 1;
        p.chroma_log2_denom = S->chroma_log2_denom;
        for (int c = 0; c < 2; c++) {
            p.chroma_weight[c][0] = S->chroma_weight[r][L][c][0];
            p.chroma_offset[c] = S->chroma_weight[r][L][c][1];
        }
    }
    return p;
}

/* Rule 4 by format (chroma_format_idc 1 or 2; at 3 Cb and Cr are luma planes): the chroma block of the 4x4 luma block (bx, by), in
 * samples of a chroma plane, for the vector (mvx, mvy) of one list.  w x h samples at (x, y); sample (i, k) of it is h264chroma's put
 * with the fractions (ax, ay) at the source position (sx + i, sy + k), each source coordinate clamped to [0, cw) x [0, ch). */
struct H264InterChroma { int w, h, x, y, sx, sy, ax, ay, cw, ch; };
H264INTER_FN H264InterChroma h264inter_chroma(int chroma_format_idc, int bx, int by, int mvx, int mvy, int chroma_dy, int mb_w, int mb_h)
{
    H264InterChroma c;
    c.w = 2;
    c.x = 2 * bx;
    c.sx = c.x + (mvx >> 3);
    c.ax = mvx & 7;
    c.cw = 8 * mb_w;
    if (chroma_format_idc == 2) {       /* mc_dir_part with ysh = 2; chroma_dy is 4:2:0's alone */
        c.h = 4;
        c.y = 4 * by;
        c.sy = c.y + (mvy >> 2);
        c.ay = (mvy * 2) & 7;          /* (my << 1) & 7 */
        c.ch = 16 * mb_h;
    } else {
        const int cy = mvy + chroma_dy;
        c.h = 2;
        c.y = 2 * by;
        c.sy = c.y + (cy >> 3);
        c.ay = cy & 7;
        c.ch = 8 * mb_h;
    }
    return c;
}

/* Rules 5 to 9 on a sample of plane pl (0 luma; 1 Cb, 2 Cr: the chroma values, at every format): p0 the sample of list 0 or of the
 * one list, p1 that of list 1 */
H264INTER_FN int h264inter_combine(const FFHipH264InterBlockPlan *p, int pl, int p0, int p1, int bd)
{
    const int c = pl == 2;
    const int ld = pl ? p->chroma_log2_denom : p->luma_log2_denom;
    const int w0 = pl ? p->chroma_weight[c][0] : p->luma_weight[0], w1 = pl ? p->chroma_weight[c][1] : p->luma_weight[1];
    const int o = pl ? p->chroma_offset[c] : p->luma_offset;
    switch (p->mode) {
    case FFHIP_H264_INTER_UNI_W:
        return pl && !p->chroma_weighted ? p0 : h264mc_weight(p0, bd, ld, w0, o);
    case FFHIP_H264_INTER_BI_AVG:
        return h264mc_avg(p0, p1);
    case FFHIP_H264_INTER_BI_W:
        return h264mc_biweight(p0, p1, bd, ld, w0, w1, o);
    default:
        return p0;
    }
}

#endif /* FFHIP_H264_INTER_RULES_H */
