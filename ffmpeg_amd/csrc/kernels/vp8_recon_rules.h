/*
 * vp8_recon_rules.h — the decoder-facing rules of VP8 macroblock reconstruction (libavcodec/vp8.c: inter_predict / vp8_mc_part /
 * vp8_mc_luma / vp8_mc_chroma, and the mode checks of intra_predict), shared by the kernels of vp8_recon_frame.hip and the
 * device-free faces ffhip_vp8_mb_preds() / ffhip_vp8_intra_modes() (shims_vp8_recon.hip), which run them on the host.  Plain
 * functions of a macroblock record (FFHipVp8Mb, include/ffhip.h) and its position; nothing here touches a sample.
 */
#ifndef FFHIP_VP8_RECON_RULES_H
#define FFHIP_VP8_RECON_RULES_H

#include <stdint.h>

#include "ffhip.h"

#if defined(__HIPCC__)
#define V8R_FN __host__ __device__ __forceinline__
#else
#define V8R_FN static inline
#endif

#define V8R_MB_COEFFS 400 /* td->block[6][4][16], then td->block_dc[16] */

/* the 2-bit code of block b (0..15 Y in raster order, 16..19 U, 20..23 V) */
V8R_FN int v8r_code(const FFHipVp8Mb &mb, int b) { return (mb.block_code[b >> 2] >> (2 * (b & 3))) & 3; }

/* does the record read coefficients at all */
V8R_FN bool v8r_coded(const FFHipVp8Mb &mb)
{
    return mb.y2 || mb.block_code[0] || mb.block_code[1] || mb.block_code[2] || mb.block_code[3] || mb.block_code[4] || mb.block_code[5];
}

/* a record the kernels act on; refs: bit r - 1 set when reference r has all three planes */
V8R_FN bool v8r_mb_ok(const FFHipVp8Mb &mb, unsigned refs, int64_t coeff_count)
{
    if (mb.ref_frame > 3 || mb.y2 > 2)
        return false;
    if (mb.ref_frame) {
        if (!((refs >> (mb.ref_frame - 1)) & 1) || mb.partitioning > FFHIP_VP8_PART_4x4)
            return false;
    } else {
        if (mb.mode > FFHIP_VP8_MODE_I4x4 || mb.chroma_mode > FFHIP_VP8_PRED_TM)
            return false;
        if (mb.mode == FFHIP_VP8_MODE_I4x4)
            for (int i = 0; i < 16; i++)
                if (mb.sub_mode[i] > FFHIP_VP8_B_TM)
                    return false;
    }
    for (int i = 0; i < 6; i++) {
        const unsigned c = mb.block_code[i];
        if (c & (c >> 1) & 0x55) /* a code of 3 */
            return false;
    }
    if (v8r_coded(mb) && ((mb.coeff_offset & 15) || mb.coeff_offset < 0 || (int64_t)mb.coeff_offset + V8R_MB_COEFFS > coeff_count))
        return false;
    return true;
}

/* ---- inter ---- */
/* subpel_idx[0][m]: the table slot of a fraction in eighths: 0, the 4-tap form for odd eighths, the 6-tap form for even ones */
V8R_FN int v8r_slot(int m) { return !m ? 0 : (m & 1) ? 1 : 2; }

/* the put_vp8_* calls of a record: vp8_mc_part() per part (luma, U, V), or for 4x4 the sixteen luma blocks and then the four chroma
 * blocks (U, V each) */
V8R_FN int v8r_npreds(int partitioning)
{
    return partitioning == FFHIP_VP8_PART_NONE ? 3 : partitioning <= FFHIP_VP8_PART_8x16 ? 6 : partitioning == FFHIP_VP8_PART_8x8 ? 12 : 24;
}

V8R_FN void v8r_luma(FFHipVp8Pred &P, int mb_x, int mb_y, int x, int y, int w, int h, int mvx, int mvy)
{
    P.plane = 0; P.x = (uint8_t)x; P.y = (uint8_t)y; P.w = (uint8_t)w; P.h = (uint8_t)h;
    P.mx = (uint8_t)((mvx * 2) & 7);
    P.my = (uint8_t)((mvy * 2) & 7);
    P.hslot = (uint8_t)v8r_slot(P.mx);
    P.vslot = (uint8_t)v8r_slot(P.my);
    P.sx = 16 * mb_x + x + (mvx >> 2);
    P.sy = 16 * mb_y + y + (mvy >> 2);
}

/* x, y, w, h in chroma samples; the MV in eighths of the half-size plane */
V8R_FN void v8r_chroma(FFHipVp8Pred &P, int plane, int mb_x, int mb_y, int x, int y, int w, int h, int mvx, int mvy, int fullpel)
{
    if (fullpel) {
        mvx &= ~7;
        mvy &= ~7;
    }
    P.plane = (uint8_t)plane; P.x = (uint8_t)x; P.y = (uint8_t)y; P.w = (uint8_t)w; P.h = (uint8_t)h;
    P.mx = (uint8_t)(mvx & 7);
    P.my = (uint8_t)(mvy & 7);
    P.hslot = (uint8_t)v8r_slot(P.mx);
    P.vslot = (uint8_t)v8r_slot(P.my);
    P.sx = 8 * mb_x + x + (mvx >> 3);
    P.sy = 8 * mb_y + y + (mvy >> 3);
}

/* call i (0 .. v8r_npreds() - 1) of an inter record, in inter_predict()'s order */
V8R_FN void v8r_pred(const FFHipVp8Mb &mb, int i, int mb_x, int mb_y, int fullpel, FFHipVp8Pred &P)
{
    P.pad[0] = P.pad[1] = P.pad[2] = 0;
    if (mb.partitioning == FFHIP_VP8_PART_4x4) {
        if (i < 16) {
            v8r_luma(P, mb_x, mb_y, 4 * (i & 3), 4 * (i >> 2), 4, 4, mb.mv[i][0], mb.mv[i][1]);
            return;
        }
        const int j = i - 16, c = j >> 1, cx = c & 1, cy = c >> 1, b = 8 * cy + 2 * cx;
        int s[2];
        for (int k = 0; k < 2; k++) {
            const int sum = mb.mv[b][k] + mb.mv[b + 1][k] + mb.mv[b + 4][k] + mb.mv[b + 5][k];
            s[k] = (sum + 2 + (sum >> 31)) >> 2; /* FF_SIGNBIT: -1 for a negative sum */
        }
        v8r_chroma(P, 1 + (j & 1), mb_x, mb_y, 4 * cx, 4 * cy, 4, 4, s[0], s[1], fullpel);
        return;
    }
    const int part = i / 3, plane = i - 3 * part;
    int x = 0, y = 0, w = 16, h = 16;
    switch (mb.partitioning) {
    case FFHIP_VP8_PART_16x8: y = 8 * part; h = 8; break;
    case FFHIP_VP8_PART_8x16: x = 8 * part; w = 8; break;
    case FFHIP_VP8_PART_8x8:  x = 8 * (part & 1); y = 8 * (part >> 1); w = h = 8; break;
    default: break;
    }
    if (plane == 0)
        v8r_luma(P, mb_x, mb_y, x, y, w, h, mb.mv[part][0], mb.mv[part][1]);
    else
        v8r_chroma(P, plane, mb_x, mb_y, x >> 1, y >> 1, w >> 1, h >> 1, mb.mv[part][0], mb.mv[part][1], fullpel);
}

/* ---- intra ---- */
/* check_intra_pred8x8_mode_emuedge (VP8) with check_dc_pred8x8_mode / check_tm_pred8x8_mode: the pred16x16[] / pred8x8[] slot of a
 * 16x16 or chroma mode at macroblock (mb_x, mb_y): a FFHIP_VP8_PRED_* value */
V8R_FN int v8r_intra_blk_mode(int mode, int mb_x, int mb_y)
{
    switch (mode) {
    case FFHIP_VP8_PRED_DC:
        return !mb_x ? (mb_y ? FFHIP_VP8_PRED_TOP_DC : FFHIP_VP8_PRED_DC_128) : (mb_y ? mode : FFHIP_VP8_PRED_LEFT_DC);
    case FFHIP_VP8_PRED_VERT:
        return !mb_y ? FFHIP_VP8_PRED_DC_127 : mode;
    case FFHIP_VP8_PRED_HOR:
        return !mb_x ? FFHIP_VP8_PRED_DC_129 : mode;
    case FFHIP_VP8_PRED_TM:
        return !mb_x ? (mb_y ? FFHIP_VP8_PRED_VERT : FFHIP_VP8_PRED_DC_129) : (mb_y ? mode : FFHIP_VP8_PRED_HOR);
    }
    return mode;
}

/* check_intra_pred4x4_mode_emuedge (VP8) with check_tm_pred4x4_mode: the pred4x4[] slot (a FFHIP_VP8_B_* value) of a sub-block whose
 * column / row of sub-blocks in the frame is bx / by (only whether they are 0 matters), and whether intra_predict() predicts into
 * its bordered copy (copy_dst) */
V8R_FN int v8r_intra_sub_mode(int mode, int bx, int by, int *copy)
{
    *copy = 0;
    switch (mode) {
    case FFHIP_VP8_B_VERT:
        if (!bx && by) {
            *copy = 1;
            return mode;
        }
        /* fall through */
    case FFHIP_VP8_B_DDL:
    case FFHIP_VP8_B_VL:
        return !by ? FFHIP_VP8_B_DC_127 : mode;
    case FFHIP_VP8_B_HOR:
        if (!by) {
            *copy = 1;
            return mode;
        }
        /* fall through */
    case FFHIP_VP8_B_HU:
        return !bx ? FFHIP_VP8_B_DC_129 : mode;
    case FFHIP_VP8_B_TM:
        return !bx ? (by ? FFHIP_VP8_B_VERT_PLAIN : FFHIP_VP8_B_DC_129) : (by ? mode : FFHIP_VP8_B_HOR_PLAIN);
    case FFHIP_VP8_B_DC:
    case FFHIP_VP8_B_DDR:
    case FFHIP_VP8_B_VR:
    case FFHIP_VP8_B_HD:
        if (!by || !bx)
            *copy = 1;
        return mode;
    }
    return mode;
}

V8R_FN void v8r_intra_modes(const FFHipVp8Mb &mb, int mb_x, int mb_y, FFHipVp8IntraModes &M)
{
    M.mode16 = (uint8_t)(mb.mode == FFHIP_VP8_MODE_I4x4 ? FFHIP_VP8_PRED_NONE : v8r_intra_blk_mode(mb.mode, mb_x, mb_y));
    M.chroma = (uint8_t)v8r_intra_blk_mode(mb.chroma_mode, mb_x, mb_y);
    for (int i = 0; i < 16; i++) {
        int copy = 0;
        M.sub[i] = mb.mode == FFHIP_VP8_MODE_I4x4 ? (uint8_t)v8r_intra_sub_mode(mb.sub_mode[i], 4 * mb_x + (i & 3), 4 * mb_y + (i >> 2), &copy) : 0;
        M.copy[i] = (uint8_t)copy;
    }
}

#endif
