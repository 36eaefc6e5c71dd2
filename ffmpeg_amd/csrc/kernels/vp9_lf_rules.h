/*
 * vp9_lf_rules.h — the control data of the VP9 loop filter, once: from a decoded block to the superblock's VP9Filter (the tail of
 * ff_vp9_decode_block and mask_edges, libavcodec/vp9block.c:1141-1262, 1433-1447: restated, not checked against the source) and from
 * the VP9Filter to the tables the frame kernels walk (filter_plane_cols / _rows, libavcodec/vp9lpf.c:27-178).  Shared by
 * host/vp9_lf_tables.c (plain C: ffhip_vp9_lf_sb_tables / _ctables), by the device-free face ffhip_vp9_lf_tables_pictures_host()
 * (shims_vp9_lf_tab.hip) and by the kernel of vp9_lf_tab_pic.hip, so this file is C that hipcc compiles for both sides: no
 * references, no lambdas, no templates.
 *
 * Every rule is a pure function of ONE item, so a lane can evaluate it on its own:
 *   - vp9lf_block():     one FFHipVp9LfBlock record -> the validated block (or "skip it");
 *   - vp9lf_mask_edges():the arguments of one mask_edges call -> Vp9LfEdges, after the 4x4-chroma early return / extension;
 *   - vp9lf_mask_row():  Vp9LfEdges + a row y of the superblock -> the bits the call ORs into mask[0][y][0..3] and mask[1][y][0..3],
 *                        each as one word (byte k = mask[.][y][k]: the layout of the struct on a little-endian machine);
 *   - vp9lf_cols_item() / vp9lf_rows_item(): one (row group, position) of filter_plane_cols / _rows -> up to four table entries.
 *     The reference's loop exit `!(hm & ~(x - 1))` is a function of the masks alone, so an item decides it for itself.
 */
#ifndef FFHIP_VP9_LF_RULES_H
#define FFHIP_VP9_LF_RULES_H

#include <stdint.h>

#include "ffhip.h"

#if defined(__HIPCC__)
#define VP9LF_FN __host__ __device__ __forceinline__
#else
#define VP9LF_FN static inline
#endif

/* ---- a block --------------------------------------------------------------------------------------------- */
typedef struct Vp9LfBlk {
    int ok;                 /* 0: the record is skipped as if its level were 0 */
    int r7, c7;             /* the first 8x8 cell inside the superblock */
    int w8, h8;             /* the size in 8x8 cells, sub-8x8 sizes count as 1 */
    int tx, uvtx, skip;     /* b->tx, b->uvtx, !b->intra && b->skip */
    int x_end, y_end;       /* the cells inside the picture */
    int col_end, row_end;   /* mask_edges' arguments of the chroma call */
    int lvl_idx;
} Vp9LfBlk;

/* `rec`: the record as one little-endian dword (pos, bs, tx_skip, lvl_idx from the low byte up).  Skipped: bs > 12, a bit above
 * bit 2 of tx_skip, a transform larger than the largest that fits the block, pos not aligned to the block's size, a first cell outside
 * the picture, lvl_idx > 63 (level[] has 64 entries). */
VP9LF_FN Vp9LfBlk vp9lf_block(uint32_t rec, int sb_row, int sb_col, int cols, int rows, int ss_h, int ss_v)
{
    Vp9LfBlk b;
    const int pos = rec & 0xFF, bs = (rec >> 8) & 0xFF, ts = (rec >> 16) & 0xFF;
    /* enum BlockSize: 64x64, 64x32, 32x64, 32x32, 32x16, 16x32, 16x16, 16x8, 8x16, 8x8, 8x4, 4x8, 4x4; log2 of the 8x8 cells, 2 bits
     * each */
    const int lw = bs <= 12 ? (int)(0x000056AFu >> (2 * bs)) & 3 : 0; /* 3 3 2 2 2 1 1 1 0 0 0 0 0 */
    const int lh = bs <= 12 ? (int)(0x000119BBu >> (2 * bs)) & 3 : 0; /* 3 2 3 2 1 2 1 0 1 0 0 0 0 */
    const int lmin = lw < lh ? lw : lh;
    const int max_tx = bs > 9 ? 0 : lmin >= 2 ? 3 : lmin + 1;
    const int row = sb_row * 8 + (pos >> 3 & 7), col = sb_col * 8 + (pos & 7);
    b.r7 = pos >> 3 & 7;
    b.c7 = pos & 7;
    b.w8 = 1 << lw;
    b.h8 = 1 << lh;
    b.tx = ts & 3;
    b.skip = ts >> 2 & 1;
    b.lvl_idx = (int)(rec >> 24);
    b.ok = bs <= 12 && !(ts & ~7) && !(pos & 0xC0) && b.tx <= max_tx && !(b.c7 & (b.w8 - 1)) && !(b.r7 & (b.h8 - 1)) && row < rows &&
           col < cols && b.lvl_idx < 64;
    b.uvtx = b.tx - ((ss_h && b.w8 * 2 == 1 << b.tx) || (ss_v && b.h8 * 2 == 1 << b.tx));
    b.x_end = cols - col < b.w8 ? cols - col : b.w8;
    b.y_end = rows - row < b.h8 ? rows - row : b.h8;
    b.col_end = (cols & 1) && col + b.w8 >= cols ? cols & 7 : 0;
    b.row_end = (rows & 1) && row + b.h8 >= rows ? rows & 7 : 0;
    return b;
}

/* ---- mask_edges ------------------------------------------------------------------------------------------ */
typedef struct Vp9LfEdges {
    int ok;                 /* 0: the call returns before it sets a bit */
    int ss_h, ss_v, r7, w, h, col_end, tx, skip;
    uint32_t t, m_col;
} Vp9LfEdges;

VP9LF_FN Vp9LfEdges vp9lf_mask_edges(int ss_h, int ss_v, int row_and_7, int col_and_7, int w, int h, int col_end, int row_end, int tx,
                                     int skip_inter)
{
    Vp9LfEdges e;
    e.ok = 1;
    if (tx == 0 && (ss_v | ss_h)) {
        /* a 4x4 chroma transform of an 8-sample luma block: the odd row / column has no edge of its own, the even one carries both */
        if (h == ss_v) {
            if (row_and_7 & 1)
                e.ok = 0;
            if (!row_end)
                h += 1;
        }
        if (w == ss_h) {
            if (col_and_7 & 1)
                e.ok = 0;
            if (!col_end)
                w += 1;
        }
    }
    e.ss_h = ss_h; e.ss_v = ss_v; e.r7 = row_and_7; e.w = w; e.h = h; e.col_end = col_end; e.tx = tx; e.skip = skip_inter;
    e.t = 1u << col_and_7;
    e.m_col = ((e.t << w) - e.t) & 0xFF; /* inside the superblock for every block vp9lf_block() passes; a word holds four masks */
    return e;
}

/* what the call ORs into row y: *colw -> mask[0][y], *roww -> mask[1][y] */
VP9LF_FN void vp9lf_mask_row(const Vp9LfEdges *e, int y, uint32_t *colw, uint32_t *roww)
{
    const int d = y - e->r7, ss_h = e->ss_h, ss_v = e->ss_v, tx = e->tx, w = e->w, h = e->h;
    const uint32_t t = e->t, m_col = e->m_col;
    const uint32_t wide_col = ss_h ? 0x01 : 0x11, wide_row = ss_v ? 0x07 : 0x03;
    uint32_t c = 0, r = 0;
    if (e->ok && d >= 0 && d < h) {
        if (tx == 0 && !e->skip) {
            /* on 32-sample edges the 8-wide filter, else the 4-wide one */
            const uint32_t m_row_8 = m_col & wide_col, m_row_4 = m_col - m_row_8, m_odd = (t << (w - 1)) - t;
            const int cid = (y & wide_row) ? 2 : 1;
            c = m_row_8 << 8 | m_row_4 << 16;
            /* on odd rows, when the odd column at the picture's right edge is not filtered, its row edge is not either */
            r = ((ss_h & ss_v) && (e->col_end & 1) && (y & 1) ? m_odd : m_col) << (8 * cid);
            if (!ss_h)
                c |= m_col << 24;
            if (!ss_v)
                r |= (ss_h && (e->col_end & 1) ? m_odd : m_col) << 24;
        } else if (!e->skip) {
            const int mask_id = tx == 1;
            const int l2h = tx + ss_h - 1, l2v = tx + ss_v - 1, step = 1 << l2v;
            const uint32_t every = l2h == 0 ? 0xFF : l2h == 1 ? 0x55 : l2h == 2 ? 0x11 : 0x01;
            const uint32_t m_row = m_col & every;
            if (ss_h && tx > 1 && (w & 1)) {
                /* an odd width: the last column edge has half a transform behind it, 8 wide instead of 16 */
                const uint32_t m_row_16 = ((t << (w - 1)) - t) & every;
                c = m_row_16 | (m_row - m_row_16) << 8;
            } else {
                c = m_row << (8 * mask_id);
            }
            if (!(d & (step - 1))) {
                if (ss_v && tx > 1 && (h & 1))
                    r = d < h - 1 ? m_col : m_col << 8; /* d == h - 1: the last row edge of an odd height, 8 wide */
                else
                    r = m_col << (8 * mask_id);
            }
        } else if (tx != 0) {
            /* a skipped inter block: its outer edges only */
            c = t << (8 * (tx == 1 || w == ss_h));
            if (d == 0)
                r = m_col << (8 * (tx == 1 || h == ss_v));
        } else {
            const uint32_t t8 = t & wide_col;
            c = t8 << 8 | (t - t8) << 16;
            if (d == 0)
                r = m_col << (8 * ((y & wide_row) ? 2 : 1));
        }
    }
    *colw = c;
    *roww = r;
}

/* ---- the tables ------------------------------------------------------------------------------------------ */
VP9LF_FN uint32_t vp9lf_entry(int wd, int L, const uint8_t *lim_lut, const uint8_t *mblim_lut)
{
    const uint32_t wd_idx = wd == 16 ? 2 : wd == 8 ? 1 : 0;
    return 0x80000000u | wd_idx << 24 | (uint32_t)(L >> 4) << 16 | (uint32_t)lim_lut[L] << 8 | mblim_lut[L];
}
/* a valid 16-wide entry: the frame kernels cannot take one on a chroma tile's last 4-sample position */
VP9LF_FN int vp9lf_entry_is_16(uint32_t e)
{
    return (e >> 31) && ((e >> 24) & 3) == 2;
}

/* filter_plane_cols: tab[p][seg], p < np positions, seg < nseg; the item: rows 2 yi (<< ss_v) .. of the mask, position xi.  `mask` is
 * mask[pl][0], `lvl` the levels; 16 items (yi < 2) x 8 when ss_v, else 32 (yi < 4) */
VP9LF_FN void vp9lf_cols_item(uint32_t *tab, int nseg, int col, int ss_h, int ss_v, const uint8_t *lvl, const uint8_t (*mask)[4],
                              const uint8_t *lim_lut, const uint8_t *mblim_lut, int yi, int xi)
{
    const int y = yi * (2 << ss_v);
    const uint8_t *h1 = mask[y], *h2 = mask[y + 1 + ss_v], *lrow = lvl + yi * (16 << ss_v);
    const unsigned hm1 = h1[0] | h1[1] | h1[2], hm13 = h1[3], hm2 = h2[1] | h2[2], hm23 = h2[3];
    const unsigned hm = hm1 | hm2 | hm13 | hm23;
    const unsigned x = 1u << xi;
    const uint8_t *l = lrow + (ss_h ? 2 * (xi >> 1) : xi);
    const int p = ss_h ? xi : 2 * xi;
    uint32_t *up = tab + p * nseg + 2 * yi, *lo = up + 1;
    if (!(hm & ~(x - 1))) /* the reference's loop has ended */
        return;
    if (col || xi) {
        if (hm1 & x) {
            *up = vp9lf_entry((h1[0] & x) ? 16 : (h1[1] & x) ? 8 : 4, l[0], lim_lut, mblim_lut);
            if (h1[0] & x) {
                /* loop_filter_16 when the lower half is 16 wide too — with the UPPER half's level; otherwise the lower
                 * half is not filtered at this position at all, whatever its own 8 / 4 bits say (vp9lpf.c:48-55) */
                if (h2[0] & x)
                    *lo = vp9lf_entry(16, l[0], lim_lut, mblim_lut);
            } else if (hm2 & x) {
                *lo = vp9lf_entry((h2[1] & x) ? 8 : 4, l[8 << ss_v], lim_lut, mblim_lut);
            }
        } else if (hm2 & x) {
            *lo = vp9lf_entry((h2[1] & x) ? 8 : 4, l[8 << ss_v], lim_lut, mblim_lut);
        }
    }
    if (!ss_h) { /* the inner edge of 4x4 transforms, 4 samples further */
        if (hm13 & x)
            up[nseg] = vp9lf_entry(4, l[0], lim_lut, mblim_lut);
        if (hm23 & x)
            lo[nseg] = vp9lf_entry(4, l[8 << ss_v], lim_lut, mblim_lut);
    }
}

/* filter_plane_rows: tab[p][seg], p = row position in units of 4 rows, seg = 8 columns; the item: row y of the mask (y < 8), column
 * pair k (< 2 when ss_h, else < 4).  `mask` is mask[pl][1] */
VP9LF_FN void vp9lf_rows_item(uint32_t *tab, int nseg, int row, int ss_h, int ss_v, const uint8_t *lvl, const uint8_t (*mask)[4],
                              const uint8_t *lim_lut, const uint8_t *mblim_lut, int y, int k)
{
    const uint8_t *vmask = mask[y], *lrow = ss_v ? lvl + 16 * (y >> 1) : lvl + 8 * y;
    const unsigned vm = vmask[0] | vmask[1] | vmask[2], vm3 = vmask[3];
    const int p = ss_v ? y : 2 * y;
    const unsigned x = 1u << (k * (2 << ss_h)), x2 = x << (1 + ss_h);
    const uint8_t *l = lrow + k * (2 << ss_h);
    uint32_t *first = tab + p * nseg + 2 * k, *second = first + 1;
    if (!(vm & ~(x - 1))) /* the loop runs on vm alone: an inner edge beyond its last bit is never reached (vp9lpf.c:116) */
        return;
    if (row || y) {
        if (vm & x) {
            *first = vp9lf_entry((vmask[0] & x) ? 16 : (vmask[1] & x) ? 8 : 4, l[0], lim_lut, mblim_lut);
            if (vmask[0] & x) {
                if (vmask[0] & x2)
                    *second = vp9lf_entry(16, l[0], lim_lut, mblim_lut);
            } else if (vm & x2) {
                *second = vp9lf_entry((vmask[1] & x2) ? 8 : 4, l[1 + ss_h], lim_lut, mblim_lut);
            }
        } else if (vm & x2) {
            *second = vp9lf_entry((vmask[1] & x2) ? 8 : 4, l[1 + ss_h], lim_lut, mblim_lut);
        }
    }
    if (!ss_v) {
        if (vm3 & x)
            first[nseg] = vp9lf_entry(4, l[0], lim_lut, mblim_lut);
        if (vm3 & x2)
            second[nseg] = vp9lf_entry(4, l[1 + ss_h], lim_lut, mblim_lut);
    }
}

/* the geometry of a chroma table where the shifts differ (FFHipVp9LfSbC): positions and segments of the column part, then of the
 * row part, which starts at npc * nsc */
#define VP9LF_C_NPC(ss_h) ((ss_h) ? 8 : 16)
#define VP9LF_C_NSC(ss_v) ((ss_v) ? 4 : 8)
#define VP9LF_C_NPR(ss_v) ((ss_v) ? 8 : 16)
#define VP9LF_C_NSR(ss_h) ((ss_h) ? 4 : 8)

/* Every item of one superblock, numbered: 0..31 the luma columns, 32..63 the luma rows, 64..95 the chroma columns, 96..127 the chroma
 * rows (of tables->uv when ss_h & ss_v, of ctables when ss_h != ss_v, none at 4:4:4; fewer than 32 where a shift halves them).  `y`
 * points to the 256 luma words, `uv` to the 64 chroma words of an FFHipVp9LfSb, `c` to the 128 words of an FFHipVp9LfSbC, all zeroed by
 * the caller.  `row` / `col`: whether the superblock is not in the picture's first row / column. */
VP9LF_FN void vp9lf_table_item(int item, uint32_t *y, uint32_t *uv, uint32_t *c, const FFHipVp9Filter *f, int row, int col, int ss_h,
                               int ss_v, const uint8_t *lim_lut, const uint8_t *mblim_lut)
{
    const int i = item & 31;
    if (item < 32) {
        vp9lf_cols_item(y, 8, col, 0, 0, f->level, f->mask[0][0], lim_lut, mblim_lut, i >> 3, i & 7);
    } else if (item < 64) {
        vp9lf_rows_item(y + 128, 8, row, 0, 0, f->level, f->mask[0][1], lim_lut, mblim_lut, i >> 2, i & 3);
    } else if (ss_h | ss_v) {
        const int both = ss_h & ss_v;
        uint32_t *tc = both ? uv : c, *tr = both ? uv + 32 : c + VP9LF_C_NPC(ss_h) * VP9LF_C_NSC(ss_v);
        if (item < 96) {
            if ((i >> 3) < (ss_v ? 2 : 4))
                vp9lf_cols_item(tc, VP9LF_C_NSC(ss_v), col, ss_h, ss_v, f->level, f->mask[1][0], lim_lut, mblim_lut, i >> 3, i & 7);
        } else if ((i & 3) < (ss_h ? 2 : 4)) {
            vp9lf_rows_item(tr, VP9LF_C_NSR(ss_h), row, ss_h, ss_v, f->level, f->mask[1][1], lim_lut, mblim_lut, i >> 2, i & 3);
        }
    }
}
#define VP9LF_TABLE_ITEMS 128

/* the chroma words on a tile's last 4-sample position, numbered 0..15: the address of word k, or NULL.  4:2:0: uv[d][7][sg], 8 words;
 * otherwise the last position's nsc column words, then the last position's nsr row words of the FFHipVp9LfSbC */
VP9LF_FN uint32_t *vp9lf_last_position(int k, uint32_t *uv, uint32_t *c, int ss_h, int ss_v)
{
    if (ss_h & ss_v)
        return k < 8 ? uv + (k >> 2) * 32 + 7 * 4 + (k & 3) : (uint32_t *)0;
    if (ss_h != ss_v) {
        const int npc = VP9LF_C_NPC(ss_h), nsc = VP9LF_C_NSC(ss_v), npr = VP9LF_C_NPR(ss_v), nsr = VP9LF_C_NSR(ss_h);
        if (k < nsc)
            return c + (npc - 1) * nsc + k;
        if (k < nsc + nsr)
            return c + npc * nsc + (npr - 1) * nsr + (k - nsc);
    }
    return (uint32_t *)0;
}
#define VP9LF_LAST_WORDS 16

#endif
