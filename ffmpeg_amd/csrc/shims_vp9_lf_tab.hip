/*
 * shims_vp9_lf_tab.hip — ffhip_vp9_lf_tables_pictures_dev(): the host checks (geometry, pointers, the level table, output / input
 * overlap through kernels/picture_check.h) and the launch of kernels/vp9_lf_tab_pic.hip on the caller's stream; and the device-free
 * faces: ffhip_vp9_lf_tables_pictures_host(), the same checks and the same rules (kernels/vp9_lf_rules.h) on host arrays, and the
 * record size.
 */
#include <string.h>

#include "kernels/common.h"
#include "kernels/h264_kernels.h"
#include "kernels/vp9_lf_rules.h"
#include "kernels/picture_check.h"

static_assert(sizeof(FFHipVp9LfBlock) == 4, "FFHipVp9LfBlock is a 4-byte record");
static_assert(sizeof(FFHipVp9Filter) == 192 && sizeof(FFHipVp9LfSb) == 1280 && sizeof(FFHipVp9LfSbC) == 512, "the tables' sizes");

extern "C" int ffhip_vp9_lf_block_record_size(void) { return (int)sizeof(FFHipVp9LfBlock); }

namespace {
constexpr int MAX_PICS = 16;          /* the limit of the other whole-picture faces */
constexpr int MAX_BLOCKS = 8 * 1364;  /* the tallest picture the filter faces take, in 8x8 blocks */

/* `n` records of `entry` bytes in a row */
FFHipSpan table_span(const void *base, ptrdiff_t n, size_t entry)
{
    return ffhip_plane_span(base, 0, n * (ptrdiff_t)entry, 1);
}

/* the argument checks of both faces */
int check(const char *who, int ss_h, int ss_v, int cols, int rows, int npics, const FFHipVp9LfTabPic *pics)
{
    if (cols < 1 || rows < 1 || cols > MAX_BLOCKS || rows > MAX_BLOCKS) {
        ffhip_set_error("%s: %d x %d 8x8 blocks (1..%d each)", who, cols, rows, MAX_BLOCKS);
        return FFHIP_EINVAL;
    }
    if ((ss_h & ~1) || (ss_v & ~1)) {
        ffhip_set_error("%s: subsampling %d, %d (0 or 1 each)", who, ss_h, ss_v);
        return FFHIP_EINVAL;
    }
    if (npics > MAX_PICS) {
        ffhip_set_error("%s: npics = %d (1..%d)", who, npics, MAX_PICS);
        return FFHIP_EINVAL;
    }
    if (const int r = ffhip_check_count(who, npics, pics, "picture"))
        return r;
    const ptrdiff_t nsb = (ptrdiff_t)((cols + 7) >> 3) * ((rows + 7) >> 3);
    for (int i = 0; i < npics; i++) {
        const FFHipVp9LfTabPic &P = pics[i];
        if (!P.sb_first || !P.tables || (!P.blocks && P.nblocks) ||
            (((uintptr_t)P.blocks | (uintptr_t)P.sb_first | (uintptr_t)P.tables | (uintptr_t)P.ctables | (uintptr_t)P.filters) & 3)) {
            ffhip_set_error("%s: picture %d: a NULL sb_first or tables, NULL blocks with nblocks %u, or blocks, sb_first or an output that is "
                            "not 4-byte aligned", who, i, P.nblocks);
            return FFHIP_EINVAL;
        }
        if (!P.ctables != (ss_h == ss_v)) {
            ffhip_set_error("%s: picture %d: ctables %s with subsampling %d, %d (required when the two differ, NULL otherwise)", who, i,
                            P.ctables ? "present" : "absent", ss_h, ss_v);
            return FFHIP_EINVAL;
        }
        for (int k = 0; k < 64; k++)
            if (P.level[k] > 63) {
                ffhip_set_error("%s: picture %d: level[%d] = %d (0..63)", who, i, k, P.level[k]);
                return FFHIP_EINVAL;
            }
    }
    /* no output of the call may overlap another one or an input: workgroups of every picture read while others write */
    FFHipSpanSet out;
    out.reserve((size_t)npics * 3);
    for (int i = 0; i < npics; i++) {
        out.add(table_span(pics[i].tables, nsb, sizeof(FFHipVp9LfSb)));
        if (pics[i].ctables)
            out.add(table_span(pics[i].ctables, nsb, sizeof(FFHipVp9LfSbC)));
        if (pics[i].filters)
            out.add(table_span(pics[i].filters, nsb, sizeof(FFHipVp9Filter)));
    }
    if (out.seal()) {
        ffhip_set_error("%s: an output overlaps another output of the call", who);
        return FFHIP_EINVAL;
    }
    for (int i = 0; i < npics; i++)
        if (out.hits(table_span(pics[i].blocks, pics[i].nblocks, sizeof(FFHipVp9LfBlock))) ||
            out.hits(table_span(pics[i].sb_first, nsb + 1, sizeof(uint32_t)))) {
            ffhip_set_error("%s: picture %d: an input overlaps an output of the call", who, i);
            return FFHIP_EINVAL;
        }
    return 0;
}
} // namespace

extern "C" int ffhip_vp9_lf_tables_pictures_dev(int ss_h, int ss_v, int cols, int rows, int npics, const FFHipVp9LfTabPic *pics, void *stream)
{
    const int r = check("ffhip_vp9_lf_tables_pictures_dev", ss_h, ss_v, cols, rows, npics, pics);
    if (r < 0)
        return r;
    if (!ffhip_have_device())
        return FFHIP_ENOSYS;
    return ffhip_launch_vp9_lf_tables_pictures(ss_h, ss_v, cols, rows, npics, pics, (hipStream_t)stream);
}

extern "C" int ffhip_vp9_lf_tables_pictures_host(int ss_h, int ss_v, int cols, int rows, int npics, const FFHipVp9LfTabPic *pics)
{
    const int r = check("ffhip_vp9_lf_tables_pictures_host", ss_h, ss_v, cols, rows, npics, pics);
    if (r < 0)
        return r;
    const int sb_cols = (cols + 7) >> 3, sb_rows = (rows + 7) >> 3;
    for (int i = 0; i < npics; i++) {
        const FFHipVp9LfTabPic &P = pics[i];
        for (int sb = 0; sb < sb_cols * sb_rows; sb++) {
            const int sb_row = sb / sb_cols, sb_col = sb - sb_row * sb_cols;
            FFHipVp9Filter f;
            memset(&f, 0, sizeof(f));
            uint32_t first, last;
            memcpy(&first, P.sb_first + sb, 4);
            memcpy(&last, P.sb_first + sb + 1, 4);
            first = first < P.nblocks ? first : P.nblocks;
            last = last < P.nblocks ? last : P.nblocks;
            for (uint32_t k = first; k < last; k++) {
                uint32_t rec;
                memcpy(&rec, P.blocks + k, 4);
                const Vp9LfBlk b = vp9lf_block(rec, sb_row, sb_col, cols, rows, ss_h, ss_v);
                const int lvl = b.ok ? P.level[b.lvl_idx] : 0;
                if (!lvl)
                    continue;
                for (int y = b.r7; y < b.r7 + b.h8 && y < 8; y++)
                    for (int x = b.c7; x < b.c7 + b.w8 && x < 8; x++)
                        f.level[y * 8 + x] = (uint8_t)lvl;
                const Vp9LfEdges ey = vp9lf_mask_edges(0, 0, b.r7, b.c7, b.x_end, b.y_end, 0, 0, b.tx, b.skip);
                const Vp9LfEdges ec = vp9lf_mask_edges(ss_h, ss_v, b.r7, b.c7, b.x_end, b.y_end, b.col_end, b.row_end, b.uvtx, b.skip);
                for (int y = 0; y < 8; y++)
                    for (int pl = 0; pl < ((ss_h | ss_v) ? 2 : 1); pl++) {
                        uint32_t w[2];
                        vp9lf_mask_row(pl ? &ec : &ey, y, &w[0], &w[1]);
                        for (int d = 0; d < 2; d++)
                            for (int m = 0; m < 4; m++)
                                f.mask[pl][d][y][m] |= (uint8_t)(w[d] >> (8 * m));
                    }
            }
            uint32_t tab[320 + 128];
            memset(tab, 0, sizeof(tab));
            for (int item = 0; item < VP9LF_TABLE_ITEMS; item++)
                vp9lf_table_item(item, tab, tab + 256, tab + 320, &f, sb_row, sb_col, ss_h, ss_v, P.lim_lut, P.mblim_lut);
            for (int k = 0; k < VP9LF_LAST_WORDS; k++)
                if (uint32_t *w = vp9lf_last_position(k, tab + 256, tab + 320, ss_h, ss_v))
                    if (vp9lf_entry_is_16(*w))
                        *w = 0;
            memcpy(P.tables + sb, tab, sizeof(FFHipVp9LfSb));
            if (P.ctables)
                memcpy(P.ctables + sb, tab + 320, sizeof(FFHipVp9LfSbC));
            if (P.filters)
                memcpy(P.filters + sb, &f, sizeof(f));
        }
    }
    return 0;
}
