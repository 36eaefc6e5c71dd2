/*
 * vp9_lf_tab_pic.hip — the VP9 loop-filter tables of whole frames in one launch (ffhip_vp9_lf_tables_pictures_dev): the FFHipVp9LfSb /
 * FFHipVp9LfSbC tables ffhip_vp9_loopfilter_frames_dev / _ssc_dev read, from one 4-byte record per decoded block.  The rules are
 * vp9_lf_rules.h's, the ones the host faces run.
 *
 * No dependency between superblocks: one workgroup of ONE wave per (superblock, picture), so the workgroup's LDS is the wave's own
 * and __syncthreads() costs a wave nothing but the wait for its own LDS traffic.  In LDS: the superblock's VP9Filter (48 words: 16
 * of levels, then mask[pl][dir][y] as one word each, byte k = mask[pl][dir][y][k]) and the 320 + 128 words of the two tables.
 *   0. both are zeroed;
 *   1. lane = record, 64 records at a time, any number of times: the lane validates its record (vp9lf_block), looks its level up, writes
 *      the level into its cells as bytes and ORs what its two mask_edges calls set into the mask words with LDS atomics (at most 32, the
 *      zero ones are not sent).  The blocks of a valid superblock are disjoint; where malformed records overlap, the masks are still the
 *      union and a cell's level is that of ANY ONE of the records that cover it (the host face: the last one);
 *   2. lane = one (row group, position) of filter_plane_cols / _rows (vp9lf_table_item, 128 of them, two per lane): the reference's loop
 *      exit is a function of the masks, so the lane decides it for itself, and no two items write the same entry;
 *   3. a 16-wide chroma entry on the tile's last position is cleared (the frame kernels cannot take one; no record set that passes
 *      vp9lf_block produces one: docs/KERNELS.md);
 *   4. the tables go out as consecutive dwords, zeros included, and the VP9Filter when the caller wants it.
 * Reads: sb_first[sb], sb_first[sb + 1] (clamped to nblocks, a decreasing pair is empty), the records between them, level[lvl_idx < 64]
 * and the two 64-entry luts at a level (< 64, checked by the face).  Writes: the superblock's own records of the outputs.
 */
#include <stddef.h>

#include "common.h"
#include "h264_kernels.h"
#include "progress_pool.h"
#include "vp9_lf_rules.h"

static_assert(sizeof(FFHipVp9LfBlock) == 4, "FFHipVp9LfBlock is read as one dword");
static_assert(sizeof(FFHipVp9Filter) == 48 * 4 && offsetof(FFHipVp9Filter, mask) == 64, "the VP9Filter is 16 + 32 words");
static_assert(sizeof(FFHipVp9LfSb) == 320 * 4 && offsetof(FFHipVp9LfSb, uv) == 256 * 4 && sizeof(FFHipVp9LfSbC) == 128 * 4, "the tables' words");
static_assert(sizeof(FFHipVp9LfTabPic) % 8 == 0, "FFHipVp9LfTabPic is staged as an array");

#define VLT_PICS 16 /* pictures per launch: their FFHipVp9LfTabPic structs travel in one progress-pool slot */
static_assert(VLT_PICS * sizeof(FFHipVp9LfTabPic) <= FFHIP_PROGRESS_SLOT_INTS * sizeof(int), "a launch's pictures fit one slot");

namespace {
__global__ __launch_bounds__(64) void k_vp9_lf_tables(const FFHipVp9LfTabPic *pics, int ss_h, int ss_v, int cols, int rows, int sb_cols)
{
    __shared__ FFHipVp9Filter filt;
    __shared__ uint32_t tab[320 + 128];
    const int lane = threadIdx.x, sb = blockIdx.x, sb_row = sb / sb_cols, sb_col = sb - sb_row * sb_cols;
    const FFHipVp9LfTabPic &P = pics[blockIdx.y];
    uint32_t *fw = reinterpret_cast<uint32_t *>(&filt), *mw = fw + 16; /* mw[(pl * 2 + dir) * 8 + y] */

    /* ---- 0. ---- */
    if (lane < 48)
        fw[lane] = 0;
    for (int i = lane; i < 320 + 128; i += 64)
        tab[i] = 0;
    __syncthreads();

    /* ---- 1. lane = record ---- */
    const uint32_t nb = P.nblocks, f0 = P.sb_first[sb], f1 = P.sb_first[sb + 1];
    const uint32_t first = f0 < nb ? f0 : nb, last = f1 < nb ? f1 : nb;
    const uint32_t *recs = reinterpret_cast<const uint32_t *>(P.blocks);
    for (uint32_t base = first; base < last; base += 64) { /* first, last: the same in every lane; base + lane <= nb: no wrap */
        if ((uint32_t)lane >= last - base)
            continue;
        const Vp9LfBlk b = vp9lf_block(recs[base + lane], sb_row, sb_col, cols, rows, ss_h, ss_v);
        const int lvl = b.ok ? P.level[b.lvl_idx] : 0;
        if (!lvl)
            continue;
        for (int y = b.r7; y < b.r7 + b.h8 && y < 8; y++)
            for (int x = b.c7; x < b.c7 + b.w8 && x < 8; x++)
                filt.level[y * 8 + x] = (uint8_t)lvl;
        const Vp9LfEdges ey = vp9lf_mask_edges(0, 0, b.r7, b.c7, b.x_end, b.y_end, 0, 0, b.tx, b.skip);
        const Vp9LfEdges ec = vp9lf_mask_edges(ss_h, ss_v, b.r7, b.c7, b.x_end, b.y_end, b.col_end, b.row_end, b.uvtx, b.skip);
        for (int y = 0; y < 8; y++) {
            uint32_t c, r;
            vp9lf_mask_row(&ey, y, &c, &r);
            if (c)
                atomicOr(mw + y, c);
            if (r)
                atomicOr(mw + 8 + y, r);
            if (ss_h | ss_v) {
                vp9lf_mask_row(&ec, y, &c, &r);
                if (c)
                    atomicOr(mw + 16 + y, c);
                if (r)
                    atomicOr(mw + 24 + y, r);
            }
        }
    }
    __syncthreads();

    /* ---- 2. lane = (row group, position) ---- */
    for (int item = lane; item < VP9LF_TABLE_ITEMS; item += 64)
        vp9lf_table_item(item, tab, tab + 256, tab + 320, &filt, sb_row, sb_col, ss_h, ss_v, P.lim_lut, P.mblim_lut);
    __syncthreads();

    /* ---- 3. ---- */
    if (lane < VP9LF_LAST_WORDS) {
        uint32_t *w = vp9lf_last_position(lane, tab + 256, tab + 320, ss_h, ss_v);
        if (w && vp9lf_entry_is_16(*w))
            *w = 0;
    }
    __syncthreads();

    /* ---- 4. ---- */
    uint32_t *out = reinterpret_cast<uint32_t *>(P.tables + sb);
    for (int i = lane; i < 320; i += 64)
        out[i] = tab[i];
    if (P.ctables) {
        uint32_t *cout = reinterpret_cast<uint32_t *>(P.ctables + sb);
        for (int i = lane; i < 128; i += 64)
            cout[i] = tab[320 + i];
    }
    if (P.filters && lane < 48)
        reinterpret_cast<uint32_t *>(P.filters + sb)[lane] = fw[lane];
}
} // namespace

int ffhip_launch_vp9_lf_tables_pictures(int ss_h, int ss_v, int cols, int rows, int npics, const FFHipVp9LfTabPic *pics, hipStream_t stream)
{
    const int sb_cols = (cols + 7) >> 3, sb_rows = (rows + 7) >> 3; /* at most 1364 x 1364 superblocks: inside the grid's x limit */
    for (int p0 = 0; p0 < npics; p0 += VLT_PICS) {
        const int n = npics - p0 < VLT_PICS ? npics - p0 : VLT_PICS;
        const int r = ffhip_progress_launch_table(stream, "ffhip_vp9_lf_tables_pictures_dev: copy or launch", pics + p0, n,
                                                  [&](FFHipVp9LfTabPic *dpics) {
            hipLaunchKernelGGL(k_vp9_lf_tables, dim3(sb_cols * sb_rows, n), dim3(64), 0, stream, dpics, ss_h, ss_v, cols, rows, sb_cols);
        });
        if (r < 0)
            return r;
    }
    return 0;
}
