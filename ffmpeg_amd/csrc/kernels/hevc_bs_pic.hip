/*
 * hevc_bs_pic.hip — HEVC deblocking boundary strengths of whole pictures in one launch (ffhip_hevc_boundary_strengths_pictures_dev):
 * bs_ver / bs_hor, the maps the in-loop filter (hevc_lf_pic.hip) reads, from the motion field, the tu marks and the slice / tile ids.
 *
 * A gather with no dependency chain: one workgroup of 256 lanes per (picture, 64 x 64 luma tile = 16 x 16 units), whatever the CTB
 * size, so a tile holds 1, 4 or 16 CTBs.
 *   1. the slice index and tile id of the up to 5 x 5 CTBs the tile and its left column / top row touch go to LDS;
 *   2. the tile's FFHipHevcMvField records plus the column to its left and the row above (clipped to the picture) go to LDS as
 *      dwords: a row of 17 records is 51 consecutive dwords of the map, so the loads are 4-byte aligned and coalesced;
 *   3. each record is resolved in place (hevc_bs_rules.h's hbs_resolve): its third dword (ref_idx, pred_flag) becomes the word
 *      with the DPB slots, the tu byte and the slice's flags, so the slice table is read once per unit, not once per comparison;
 *   4. one lane per unit computes its vertical and its horizontal segment from LDS alone; two cross-lane moves collect four units
 *      along x, and every fourth lane stores one dword per map (bytes where a map's base or stride is not 4-byte aligned, or the
 *      row ends inside the dword).
 * Every entry inside w4 x h4 is written once, by the workgroup of its tile; nothing else is.  Records are 3 dwords apart in LDS:
 * consecutive lanes hit distinct banks.
 */
#include <stddef.h>

#include "common.h"
#include "h264_kernels.h"
#include "hevc_bs_rules.h"

static_assert(sizeof(FFHipHevcMvField) == 12, "FFHipHevcMvField is read as three dwords");
static_assert(sizeof(FFHipHevcBsSlice) == 36, "FFHipHevcBsSlice is a 36-byte record");
static_assert(sizeof(FFHipHevcBsPic) % 8 == 0, "FFHipHevcBsPic is staged as an array");

#define HBP_PICS 16 /* pictures per launch: their FFHipHevcBsPic structs travel in one progress-pool slot */
static_assert(HBP_PICS * sizeof(FFHipHevcBsPic) <= FFHIP_PROGRESS_SLOT_INTS * sizeof(int), "a launch's pictures fit one slot");

namespace {
constexpr int T = 16;      /* units per tile side */
constexpr int TP = T + 1;  /* with the column to the left / the row above */
constexpr int NCTB = 5;    /* CTBs per side a tile and its neighbours touch, at most (16-sample CTBs) */

__global__ __launch_bounds__(256) void k_hevc_bs_pic(const FFHipHevcBsPic *pics, int w4, int h4, int lctb, int ctb_w, int ctb_h, int tiles_x)
{
    __shared__ uint32_t unit[TP * TP * 3]; /* [row][col] of 3 dwords; row 0 / col 0: the neighbours above / to the left */
    __shared__ uint32_t ctbs[NCTB * NCTB]; /* slice index | tile id << 16 */
    const int tid = threadIdx.x, ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const FFHipHevcBsPic &P = pics[blockIdx.y];
    const int ux0 = tx * T, uy0 = ty * T;
    /* the units staged: [sx0, sx1) x [sy0, sy1) */
    const int sx0 = max(ux0 - 1, 0), sy0 = max(uy0 - 1, 0), sx1 = min(ux0 + T, w4), sy1 = min(uy0 + T, h4);
    const int lu = lctb - 2, cx0 = sx0 >> lu, cy0 = sy0 >> lu; /* the first CTB column / row staged */

    /* ---- 1. CTB ids ---- */
    if (tid < NCTB * NCTB) {
        const int j = tid / NCTB, i = tid - j * NCTB, cx = cx0 + i, cy = cy0 + j;
        if (cx < ctb_w && cy < ctb_h && cx <= (sx1 - 1) >> lu && cy <= (sy1 - 1) >> lu) {
            const int a = cy * ctb_w + cx;
            ctbs[tid] = (uint32_t)P.ctb_slice[a] | (P.ctb_tile ? (uint32_t)P.ctb_tile[a] << 16 : 0u);
        }
    }
    /* ---- 2. the records, a dword per item ---- */
    const int nd = (sx1 - sx0) * 3, nrows = sy1 - sy0;
    const uint32_t *mvf = reinterpret_cast<const uint32_t *>(P.mvf);
    for (int i = tid; i < nd * nrows; i += 256) {
        const int r = i / nd, d = i - r * nd;
        unit[((sy0 + r - uy0 + 1) * TP + (sx0 - ux0 + 1)) * 3 + d] = mvf[((ptrdiff_t)(sy0 + r) * P.mvf_stride + sx0) * 3 + d];
    }
    __syncthreads();
    /* ---- 3. resolve in place ---- */
    const int nu = sx1 - sx0;
    for (int i = tid; i < nu * nrows; i += 256) {
        const int r = i / nu, ux = sx0 + (i - r * nu), uy = sy0 + r;
        uint32_t *u = unit + ((uy - uy0 + 1) * TP + (ux - ux0 + 1)) * 3;
        const unsigned slice = ctbs[((uy >> lu) - cy0) * NCTB + ((ux >> lu) - cx0)] & 0xFFFF;
        u[2] = hbs_resolve(u[0], u[1], u[2], P.tu[(ptrdiff_t)uy * P.tu_stride + ux], P.slices, P.nslices, slice).info;
    }
    __syncthreads();
    /* ---- 4. one lane per unit; lanes outside the picture carry zeros through the cross-lane moves ---- */
    const int lx = tid & (T - 1), ly = tid >> 4, ux = ux0 + lx, uy = uy0 + ly;
    uint32_t w = 0;
    if (ux < w4 && uy < h4) {
        auto at = [&](int x, int y) {
            const uint32_t *u = unit + ((y - uy0 + 1) * TP + (x - ux0 + 1)) * 3;
            HbsUnit v;
            v.mv[0] = u[0]; v.mv[1] = u[1]; v.info = u[2];
            return v;
        };
        auto ctb = [&](int x, int y) { return ctbs[((y >> lu) - cy0) * NCTB + ((x >> lu) - cx0)]; };
        const HbsUnit q = at(ux, uy);
        const uint32_t cq = ctb(ux, uy);
        const bool across = P.loop_filter_across_tiles != 0;
        if (hbs_on_grid(ux)) {
            const uint32_t cp = ctb(ux - 1, uy);
            w = (uint32_t)hbs_segment(at(ux - 1, uy), q, 0, (cp & 0xFFFF) == (cq & 0xFFFF), cp >> 16 == cq >> 16, across);
        }
        if (hbs_on_grid(uy)) {
            const uint32_t cp = ctb(ux, uy - 1);
            w |= (uint32_t)hbs_segment(at(ux, uy - 1), q, 1, (cp & 0xFFFF) == (cq & 0xFFFF), cp >> 16 == cq >> 16, across) << 8;
        }
    }
    /* w: ver | hor << 8 of this unit.  Rows are 16 lanes of one wave, so lanes lx + 1 .. lx + 3 are this lane's neighbours */
    w |= (uint32_t)__shfl_down((int)w, 1) << 16; /* ver0, hor0, ver1, hor1 */
    const uint32_t w2 = (uint32_t)__shfl_down((int)w, 2);
    if ((lx & 3) || ux >= w4 || uy >= h4)
        return;
    const uint32_t ver = (w & 0xFF) | (w >> 8 & 0xFF00) | (w2 & 0xFF) << 16 | (w2 >> 16 & 0xFF) << 24;
    const uint32_t hor = (w >> 8 & 0xFF) | (w >> 16 & 0xFF00) | (w2 >> 8 & 0xFF) << 16 | (w2 >> 24) << 24;
    const int n = min(4, w4 - ux); /* 4, or 2 at the end of a row */
    const ptrdiff_t o = (ptrdiff_t)uy * P.bs_stride + ux;
    uint8_t *const dst[2] = { P.bs_ver + o, P.bs_hor + o };
    const uint32_t val[2] = { ver, hor };
#pragma unroll
    for (int m = 0; m < 2; m++) {
        if (n == 4 && !((uintptr_t)dst[m] & 3)) {
            *reinterpret_cast<uint32_t *>(dst[m]) = val[m];
        } else {
            for (int k = 0; k < n; k++)
                dst[m][k] = (uint8_t)(val[m] >> (8 * k));
        }
    }
}
} // namespace

int ffhip_launch_hevc_boundary_strengths_pictures(int width, int height, int log2_ctb, int npics, const FFHipHevcBsPic *pics, hipStream_t stream)
{
    const int C = 1 << log2_ctb, ctb_w = (width + C - 1) / C, ctb_h = (height + C - 1) / C;
    const int w4 = width >> 2, h4 = height >> 2, tiles_x = (w4 + T - 1) / T, tiles_y = (h4 + T - 1) / T;
    for (int p0 = 0; p0 < npics; p0 += HBP_PICS) {
        const int n = npics - p0 < HBP_PICS ? npics - p0 : HBP_PICS;
        const int r = ffhip_progress_launch_table(stream, "ffhip_hevc_boundary_strengths_pictures_dev: copy or launch", pics + p0, n,
                                                  [&](FFHipHevcBsPic *dpics) {
            hipLaunchKernelGGL(k_hevc_bs_pic, dim3(tiles_x * tiles_y, n), dim3(256), 0, stream, dpics, w4, h4, log2_ctb, ctb_w, ctb_h, tiles_x);
        });
        if (r < 0)
            return r;
    }
    return 0;
}
