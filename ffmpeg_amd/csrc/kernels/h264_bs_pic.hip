/*
 * h264_bs_pic.hip — H.264 deblocking edge parameters of whole pictures in one launch (ffhip_h264_edge_params_pictures_dev): the
 * FFHipH264Edge tables ffhip_h264_deblock_frames_dev / _chroma_dev / _dev_hbd read, from the macroblock records, the motion field and
 * the slice table.
 *
 * A gather with no dependency chain: one workgroup of 256 lanes per (picture, tile of 4 x 4 macroblocks = 16 x 16 blocks).
 *   1. the up to 5 x 5 macroblock records of the tile, the column to its left and the row above go to LDS resolved
 *      (h264_bs_rules.h's h264bs_resolve_mb): the slice table is read once per macroblock for everything but the references;
 *   2. the tile's FFHipH264MvField records plus the column to its left and the row above (clipped to the picture) go to LDS as
 *      dwords: a row of 17 records is 51 consecutive dwords of the map, so the loads are 4-byte aligned and coalesced;
 *   3. each record is resolved in place (h264bs_resolve_blk): its third dword (ref_idx) becomes the two pictures it refers to
 *      and the vector of an unused list becomes 0, so the slice's lists are read once per block, not once per comparison;
 *   4. one lane per output record, 16 per macroblock, from LDS alone.  A wave is one macroblock row of the tile: lanes 0..31 write the 32
 *      consecutive luma records of its four macroblocks, lanes 32..47 the 16 consecutive Cb records, lanes 48..63 the Cr ones, each
 *      lane one whole 12-byte record as three dwords.  A chroma lane derives the bS of its luma edge again: the blocks are in LDS,
 *      and no lane waits for another.  That is the 4:2:0 instantiation (32 + 16 + 16 records a wave).  At 4:2:2 a wave has 32 + 24 + 24
 *      records (six per macroblock and chroma plane) and at 4:4:4 32 + 32 + 32 (the chroma tables in the luma layout): slot s = lane and
 *      then lane + 64 over luma, Cb, Cr in that order, so consecutive lanes still write consecutive records of one table, and the second
 *      pass has 16 / 32 live lanes.
 * Every record of a macroblock inside the picture is written once, by the workgroup of its tile; nothing else is.
 */
#include <stddef.h>

#include "common.h"
#include "h264_kernels.h"
#include "h264_bs_rules.h"

static_assert(sizeof(FFHipH264MvField) == 12, "FFHipH264MvField is read as three dwords");
static_assert(sizeof(FFHipH264BsMb) == 8, "FFHipH264BsMb is an 8-byte record");
static_assert(sizeof(FFHipH264BsSlice) == 72, "FFHipH264BsSlice is a 72-byte record");
static_assert(sizeof(FFHipH264Edge) == 12, "FFHipH264Edge is written as three dwords");
static_assert(sizeof(FFHipH264BsPic) % 8 == 0, "FFHipH264BsPic is staged as an array");

#define H4P_PICS 16 /* pictures per launch: their FFHipH264BsPic structs travel in one progress-pool slot */
static_assert(H4P_PICS * sizeof(FFHipH264BsPic) <= FFHIP_PROGRESS_SLOT_INTS * sizeof(int), "a launch's pictures fit one slot");

namespace {
constexpr int TM = 4;          /* macroblocks per tile side */
constexpr int TMP = TM + 1;    /* with the column to the left / the row above */
constexpr int T = 4 * TM;      /* blocks per tile side */
constexpr int TP = T + 1;

/* FMT: 1 the 4:2:0 chroma tables (a picture without them has NULL cb: monochrome), 2 the 4:2:2 ones, 3 the 4:4:4 ones */
template <int FMT>
__global__ __launch_bounds__(256) void k_h264_edge_params(const FFHipH264BsPic *pics, int mb_w, int mb_h, int field, int qp_bd_offset, int tiles_x)
{
    constexpr int CPER = FMT == 3 ? 8 : FMT == 2 ? 6 : 4; /* records of a macroblock in cb / cr */
    __shared__ uint32_t unit[TP * TP * 3]; /* [row][col] of 3 dwords; row 0 / col 0: the neighbours above / to the left */
    __shared__ uint32_t mbs[TMP * TMP * 2]; /* H264BsMb, the same arrangement */
    const int tid = threadIdx.x, ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const FFHipH264BsPic &P = pics[blockIdx.y];
    const int mx0 = tx * TM, my0 = ty * TM, ux0 = mx0 * 4, uy0 = my0 * 4, w4 = mb_w * 4, h4 = mb_h * 4;
    /* the macroblocks and the blocks staged: [smx0, smx1) x [smy0, smy1), [sx0, sx1) x [sy0, sy1) */
    const int smx0 = max(mx0 - 1, 0), smy0 = max(my0 - 1, 0), smx1 = min(mx0 + TM, mb_w), smy1 = min(my0 + TM, mb_h);
    const int sx0 = max(ux0 - 1, 0), sy0 = max(uy0 - 1, 0), sx1 = min(ux0 + T, w4), sy1 = min(uy0 + T, h4);

    /* ---- 1. the macroblocks ---- */
    if (tid < TMP * TMP) {
        const int j = tid / TMP, i = tid - j * TMP, mx = mx0 - 1 + i, my = my0 - 1 + j;
        if (mx >= smx0 && mx < smx1 && my >= smy0 && my < smy1) {
            const H264BsMb r = h264bs_resolve_mb(P.mb[(ptrdiff_t)my * mb_w + mx], P.slices, P.nslices);
            mbs[tid * 2] = r.a;
            mbs[tid * 2 + 1] = r.b;
        }
    }
    /* ---- 2. the motion records, a dword per item ---- */
    const int nd = (sx1 - sx0) * 3, nrows = sy1 - sy0;
    const uint32_t *mvf = reinterpret_cast<const uint32_t *>(P.mvf);
    for (int i = tid; i < nd * nrows; i += 256) {
        const int r = i / nd, d = i - r * nd;
        unit[((sy0 + r - uy0 + 1) * TP + (sx0 - ux0 + 1)) * 3 + d] = mvf[((ptrdiff_t)(sy0 + r) * P.mvf_stride + sx0) * 3 + d];
    }
    __syncthreads();
    auto mb_at = [&](int mx, int my) {
        const uint32_t *m = mbs + ((my - my0 + 1) * TMP + (mx - mx0 + 1)) * 2;
        H264BsMb v;
        v.a = m[0]; v.b = m[1];
        return v;
    };
    /* ---- 3. resolve in place ---- */
    const int nu = sx1 - sx0;
    for (int i = tid; i < nu * nrows; i += 256) {
        const int r = i / nu, ux = sx0 + (i - r * nu), uy = sy0 + r;
        uint32_t *u = unit + ((uy - uy0 + 1) * TP + (ux - ux0 + 1)) * 3;
        const H264BsBlk b = h264bs_resolve_blk(u[0], u[1], u[2], mb_at(ux >> 2, uy >> 2), P.slices);
        u[0] = b.mv[0]; u[1] = b.mv[1]; u[2] = b.refs;
    }
    __syncthreads();
    /* ---- 4. one lane per record ---- */
    const int lane = tid & 63, my = my0 + (tid >> 6);
    if constexpr (FMT <= 1) {
        /* 32 + 16 + 16 records, one pass; this branch is the kernel as it was before it had a format, statement for statement, so that
         * the 4:2:0 instantiation stays the code it was */
        const bool chroma = lane >= 32;
        const int mx = mx0 + (chroma ? (lane & 15) >> 2 : lane >> 3), dir = chroma ? (lane >> 1) & 1 : (lane >> 2) & 1;
        const int e = chroma ? (lane & 1) * 2 : lane & 3, plane = (lane >> 4) & 1; /* of a chroma lane: 0 Cb, 1 Cr */
        if (mx >= mb_w || my >= mb_h || (chroma && !P.cb))
            return;
        const H264BsMb q = mb_at(mx, my);
        const bool border = dir ? my == 0 : mx == 0;
        const H264BsMb p = e || border ? q : mb_at(mx - (dir ? 0 : 1), my - (dir ? 1 : 0));
        const uint32_t bs = h264bs_edge_bs(p, q, border, dir, e, field, [&](int x, int y) {
            const uint32_t *u = unit + ((my * 4 + y - uy0 + 1) * TP + (mx * 4 + x - ux0 + 1)) * 3;
            H264BsBlk v;
            v.mv[0] = u[0]; v.mv[1] = u[1]; v.refs = u[2];
            return v;
        });
        uint32_t out[3];
        h264bs_pack(chroma, dir, bs, bs ? h264bs_edge_qp(p, q, e, chroma ? P.chroma_qp + plane * H264BS_QP_ENTRIES : nullptr) : 0, q, qp_bd_offset, out);
        const ptrdiff_t mb = (ptrdiff_t)my * mb_w + mx;
        FFHipH264Edge *rec = chroma ? (plane ? P.cr : P.cb) + (mb * 2 + dir) * 2 + (e >> 1) : P.luma + (mb * 2 + dir) * 4 + e;
        uint32_t *o = reinterpret_cast<uint32_t *>(rec);
        o[0] = out[0]; o[1] = out[1]; o[2] = out[2];
    } else {
        /* 32 + 24 + 24 (4:2:2) or 32 + 32 + 32 (4:4:4) records: slot s = lane, then lane + 64; the slots of a table are consecutive
         * records of it */
        constexpr int CROW = TM * CPER; /* a plane's chroma records of the wave */
#pragma unroll
        for (int s = lane; s < 32 + 2 * CROW; s += 64) {
            const bool chroma = s >= 32;
            const int c = chroma ? s - 32 : s, plane = chroma && c >= CROW, i = plane ? c - CROW : c; /* i: the record within its table's run */
            /* the luma layout: 8 records per macroblock; 4:2:2 chroma: 6, k 0, 1 the vertical edges x = 0, 4 (luma edges 0, 2), k 2..5 the
             * horizontal edges y = 4 (k - 2), which take h264bs_edge_bs's c422h form */
            const bool six = FMT == 2 && chroma;
            const int m = six ? i / 6 : i >> 3, k = six ? i - m * 6 : i & 7, mx = mx0 + m;
            const int dir = six ? k >= 2 : k >> 2, e = six ? (k < 2 ? 2 * k : k - 2) : k & 3;
            if (mx >= mb_w || my >= mb_h || (chroma && !P.cb))
                continue;
            const H264BsMb q = mb_at(mx, my);
            const bool border = dir ? my == 0 : mx == 0;
            const H264BsMb p = e || border ? q : mb_at(mx - (dir ? 0 : 1), my - (dir ? 1 : 0));
            const uint32_t bs = h264bs_edge_bs(p, q, border, dir, e, field, [&](int x, int y) {
                const uint32_t *u = unit + ((my * 4 + y - uy0 + 1) * TP + (mx * 4 + x - ux0 + 1)) * 3;
                H264BsBlk v;
                v.mv[0] = u[0]; v.mv[1] = u[1]; v.refs = u[2];
                return v;
            }, six && dir);
            uint32_t out[3];
            h264bs_pack(six, dir, bs, bs ? h264bs_edge_qp(p, q, e, chroma ? P.chroma_qp + plane * H264BS_QP_ENTRIES : nullptr) : 0, q, qp_bd_offset, out);
            const ptrdiff_t mb = (ptrdiff_t)my * mb_w + mx;
            FFHipH264Edge *rec = chroma ? (plane ? P.cr : P.cb) + mb * CPER + k : P.luma + mb * 8 + k;
            uint32_t *o = reinterpret_cast<uint32_t *>(rec);
            o[0] = out[0]; o[1] = out[1]; o[2] = out[2];
        }
    }
}
} // namespace

/* fmt: the format of the chroma tables, 1 (a picture with NULL cb has none), 2 or 3 */
int ffhip_launch_h264_edge_params_pictures(int fmt, int mb_w, int mb_h, int field, int qp_bd_offset, int npics, const FFHipH264BsPic *pics,
                                           hipStream_t stream)
{
    const auto kernel = fmt == 3 ? k_h264_edge_params<3> : fmt == 2 ? k_h264_edge_params<2> : k_h264_edge_params<1>;
    const int tiles_x = (mb_w + TM - 1) / TM, tiles_y = (mb_h + TM - 1) / TM; /* at most 1024 x 1024 tiles: inside the grid's x limit */
    for (int p0 = 0; p0 < npics; p0 += H4P_PICS) {
        const int n = npics - p0 < H4P_PICS ? npics - p0 : H4P_PICS;
        const int r = ffhip_progress_launch_table(stream, "ffhip_h264_edge_params_pictures_dev: copy or launch", pics + p0, n,
                                                  [&](FFHipH264BsPic *dpics) {
            hipLaunchKernelGGL(kernel, dim3(tiles_x * tiles_y, n), dim3(256), 0, stream, dpics, mb_w, mb_h, field, qp_bd_offset, tiles_x);
        });
        if (r < 0)
            return r;
    }
    return 0;
}
