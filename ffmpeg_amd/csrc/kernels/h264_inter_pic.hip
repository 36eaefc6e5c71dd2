/*
 * h264_inter_pic.hip — H.264 inter prediction of whole pictures in one launch (ffhip_h264_inter_pictures_dev and its _fmt face): the
 * predicted samples of every inter macroblock from the macroblock records, the 4x4 motion field and the slice table the
 * edge-parameter face (h264_bs_pic.hip) takes, both lists and the weighting combined in registers, every sample written once.
 *
 * One workgroup of 4 waves per (picture, macroblock); an intra macroblock's workgroup exits at once.  Wave q takes the 8x8 quadrant q
 * as four 4x4 blocks of 16 lanes, a lane per luma sample.  Nothing is shared between waves, so there is no workgroup barrier:
 *   1. every lane resolves its block's plan (h264_inter_rules.h): the 16 lanes of a block read the same words, which broadcast;
 *   2. per list: the 16 lanes of a block fetch the clamped 9x9 reference window of the block (only the rows / columns the position's
 *      filter reads) into wave-private LDS, then each lane filters its sample from LDS; lanes 0..7 of the block compute the 2x2 Cb and
 *      Cr samples straight from the (cached) reference, 4 reads each.  List 0's samples stay in registers while list 1 is computed;
 *   3. average / weight / biweight in registers;
 *   4. the samples go through a wave-private LDS tile and leave as whole rows of a block: one 4-sample store per luma row and one
 *      2-sample store per chroma row.  Nothing goes to HBM between the lists.
 * The chroma format is a template parameter FMT:
 *   FMT 1  4:2:0 and monochrome, as above;
 *   FMT 2  4:2:2: a block's 2x4 Cb plus 2x4 Cr samples are exactly its 16 lanes, so every lane is a chroma lane (lane j: plane j >> 3,
 *          sample (j & 1, (j >> 1) & 3)); the chroma tile has 16 entries per block and leaves as four 2-sample rows per plane;
 *   FMT 3  4:4:4: steps 2 to 4 run once per plane on the plane's reference and destination, with the chroma values of the plan for
 *          Cb and Cr; the plan and the vectors stay resolved once in registers, and the window's reuse by the next plane lies behind the
 *          same ffhip_wave_sync() pairs as its reuse by the next list.
 * The interpolation and the weighting are h264_mc_rules.h's per-sample statements, which h264_hbd.hip's kernels run too; the source
 * coordinates are clamped as FFHIP_MC_EMU records are.
 */
#include <stddef.h>

#include "common.h"
#include "h264_kernels.h"
#include "h264_inter_rules.h"
#include "h264_mc_rules.h"

static_assert(sizeof(FFHipH264MvField) == 12 && sizeof(FFHipH264BsMb) == 8, "the records of the edge-parameter face");
static_assert(sizeof(FFHipH264InterSlice) == 2888, "FFHipH264InterSlice is a 2888-byte record");
static_assert(sizeof(FFHipH264InterRef) == 56, "FFHipH264InterRef is a 56-byte record");
static_assert(sizeof(FFHipH264InterPic) == 1880, "FFHipH264InterPic is staged as an array");
static_assert(sizeof(FFHipH264InterBlockPlan) == 28, "FFHipH264InterBlockPlan is a 28-byte record");

#define H4I_PICS 16 /* pictures per launch: their FFHipH264InterPic structs travel in one progress-pool slot */
static_assert(H4I_PICS * sizeof(FFHipH264InterPic) <= FFHIP_PROGRESS_SLOT_INTS * sizeof(int), "a launch's pictures fit one slot");

namespace {
constexpr int WIN = 9;              /* a 4x4 block's window: 2 samples before, 3 after */
constexpr int WIN_PITCH = 84;       /* uint16_t entries per block window (81 used) */

/* a lane's sample in its block's LDS window */
struct WinSrc {
    const uint16_t *w0;
    __device__ __forceinline__ int at(int dx, int dy) const { return (int)w0[dy * WIN + dx]; }
};
/* a chroma sample of a reference plane of cw x ch samples, at clamped coordinates */
template <typename P>
struct ClampSrc {
    const uint8_t *base;
    ptrdiff_t s;
    int x0, y0, cw, ch;
    __device__ __forceinline__ int at(int dx, int dy) const
    {
        return (int)reinterpret_cast<const P *>(base + (ptrdiff_t)min(max(y0 + dy, 0), ch - 1) * s)[min(max(x0 + dx, 0), cw - 1)];
    }
};

/* 8 waves per SIMD asked for by name: left to itself the 4:2:2 form takes 65 VGPRs, one past the step (with it 63, no scratch) */
template <typename P, int FMT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8)))
void k_h264_inter_pic(const FFHipH264InterPic *pics, int mb_w, int mb_h, int bd, int chroma)
{
    constexpr int CT = FMT == 2 ? 16 : 8;                   /* chroma tile entries per block */
    constexpr int WAVE_LDS = 4 * WIN_PITCH + 64 + 4 * CT;   /* four windows, the luma tile, the chroma tile */
    __shared__ uint16_t lds[4 * WAVE_LDS];
    const FFHipH264InterPic &Pc = pics[blockIdx.z];
    const int mx = blockIdx.x, my = blockIdx.y;
    const FFHipH264BsMb m = Pc.mb[(ptrdiff_t)my * mb_w + mx];
    if (m.flags & 1)
        return;
    const int t = threadIdx.x, q = t >> 6, lane = t & 63, k = lane >> 4, j = lane & 15, x4 = j & 3, y4 = j >> 2;
    const int bx = mx * 4 + (q & 1) * 2 + (k & 1), by = my * 4 + (q >> 1) * 2 + (k >> 1);   /* the block, in 4x4 units of the picture */
    const FFHipH264MvField f = Pc.mvf[(ptrdiff_t)by * Pc.mvf_stride + bx];
    const FFHipH264InterBlockPlan plan = h264inter_plan(&m, &f, Pc.slices, Pc.nslices, Pc.nrefs);
    const bool live = plan.mode != FFHIP_H264_INTER_SKIP, bi = plan.mode >= FFHIP_H264_INTER_BI_AVG;
    const bool has_c = chroma && Pc.dst[1], clane = FMT != 3 && has_c && (FMT == 2 || j < 8);
    /* a chroma lane's plane (0 Cb, 1 Cr) and sample of the block's 2x2 (2x4 at 4:2:2) chroma block */
    const int cpl = FMT == 2 ? j >> 3 : (j >> 2) & 1, cxs = j & 1, cys = FMT == 2 ? (j >> 1) & 3 : (j >> 1) & 1;
    uint16_t *win = lds + q * WAVE_LDS + k * WIN_PITCH, *ytile = lds + q * WAVE_LDS + 4 * WIN_PITCH, *ctile = ytile + 64;
    const int pw = mb_w * 16, ph = mb_h * 16, maxv = (1 << bd) - 1;
    const int nplanes = FMT == 3 && has_c ? 3 : 1;          /* the planes that take the luma path */

#pragma unroll 1
    for (int p = 0; p < nplanes; p++) {
        int pl[2] = { 0, 0 }, pc[2] = { 0, 0 };
#pragma unroll
        for (int n = 0; n < 2; n++) {
            const bool on = live && (n == 0 || bi);
            const int L = bi ? n : plan.list;
            const int mvx = L ? f.mv[1][0] : f.mv[0][0], mvy = L ? f.mv[1][1] : f.mv[0][1], fx = mvx & 3, fy = mvy & 3;
            const FFHipH264InterRef &R = Pc.ref[on ? (n ? plan.slot[1] : plan.slot[0]) : 0];
            if (on) {
                /* the window's origin is 2 left of / above the block's source position */
                const int ox = bx * 4 + (mvx >> 2) - 2, oy = by * 4 + (mvy >> 2) - 2;
                const uint8_t *base = FMT == 3 ? R.base[p] : R.base[0];
                const ptrdiff_t s = FMT == 3 ? R.stride[p] : R.stride[0];
                for (int i = j; i < WIN * WIN; i += 16) {
                    const int r = i / WIN, c = i - r * WIN;
                    if ((!fy && (r < 2 || r > 5)) || (!fx && (c < 2 || c > 5)))
                        continue;
                    const int yy = min(max(oy + r, 0), ph - 1), xx = min(max(ox + c, 0), pw - 1);
                    win[i] = reinterpret_cast<const P *>(base + (ptrdiff_t)yy * s)[xx];
                }
            }
            ffhip_wave_sync();
            if (on) {
                const WinSrc S = { win + (y4 + 2) * WIN + x4 + 2 };
                H264MC_LUMA(pl[n], S, fx, fy, maxv);
                if (clane) {
                    const H264InterChroma C = h264inter_chroma(FMT, bx, by, mvx, mvy, R.chroma_dy, mb_w, mb_h);
                    const ClampSrc<P> Sc = { R.base[1 + cpl], R.stride[1 + cpl], C.sx + cxs, C.sy + cys, C.cw, C.ch };
                    pc[n] = h264mc_chroma(Sc, C.ax, C.ay);
                }
            }
            ffhip_wave_sync(); /* list 1's window, or the next plane's, overwrites list 0's */
        }

        /* ---- 3. the lists combined ---- */
        const int yv = h264inter_combine(&plan, FMT == 3 ? p : 0, pl[0], pl[1], bd);

        /* ---- 4. whole rows of a block ---- */
        ytile[lane] = (uint16_t)yv;
        if (FMT != 3 && (FMT == 2 || j < 8))
            ctile[k * CT + j] = (uint16_t)h264inter_combine(&plan, 1 + cpl, pc[0], pc[1], bd);
        ffhip_wave_sync();
        if (!live)
            continue;
        if (x4 == 0) { /* lanes j = 0, 4, 8, 12: row y4 of the block, 4 samples; dst base and stride are multiples of 4 samples */
            const uint16_t *r = ytile + k * 16 + y4 * 4;
            uint8_t *d = (FMT == 3 ? Pc.dst[p] : Pc.dst[0]) + (ptrdiff_t)(by * 4 + y4) * (FMT == 3 ? Pc.dst_stride[p] : Pc.dst_stride[0]) +
                         (size_t)bx * 4 * sizeof(P);
            if (sizeof(P) == 1)
                *reinterpret_cast<uint32_t *>(d) = pack4(r[0], r[1], r[2], r[3]);
            else
                *reinterpret_cast<uint2 *>(d) = make_uint2((uint32_t)r[0] | (uint32_t)r[1] << 16, (uint32_t)r[2] | (uint32_t)r[3] << 16);
        } else if (FMT != 3 && has_c && (x4 == 1 || (FMT == 2 && x4 == 2))) {
            /* 4:2:0: lanes j = 1, 5, 9, 13: chroma row (y4 & 1) of plane (y4 >> 1); 4:2:2: lanes with x4 = 1 / 2: row y4 of Cb / Cr; 2 samples */
            const int c = FMT == 2 ? x4 - 1 : y4 >> 1, row = FMT == 2 ? y4 : y4 & 1, rows = FMT == 2 ? 4 : 2;
            const uint16_t *r = ctile + k * CT + (c * rows + row) * 2;
            uint8_t *d = Pc.dst[1 + c] + (ptrdiff_t)(by * rows + row) * Pc.dst_stride[1 + c] + (size_t)bx * 2 * sizeof(P);
            if (sizeof(P) == 1)
                *reinterpret_cast<uint16_t *>(d) = (uint16_t)(r[0] | r[1] << 8);
            else
                *reinterpret_cast<uint32_t *>(d) = (uint32_t)r[0] | (uint32_t)r[1] << 16;
        }
    }
}

template <typename P>
void launch(int fmt, dim3 grid, hipStream_t stream, const FFHipH264InterPic *dpics, int mb_w, int mb_h, int bd)
{
    if (fmt == 3)
        hipLaunchKernelGGL((k_h264_inter_pic<P, 3>), grid, dim3(256), 0, stream, dpics, mb_w, mb_h, bd, 1);
    else if (fmt == 2)
        hipLaunchKernelGGL((k_h264_inter_pic<P, 2>), grid, dim3(256), 0, stream, dpics, mb_w, mb_h, bd, 1);
    else
        hipLaunchKernelGGL((k_h264_inter_pic<P, 1>), grid, dim3(256), 0, stream, dpics, mb_w, mb_h, bd, fmt);
}
} // namespace

int ffhip_launch_h264_inter_pictures(int bd, int chroma_format_idc, int mb_w, int mb_h, int npics, const FFHipH264InterPic *pics, hipStream_t stream)
{
    for (int p0 = 0; p0 < npics; p0 += H4I_PICS) {
        const int n = npics - p0 < H4I_PICS ? npics - p0 : H4I_PICS;
        const int r = ffhip_progress_launch_table(stream, "ffhip_h264_inter_pictures_dev: copy or launch", pics + p0, n,
                                                  [&](FFHipH264InterPic *dpics) {
            const dim3 grid(mb_w, mb_h, n); /* at most 4096 x 4096 x 16 */
            if (bd > 8)
                launch<uint16_t>(chroma_format_idc, grid, stream, dpics, mb_w, mb_h, bd);
            else
                launch<uint8_t>(chroma_format_idc, grid, stream, dpics, mb_w, mb_h, bd);
        });
        if (r < 0)
            return r;
    }
    return 0;
}
