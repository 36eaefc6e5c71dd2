/*
 * hevc_inter_pic.hip — HEVC inter reconstruction of whole pictures in one launch (ffhip_hevc_inter_pictures_dev), 8 / 10 / 12 bits.
 *
 * Prediction blocks read reference pictures only, never the picture being written, so a picture's inter CUs carry no dependency
 * chain: one workgroup (4 waves) per (picture, CTB), no hand-offs.  Per plane the workgroup
 *   1. predicts the CTB's PUs, wave w taking PUs w, w + 4, ... (a small PU keeps one wave busy, not the workgroup), into an LDS tile
 *      of the CTB's samples, and marks what it wrote in a coverage mask (a bit per sample);
 *   2. after a barrier, adds the CTB's inter TU residuals to the covered samples of the tile and clips;
 *   3. after a barrier, stores the covered samples to the plane row-wise, four at a time where a quad is fully covered.
 * What no PU covers (intra and PCM CUs, the stride padding, anything outside the picture) is never written.
 *
 * Interpolation is H.265 8.5.3.3.3 in the reference's integer order (h2656_inter_template.c / hevc/dsp_template.c, the oracle's
 * ffo_hevc_mc_bd / ffo_hevc_mc_w_bd): the horizontal pass drops bd - 8 bits into an int16 row buffer (wave-private LDS, up to
 * (64 + 7) x 64), the vertical pass sums it >> 6; one-dimensional phases filter the reference directly, integer positions shift by
 * 14 - bd.  Every reference sample is fetched with its coordinates clamped to the plane (xInt = Clip3(0, pic_width - 1, ...)),
 * which is what emulated_edge_mc gives the reference decoder for a window that leaves the picture and a no-op inside it, so MVs may
 * point anywhere.  A bi-predicted PU keeps its list-0 14-bit intermediate in its own area of the tile (PUs of a CTB are disjoint)
 * and combines list 1 with it there: nothing goes back to HBM between the lists.
 *
 * A lane computes one sample at a time (the block's samples are spread over the wave with a float reciprocal of the block width: the
 * row index is exact for the < 4544 items of a block).  Records are checked before they are used (include/ffhip.h lists what is
 * malformed); a malformed PU or TU is skipped.
 */
#include <stddef.h>

#include "common.h"
#include "h264_kernels.h"
#include "hevc_mc_rules.h"

static_assert(sizeof(FFHipHevcInterPU) == 20, "FFHipHevcInterPU is a 20-byte record");
static_assert(sizeof(FFHipHevcInterTU) == 12, "FFHipHevcInterTU is a 12-byte record");
static_assert(sizeof(FFHipHevcInterSlice) == 424, "FFHipHevcInterSlice is a 424-byte record");
static_assert(sizeof(FFHipHevcInterPic) % 8 == 0, "FFHipHevcInterPic is staged as an array");

#define HIP_PICS 16 /* pictures per launch: their FFHipHevcInterPic structs travel in one progress-pool slot */
static_assert(HIP_PICS * sizeof(FFHipHevcInterPic) <= FFHIP_PROGRESS_SLOT_INTS * sizeof(int), "a launch's pictures fit one slot");

namespace {
constexpr int TILE = 64;            /* the tile's row pitch: a CTB plane is at most 64 x 64 */
constexpr int ROWS = 64 + 7;        /* rows of the horizontal pass: h + TAPS - 1 */

/* one list of one block: the reference plane (clamped to rw x rh samples), the block's integer origin in it and its phases */
struct HipSrc {
    const uint8_t *base;
    ptrdiff_t stride;
    int rw, rh, xi, yi, mx, my;
};

template <typename PIX>
__device__ __forceinline__ int hip_ref(const HipSrc &s, int x, int y)
{
    const int cx = min(max(x, 0), s.rw - 1), cy = min(max(y, 0), s.rh - 1);
    return reinterpret_cast<const PIX *>(s.base + (ptrdiff_t)cy * s.stride)[cx];
}

template <typename PIX>
struct HipWin { /* a source of hevc_mc_rules.h: the samples around (x, y) of the plane */
    const HipSrc &s;
    int x, y;
    __device__ __forceinline__ int at(int dx, int dy) const { return hip_ref<PIX>(s, x + dx, y + dy); }
};

/* mode: HEVCMC_PUT leaves the 14-bit intermediate in the tile (list 0 of a bi block); the others leave pixels, HEVCMC_BI / HEVCMC_BI_W
 * reading list 0's intermediate from the same tile positions.  wx0 / wx1 / ox / denom as the reference's output stages (ox already
 * scaled).  The steps and stages are hevc_mc_rules.h's; the two loops over the block are written out here (the header says why). */
template <typename PIX, bool CHROMA>
__device__ __forceinline__ void hip_predict(int16_t *tile, int16_t *tmp, const HipSrc &s, int lx, int ly, int bw, int bh, int mode, int wx0,
                                            int wx1, int ox, int denom, int bd, int lane)
{
    constexpr int TAPS = CHROMA ? 4 : 8, B = hevcmc_before<TAPS>();
    int hf[TAPS], vf[TAPS];
    hevcmc_taps_c<TAPS>(s.mx, s.my, hf, vf);
    const float inv = 1.0f / (float)bw;
    if (s.mx && s.my) { /* first pass over rows -B .. bh + TAPS - 2 - B */
        const int items = bw * (bh + TAPS - 1);
        for (int i = lane; i < items; i += 64) {
            const int r = (int)(((float)i + 0.5f) * inv), x = i - r * bw;
            int acc = 0;
#pragma unroll
            for (int t = 0; t < TAPS; t++)
                acc += hf[t] * hip_ref<PIX>(s, s.xi + x + t - B, s.yi + r - B);
            tmp[r * TILE + x] = (int16_t)hevcmc_first(acc, bd);
        }
        ffhip_wave_sync();
    }
    const int wsh = hevcmc_wshift(denom, bd);
    for (int i = lane; i < bw * bh; i += 64) {
        const int y = (int)(((float)i + 0.5f) * inv), x = i - y * bw;
        int val = 0;
        if (s.mx && s.my) {
#pragma unroll
            for (int t = 0; t < TAPS; t++)
                val += vf[t] * tmp[(y + t) * TILE + x];
            val = hevcmc_second(val);
        } else {
            val = hevcmc_direct<TAPS>(HipWin<PIX>{ s, s.xi + x, s.yi + y }, hf, vf, s.mx, s.my, bd);
        }
        int16_t &d = tile[(ly + y) * TILE + lx + x];
        d = (int16_t)hevcmc_out(mode, val, mode >= HEVCMC_BI ? d : 0, wx0, wx1, ox, wsh, bd);
    }
    ffhip_wave_sync(); /* tmp is reused by the next pass */
}
} // namespace

/* grid: (ctb_w * ctb_h, pictures); 4 waves per workgroup */
template <typename PIX>
__global__ __launch_bounds__(256) void k_hevc_inter_pic(const FFHipHevcInterPic *__restrict__ pics, int cfi, int width, int height, int log2_ctb,
                                                        int ctb_w, int bd)
{
    constexpr int PS = (int)sizeof(PIX);
    __shared__ int16_t tile[TILE * TILE];
    __shared__ unsigned long long cov[TILE];
    __shared__ int16_t tmp_all[4][ROWS * TILE];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const FFHipHevcInterPic &P = pics[blockIdx.y];
    const int a = (int)blockIdx.x, cy = a / ctb_w, cx = a - cy * ctb_w, C = 1 << log2_ctb;
    const int k0 = P.pu_ctb_start[a], k1 = P.pu_ctb_start[a + 1];
    if (k0 >= k1)
        return; /* no inter samples in this CTB */
    const int nplanes = cfi ? 3 : 1, nslices = P.nslices, nrefs = P.nrefs;
    const int px0 = cx * C, py0 = cy * C, px1 = min(px0 + C, width), py1 = min(py0 + C, height);
    int16_t *const tmp = tmp_all[wave];

    for (int p = 0; p < nplanes; p++) {
        const int hs = p && cfi != 3, vs = p && cfi == 1;
        const int lcw = log2_ctb - hs, Cw = 1 << lcw, Ch = C >> vs, pw = width >> hs, ph = height >> vs;
        const int cx0 = cx * Cw, cy0 = cy * Ch;
        if (tid < TILE)
            cov[tid] = 0;
        __syncthreads();

        /* ---- 1. the CTB's PUs, a wave each ---- */
        for (int k = k0 + wave; k < k1; k += 4) {
            const FFHipHevcInterPU R = P.pus[k];
            const int x = R.x, y = R.y, w = R.w, h = R.h, fl = R.flags & 3, sl = R.slice;
            bool ok = w >= 4 && w <= 64 && h >= 4 && h <= 64 && !((w | h) & 3) && fl && sl < nslices && x >= px0 && x + w <= px1 &&
                      y >= py0 && y + h <= py1;
            if (!ok)
                continue;
            const FFHipHevcInterSlice &S = P.slices[sl];
            int slot[2] = { 0, 0 };
#pragma unroll
            for (int l = 0; l < 2; l++)
                if (fl >> l & 1) {
                    const int ri = R.ref_idx[l], nr = S.num_ref[l];
                    ok = ok && nr <= 16 && ri < nr;
                    if (ok) {
                        slot[l] = S.ref[l][ri];
                        ok = slot[l] < nrefs;
                    }
                }
            if (!ok)
                continue;
            const int bx = x >> hs, by = y >> vs, bw = w >> hs, bh = h >> vs, lx = bx - cx0, ly = by - cy0;
            HipSrc src[2];
#pragma unroll
            for (int l = 0; l < 2; l++) {
                const FFHipHevcInterRef &Rf = P.ref[slot[l]];
                const int mvx = R.mv[l][0], mvy = R.mv[l][1];
                src[l].base = Rf.base[p];
                src[l].stride = Rf.stride[p];
                src[l].rw = pw;
                src[l].rh = ph;
                if (p == 0) {
                    src[l].xi = bx + (mvx >> 2);
                    src[l].yi = by + (mvy >> 2);
                    src[l].mx = mvx & 3;
                    src[l].my = mvy & 3;
                } else { /* chroma_mc_uni / chroma_mc_bi: the phase in eighths whatever the subsampling */
                    src[l].xi = bx + (mvx >> (2 + hs));
                    src[l].yi = by + (mvy >> (2 + vs));
                    src[l].mx = (mvx & ((4 << hs) - 1)) << (1 - hs);
                    src[l].my = (mvy & ((4 << vs) - 1)) << (1 - vs);
                }
            }
            const bool weighted = S.weighted;
            const int denom = p ? S.chroma_log2_denom : S.luma_log2_denom, c = p - 1;
            auto wt = [&](int l, int ri) { return p ? S.chroma_weight[l][ri][c] : S.luma_weight[l][ri]; };
            auto of = [&](int l, int ri) { return hevcmc_offset(p ? S.chroma_offset[l][ri][c] : S.luma_offset[l][ri], bd); };
            if (fl == 3) {
                const int r0 = R.ref_idx[0], r1 = R.ref_idx[1];
                if (p)
                    hip_predict<PIX, true>(tile, tmp, src[0], lx, ly, bw, bh, HEVCMC_PUT, 0, 0, 0, 0, bd, lane);
                else
                    hip_predict<PIX, false>(tile, tmp, src[0], lx, ly, bw, bh, HEVCMC_PUT, 0, 0, 0, 0, bd, lane);
                const int mode = weighted ? HEVCMC_BI_W : HEVCMC_BI;
                const int w0 = weighted ? wt(0, r0) : 0, w1 = weighted ? wt(1, r1) : 0, o = weighted ? of(0, r0) + of(1, r1) : 0;
                if (p)
                    hip_predict<PIX, true>(tile, tmp, src[1], lx, ly, bw, bh, mode, w0, w1, o, denom, bd, lane);
                else
                    hip_predict<PIX, false>(tile, tmp, src[1], lx, ly, bw, bh, mode, w0, w1, o, denom, bd, lane);
            } else {
                const int l = fl >> 1, ri = R.ref_idx[l];
                const int mode = weighted ? HEVCMC_UNI_W : HEVCMC_UNI;
                const int w0 = weighted ? wt(l, ri) : 0, o = weighted ? of(l, ri) : 0;
                const HipSrc &su = l ? src[1] : src[0];
                if (p)
                    hip_predict<PIX, true>(tile, tmp, su, lx, ly, bw, bh, mode, w0, 0, o, denom, bd, lane);
                else
                    hip_predict<PIX, false>(tile, tmp, su, lx, ly, bw, bh, mode, w0, 0, o, denom, bd, lane);
            }
            if (lane < bh)
                atomicOr(&cov[ly + lane], (bw == 64 ? ~0ull : (1ull << bw) - 1) << lx);
        }
        __syncthreads();

        /* ---- 2. the CTB's inter TUs: residual into the covered samples, clipped ---- */
        const FFHipHevcInterPlane &D = P.plane[p];
        const int t0 = D.tu_ctb_start[a], t1 = D.tu_ctb_start[a + 1], maxv = (1 << bd) - 1;
        for (int k = t0 + wave; k < t1; k += 4) {
            const FFHipHevcInterTU T = D.tus[k];
            const int lg = T.log2_size, N = 1 << (lg & 7), x = T.x, y = T.y;
            if (lg < 2 || lg > 5 || T.res_offset < 0 || x < cx0 || x + N > min(cx0 + Cw, pw) || y < cy0 || y + N > min(cy0 + Ch, ph))
                continue;
            const int16_t *res = D.res + T.res_offset;
            for (int i = lane; i < N * N; i += 64) {
                const int yy = y - cy0 + (i >> lg), xx = x - cx0 + (i & (N - 1));
                if (cov[yy] >> xx & 1) {
                    int16_t &d = tile[yy * TILE + xx];
                    d = (int16_t)min(max(d + res[i], 0), maxv);
                }
            }
        }
        __syncthreads();

        /* ---- 3. the covered samples to the plane, a quad per item ---- */
        uint8_t *const base = D.base;
        const ptrdiff_t stride = D.stride;
        const int lq = lcw - 2;
        for (int i = tid; i < (Ch * Cw) >> 2; i += 256) {
            const int r = i >> lq, c = (i - (r << lq)) << 2;
            const unsigned m = (unsigned)(cov[r] >> c) & 15;
            if (!m)
                continue;
            PIX *d = reinterpret_cast<PIX *>(base + (ptrdiff_t)(cy0 + r) * stride) + cx0 + c;
            const int16_t *t = &tile[r * TILE + c];
            if (m == 15) { /* base and stride are 4-sample aligned */
                if (PS == 1)
                    *reinterpret_cast<uint32_t *>(d) = (uint32_t)(uint8_t)t[0] | (uint32_t)(uint8_t)t[1] << 8 | (uint32_t)(uint8_t)t[2] << 16 |
                                                       (uint32_t)(uint8_t)t[3] << 24;
                else
                    *reinterpret_cast<uint2 *>(d) = make_uint2((uint32_t)(uint16_t)t[0] | (uint32_t)(uint16_t)t[1] << 16,
                                                               (uint32_t)(uint16_t)t[2] | (uint32_t)(uint16_t)t[3] << 16);
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (m >> j & 1)
                        d[j] = (PIX)t[j];
            }
        }
        __syncthreads(); /* the next plane reuses the tile and the mask */
    }
}

int ffhip_launch_hevc_inter_pictures(int bd, int cfi, int width, int height, int log2_ctb, int npics, const FFHipHevcInterPic *pics,
                                     hipStream_t stream)
{
    const int C = 1 << log2_ctb, ctb_w = (width + C - 1) / C, ctb_h = (height + C - 1) / C;
    for (int p0 = 0; p0 < npics; p0 += HIP_PICS) {
        const int n = npics - p0 < HIP_PICS ? npics - p0 : HIP_PICS;
        /* the pictures travel with their DPB tables */
        const int r = ffhip_progress_launch_table(stream, "ffhip_hevc_inter_pictures_dev: copy or launch", pics + p0, n,
                                                  [&](FFHipHevcInterPic *dpics) {
            if (bd > 8)
                hipLaunchKernelGGL(k_hevc_inter_pic<uint16_t>, dim3(ctb_w * ctb_h, n), dim3(256), 0, stream, dpics, cfi, width, height, log2_ctb,
                                   ctb_w, bd);
            else
                hipLaunchKernelGGL(k_hevc_inter_pic<uint8_t>, dim3(ctb_w * ctb_h, n), dim3(256), 0, stream, dpics, cfi, width, height, log2_ctb,
                                   ctb_w, 8);
        });
        if (r < 0)
            return r;
    }
    return 0;
}
