/*
 * vp9_inter_frame.hip — VP9 inter reconstruction of whole frames in one launch (ffhip_vp9_inter_frames_dev), 8 / 10 / 12 bits.
 *
 * Prediction reads reference frames only, never the frame being written, so the inter blocks of a frame carry no dependency chain:
 * one workgroup (4 waves) per (frame, superblock), no hand-offs.  Per plane the workgroup
 *   1. predicts the superblock's records of that plane, wave w taking records w, w + 4, ..., into an LDS tile of the superblock's
 *      samples, and marks what it wrote in a coverage mask (a bit per sample); a compound record averages its second reference into
 *      the same tile positions;
 *   2. after a barrier, runs the superblock's TUs of the plane, a wave each, through the butterfly network of vp9_itxfm.hip
 *      (vp9_itxfm_net.inc, 32-bit at 8 bits, 64-bit above; vp9_itxfm_tile.h) and adds them to the covered samples of the tile;
 *   3. after a barrier, stores the covered samples inside the decoded area to the plane, four at a time where a quad is covered.
 * What no record covers (intra blocks, the stride padding, anything outside the decoded area) is never written.
 *
 * Interpolation is vp9dsp_template.c's (the oracle's ffo_vp9_mc_bd) as vp9_mc_rules.h states it: 8-tap passes
 * clip((sum + 64) >> 7), the 2-D form through pixel-type temporaries of rows -3 .. h + 3 (wave-private LDS), bilinear
 * a + ((m (b - a) + 8) >> 4) over rows 0 .. h, full-sample copies.  Every reference sample is fetched with its coordinates
 * clamped to the reference's real size, which is what emulated_edge_mc gives mc_luma_unscaled / mc_chroma_unscaled, so MVs may
 * point anywhere.  A lane computes one sample at a time; block sizes are powers of two, so a block's samples are spread over the
 * wave by shifts.  Records are checked before they are used (include/ffhip.h lists what is malformed); a malformed record or TU is
 * skipped.
 *
 * ffhip_vp9_inter_frames_scaled_dev() runs the SCALED instantiation when a launch has a reference of another size: each reference
 * carries its own real size, scale and step (staged behind the frames in the same progress-pool slot), and a record of the SCALED
 * template (FFHIP_VP9_PRED_SCALED) from such a reference takes mc_luma_scaled / mc_chroma_scaled: the MV clipped to its box, the
 * scaled origin and phase, then smc's 2-D form (output x around (mx + x dx) >> 4 with the taps of (mx + x dx) & 15, phase 0 a copy)
 * through the same clamped gather and tap code.  smc's horizontal pass needs up to 134 rows at 2x down; it runs in strips of 32
 * output rows, whose rows -3 .. ((15 + 31 dy) >> 4) + 4 fit the TROWS temporaries at any step up to 32, so both instantiations have
 * the same LDS.  Launches without such a reference run the unscaled instantiation, today's kernel.
 */
#include <stddef.h>
#include <type_traits>

#include "common.h"
#include "h264_kernels.h"
#include "vp9_itxfm_tile.h"
#include "vp9_mc_rules.h"

static_assert(sizeof(FFHipVp9InterPred) == 20, "FFHipVp9InterPred is a 20-byte record");
static_assert(sizeof(FFHipVp9InterTU) == 12, "FFHipVp9InterTU is a 12-byte record");
static_assert(sizeof(FFHipVp9InterPic) % 8 == 0, "FFHipVp9InterPic is staged as an array");

#define VIF_PICS 16 /* frames per launch: their FFHipVp9InterPic structs travel in one progress-pool slot */
static_assert(VIF_PICS * sizeof(FFHipVp9InterPic) <= FFHIP_PROGRESS_SLOT_INTS * sizeof(int), "a launch's frames fit one slot");

/* the references of one frame of a scaled launch: luma real size, scale (<< 14) and step per reference, 0 scale for an unscaled one */
struct VifRefScale {
    int32_t rw[3], rh[3];
    int32_t scale[3][2], step[3][2];
};
static_assert(VIF_PICS * (sizeof(FFHipVp9InterPic) + sizeof(VifRefScale)) <= FFHIP_PROGRESS_SLOT_INTS * sizeof(int),
              "a scaled launch's frames and reference scales fit one slot");

namespace {
constexpr int TILE = 64;          /* the tile's row pitch: a superblock plane is at most 64 x 64 */
constexpr int TROWS = 64 + 7;     /* rows of the 2-D form's horizontal pass */

/* one reference of one block: the plane (clamped to rw x rh samples), the block's integer origin in it and its phases (sixteenths) */
struct VifSrc {
    const uint8_t *base;
    ptrdiff_t stride;
    int rw, rh, xi, yi, mx, my;
};

template <typename PIX>
__device__ __forceinline__ int vif_ref(const VifSrc &s, int x, int y)
{
    const int cx = min(max(x, 0), s.rw - 1), cy = min(max(y, 0), s.rh - 1);
    return reinterpret_cast<const PIX *>(s.base + (ptrdiff_t)cy * s.stride)[cx];
}

/* put (AVG false) or avg (AVG true) of a w x h block at tile position (lx, ly); tmp: the wave's temporaries */
template <typename PIX, bool AVG>
__device__ __forceinline__ void vif_predict(uint16_t *tile, PIX *tmp, const VifSrc &s, int lx, int ly, int lgw, int h, int filter, int maxv,
                                            int lane)
{
    const int w = 1 << lgw;
    if (s.mx && s.my) { /* the horizontal pass over rows -3 .. h + 3 (bilinear: 0 .. h) into pixel temporaries: vp9mc_before() and
                         * vp9mc_rows() at a step of 16, written out (as the calls, the 16-bit kernels take one VGPR more) */
        const int r0 = filter == 3 ? 0 : -3, rows = filter == 3 ? h + 1 : h + 7;
        for (int i = lane; i < rows << lgw; i += 64) {
            const int r = i >> lgw, x = i & (w - 1), yy = s.yi + r + r0;
            tmp[r * TILE + x] = (PIX)vp9mc_pass(filter, s.mx, maxv, [&](int k) { return vif_ref<PIX>(s, s.xi + x + k, yy); });
        }
        ffhip_wave_sync();
    }
    for (int i = lane; i < h << lgw; i += 64) {
        const int y = i >> lgw, x = i & (w - 1);
        int v;
        if (s.mx && s.my) {
            const PIX *t = tmp + (y + (filter == 3 ? 0 : 3)) * TILE + x;
            v = vp9mc_pass(filter, s.my, maxv, [&](int k) { return (int)t[k * TILE]; });
        } else if (s.mx) {
            v = vp9mc_pass(filter, s.mx, maxv, [&](int k) { return vif_ref<PIX>(s, s.xi + x + k, s.yi + y); });
        } else if (s.my) {
            v = vp9mc_pass(filter, s.my, maxv, [&](int k) { return vif_ref<PIX>(s, s.xi + x, s.yi + y + k); });
        } else {
            v = vif_ref<PIX>(s, s.xi + x, s.yi + y);
        }
        uint16_t &d = tile[(ly + y) * TILE + lx + x];
        d = (uint16_t)(AVG ? vp9mc_avg(d, v) : v);
    }
    ffhip_wave_sync(); /* tmp is reused by the next pass; an avg pass reads what this lane's put wrote */
}

constexpr int SROWS = 32; /* output rows per strip of the scaled 2-D form */
static_assert(vp9mc_rows(0, 15, SROWS, 32) <= TROWS, "a strip's horizontal pass fits the temporaries at any step up to 32");

/* smc (vp9dsp_template.c, the oracle's ffo_vp9_smc_bd), put or avg of a w x h block at tile position (lx, ly) with steps dx, dy: the
 * horizontal pass over the rows a strip of output rows reads, into pixel temporaries, then the vertical pass.  Phase 0 is a copy */
template <typename PIX, bool AVG>
__device__ __forceinline__ void vif_predict_scaled(uint16_t *tile, PIX *tmp, const VifSrc &s, int dx, int dy, int lx, int ly, int lgw, int h,
                                                   int filter, int maxv, int lane)
{
    const int w = 1 << lgw, before = vp9mc_before(filter);
    for (int y0 = 0; y0 < h; y0 += SROWS) {
        const int sh = min(h - y0, SROWS), p0 = vp9mc_pos(s.my, y0, dy), m0 = vp9mc_frac(p0);
        const int ry = s.yi + vp9mc_whole(p0) - before, rows = vp9mc_rows(filter, m0, sh, dy);
        for (int i = lane; i < rows << lgw; i += 64) {
            const int r = i >> lgw, x = i & (w - 1), pos = vp9mc_pos(s.mx, x, dx), xx = s.xi + vp9mc_whole(pos);
            tmp[r * TILE + x] = (PIX)vp9mc_pass0(filter, vp9mc_frac(pos), maxv, [&](int k) { return vif_ref<PIX>(s, xx + k, ry + r); });
        }
        ffhip_wave_sync();
        for (int i = lane; i < sh << lgw; i += 64) {
            const int y = i >> lgw, x = i & (w - 1), pos = vp9mc_pos(m0, y, dy);
            const PIX *t = tmp + (vp9mc_whole(pos) + before) * TILE + x;
            const int v = vp9mc_pass0(filter, vp9mc_frac(pos), maxv, [&](int k) { return (int)t[k * TILE]; });
            uint16_t &d = tile[(ly + y0 + y) * TILE + lx + x];
            d = (uint16_t)(AVG ? vp9mc_avg(d, v) : v);
        }
        ffhip_wave_sync(); /* the next strip or pass reuses tmp */
    }
}

/* scale_mv (vp9recon.c): ((int64) n * scale) >> 14, flooring */
__device__ __forceinline__ int vif_scale_mv(int n, int scale) { return (int)(((long long)n * scale) >> 14); }

} // namespace

/* grid: (sb_w * sb_h, frames); 4 waves per workgroup.  SCALED: the frames' VifRefScale tables follow pics[0 .. VIF_PICS) */
template <typename PIX, bool SCALED>
__global__ __launch_bounds__(256) void k_vp9_inter_frame(const FFHipVp9InterPic *__restrict__ pics, int ss_h, int ss_v, int width, int height,
                                                         int sb_w, int bd)
{
    constexpr int PS = (int)sizeof(PIX);
    constexpr bool HBD = PS == 2;
    __shared__ uint16_t tile[TILE * TILE];
    __shared__ unsigned long long cov[TILE];
    __shared__ __align__(16) PIX tmp_all[4][TROWS * TILE]; /* 2-D temporaries, or a TU's first-pass output (32 x 32 coefficients) */
    static_assert(TROWS * TILE * PS >= 32 * 32 * (HBD ? 4 : 2), "a TU's intermediate fits the wave's temporaries");
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const FFHipVp9InterPic &P = pics[blockIdx.y];
    const int a = (int)blockIdx.x, sy = a / sb_w, sx = a - sy * sb_w;
    const int k0 = P.pred_sb_start[a], k1 = P.pred_sb_start[a + 1];
    if (k0 >= k1)
        return; /* no inter samples in this superblock */
    const int nrefs = P.nrefs, maxv = (1 << bd) - 1;
    const int dw = ((width + 7) >> 3) << 3, dh = ((height + 7) >> 3) << 3; /* the decoded area, luma */
    const VifRefScale *const RS = SCALED ? reinterpret_cast<const VifRefScale *>(pics + VIF_PICS) + blockIdx.y : nullptr;
    PIX *const tmp = tmp_all[wave];

    for (int p = 0; p < 3; p++) {
        const int hs = p ? ss_h : 0, vs = p ? ss_v : 0, chroma = p ? 1 : 0;
        const int Cw = TILE >> hs, Ch = TILE >> vs, x0 = sx * Cw, y0 = sy * Ch;
        const int rw = (width + hs) >> hs, rh = (height + vs) >> vs; /* the references' real size */
        if (tid < TILE)
            cov[tid] = 0;
        __syncthreads();

        /* ---- 1. the superblock's predictions of this plane, a wave each ---- */
        for (int k = k0 + wave; k < k1; k += 4) {
            const FFHipVp9InterPred R = P.preds[k];
            const int fl = R.flags, w = R.w, h = R.h, filter = R.filter, x = R.x, y = R.y;
            if ((fl & (SCALED ? ~7 : ~3)) || ((fl >> 1) & 1) != chroma)
                continue;
            const bool comp = fl & 1;
            const bool ok = w >= 4 && w <= 64 && !(w & (w - 1)) && h >= 4 && h <= 64 && !(h & (h - 1)) && filter <= 3 && R.ref[0] < nrefs &&
                            (!comp || R.ref[1] < nrefs) && x >= x0 && x + w <= x0 + Cw && y >= y0 && y + h <= y0 + Ch;
            if (!ok)
                continue;
            /* the clip box of a SCALED-template call: (px, py, pw, ph) */
            const bool sc_rec = SCALED && (fl & FFHIP_VP9_PRED_SCALED);
            const int px = R.box[0] & 15, py = R.box[0] >> 4, lpw = R.box[1] & 15, lph = R.box[1] >> 4;
            if (sc_rec && (lpw < 2 || lpw > 6 || lph < 2 || lph > 6 || px + w > (1 << lpw) || py + h > (1 << lph)))
                continue;
            const int lgw = __builtin_ctz(w), lx = x - x0, ly = y - y0;
            for (int l = 0; l <= (int)comp; l++) {
                const FFHipVp9InterRef &Rf = P.ref[l ? R.ref[1] : R.ref[0]]; /* selects: R stays in registers */
                const int mvx = l ? R.mv[1][0] : R.mv[0][0], mvy = l ? R.mv[1][1] : R.mv[0][1];
                VifSrc s;
                s.base = Rf.base[p];
                s.stride = Rf.stride[p];
                s.rw = rw;
                s.rh = rh;
                if (SCALED) {
                    const int ri = l ? R.ref[1] : R.ref[0];
                    s.rw = (RS->rw[ri] + hs) >> hs; /* this reference's real size */
                    s.rh = (RS->rh[ri] + vs) >> vs;
                    const int scx = RS->scale[ri][0], scy = RS->scale[ri][1];
                    if (sc_rec && scx) { /* mc_luma_scaled / mc_chroma_scaled */
                        int mx, my;
                        if (hs) { /* libvpx's rounding (webm issue 820) */
                            const int mv = min(max(mvx, -(x + (1 << lpw) - px + 4) * 16), ((width + 7) >> 3) * 64 - (x - px - 3) * 16);
                            mx = vif_scale_mv(mv, scx) + (vif_scale_mv(x * 16, scx) & ~15) + (vif_scale_mv(x * 32, scx) & 15);
                        } else {
                            const int mv = min(max(mvx, -(x + (1 << lpw) - px + 4) * 8), ((width + 7) >> 3) * 64 - (x - px - 3) * 8);
                            mx = vif_scale_mv(mv * 2, scx) + vif_scale_mv(x * 16, scx);
                        }
                        if (vs) {
                            const int mv = min(max(mvy, -(y + (1 << lph) - py + 4) * 16), ((height + 7) >> 3) * 64 - (y - py - 3) * 16);
                            my = vif_scale_mv(mv, scy) + (vif_scale_mv(y * 16, scy) & ~15) + (vif_scale_mv(y * 32, scy) & 15);
                        } else {
                            const int mv = min(max(mvy, -(y + (1 << lph) - py + 4) * 8), ((height + 7) >> 3) * 64 - (y - py - 3) * 8);
                            my = vif_scale_mv(mv * 2, scy) + vif_scale_mv(y * 16, scy);
                        }
                        s.xi = mx >> 4;
                        s.yi = my >> 4;
                        s.mx = mx & 15;
                        s.my = my & 15;
                        const int dx = RS->step[ri][0], dy = RS->step[ri][1];
                        if (l)
                            vif_predict_scaled<PIX, true>(tile, tmp, s, dx, dy, lx, ly, lgw, h, filter, maxv, lane);
                        else
                            vif_predict_scaled<PIX, false>(tile, tmp, s, dx, dy, lx, ly, lgw, h, filter, maxv, lane);
                        continue;
                    }
                }
                if (!chroma) {
                    s.xi = x + (mvx >> 3);
                    s.yi = y + (mvy >> 3);
                    s.mx = (mvx & 7) << 1;
                    s.my = (mvy & 7) << 1;
                } else { /* mc_chroma_unscaled: the MV in sixteenths of a chroma sample */
                    const int mx = mvx * (1 << !ss_h), my = mvy * (1 << !ss_v);
                    s.xi = x + (mx >> 4);
                    s.yi = y + (my >> 4);
                    s.mx = mx & 15;
                    s.my = my & 15;
                }
                if (l)
                    vif_predict<PIX, true>(tile, tmp, s, lx, ly, lgw, h, filter, maxv, lane);
                else
                    vif_predict<PIX, false>(tile, tmp, s, lx, ly, lgw, h, filter, maxv, lane);
            }
            if (lane < h)
                atomicOr(&cov[ly + lane], (w == 64 ? ~0ull : (1ull << w) - 1) << lx);
        }
        __syncthreads();

        /* ---- 2. the superblock's TUs of this plane: residuals into the covered samples ---- */
        const FFHipVp9InterPlane &D = P.plane[p];
        const int t0 = D.tu_sb_start[a], t1 = D.tu_sb_start[a + 1];
        for (int k = t0 + wave; k < t1; k += 4) {
            const FFHipVp9InterTU T = D.tus[k];
            const int tx = T.tx, N = tx == 4 ? 4 : 4 << (tx & 3), x = T.x, y = T.y;
            if (tx > 4 || ((x | y) & (N - 1)) || x < x0 || x + N > x0 + Cw || y < y0 || y + N > y0 + Ch)
                continue;
            const void *co = HBD ? (const void *)(static_cast<const int32_t *>(D.coeffs) + T.coeff_offset)
                                 : (const void *)(static_cast<const int16_t *>(D.coeffs) + T.coeff_offset);
            const int lx = x - x0, ly = y - y0, tp = T.txtp;
            const bool dc = T.dc_only != 0;
            switch (tx) {
            case 0: vif_tu<2, false, HBD, TILE, true>(tile, cov, tmp, co, tp, dc, lx, ly, maxv, lane); break;
            case 1: vif_tu<3, false, HBD, TILE, true>(tile, cov, tmp, co, tp, dc, lx, ly, maxv, lane); break;
            case 2: vif_tu<4, false, HBD, TILE, true>(tile, cov, tmp, co, tp, dc, lx, ly, maxv, lane); break;
            case 3: vif_tu<5, false, HBD, TILE, true>(tile, cov, tmp, co, tp, dc, lx, ly, maxv, lane); break;
            default: vif_tu<2, true, HBD, TILE, true>(tile, cov, tmp, co, tp, dc, lx, ly, maxv, lane); break;
            }
        }
        __syncthreads();

        /* ---- 3. the covered samples inside the decoded area to the plane, a quad per item ---- */
        uint8_t *const base = D.base;
        const ptrdiff_t stride = D.stride;
        const int xe = min(Cw, (dw >> hs) - x0), ye = min(Ch, (dh >> vs) - y0); /* multiples of 4 */
        const int lq = __builtin_ctz(Cw) - 2;
        for (int i = tid; i < (Ch * Cw) >> 2; i += 256) {
            const int r = i >> lq, c = (i - (r << lq)) << 2;
            if (r >= ye || c >= xe)
                continue;
            const unsigned m = (unsigned)(cov[r] >> c) & 15;
            if (!m)
                continue;
            PIX *d = reinterpret_cast<PIX *>(base + (ptrdiff_t)(y0 + r) * stride) + x0 + c;
            const uint16_t *t = &tile[r * TILE + c];
            if (m == 15) { /* base and stride are 4-sample aligned */
                if (PS == 1)
                    *reinterpret_cast<uint32_t *>(d) = (uint32_t)(uint8_t)t[0] | (uint32_t)(uint8_t)t[1] << 8 | (uint32_t)(uint8_t)t[2] << 16 |
                                                       (uint32_t)(uint8_t)t[3] << 24;
                else
                    *reinterpret_cast<uint2 *>(d) = make_uint2((uint32_t)t[0] | (uint32_t)t[1] << 16, (uint32_t)t[2] | (uint32_t)t[3] << 16);
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

int ffhip_launch_vp9_inter_frames(int bd, int ss_h, int ss_v, int width, int height, int npics, const FFHipVp9InterPic *pics, hipStream_t stream)
{
    const int cols = (width + 7) >> 3, rows = (height + 7) >> 3, sb_w = (cols + 7) >> 3, sb_h = (rows + 7) >> 3;
    for (int p0 = 0; p0 < npics; p0 += VIF_PICS) {
        const int n = npics - p0 < VIF_PICS ? npics - p0 : VIF_PICS;
        /* the frames travel with their reference tables */
        const int r = ffhip_progress_launch_table(stream, "ffhip_vp9_inter_frames_dev: copy or launch", pics + p0, n, [&](FFHipVp9InterPic *dpics) {
            if (bd > 8)
                hipLaunchKernelGGL((k_vp9_inter_frame<uint16_t, false>), dim3(sb_w * sb_h, n), dim3(256), 0, stream, dpics, ss_h, ss_v, width, height,
                                   sb_w, bd);
            else
                hipLaunchKernelGGL((k_vp9_inter_frame<uint8_t, false>), dim3(sb_w * sb_h, n), dim3(256), 0, stream, dpics, ss_h, ss_v, width, height,
                                   sb_w, 8);
        });
        if (r < 0)
            return r;
    }
    return 0;
}


int ffhip_launch_vp9_inter_frames_scaled(int bd, int ss_h, int ss_v, int width, int height, int npics, const FFHipVp9InterPicScaled *pics,
                                         hipStream_t stream)
{
    const int cols = (width + 7) >> 3, rows = (height + 7) >> 3, sb_w = (cols + 7) >> 3, sb_h = (rows + 7) >> 3;
    struct Staged { /* one slot's image: the frames, then their reference scales */
        FFHipVp9InterPic pic[VIF_PICS];
        VifRefScale rs[VIF_PICS];
    };
    static_assert(offsetof(Staged, rs) == VIF_PICS * sizeof(FFHipVp9InterPic), "the kernel finds the scales behind VIF_PICS frames");
    for (int p0 = 0; p0 < npics; p0 += VIF_PICS) {
        const int n = npics - p0 < VIF_PICS ? npics - p0 : VIF_PICS;
        Staged st = {};
        bool scaled = false;
        for (int i = 0; i < n; i++) {
            const FFHipVp9InterPicScaled &S = pics[p0 + i];
            st.pic[i] = S.pic;
            for (int r = 0; r < S.pic.nrefs; r++) {
                VifRefScale &R = st.rs[i];
                R.rw[r] = S.ref_w[r];
                R.rh[r] = S.ref_h[r];
                if (S.ref_w[r] != width || S.ref_h[r] != height) { /* vp9.c: mvscale / mvstep */
                    R.scale[r][0] = (S.ref_w[r] << 14) / width;
                    R.scale[r][1] = (S.ref_h[r] << 14) / height;
                    R.step[r][0] = (16 * R.scale[r][0]) >> 14;
                    R.step[r][1] = (16 * R.scale[r][1]) >> 14;
                    scaled = true;
                }
            }
        }
        if (!scaled) { /* no reference of another size: today's kernel on the frames */
            const int r = ffhip_launch_vp9_inter_frames(bd, ss_h, ss_v, width, height, n, st.pic, stream);
            if (r < 0)
                return r;
            continue;
        }
        const int r = ffhip_progress_launch_table(stream, "ffhip_vp9_inter_frames_scaled_dev: copy or launch", &st, 1, [&](Staged *dst) {
            FFHipVp9InterPic *dpics = dst->pic;
            if (bd > 8)
                hipLaunchKernelGGL((k_vp9_inter_frame<uint16_t, true>), dim3(sb_w * sb_h, n), dim3(256), 0, stream, dpics, ss_h, ss_v, width,
                                   height, sb_w, bd);
            else
                hipLaunchKernelGGL((k_vp9_inter_frame<uint8_t, true>), dim3(sb_w * sb_h, n), dim3(256), 0, stream, dpics, ss_h, ss_v, width,
                                   height, sb_w, 8);
        });
        if (r < 0)
            return r;
    }
    return 0;
}
