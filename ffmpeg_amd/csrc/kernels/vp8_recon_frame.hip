/*
 * vp8_recon_frame.hip — VP8 reconstruction of whole frames (ffhip_vp8_recon_frames_dev): what decode_mb_row_no_filter() of
 * libavcodec/vp8.c does per macroblock — inter_predict() or intra_predict(), then idct_mb() — from one FFHipVp8Mb record per
 * macroblock, up to 16 frames per launch.  Two launches on the caller's stream; the record rules are vp8_recon_rules.h's, which the
 * device-free faces run on the host.
 *
 * k_vp8_recon_inter: one wave per (frame, macroblock), four per workgroup; no macroblock depends on another.  Intra and malformed
 * records return at once.  Each put_vp8_* call of the record (v8r_pred) runs in two passes over the wave: the rows it needs,
 * filtered along x, into a uint8 LDS temporary (the reference's tmp_array; a copy when the fraction is 0), then the columns into the
 * macroblock's tile in LDS.  Reference samples are gathered from global memory with coordinates clamped to the plane, which is
 * what emulated_edge_mc leaves: the footprint of a call is at most 21 x 21 bytes that neighbouring waves read too, so it is served
 * by the caches, and no padded copy is staged.  (LDS staging of the footprint has not been measured against this.)  The residuals of
 * the 24 blocks are computed by 24 lanes into LDS, added to the tile, and the 16x16 and the two 8x8 leave once, in dwords.
 *
 * k_vp8_recon_intra: one wave per (frame, macroblock row), rows claimed by ticket t = row * npics + frame (the row above has the
 * smaller ticket; the grid is min(units, resident capacity)).  Macroblock x reads the row above up to the four samples above-right
 * of it, so it starts once the row above has finished min(x + 2, mb_w) macroblocks (row_handoff.h).  Inter macroblocks were finished
 * by the launch before: a wave finds its intra macroblocks 64 records at a time with a ballot, passes over the others and counts
 * them; a row without intra macroblocks costs those loads and one store of the counter.  The tile holds the macroblock with the row
 * above (running on to the top-right) and the column to its left: luma rows -1..15 x columns -4..19, chroma rows -1..7 x columns
 * -4..7; outside the frame the border is virtual (127 above, 129 to the left).  The left column is carried over in LDS from the
 * macroblock before when this wave wrote it, and read from the frame otherwise.  An I4x4 macroblock runs its sixteen sub-blocks
 * in order, each from its edge line E[] (left bottom-up, corner, top, top-right: the line h264_intra_mb.h's rules read), prediction
 * and residual in one step; the VP8 forms are h264_pred_codec.inc's.
 */
#include <stddef.h>

#include "common.h"
#include "h264_intra_mb.h"
#include "progress_pool.h"
#include "row_handoff.h"
#include "vp8_kernels.h"
#include "vp8_recon_rules.h"

static_assert(sizeof(FFHipVp8Mb) == 96, "FFHipVp8Mb is a 96-byte record");
static_assert(sizeof(FFHipVp8Pred) == 20, "FFHipVp8Pred is a 20-byte record");
static_assert(sizeof(FFHipVp8IntraModes) == 34, "FFHipVp8IntraModes is 34 bytes");

#define V8R_PICS 16   /* frames per launch (the set is a kernel argument: 16 x 120 bytes) */
#define V8R_PER_CU 8  /* resident waves per CU the intra grid counts on */
#define V8R_YP 24     /* luma tile pitch: columns -4..19 */
#define V8R_CP 12     /* chroma tile pitch: columns -4..7 */

namespace {
struct V8rPicSet {
    FFHipVp8ReconPic pic[V8R_PICS];
};

__device__ __forceinline__ unsigned v8r_refs(const FFHipVp8ReconPic &P)
{
    unsigned m = 0;
    for (int r = 0; r < 3; r++)
        if (P.ref[r][0] && P.ref[r][1] && P.ref[r][2])
            m |= 1u << r;
    return m;
}

/* a value every lane holds alike (a field of the record in LDS): tells the compiler so, and the branches on it stay scalar */
__device__ __forceinline__ int v8r_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

/* lanes 0..23: what block `lane` adds, Res[lane][4 r + c]: the WHT per y2 into the luma blocks' DCs, then the block per its code */
__device__ __forceinline__ void v8r_residuals(const FFHipVp8Mb &mb, const int16_t *co, int lane, int (*Res)[16])
{
    if (lane >= 24)
        return;
    int z[16];
#pragma unroll
    for (int k = 0; k < 16; k++)
        z[k] = 0;
    /* vp8_luma_dc_wht across lanes 0..15, lane 4 r + c holding dc[4 r + c]: down the columns (stored to int16 as the reference's dc[]),
     * then along the rows; the lane ends with what block[r][c][0] receives */
    const int y2 = v8r_uniform(mb.y2);
    int wht = 0;
    if (y2 == 2) {
        const int r = (lane >> 2) & 3, c = lane & 3;
        const int v = co[384 + (lane & 15)];
        const int a0 = __shfl(v, c), a1 = __shfl(v, 4 + c), a2 = __shfl(v, 8 + c), a3 = __shfl(v, 12 + c);
        int t0 = a0 + a3, t1 = a1 + a2, t2 = a1 - a2, t3 = a0 - a3;
        const int w = (int16_t)(r == 0 ? t0 + t1 : r == 1 ? t3 + t2 : r == 2 ? t0 - t1 : t3 - t2);
        const int b0 = __shfl(w, 4 * r), b1 = __shfl(w, 4 * r + 1), b2 = __shfl(w, 4 * r + 2), b3 = __shfl(w, 4 * r + 3);
        t0 = b0 + b3 + 3, t1 = b1 + b2, t2 = b1 - b2, t3 = b0 - b3 + 3;
        wht = (int16_t)((c == 0 ? t0 + t1 : c == 1 ? t3 + t2 : c == 2 ? t0 - t1 : t3 - t2) >> 3);
    }
    const int code = v8r_code(mb, lane);
    if (code) {
        const int16_t *b = co + 16 * lane;
        int dc = b[0];
        if (lane < 16 && y2 == 1)
            dc = (int16_t)((co[384] + 3) >> 3); /* vp8_luma_dc_wht_dc */
        else if (lane < 16 && y2 == 2)
            dc = wht;
        if (code == 1) { /* vp8_idct_dc_add */
            const int v = (dc + 4) >> 3;
#pragma unroll
            for (int k = 0; k < 16; k++)
                z[k] = v;
        } else {
            int16_t c[16];
#pragma unroll
            for (int k = 0; k < 16; k++)
                c[k] = b[k];
            c[0] = (int16_t)dc;
            vp8_idct16(c, z);
        }
    }
#pragma unroll
    for (int k = 0; k < 16; k++)
        Res[lane][k] = z[k];
}

/* the VP8 forms of h264_pred_codec.inc over callables */
template <class T, class LR, class LT>
__device__ __forceinline__ int v8r_codec_form(int mode, int x, int y, const T &t, const LR &lraw, const LT &lt)
{
    auto l = [&](int i) -> int { return lraw(i); };
    auto clip = [](int v) -> int { return v < 0 ? 0 : v > 255 ? 255 : v; };
    int v = 0;
#define HP_CODEC_LT lt()
#include "h264_pred_codec.inc"
#undef HP_CODEC_LT
    return v;
}

/* pred16x16[] (N 16: H.264's DC forms) / pred8x8[] (N 8: the RV40 DC forms VP8 installs) of slot `eff` (FFHIP_VP8_PRED_*) for the
 * N x N block whose sample (0, 0) is at T: both DC families are hp_sides_dc (h264_pred_rules.h) over the sides the slot takes */
template <int N>
__device__ __forceinline__ int v8r_blk_dc(int eff, const uint8_t *T, int pitch)
{
    const bool left = eff == FFHIP_VP8_PRED_DC || eff == FFHIP_VP8_PRED_LEFT_DC, top = eff == FFHIP_VP8_PRED_DC || eff == FFHIP_VP8_PRED_TOP_DC;
    int sl = 0, st = 0;
    if (left)
        for (int i = 0; i < N; i++)
            sl += T[i * pitch - 1];
    if (top)
        for (int i = 0; i < N; i++)
            st += T[i - pitch];
    return hp_sides_dc<N>(left, top, sl, st, 128);
}
template <int N>
__device__ __forceinline__ int v8r_blk_sample(int eff, int dc, const uint8_t *T, int pitch, int x, int y)
{
    switch (eff) {
    case FFHIP_VP8_PRED_HOR:    return T[y * pitch - 1];
    case FFHIP_VP8_PRED_VERT:   return T[x - pitch];
    case FFHIP_VP8_PRED_TM:
        return v8r_codec_form(N == 16 ? FFHIP_H264_PREDV16_TM_VP8 : FFHIP_H264_PREDV8_TM_VP8, x, y, [&](int i) -> int { return T[i - pitch]; },
                              [&](int i) -> int { return T[i * pitch - 1]; }, [&]() -> int { return T[-pitch - 1]; });
    case FFHIP_VP8_PRED_DC_127: return 127;
    case FFHIP_VP8_PRED_DC_129: return 129;
    default:                    return dc;
    }
}

/* H.264's pred4x4[mode] (a directional mode, or 0 / 1 for plain VERT / HOR) through imb_p4_entry (h264_intra_mb.h): three samples of
 * the edge line and a weighting, the same straight line in every lane — hp_dir_sample<4>'s switch branches per lane on x and y */
__device__ __forceinline__ int v8r_h264_sample(int mode, const int *E, int x, int y)
{
    const uint32_t c = imb_p4_entry(mode, x, y);
    const int e0 = E[c & 15], e1 = E[(c >> 4) & 15], e2 = E[(c >> 8) & 15], kind = (int)(c >> 12);
    return kind == 0 ? hp_a3(e0, e1, e2) : kind == 1 ? hp_a2(e0, e1) : e0;
}

/* pred4x4[eff] (FFHIP_VP8_B_*) over the sub-block's edge line E[]: 0..3 the left column bottom-up, 4 the corner, 5..8 the row above,
 * 9..12 the top-right */
__device__ __forceinline__ int v8r_sub_sample(int eff, const int *E, int x, int y)
{
    int code;
    switch (eff) {
    case FFHIP_VP8_B_DC_127:     return 127;
    case FFHIP_VP8_B_DC_129:     return 129;
    case FFHIP_VP8_B_VERT:       code = FFHIP_H264_PREDV_VERT_VP8; break;
    case FFHIP_VP8_B_HOR:        code = FFHIP_H264_PREDV_HOR_VP8; break;
    case FFHIP_VP8_B_VL:         code = FFHIP_H264_PREDV_VL_VP8; break;
    case FFHIP_VP8_B_TM:         code = FFHIP_H264_PREDV_TM_VP8; break;
    case FFHIP_VP8_B_DC:         return hp_dir_dc<4>(2, E);
    case FFHIP_VP8_B_VERT_PLAIN: return v8r_h264_sample(0, E, x, y);
    case FFHIP_VP8_B_HOR_PLAIN:  return v8r_h264_sample(1, E, x, y);
    default:                     return v8r_h264_sample(eff, E, x, y); /* DDL, DDR, VR, HD, HU: H.264's */
    }
    return v8r_codec_form(code, x, y, [&](int i) -> int { return E[5 + i]; }, [&](int i) -> int { return E[3 - i]; },
                          [&]() -> int { return E[4]; });
}

__device__ __forceinline__ int v8r_clampi(int v, int hi) { return min(max(v, 0), hi); }
/* the same value, opaque to the compiler's hoisting */
__device__ __forceinline__ int v8r_fresh(int v)
{
    asm volatile("" : "+v"(v));
    return v;
}
} // namespace

__global__ __launch_bounds__(256) void k_vp8_recon_inter(V8rPicSet S, int npics, int mb_w, int mb_h, ptrdiff_t stride_y, ptrdiff_t stride_uv,
                                                         int bilinear, int fullpel)
{
    __shared__ __align__(16) uint8_t Tile[4][384]; /* Y 16 x 16, U 8 x 8 at 256, V 8 x 8 at 320 */
    __shared__ __align__(16) uint8_t Tmp[4][21 * 16];
    __shared__ int ResAll[4][24][16];
    __shared__ __align__(16) FFHipVp8Mb MbAll[4]; /* the wave's record, read once */
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, per = mb_w * mb_h;
    const int id = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + wave);
    if (id >= npics * per)
        return;
    const int f = id / per, m = id - f * per, mb_y = m / mb_w, mb_x = m - mb_y * mb_w;
    const FFHipVp8ReconPic &P = S.pic[f];
    if (!P.mbs[m].ref_frame)
        return;
    if (lane < (int)sizeof(FFHipVp8Mb) / 4)
        reinterpret_cast<uint32_t *>(&MbAll[wave])[lane] = reinterpret_cast<const uint32_t *>(&P.mbs[m])[lane];
    ffhip_wave_sync();
    const FFHipVp8Mb &mb = MbAll[wave];
    const int rf = mb.ref_frame;
    if (!v8r_mb_ok(mb, v8r_refs(P), P.coeff_count))
        return;
    uint8_t *tile = Tile[wave], *tmp = Tmp[wave];
    int (*Res)[16] = ResAll[wave];

    const int n = v8r_npreds(mb.partitioning);
    for (int i = 0; i < n; i++) {
        FFHipVp8Pred Q;
        v8r_pred(mb, i, mb_x, mb_y, fullpel, Q);
        const int W = (Q.plane ? 8 : 16) * mb_w, H = (Q.plane ? 8 : 16) * mb_h, w = Q.w, h = Q.h, lw = w == 16 ? 4 : w == 8 ? 3 : 2;
        const ptrdiff_t ss = Q.plane ? stride_uv : stride_y;
        const uint8_t *src = P.ref[rf - 1][Q.plane];
        const int hs = Q.hslot, vs = Q.vslot, mx = Q.mx, my = Q.my;
        /* the rows the column pass reads: 6 taps from 2 above to 3 below, 4 taps from 1 above to 2 below, bilinear 1 below */
        const int before = !vs || bilinear ? 0 : vs == 2 ? 2 : 1, rows = h + (!vs ? 0 : bilinear ? 1 : vs == 2 ? 5 : 3);
        const uint8_t *FH = c_vp8_subpel[(hs && !bilinear ? mx : 1) - 1], *FV = c_vp8_subpel[(vs && !bilinear ? my : 1) - 1];
        for (int k = lane; k < rows * w; k += 64) {
            const int y = k >> lw, x = k & (w - 1);
            const uint8_t *row = src + (ptrdiff_t)v8r_clampi(Q.sy - before + y, H - 1) * ss;
            auto px = [&](int dx) -> int { return row[v8r_clampi(Q.sx + x + dx, W - 1)]; };
            int v;
            if (!hs) {
                v = px(0);
            } else if (bilinear) {
                v = ((8 - mx) * px(0) + mx * px(1) + 4) >> 3;
            } else {
                int sum = FH[2] * px(0) - FH[1] * px(-1) + FH[3] * px(1) - FH[4] * px(2);
                if (hs == 2)
                    sum += FH[0] * px(-2) + FH[5] * px(3);
                v = vp8_u8((sum + 64) >> 7);
            }
            tmp[k] = (uint8_t)v;
        }
        ffhip_wave_sync();
        const int base = Q.plane ? 256 + 64 * (Q.plane - 1) : 0, pitch = Q.plane ? 8 : 16;
        for (int k = lane; k < h * w; k += 64) {
            const int y = k >> lw, x = k & (w - 1);
            const uint8_t *o = tmp + (y + before) * w + x;
            int v;
            if (!vs) {
                v = o[0];
            } else if (bilinear) {
                v = ((8 - my) * o[0] + my * o[w] + 4) >> 3;
            } else {
                int sum = FV[2] * o[0] - FV[1] * o[-w] + FV[3] * o[w] - FV[4] * o[2 * w];
                if (vs == 2)
                    sum += FV[0] * o[-2 * w] + FV[5] * o[3 * w];
                v = vp8_u8((sum + 64) >> 7);
            }
            tile[base + (Q.y + y) * pitch + Q.x + x] = (uint8_t)v;
        }
        ffhip_wave_sync();
    }

    const bool coded = v8r_coded(mb);
    if (coded) {
        v8r_residuals(mb, P.coeffs + mb.coeff_offset, lane, Res);
        ffhip_wave_sync();
    }
    /* the 96 dwords of the macroblock: 64 luma (row r, dword c), 16 U, 16 V */
    for (int k = lane; k < 96; k += 64) {
        const int plane = k < 64 ? 0 : 1 + ((k - 64) >> 4), q = k < 64 ? k : (k - 64) & 15;
        const int r = plane ? q >> 1 : q >> 2, c = plane ? q & 1 : q & 3;
        const int base = plane ? 256 + 64 * (plane - 1) : 0, pitch = plane ? 8 : 16, bs = plane ? 8 : 16;
        const int blk = plane ? 16 + 4 * (plane - 1) + 2 * (r >> 2) + c : 4 * (r >> 2) + c;
        uint32_t p = *reinterpret_cast<const uint32_t *>(tile + base + r * pitch + 4 * c);
        if (coded) {
            const int *z = Res[blk] + 4 * (r & 3);
            p = pack4(clip_u8((int)(p & 0xFF) + z[0]), clip_u8((int)((p >> 8) & 0xFF) + z[1]), clip_u8((int)((p >> 16) & 0xFF) + z[2]),
                      clip_u8((int)(p >> 24) + z[3]));
        }
        uint8_t *dst = (plane == 0 ? P.y : plane == 1 ? P.u : P.v) + (ptrdiff_t)(mb_y * bs + r) * (plane ? stride_uv : stride_y) + mb_x * bs + 4 * c;
        *reinterpret_cast<uint32_t *>(dst) = p;
    }
}

__global__ __launch_bounds__(64) void k_vp8_recon_intra(V8rPicSet S, int npics, int mb_w, int mb_h, ptrdiff_t stride_y, ptrdiff_t stride_uv,
                                                        int *progress_all, int *fail)
{
    __shared__ __align__(16) uint8_t Ty[17 * V8R_YP];    /* sample (r, c) at [(r + 1) * V8R_YP + c + 4] */
    __shared__ __align__(16) uint8_t Tc[2][9 * V8R_CP];  /* sample (r, c) at [(r + 1) * V8R_CP + c + 4] */
    __shared__ int Res[24][16];
    __shared__ int E[16];
    __shared__ __align__(16) FFHipVp8Mb Mb; /* the macroblock's record, read once */
    const int lane0 = (int)threadIdx.x;
    const int units = npics * mb_h;
    int *const ticket = progress_all + units;
    uint8_t *const Y0 = Ty + V8R_YP + 4; /* the macroblock's sample (0, 0) */

    for (;;) {
        const int t = ffhip_row_ticket(ticket, lane0);
        if (t >= units)
            return;
        const int row = t / npics, f = t - row * npics;
        /* what the row needs of its frame, in locals: the set is indexed once per row */
        uint8_t *const pl[3] = { S.pic[f].y, S.pic[f].u, S.pic[f].v };
        const ptrdiff_t st[3] = { stride_y, stride_uv, stride_uv };
        const FFHipVp8Mb *const rec = S.pic[f].mbs + (ptrdiff_t)row * mb_w;
        const int16_t *const coeffs = S.pic[f].coeffs;
        const int64_t coeff_count = S.pic[f].coeff_count;
        const unsigned refs = v8r_refs(S.pic[f]);
        int *const progress = progress_all + f * mb_h + row; /* [0]: this row's counter, [-1]: the row above's */
        const bool publish = row + 1 < mb_h;
        int known = 0, done = 0, last = -2; /* last: the macroblock the tile holds, written by this wave */

        for (int cx0 = 0; cx0 < mb_w; cx0 += 64) {
            const int xx = cx0 + lane0;
            uint64_t todo = __ballot(xx < mb_w && rec[xx].ref_frame == 0);
            while (todo) {
                const int cx = cx0 + __builtin_ctzll(todo);
                todo &= todo - 1;
                /* the lane number afresh per macroblock: the lane predicates below (lane < 9, lane < 13, ...) are then a compare each
                 * where they are used, not masks computed before the loops and held in scalar register pairs all the way */
                const int lane = v8r_fresh(lane0);
                ffhip_wave_sync(); /* the record before is no longer read */
                if (lane < (int)sizeof(FFHipVp8Mb) / 4)
                    reinterpret_cast<uint32_t *>(&Mb)[lane] = reinterpret_cast<const uint32_t *>(&rec[cx])[lane];
                ffhip_wave_sync();
                const FFHipVp8Mb &mb = Mb;
                if (!v8r_mb_ok(mb, refs, coeff_count))
                    continue; /* writes nothing; still counted */
                /* what this row has passed over is final since the launch before */
                if (publish && done < cx) {
                    ffhip_row_publish(&progress[0], cx, lane);
                    done = cx;
                }
                if (row > 0 && !ffhip_row_wait(&progress[-1], min(cx + 2, mb_w), known, fail, lane))
                    return;

                /* ---- the column to the left, corner included: rows -1..15 (luma), -1..7 (chroma) ---- */
                if (lane < 35) {
                    const int p = lane < 17 ? 0 : 1 + (lane - 17) / 9, r = lane < 17 ? lane - 1 : (lane - 17) % 9 - 1;
                    const int bs = p ? 8 : 16, pitch = p ? V8R_CP : V8R_YP;
                    uint8_t *T = p ? Tc[p - 1] : Ty;
                    int v;
                    if (row == 0 && r < 0)
                        v = 127;
                    else if (cx == 0)
                        v = 129;
                    else if (last == cx - 1)
                        v = T[(r + 1) * pitch + 4 + bs - 1];
                    else
                        v = ffhip_row_ld<uint8_t>(pl[p] + (ptrdiff_t)(row * bs + r) * st[p] + cx * bs - 1);
                    T[(r + 1) * pitch + 3] = (uint8_t)v;
                }
                ffhip_wave_sync();
                /* ---- the row above: luma columns 0..19 (16..19: in the last column the sample at 15, repeated), chroma 0..7 ---- */
                if (lane < 9) {
                    const int p = lane < 5 ? 0 : lane < 7 ? 1 : 2, c = lane < 5 ? lane : (lane - 5) & 1;
                    const int bs = p ? 8 : 16;
                    uint8_t *T = p ? Tc[p - 1] : Ty;
                    uint32_t v = 0x7F7F7F7Fu;
                    if (row > 0) {
                        const bool splat = c == 4 && cx == mb_w - 1;
                        v = ffhip_row_ld<uint32_t>(pl[p] + (ptrdiff_t)(row * bs - 1) * st[p] + cx * bs + 4 * (splat ? 3 : c));
                        if (splat)
                            v = (v >> 24) * 0x01010101u;
                    }
                    *reinterpret_cast<uint32_t *>(T + 4 + 4 * c) = v;
                }
                /* ---- the residuals ---- */
                if (v8r_coded(mb)) {
                    v8r_residuals(mb, coeffs + mb.coeff_offset, lane, Res);
                } else {
                    for (int k = lane; k < 24 * 16; k += 64)
                        (&Res[0][0])[k] = 0;
                }
                ffhip_wave_sync();

                /* ---- chroma: the 8x8 of each plane, a sample per lane ---- */
                {
                    const int eff = v8r_uniform(v8r_intra_blk_mode(mb.chroma_mode, cx, row)), x = lane & 7, y = lane >> 3;
                    const int blk = 2 * (y >> 2) + (x >> 2), zi = 4 * (y & 3) + (x & 3);
                    int v[2];
#pragma unroll
                    for (int p = 0; p < 2; p++) {
                        const uint8_t *C0 = Tc[p] + V8R_CP + 4;
                        v[p] = vp8_u8(v8r_blk_sample<8>(eff, v8r_blk_dc<8>(eff, C0, V8R_CP), C0, V8R_CP, x, y) + Res[16 + 4 * p + blk][zi]);
                    }
                    Tc[0][(y + 1) * V8R_CP + 4 + x] = (uint8_t)v[0];
                    Tc[1][(y + 1) * V8R_CP + 4 + x] = (uint8_t)v[1];
                }
                /* ---- luma ---- */
                const int mode = v8r_uniform(mb.mode);
                if (mode != FFHIP_VP8_MODE_I4x4) {
                    const int eff = v8r_uniform(v8r_intra_blk_mode(mode, cx, row)), y = lane >> 2, bx = lane & 3;
                    const int dc = v8r_blk_dc<16>(eff, Y0, V8R_YP);
                    const int *z = Res[4 * (y >> 2) + bx] + 4 * (y & 3);
                    int v[4];
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        v[j] = clip_u8(v8r_blk_sample<16>(eff, dc, Y0, V8R_YP, 4 * bx + j, y) + z[j]);
                    *reinterpret_cast<uint32_t *>(Y0 + y * V8R_YP + 4 * bx) = pack4(v[0], v[1], v[2], v[3]);
                } else {
#pragma unroll 1
                    for (int b = 0; b < 16; b++) {
                        const int bx = b & 3, by = b >> 2;
                        int copy;
                        const int eff = v8r_uniform(v8r_intra_sub_mode(mb.sub_mode[b], 4 * cx + bx, 4 * row + by, &copy));
                        ffhip_wave_sync(); /* the sub-block before is in the tile */
                        if (lane < 13) {
                            const uint8_t *B = Y0 + 4 * by * V8R_YP + 4 * bx; /* the sub-block's sample (0, 0) */
                            int v;
                            if (lane < 4)
                                v = B[(3 - lane) * V8R_YP - 1];
                            else if (lane < 9)
                                v = B[-V8R_YP + lane - 5];
                            else /* the last column of sub-blocks reads above-right of the macroblock in every row */
                                v = bx == 3 ? Y0[-V8R_YP + 16 + lane - 9] : B[-V8R_YP + lane - 5];
                            E[lane] = v;
                        }
                        ffhip_wave_sync();
                        if (lane < 16) {
                            const int x = lane & 3, y = lane >> 2;
                            Y0[(4 * by + y) * V8R_YP + 4 * bx + x] = (uint8_t)vp8_u8(v8r_sub_sample(eff, E, x, y) + Res[b][lane]);
                        }
                    }
                }
                ffhip_wave_sync();

                /* ---- the macroblock to the frame: 64 luma dwords, 2 x 16 chroma dwords ---- */
                ffhip_row_st<uint32_t>(pl[0] + (ptrdiff_t)(row * 16 + (lane >> 2)) * stride_y + cx * 16 + 4 * (lane & 3),
                                       *reinterpret_cast<const uint32_t *>(Y0 + (lane >> 2) * V8R_YP + 4 * (lane & 3)));
                if (lane < 32) {
                    const int p = lane >> 4, r = (lane >> 1) & 7, c = lane & 1;
                    ffhip_row_st<uint32_t>(pl[1 + p] + (ptrdiff_t)(row * 8 + r) * stride_uv + cx * 8 + 4 * c,
                                           *reinterpret_cast<const uint32_t *>(Tc[p] + (r + 1) * V8R_CP + 4 + 4 * c));
                }
                last = cx;
                /* ---- its stores are acknowledged, then the counter moves ---- */
                if (publish) {
                    ffhip_row_publish(&progress[0], cx + 1, lane);
                    done = cx + 1;
                }
                ffhip_wave_sync(); /* the tile's last column is carried over next */
            }
        }
        if (publish && done < mb_w)
            ffhip_row_publish(&progress[0], mb_w, lane0);
    }
}

int ffhip_launch_vp8_recon_frames(int mb_w, int mb_h, int bilinear, int fullpel_chroma, int npics, const FFHipVp8ReconPic *pics,
                                  ptrdiff_t stride_y, ptrdiff_t stride_uv, hipStream_t stream)
{
    /* a launch's counters (one per macroblock row and frame) and its ticket fit one progress slot */
    int per = (FFHIP_PROGRESS_SLOT_INTS - 1) / mb_h;
    per = per < V8R_PICS ? per : V8R_PICS;
    const int cap = ffhip_cu_count() * V8R_PER_CU;
    for (int p0 = 0; p0 < npics; p0 += per) {
        const int n = npics - p0 < per ? npics - p0 : per;
        V8rPicSet S;
        for (int i = 0; i < V8R_PICS; i++)
            S.pic[i] = pics[p0 + (i < n ? i : 0)];
        /* no keyframe hint: an all-intra batch costs the inter launch its early returns */
        hipLaunchKernelGGL(k_vp8_recon_inter, dim3(cdiv(n * mb_w * mb_h, 4)), dim3(256), 0, stream, S, n, mb_w, mb_h, stride_y, stride_uv, bilinear,
                           fullpel_chroma);
        LAUNCH_CHECK();
        const int units = n * mb_h;
        const int r = ffhip_progress_launch(units + 1, stream, "ffhip_vp8_recon_frames_dev: kernel launch", [&](const FFHipProgressSlot &ps) {
            const int grid = units < cap ? units : cap;
            hipLaunchKernelGGL(k_vp8_recon_intra, dim3(grid), dim3(64), 0, stream, S, n, mb_w, mb_h, stride_y, stride_uv, ps.prog, ps.fail);
            return hipGetLastError();
        });
        if (r < 0)
            return r;
    }
    return 0;
}
