/*
 * hevc_intra_pic.hip — HEVC intra reconstruction of whole pictures in one launch (ffhip_hevc_intra_pictures_dev), 8 / 10 / 12 bits.
 *
 * An intra block reads the reconstructed samples of its left, top-left, top, top-right and bottom-left neighbours, each finished only
 * after its own prediction and residual add, so a picture's intra blocks are one dependency chain (the decoder's z-scan order inside
 * a CTB, CTB to CTB across).  Here one wave per (picture, plane, CTB row) walks its row's CTBs left to right; CTB x of row y needs
 * only CTBs x - 1 of its own row and x - 1 .. x + 1 of row y - 1, so it starts once row y - 1 has finished CTB x + 1 — the only
 * cross-row dependency HEVC intra prediction has (the rows below are later in decoding order with or without tiles: a neighbour in
 * another tile or slice is unavailable, and the caller's masks say so).  Planes are independent chains.
 *
 * Inside a CTB the wave reconstructs on an LDS tile of 16-bit samples, rows -1 .. Ch-1 and columns -1 .. 2Cw-1 of the CTB (Cw x Ch:
 * the CTB in this plane): row -1 is the bottom line of the row above (the corner, the CTB's top and its top-right), read after the
 * wait; column -1 is the previous CTB's right column, kept in the tile; the CTB itself is pre-filled from the plane (the inter and PCM
 * samples are final when the launch starts).  Each block gathers its reference line out of the tile, substitutes and filters it with
 * the rules of hevc_intra_rules.h (shared with k_hevc_intra), predicts, adds its residual, clips, and writes the result to the tile
 * and to the plane — only the samples of its own block, so what no record covers is never written.
 *
 * Hand-off between rows: row_handoff.h, lag 1 (CTB x reads the top-right CTB x + 1 of the row above), rows mapped to workgroups by
 * blockIdx: the row a wave waits for (blockIdx.x - 1, same blockIdx.y) was dispatched before it.
 */
#include <stddef.h>

#include "hevc_intra_rules.h"
#include "row_handoff.h"

static_assert(sizeof(FFHipHevcIntraTU) == 16, "FFHipHevcIntraTU is a 16-byte record");

#define HIP_PICS 16                     /* pictures per launch (the set is a kernel argument: 16 x 120 bytes) */
#define HIP_TILE (65 * 129)             /* (Ch + 1) x (2 Cw + 1) samples at most: a 64 x 64 CTB */

namespace {
struct HipPicSet {
    FFHipHevcIntraPic pic[HIP_PICS];
};

template <typename PIX, typename Q>
__device__ __forceinline__ void quad_to_tile(uint16_t *t, Q q)
{
#pragma unroll
    for (int j = 0; j < 4; j++)
        t[j] = (PIX)(q >> (j * 8 * sizeof(PIX)));
}
} // namespace

/* grid: (planes x ctb_h, pictures); one wave per workgroup */
template <typename PIX>
__global__ __launch_bounds__(64) void k_hevc_intra_pic(HipPicSet S, int nplanes, int cfi, int width, int height, int log2_ctb, int ctb_w,
                                                       int ctb_h, int *progress_all, int *fail, int bd)
{
    typedef typename FFHipQuad<PIX>::T Q;
    constexpr int PS = (int)sizeof(PIX);
    __shared__ uint16_t T[HIP_TILE];
    __shared__ int S0[HI_LINE], S1[HI_LINE];
    const int lane = (int)threadIdx.x;
    const int p = (int)blockIdx.x / ctb_h, row = (int)blockIdx.x - p * ctb_h;
    const FFHipHevcIntraPlane &P = S.pic[blockIdx.y].plane[p];
    uint8_t *const base = P.base;
    const ptrdiff_t stride = P.stride;
    const FFHipHevcIntraTU *const tus = P.tus;
    const int32_t *const ctb_start = P.ctb_start;
    const int16_t *const res = P.res;
    const int hs = p && cfi != 3, vs = p && cfi == 1;
    const int Cw = (1 << log2_ctb) >> hs, Ch = (1 << log2_ctb) >> vs, TP = 2 * Cw + 1;
    const int pw = width >> hs, ph = height >> vs, cy0 = row * Ch;
    const int maxv = (1 << bd) - 1;
    int *const progress = progress_all + ((size_t)blockIdx.y * nplanes + p) * ctb_h + row; /* [0]: this row's counter, [-1]: the row above's */
    const bool publish = row + 1 < ctb_h;
#define TI(r, c) (((r) + 1) * TP + (c) + 1)

    for (int i = lane; i < (Ch + 1) * TP; i += 64)
        T[i] = 0;
    ffhip_wave_sync();
    int known = 0;          /* last value seen of the counter of the row above */
    bool have_left = false; /* column -1 of the next CTB is column Cw - 1 of the tile */
    for (int cx = 0; cx < ctb_w; cx++) {
        const int a = row * ctb_w + cx;
        const int k0 = __builtin_amdgcn_readfirstlane(ctb_start[a]), k1 = __builtin_amdgcn_readfirstlane(ctb_start[a + 1]);
        const int cx0 = cx * Cw;
        if (k0 < k1) {
            /* ---- column -1: the previous CTB's right column (from the tile, or from the plane when that CTB had no records) ---- */
            if (have_left) {
                for (int r = lane; r < Ch; r += 64)
                    T[TI(r, -1)] = T[TI(r, Cw - 1)];
            } else if (cx > 0) {
                for (int r = lane; r < Ch && cy0 + r < ph; r += 64)
                    T[TI(r, -1)] = *reinterpret_cast<const PIX *>(base + (ptrdiff_t)(cy0 + r) * stride + (cx0 - 1) * PS);
            }
            ffhip_wave_sync();
            /* ---- the CTB as the plane holds it, clipped to the picture ---- */
            const int qw = Cw >> 2;
            for (int i = lane; i < Ch * qw; i += 64) {
                const int r = i / qw, c = 4 * (i - r * qw);
                if (cy0 + r < ph && cx0 + c < pw)
                    quad_to_tile<PIX>(&T[TI(r, c)], *reinterpret_cast<const Q *>(base + (ptrdiff_t)(cy0 + r) * stride + (cx0 + c) * PS));
            }
            /* ---- the row above has finished CTB cx + 1 ---- */
            if (row > 0) {
                const int want = min(cx + 2, ctb_w);
                /* ffhip_row_wait() of row_handoff.h, kept inline: the helper form compiles to another schedule here (see docs/EXPERIMENTS.md) */
                int spins = 0;
                while (known < want) {
                    known = __hip_atomic_load(&progress[-1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (known >= want)
                        break;
                    __builtin_amdgcn_s_sleep(2);
                    if (++spins > (1 << 24)) { /* never in a correct run; do not hang the device */
                        if (lane == 0)
                            __hip_atomic_store(fail, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                        return;
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); /* the neighbour loads are issued after the counter was seen */
                /* row -1, columns -4 .. 2Cw - 1 in quads (column -1 is the last sample of the first); widths are multiples of 4 */
                const int c = 4 * lane - 4;
                if (lane <= 2 * qw && cx0 + c >= 0 && cx0 + c < pw) {
                    const Q q = ffhip_row_ld<Q>(base + (ptrdiff_t)(cy0 - 1) * stride + (cx0 + c) * PS);
                    if (c < 0)
                        T[TI(-1, -1)] = (PIX)(q >> (3 * 8 * PS));
                    else
                        quad_to_tile<PIX>(&T[TI(-1, c)], q);
                }
            }
            ffhip_wave_sync();

            /* ---- the CTB's blocks in decoding order ---- */
            FFHipHevcIntraTU nx = tus[k0];
            for (int k = k0; k < k1; k++) {
                const FFHipHevcIntraTU R = nx;
                nx = tus[k + 1 < k1 ? k + 1 : k]; /* the next record leaves while this one is worked on */
                const int log2 = R.log2_size, mode = R.mode, cidx = R.c_idx_unit & 3, luh = (R.c_idx_unit >> 2) & 3,
                          luv = (R.c_idx_unit >> 4) & 3;
                const int N = 1 << (log2 & 7), n2 = 2 * N, x0 = R.x, y0 = R.y;
                const bool ok = log2 >= 2 && log2 <= 5 && mode <= 34 && luv <= 2 && luh <= 2 && (n2 >> luv) <= 16 && (n2 >> luh) <= 16 &&
                                !((x0 | y0) & 3) && x0 >= cx0 && x0 + N <= min(cx0 + Cw, pw) && y0 >= cy0 && y0 + N <= min(cy0 + Ch, ph);
                if (!ok)
                    continue;
                const int lx = x0 - cx0, ly = y0 - cy0, qn = N >> 2, items = N * qn;
                /* the residual leaves first: it is used last */
                int16_t rv[4][4];
                const bool has_res = R.res_offset >= 0;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int it = lane + 64 * j, y = it / qn, xq = 4 * (it - y * qn);
#pragma unroll
                    for (int e = 0; e < 4; e++)
                        rv[j][e] = has_res && it < items ? res[(size_t)R.res_offset + (size_t)y * N + xq + e] : (int16_t)0;
                }
                /* 1. the line out of the tile, substituted (8.4.4.2.2); rows below the CTB are never available: clamped */
                int nl;
                const uint64_t m = hi_unit_mask(R.avail_left, R.avail_top, R.flags & FFHIP_HEVC_INTRA_CORNER, n2, luv, luh, &nl);
                for (int i = lane; i <= 4 * N; i += 64) {
                    const int s = hi_subst_src(i, m, n2, nl, luv, luh);
                    int v = 1 << (bd - 1);
                    if (s >= 0)
                        v = s < n2 ? T[TI(min(ly + n2 - 1 - s, Ch - 1), lx - 1)] : s == n2 ? T[TI(ly - 1, lx - 1)] : T[TI(ly - 1, lx + s - n2 - 1)];
                    S0[i] = v;
                }
                ffhip_wave_sync();
                /* 2. filtering (8.4.4.2.3) */
                hi_filter_line(S0, S1, lane, N, log2, mode, cidx, true, R.flags, bd);
                ffhip_wave_sync();
                /* 3. prediction + residual, clipped: lane = 4 samples of one row, into the tile and the plane */
                const int dc = mode == 1 ? hi_dc(S1, N, log2) : 0;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int it = lane + 64 * j;
                    if (it < items) {
                        const int y = it / qn, xq = 4 * (it - y * qn);
                        Q q = 0;
#pragma unroll
                        for (int e = 0; e < 4; e++) {
                            const int v = min(max(hi_sample<PIX>(S1, N, log2, mode, cidx, xq + e, y, dc, maxv) + rv[j][e], 0), maxv);
                            T[TI(ly + y, lx + xq + e)] = (uint16_t)v;
                            q |= (Q)v << (e * 8 * PS);
                        }
                        ffhip_row_st<Q>(base + (ptrdiff_t)(y0 + y) * stride + (x0 + xq) * PS, q);
                    }
                }
                ffhip_wave_sync(); /* S0 / S1 and the tile are read by the next block */
            }
            have_left = true;
        } else {
            have_left = false;
        }
        /* ---- CTB cx is done: its stores are acknowledged, then the counter moves ---- */
        if (publish) {
            ffhip_row_publish(&progress[0], cx + 1, lane);
        }
    }
#undef TI
}

int ffhip_launch_hevc_intra_pictures(int bd, int cfi, int width, int height, int log2_ctb, int npics, const FFHipHevcIntraPic *pics,
                                     hipStream_t stream)
{
    const int C = 1 << log2_ctb, ctb_w = (width + C - 1) / C, ctb_h = (height + C - 1) / C, nplanes = cfi ? 3 : 1;
    const int rows = nplanes * ctb_h; /* progress counters of one picture: <= FFHIP_PROGRESS_SLOT_INTS (checked by the face) */
    int per = FFHIP_PROGRESS_SLOT_INTS / rows;
    per = per < HIP_PICS ? per : HIP_PICS;
    for (int p0 = 0; p0 < npics; p0 += per) {
        const int n = npics - p0 < per ? npics - p0 : per;
        HipPicSet S;
        for (int i = 0; i < HIP_PICS; i++)
            S.pic[i] = pics[p0 + (i < n ? i : 0)];
        const int r = ffhip_progress_launch(rows * n, stream, "kernel launch", [&](const FFHipProgressSlot &ps) {
            if (bd > 8)
                hipLaunchKernelGGL(k_hevc_intra_pic<uint16_t>, dim3(rows, n), dim3(64), 0, stream, S, nplanes, cfi, width, height, log2_ctb, ctb_w, ctb_h,
                                   ps.prog, ps.fail, bd);
            else
                hipLaunchKernelGGL(k_hevc_intra_pic<uint8_t>, dim3(rows, n), dim3(64), 0, stream, S, nplanes, cfi, width, height, log2_ctb, ctb_w, ctb_h,
                                   ps.prog, ps.fail, 8);
            return hipGetLastError();
        });
        if (r < 0)
            return r;
    }
    return 0;
}
