/*
 * vp9_intra_frame.hip — VP9 intra reconstruction of whole frames in one launch (ffhip_vp9_intra_frames_dev), 8 / 10 / 12 bits.
 *
 * An intra block reads the reconstructed samples of its left, top-left and top neighbours (its 4x4 top-right samples never leave the
 * block: check_intra_mode takes them only while x < w4 - 1), each final only after its own prediction and residual add, so a
 * frame's intra blocks form one dependency chain per plane.  Superblock c of row r needs superblocks c - 1 of its own row and
 * c - 1, c of row r - 1, so one wave per (frame, plane, superblock row) walks its row left to right and starts superblock c once row
 * r - 1 has finished superblock c (lag 0).  Planes are independent chains, and so are frames.
 *
 * Inside a superblock the wave reconstructs on an LDS tile of 16-bit samples, rows -1 .. Ch - 1 and columns -1 .. Cw - 1 (Cw x Ch:
 * the superblock in this plane): the body is filled from the plane (inter samples are final when the launch starts), column -1 is
 * the previous superblock's right column (kept in the tile, or read from the plane when that superblock had no records), and row -1
 * is the bottom line of the row above, read after the wait.  Each record gathers its edge line out of the tile with the clamps and
 * substitutes of check_intra_mode (restated in plane coordinates in include/ffhip.h), predicts with the per-sample rules of
 * vp9_intra_rules.h (shared with k_vp9_intra), adds its residual with vp9_itxfm_tile.h (shared with k_vp9_inter_frame), which clips,
 * and writes its samples inside the decoded area to the tile and to the plane.  What no record covers is never written.
 *
 * Hand-off between rows: row_handoff.h, lag 0 (superblock c reads nothing right of superblock c of the row above), work units by
 * ticket t = row * chains + chain; the grid is min(units, resident capacity).
 */
#include <stddef.h>

#include "common.h"
#include "h264_kernels.h"
#include "row_handoff.h"
#include "vp9_intra_rules.h"
#include "vp9_itxfm_tile.h"

static_assert(sizeof(FFHipVp9IntraRec) == 12, "FFHipVp9IntraRec is a 12-byte record");

#define VIA_PICS 16              /* frames per launch (the set is a kernel argument: 16 x 128 bytes) */
#define VIA_TP 65                /* the tile's row pitch: column -1 .. 63 */
#define VIA_PER_CU 4             /* resident waves per CU the grid counts on: the 16-bit kernel's 256 VGPRs allow one wave per SIMD */

namespace {
struct ViaPicSet {
    FFHipVp9IntraPic pic[VIA_PICS];
};

template <typename PIX, typename Q>
__device__ __forceinline__ void via_quad_to_tile(uint16_t *t, Q q)
{
#pragma unroll
    for (int j = 0; j < 4; j++)
        t[j] = (PIX)(q >> (j * 8 * sizeof(PIX)));
}

/* check_intra_mode's mode_conv[mode][have_left][have_top] */
__device__ __forceinline__ int via_conv(int mode, bool l, bool t)
{
    if (l && t)
        return mode;
    switch (mode) {
    case 0: case 3: case 7: return t ? mode : 13;          /* VERT, DIAG_DOWN_LEFT, VERT_LEFT: DC_127 without top */
    case 1: case 8: return l ? mode : 14;                  /* HOR, HOR_UP: DC_129 without left */
    case 2: return l ? 10 : t ? 11 : 12;                   /* DC: LEFT_DC / TOP_DC / DC_128 */
    case 9: return l ? 1 : t ? 0 : 14;                     /* TM: HOR / VERT / DC_129 */
    default: return mode;                                  /* DIAG_DOWN_RIGHT, VERT_RIGHT, HOR_DOWN */
    }
}

/* prediction of one N x N record into the tile at (lx, ly) from the edge line E (LDS) */
template <int LOG2>
__device__ __forceinline__ void via_predict(uint16_t *T, const int *E, int mode, int lx, int ly, int bd, int maxv, int lane)
{
    constexpr int N = 1 << LOG2;
    const int dc = vi_dc<LOG2>(mode, E, bd);
    for (int i = lane; i < N * N; i += 64) {
        const int y = i >> LOG2, x = i & (N - 1);
        T[(ly + y) * VIA_TP + lx + x] = (uint16_t)vi_sample<LOG2, int>(mode, E, x, y, dc, maxv);
    }
}
} // namespace

/* one wave per workgroup; work units (frame, plane, superblock row) by ticket */
template <typename PIX>
__global__ __launch_bounds__(64) void k_vp9_intra_frame(ViaPicSet S, int npics, int ss_h, int ss_v, int width, int height, int sb_w, int sb_h,
                                                        int *progress_all, int *fail, int bd)
{
    typedef typename FFHipQuad<PIX>::T Q;
    constexpr int PS = (int)sizeof(PIX);
    constexpr bool HBD = PS == 2;
    __shared__ uint16_t Tall[VIA_TP * 65];
    __shared__ int E[32 + 1 + 32];
    __shared__ __align__(16) uint8_t mine[32 * 32 * (HBD ? 4 : 2)]; /* a TU's first-pass output */
    uint16_t *const T = Tall + VIA_TP + 1;                           /* T[r * VIA_TP + c], r and c from -1 */
    const int lane = (int)threadIdx.x;
    const int chains = npics * 3, units = chains * sb_h;
    int *const ticket = progress_all + units;
    const int cols = (width + 7) >> 3, rows = (height + 7) >> 3;
    const int maxv = (1 << bd) - 1, base1 = 128 << (bd - 8);

    for (;;) {
        const int t = ffhip_row_ticket(ticket, lane);
        if (t >= units)
            return;
        const int row = t / chains, chain = t - row * chains, f = chain / 3, p = chain - 3 * f;
        const FFHipVp9IntraPlane &P = S.pic[f].plane[p];
        uint8_t *const pbase = P.base;
        const ptrdiff_t stride = P.stride;
        const FFHipVp9IntraRec *const recs = P.recs;
        const int32_t *const sb_start = P.rec_sb_start;
        const void *const coeffs = P.coeffs;
        const int log2_tiles = S.pic[f].log2_tile_cols;
        const int hs = p ? ss_h : 0, vs = p ? ss_v : 0;
        const int Cw = 64 >> hs, Ch = 64 >> vs, qw = Cw >> 2;
        const int dw = (cols * 8) >> hs, dh = (rows * 8) >> vs, cy0 = row * Ch;
        int *const progress = progress_all + chain * sb_h + row; /* [0]: this row's counter, [-1]: the row above's */
        const bool publish = row + 1 < sb_h;
        int known = 0;          /* last value seen of the counter of the row above */
        bool left_in_tile = false;
        int tile_start = 0;     /* the current tile column's first superblock */

        for (int cx = 0; cx < sb_w; cx++) {
            const int a = row * sb_w + cx;
            const int k0 = __builtin_amdgcn_readfirstlane(sb_start[a]), k1 = __builtin_amdgcn_readfirstlane(sb_start[a + 1]);
            const int cx0 = cx * Cw;
            for (int i = 1; i < (1 << log2_tiles); i++) { /* set_tile_offset: tile column i starts at min((i * sb_w) >> log2, sb_w) */
                const int s = min((i * sb_w) >> log2_tiles, sb_w);
                if (s == cx)
                    tile_start = cx;
            }
            const int ts = (tile_start * 64) >> hs;
            if (k0 < k1) {
                /* ---- column -1: the previous superblock's right column ---- */
                if (left_in_tile) {
                    for (int r = lane; r < Ch; r += 64)
                        T[r * VIA_TP - 1] = T[r * VIA_TP + Cw - 1];
                } else if (cx > 0) {
                    for (int r = lane; r < Ch && cy0 + r < dh; r += 64)
                        T[r * VIA_TP - 1] = *reinterpret_cast<const PIX *>(pbase + (ptrdiff_t)(cy0 + r) * stride + (cx0 - 1) * PS);
                }
                ffhip_wave_sync();
                /* ---- the superblock as the plane holds it, clipped to the decoded area ---- */
                for (int i = lane; i < Ch * qw; i += 64) {
                    const int r = i / qw, c = 4 * (i - r * qw);
                    if (cy0 + r < dh && cx0 + c < dw)
                        via_quad_to_tile<PIX>(&T[r * VIA_TP + c], *reinterpret_cast<const Q *>(pbase + (ptrdiff_t)(cy0 + r) * stride + (cx0 + c) * PS));
                }
                /* ---- the row above has finished superblock cx ---- */
                if (row > 0) {
                    const int want = cx + 1;
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
                    /* row -1, columns -4 .. Cw - 1 in quads (column -1 is the last sample of the first); dw is a multiple of 4 */
                    const int c = 4 * lane - 4;
                    if (lane <= qw && cx0 + c >= 0 && cx0 + c < dw) {
                        const Q q = ffhip_row_ld<Q>(pbase + (ptrdiff_t)(cy0 - 1) * stride + (cx0 + c) * PS);
                        if (c < 0)
                            T[-VIA_TP - 1] = (PIX)(q >> (3 * 8 * PS));
                        else
                            via_quad_to_tile<PIX>(&T[-VIA_TP + c], q);
                    }
                }
                ffhip_wave_sync();

                /* ---- the superblock's records in decoding order ---- */
                for (int k = k0; k < k1; k++) {
                    const FFHipVp9IntraRec R = recs[k];
                    const int tx = R.tx, coded = R.mode, txtp = R.txtp, fl = R.flags, x = R.x, y = R.y;
                    const int lg = tx == 4 ? 2 : 2 + (tx & 3), N = 1 << lg;
                    const bool ok = tx <= 4 && coded <= 9 && txtp <= 3 && !(fl & ~7) && !((fl & 2) && !(fl & 1)) && !((x | y) & (N - 1)) &&
                                    x >= cx0 && x + N <= cx0 + Cw && y >= cy0 && y + N <= cy0 + Ch && x < dw && y < dh &&
                                    !(N == 4 && (fl & 4) && x + 8 > cx0 + Cw);
                    if (!ok)
                        continue;
                    const int lx = x - cx0, ly = y - cy0;
                    const bool have_top = y > 0, have_left = x > ts, have_right = fl & 4;
                    const int mode = via_conv(coded, have_left, have_top);
                    /* 1. the edge line: left (bottom to top; top to bottom for HOR_UP), the corner, top[0 .. max(N, 8) - 1] */
                    for (int i = lane; i < 2 * N + 1 + (N == 4 ? 4 : 0); i += 64) {
                        int v;
                        if (i < N) {
                            const int d = mode == 8 ? i : N - 1 - i; /* rows down from y */
                            v = have_left ? T[(min(y + d, dh - 1) - cy0) * VIA_TP + lx - 1] : base1 + 1;
                        } else if (i == N) {
                            v = !have_top ? base1 - 1 : have_left ? T[(ly - 1) * VIA_TP + lx - 1] : base1 + 1;
                        } else {
                            const int j = i - N - 1;
                            if (!have_top)
                                v = base1 - 1;
                            else if (j < N)
                                v = T[(ly - 1) * VIA_TP + min(x + j, dw - 1) - cx0];
                            else if (have_right && x + 8 <= dw)
                                v = T[(ly - 1) * VIA_TP + lx + j];
                            else
                                v = T[(ly - 1) * VIA_TP + min(x + 3, dw - 1) - cx0];
                        }
                        E[i] = v;
                    }
                    ffhip_wave_sync();
                    /* 2. prediction into the tile */
                    switch (lg) {
                    case 2: via_predict<2>(T, E, mode, lx, ly, bd, maxv, lane); break;
                    case 3: via_predict<3>(T, E, mode, lx, ly, bd, maxv, lane); break;
                    case 4: via_predict<4>(T, E, mode, lx, ly, bd, maxv, lane); break;
                    default: via_predict<5>(T, E, mode, lx, ly, bd, maxv, lane); break;
                    }
                    ffhip_wave_sync();
                    /* 3. the residual, added and clipped in the tile */
                    if (fl & 1) {
                        const void *co = HBD ? (const void *)(static_cast<const int32_t *>(coeffs) + R.coeff_offset)
                                             : (const void *)(static_cast<const int16_t *>(coeffs) + R.coeff_offset);
                        const bool dc = fl & 2;
                        switch (tx) {
                        case 0: vif_tu<2, false, HBD, VIA_TP, false>(T, nullptr, mine, co, txtp, dc, lx, ly, maxv, lane); break;
                        case 1: vif_tu<3, false, HBD, VIA_TP, false>(T, nullptr, mine, co, txtp, dc, lx, ly, maxv, lane); break;
                        case 2: vif_tu<4, false, HBD, VIA_TP, false>(T, nullptr, mine, co, txtp, dc, lx, ly, maxv, lane); break;
                        case 3: vif_tu<5, false, HBD, VIA_TP, false>(T, nullptr, mine, co, txtp, dc, lx, ly, maxv, lane); break;
                        default: vif_tu<2, true, HBD, VIA_TP, false>(T, nullptr, mine, co, txtp, dc, lx, ly, maxv, lane); break;
                        }
                        ffhip_wave_sync();
                    }
                    /* 4. the record's samples inside the decoded area to the plane, a quad per item */
                    const int qn = N >> 2;
                    for (int i = lane; i < N * qn; i += 64) {
                        const int r = i / qn, c = 4 * (i - r * qn);
                        if (y + r < dh && x + c < dw) {
                            const uint16_t *s = &T[(ly + r) * VIA_TP + lx + c];
                            Q q = 0;
#pragma unroll
                            for (int e = 0; e < 4; e++)
                                q |= (Q)(PIX)s[e] << (e * 8 * PS);
                            ffhip_row_st<Q>(pbase + (ptrdiff_t)(y + r) * stride + (x + c) * PS, q);
                        }
                    }
                }
                left_in_tile = true;
            } else {
                left_in_tile = false;
            }
            /* ---- superblock cx is done: its stores are acknowledged, then the counter moves ---- */
            if (publish) {
                ffhip_row_publish(&progress[0], cx + 1, lane);
            }
        }
        ffhip_wave_sync(); /* the tile is reused by the next unit */
    }
}

int ffhip_launch_vp9_intra_frames(int bd, int ss_h, int ss_v, int width, int height, int npics, const FFHipVp9IntraPic *pics, hipStream_t stream)
{
    const int cols = (width + 7) >> 3, rows = (height + 7) >> 3, sb_w = (cols + 7) >> 3, sb_h = (rows + 7) >> 3;
    /* a launch's counters (3 per superblock row and frame) and its ticket fit one progress slot: 3 * 1024 + 1 at most per frame */
    int per = (FFHIP_PROGRESS_SLOT_INTS - 1) / (3 * sb_h);
    per = per < VIA_PICS ? per : VIA_PICS;
    const int cap = ffhip_cu_count() * VIA_PER_CU;
    for (int p0 = 0; p0 < npics; p0 += per) {
        const int n = npics - p0 < per ? npics - p0 : per;
        ViaPicSet S;
        for (int i = 0; i < VIA_PICS; i++)
            S.pic[i] = pics[p0 + (i < n ? i : 0)];
        const int units = 3 * n * sb_h;
        const int r = ffhip_progress_launch(units + 1, stream, "ffhip_vp9_intra_frames_dev: kernel launch", [&](const FFHipProgressSlot &ps) {
            const int grid = units < cap ? units : cap;
            if (bd > 8)
                hipLaunchKernelGGL(k_vp9_intra_frame<uint16_t>, dim3(grid), dim3(64), 0, stream, S, n, ss_h, ss_v, width, height, sb_w, sb_h, ps.prog,
                                   ps.fail, bd);
            else
                hipLaunchKernelGGL(k_vp9_intra_frame<uint8_t>, dim3(grid), dim3(64), 0, stream, S, n, ss_h, ss_v, width, height, sb_w, sb_h, ps.prog,
                                   ps.fail, 8);
            return hipGetLastError();
        });
        if (r < 0)
            return r;
    }
    return 0;
}
