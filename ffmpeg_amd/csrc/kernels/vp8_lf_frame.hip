/*
 * vp8_lf_frame.hip — the VP8 loop filter of whole frames in one launch (ffhip_vp8_loopfilter_frames_dev): filter_mb() /
 * filter_mb_simple() of libavcodec/vp8.c over every macroblock in raster order, up to 16 frames per launch.
 *
 * Macroblock (x, y) reads p3..q3 across its top edge, rows -4..-1 of its columns; they are final once the row above has filtered
 * (x + 1, y - 1), whose left edge writes columns 13..15 of (x, y - 1).  It writes rows -3..-1 of the same columns, which nothing in
 * the row above touches after (x + 1, y - 1).  So one wave per (frame, macroblock row) walks its row left to right and starts
 * macroblock x once the row above has finished min(x + 2, mb_w) macroblocks.  Frames are independent chains.
 *
 * A wave keeps the macroblock and its 4-sample halo in LDS: luma rows -4..15 x columns -4..15 (pitch 20), each chroma plane rows
 * -4..7 x columns -4..7 (pitch 12).  Columns -4..-1 are carried over from the previous macroblock's tile (its columns 12..15, final
 * for this wave), rows 0..15 of the macroblock's own columns are plain loads issued before the wait (nothing writes them in this
 * launch before this wave does), and rows -4..-1 are agent-scope loads issued after it.  The column edges run with a lane per row
 * (luma 0..15, U 16..23, V 24..31) in registers, left to right; the row edges with a lane per column, top to bottom: the order
 * filter_mb keeps within one plane (planes are independent).  The tile then goes back to the frame in dwords, halo included (its
 * untouched samples are final and nothing else writes them at that point).
 *
 * Hand-off between rows: row_handoff.h, lag 1 (the left edge of macroblock x + 1 of the row above writes into the rows this one
 * reads), work units by ticket t = row * npics + frame; the grid is min(units, resident capacity).
 */
#include <stddef.h>

#include "common.h"
#include "progress_pool.h"
#include "row_handoff.h"
#include "vp8_kernels.h"

static_assert(sizeof(FFHipVp8FilterStrength) == 3, "FFHipVp8FilterStrength mirrors VP8FilterStrength");

#define V8F_PICS 16   /* frames per launch (the set is a kernel argument: 16 x 32 bytes) */
#define V8F_PER_CU 8  /* resident waves per CU the grid counts on */
#define V8F_YP 20     /* luma tile pitch: columns -4..15 */
#define V8F_CP 12     /* chroma tile pitch: columns -4..7 */

namespace {
struct V8fPicSet {
    FFHipVp8LfPic pic[V8F_PICS];
};

/* hev_thresh_lut[keyframe][filter_level] (vp8.c filter_mb) */
__constant__ uint8_t c_vp8_hev_lut[2][64] = {
    { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2,
      2, 2, 2, 2, 2, 2, 2, 2, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3 },
    { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
      1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2 },
};


/* the dword item k of a macroblock's tiles: plane (0 Y, 1 U, 2 V), tile row, dword column, for `rows` x `dw` dwords per plane */
struct V8fItem {
    int plane, r, c;
};
__device__ __forceinline__ bool v8f_item(int k, int nplanes, int yrows, int ydw, int crows, int cdw, V8fItem &it)
{
    if (k < yrows * ydw) {
        it.plane = 0; it.r = k / ydw; it.c = k - it.r * ydw;
        return true;
    }
    k -= yrows * ydw;
    if (nplanes == 1 || k >= 2 * crows * cdw)
        return false;
    it.plane = 1 + k / (crows * cdw);
    k -= (it.plane - 1) * crows * cdw;
    it.r = k / cdw; it.c = k - it.r * cdw;
    return true;
}

/* one line of 20 (luma) or 12 (chroma) samples, sample s at v[s + 4]: the edges at 0 (when `first`), then 4, 8, 12 (luma) / 4
 * (chroma) when `inner`, in that order */
__device__ __forceinline__ void v8f_line(int (&v)[20], bool luma, bool first, bool inner, int kind_mb, int kind_in, int mbE, int bE, int I,
                                         int H)
{
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const bool on = e == 0 ? first : (inner && (luma || e == 1));
        if (!on)
            continue;
        int w[8];
#pragma unroll
        for (int k = 0; k < 8; k++)
            w[k] = v[4 * e + k];
        vp8_lf_line(w, e == 0 ? kind_mb : kind_in, e == 0 ? mbE : bE, I, H);
#pragma unroll
        for (int k = 1; k < 7; k++)
            v[4 * e + k] = w[k];
    }
}
} // namespace

__global__ __launch_bounds__(64) void k_vp8_lf_frame(V8fPicSet S, int npics, int mb_w, int mb_h, ptrdiff_t stride_y, ptrdiff_t stride_uv,
                                                     int simple, int keyframe, int *progress_all, int *fail)
{
    __shared__ __align__(16) uint8_t Ty[20 * V8F_YP];
    __shared__ __align__(16) uint8_t Tc[2][12 * V8F_CP];
    const int lane = (int)threadIdx.x;
    const int units = npics * mb_h, nplanes = simple ? 1 : 3;
    int *const ticket = progress_all + units;
    const int kind_mb = simple ? VP8_LF_SIMPLE : VP8_LF_MBEDGE, kind_in = simple ? VP8_LF_SIMPLE : VP8_LF_INNER;

    for (;;) {
        const int t = ffhip_row_ticket(ticket, lane);
        if (t >= units)
            return;
        const int row = t / npics, f = t - row * npics;
        const FFHipVp8LfPic &P = S.pic[f];
        uint8_t *const pl[3] = { P.y, P.u, P.v };
        const ptrdiff_t st[3] = { stride_y, stride_uv, stride_uv };
        const FFHipVp8FilterStrength *const rec = P.strength + (ptrdiff_t)row * mb_w;
        int *const progress = progress_all + f * mb_h + row; /* [0]: this row's counter, [-1]: the row above's */
        const bool publish = row + 1 < mb_h;
        int known = 0;

        for (int cx = 0; cx < mb_w; cx++) {
            /* ---- columns -4..-1: the previous macroblock's columns 12..15 ---- */
            if (cx > 0) {
                if (lane < 20)
                    reinterpret_cast<uint32_t *>(Ty)[lane * 5] = reinterpret_cast<const uint32_t *>(Ty)[lane * 5 + 4];
                else if (!simple && lane < 44) {
                    const int p = (lane - 20) / 12, r = lane - 20 - 12 * p;
                    reinterpret_cast<uint32_t *>(Tc[p])[r * 3] = reinterpret_cast<const uint32_t *>(Tc[p])[r * 3 + 2];
                }
                ffhip_wave_sync();
            }
            /* ---- rows 0..15 of the macroblock's own columns ---- */
            for (int k = lane; k < 64 + 32; k += 64) {
                V8fItem it;
                if (!v8f_item(k, nplanes, 16, 4, 8, 2, it))
                    break;
                const int bs = it.plane ? 8 : 16, pitch = it.plane ? V8F_CP : V8F_YP;
                const uint8_t *src = pl[it.plane] + (ptrdiff_t)(row * bs + it.r) * st[it.plane] + cx * bs + 4 * it.c;
                uint8_t *T = it.plane ? Tc[it.plane - 1] : Ty;
                *reinterpret_cast<uint32_t *>(T + (4 + it.r) * pitch + 4 + 4 * it.c) = *reinterpret_cast<const uint32_t *>(src);
            }
            /* ---- the row above has finished min(cx + 2, mb_w) macroblocks: rows -4..-1 ---- */
            if (row > 0) {
                const int want = min(cx + 2, mb_w);
                if (!ffhip_row_wait(&progress[-1], want, known, fail, lane))
                    return;
                V8fItem it;
                if (lane < 32 && v8f_item(lane, nplanes, 4, 4, 4, 2, it)) {
                    const int bs = it.plane ? 8 : 16, pitch = it.plane ? V8F_CP : V8F_YP;
                    const uint8_t *src = pl[it.plane] + (ptrdiff_t)(row * bs - 4 + it.r) * st[it.plane] + cx * bs + 4 * it.c;
                    uint8_t *T = it.plane ? Tc[it.plane - 1] : Ty;
                    *reinterpret_cast<uint32_t *>(T + it.r * pitch + 4 + 4 * it.c) = ffhip_row_ld<uint32_t>(src);
                }
            }
            ffhip_wave_sync();

            /* ---- the macroblock's filters ---- */
            const FFHipVp8FilterStrength R = rec[cx];
            const int level = R.filter_level, ilim = R.inner_limit;
            const bool ok = level > 0 && level <= 63 && ilim <= 63 && R.inner_filter <= 1;
            if (ok) {
                const bool inner = R.inner_filter;
                const int bE = 2 * level + ilim, mbE = bE + 4, H = c_vp8_hev_lut[keyframe][level];
                const bool luma = lane < 16, active = luma || (!simple && lane < 32);
                const int p = luma ? 0 : 1 + ((lane - 16) >> 3), i = luma ? lane : (lane - 16) & 7;
                uint8_t *T = p ? Tc[p - 1] : Ty;
                const int pitch = p ? V8F_CP : V8F_YP, n = p ? 12 : 20;
                int v[20];
                /* column edges: a lane per row i (tile row 4 + i) */
                if (active) {
#pragma unroll
                    for (int k = 0; k < 20; k++)
                        v[k] = k < n ? T[(4 + i) * pitch + k] : 0;
                    v8f_line(v, luma, cx > 0, inner, kind_mb, kind_in, mbE, bE, ilim, H);
#pragma unroll
                    for (int k = 0; k < 20; k++)
                        if (k < n)
                            T[(4 + i) * pitch + k] = (uint8_t)v[k];
                }
                ffhip_wave_sync();
                /* row edges: a lane per column i (tile column 4 + i) */
                if (active) {
#pragma unroll
                    for (int k = 0; k < 20; k++)
                        v[k] = k < n ? T[k * pitch + 4 + i] : 0;
                    v8f_line(v, luma, row > 0, inner, kind_mb, kind_in, mbE, bE, ilim, H);
#pragma unroll
                    for (int k = 0; k < 20; k++)
                        if (k < n)
                            T[k * pitch + 4 + i] = (uint8_t)v[k];
                }
                ffhip_wave_sync();
                /* ---- the tile back to the frame: rows from -4 (row > 0) or 0, columns from -4 (cx > 0) or 0 ---- */
                const int r0 = row > 0 ? 0 : 4, c0 = cx > 0 ? 0 : 1;
                const int yrows = 20 - r0, ydw = 5 - c0, crows = 12 - r0, cdw = 3 - c0;
                for (int k = lane; k < yrows * ydw + 2 * crows * cdw; k += 64) {
                    V8fItem it;
                    if (!v8f_item(k, nplanes, yrows, ydw, crows, cdw, it))
                        break;
                    const int bs = it.plane ? 8 : 16, pitch = it.plane ? V8F_CP : V8F_YP, tr = r0 + it.r, tc = c0 + it.c;
                    const uint8_t *T = it.plane ? Tc[it.plane - 1] : Ty;
                    uint8_t *dst = pl[it.plane] + (ptrdiff_t)(row * bs - 4 + tr) * st[it.plane] + cx * bs - 4 + 4 * tc;
                    ffhip_row_st<uint32_t>(dst, *reinterpret_cast<const uint32_t *>(T + tr * pitch + 4 * tc));
                }
            }
            /* ---- macroblock cx is done: its stores are acknowledged, then the counter moves ---- */
            if (publish) {
                ffhip_row_publish(&progress[0], cx + 1, lane);
            }
            ffhip_wave_sync(); /* the tile's columns 12..15 are carried over next */
        }
    }
}

int ffhip_launch_vp8_lf_frames(int filter_type, int keyframe, int mb_w, int mb_h, int npics, const FFHipVp8LfPic *pics, ptrdiff_t stride_y,
                               ptrdiff_t stride_uv, hipStream_t stream)
{
    /* a launch's counters (one per macroblock row and frame) and its ticket fit one progress slot */
    int per = (FFHIP_PROGRESS_SLOT_INTS - 1) / mb_h;
    per = per < V8F_PICS ? per : V8F_PICS;
    const int cap = ffhip_cu_count() * V8F_PER_CU;
    for (int p0 = 0; p0 < npics; p0 += per) {
        const int n = npics - p0 < per ? npics - p0 : per;
        V8fPicSet S;
        for (int i = 0; i < V8F_PICS; i++)
            S.pic[i] = pics[p0 + (i < n ? i : 0)];
        const int units = n * mb_h;
        const int r = ffhip_progress_launch(units + 1, stream, "ffhip_vp8_loopfilter_frames_dev: kernel launch", [&](const FFHipProgressSlot &ps) {
            const int grid = units < cap ? units : cap;
            hipLaunchKernelGGL(k_vp8_lf_frame, dim3(grid), dim3(64), 0, stream, S, n, mb_w, mb_h, stride_y, stride_uv, filter_type, keyframe,
                               ps.prog, ps.fail);
            return hipGetLastError();
        });
        if (r < 0)
            return r;
    }
    return 0;
}
