/* vp8_kernels.h — the VP8 kernels' launchers (vp8_dsp.hip, vp8_lf_frame.hip) and the loop-filter rules they share.  Internal to
 * libffhip; the faces that validate the arguments are in shims_vp8.hip. */
#ifndef FFHIP_VP8_KERNELS_H
#define FFHIP_VP8_KERNELS_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ffhip.h"

/* one loop-filter member call of the host-pointer faces: `lines` lines across the edge whose q0 sample of line 0 is at offset */
struct Vp8LfEdge {
    int32_t offset;   /* bytes into the base */
    uint8_t kind;     /* VP8_LF_MBEDGE, VP8_LF_INNER, VP8_LF_SIMPLE */
    uint8_t dir;      /* 0: h_ members (a column edge: the line runs along the row), 1: v_ members (a row edge) */
    uint8_t lines;    /* 16 or 8 */
    uint8_t E, I, H;
    uint8_t pad[2];
};
static_assert(sizeof(Vp8LfEdge) == 12, "Vp8LfEdge is a 12-byte record");
#define VP8_LF_MBEDGE 0
#define VP8_LF_INNER  1
#define VP8_LF_SIMPLE 2

int ffhip_launch_vp8_wht(int16_t *coeffs, const FFHipVp8WhtRec *recs, int n, hipStream_t stream);
int ffhip_launch_vp8_idct(uint8_t *dst, ptrdiff_t stride, int16_t *coeffs, const FFHipVp8IdctRec *recs, int n, hipStream_t stream);
int ffhip_launch_vp8_mc(uint8_t *dst, ptrdiff_t dststride, const uint8_t *src, ptrdiff_t srcstride, const FFHipVp8McRec *recs, int n,
                        hipStream_t stream);
int ffhip_launch_vp8_lf_edges(uint8_t *base, ptrdiff_t stride, const Vp8LfEdge *edges, int n, hipStream_t stream);
/* arguments validated by ffhip_vp8_loopfilter_frames_dev() */
int ffhip_launch_vp8_lf_frames(int filter_type, int keyframe, int mb_w, int mb_h, int npics, const FFHipVp8LfPic *pics, ptrdiff_t stride_y,
                               ptrdiff_t stride_uv, hipStream_t stream);

#ifdef __HIPCC__
/* vp8dsp.c's loop filter on one line v[0..7] = p3 p2 p1 p0 q0 q1 q2 q3 (8-bit samples in ints), in place:
 *   simple_limit: 2|p0 - q0| + (|p1 - q1| >> 1) <= E;  normal_limit: simple_limit and the six inner differences <= I;
 *   hev: |p1 - p0| > H || |q1 - q0| > H;
 *   filter_common(is4tap): a = clip_int8(3 (q0 - p0) [+ clip_int8(p1 - q1)]), f1 = min(a + 4, 127) >> 3, f2 = min(a + 3, 127) >> 3,
 *     p0 += f2, q0 -= f1 (clamped to 0..255); without is4tap also p1 += (f1 + 1) >> 1, q1 -= the same;
 *   filter_mbedge: w = clip_int8(clip_int8(p1 - q1) + 3 (q0 - p0)), a = (27 w + 63) >> 7, (18 w + 63) >> 7, (9 w + 63) >> 7 on
 *     p0 / q0, p1 / q1, p2 / q2.
 * MB-edge members: hev ? common(4-tap) : mbedge; inner members: common(hev); simple members: simple_limit, then common(4-tap). */
__device__ __forceinline__ int vp8_c8(int v) { return min(max(v, -128), 127); }
__device__ __forceinline__ int vp8_u8(int v) { return min(max(v, 0), 255); }
__device__ __forceinline__ void vp8_lf_line(int (&v)[8], int kind, int E, int I, int H)
{
    const int p3 = v[0], p2 = v[1], p1 = v[2], p0 = v[3], q0 = v[4], q1 = v[5], q2 = v[6], q3 = v[7];
    if (2 * abs(p0 - q0) + (abs(p1 - q1) >> 1) > E)
        return;
    if (kind != VP8_LF_SIMPLE && (abs(p3 - p2) > I || abs(p2 - p1) > I || abs(p1 - p0) > I || abs(q3 - q2) > I || abs(q2 - q1) > I ||
                                  abs(q1 - q0) > I))
        return;
    const bool hv = kind == VP8_LF_SIMPLE || abs(p1 - p0) > H || abs(q1 - q0) > H;
    if (kind == VP8_LF_MBEDGE && !hv) {
        const int w = vp8_c8(vp8_c8(p1 - q1) + 3 * (q0 - p0));
        const int a0 = (27 * w + 63) >> 7, a1 = (18 * w + 63) >> 7, a2 = (9 * w + 63) >> 7;
        v[1] = vp8_u8(p2 + a2); v[2] = vp8_u8(p1 + a1); v[3] = vp8_u8(p0 + a0);
        v[4] = vp8_u8(q0 - a0); v[5] = vp8_u8(q1 - a1); v[6] = vp8_u8(q2 - a2);
        return;
    }
    const int a = vp8_c8(3 * (q0 - p0) + (hv ? vp8_c8(p1 - q1) : 0));
    const int f1 = min(a + 4, 127) >> 3, f2 = min(a + 3, 127) >> 3;
    v[3] = vp8_u8(p0 + f2);
    v[4] = vp8_u8(q0 - f1);
    if (!hv) {
        const int b = (f1 + 1) >> 1;
        v[2] = vp8_u8(p1 + b);
        v[5] = vp8_u8(q1 - b);
    }
}
#endif

#endif
