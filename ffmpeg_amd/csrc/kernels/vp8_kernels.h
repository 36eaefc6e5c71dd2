/* vp8_kernels.h — the VP8 kernels' launchers (vp8_dsp.hip, vp8_lf_frame.hip, vp8_recon_frame.hip) and the loop-filter, tap and
 * transform rules they share.  Internal to
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
/* arguments validated by ffhip_vp8_recon_frames_dev() (vp8_recon_frame.hip) */
int ffhip_launch_vp8_recon_frames(int mb_w, int mb_h, int bilinear, int fullpel_chroma, int npics, const FFHipVp8ReconPic *pics,
                                  ptrdiff_t stride_y, ptrdiff_t stride_uv, hipStream_t stream);

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
/* subpel_filters[mx - 1] (vp8dsp.c): taps F0..F5 for the samples at -2..3; FILTER_6TAP = cm[(F2 s0 - F1 s-1 + F0 s-2 + F3 s1 - F4 s2 +
 * F5 s3 + 64) >> 7], FILTER_4TAP drops F0 and F5 */
static __constant__ uint8_t c_vp8_subpel[7][6] = {
    { 0, 6, 123, 12, 1, 0 }, { 2, 11, 108, 36, 8, 1 }, { 0, 9, 93, 50, 6, 0 }, { 3, 16, 77, 77, 16, 3 },
    { 0, 6, 50, 93, 9, 0 },  { 1, 8, 36, 108, 11, 2 }, { 0, 1, 12, 123, 6, 0 },
};

/* vp8_luma_dc_wht_c on the 16 DCs d[] (overwritten: the first pass stores into the int16 dc[] as the reference does, so its sums wrap
 * to 16 bits the same way): o[4 i + j] is what block[i][j][0] receives */
__device__ __forceinline__ void vp8_wht16(int16_t (&d)[16], int16_t (&o)[16])
{
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const int t0 = d[c] + d[12 + c], t1 = d[4 + c] + d[8 + c], t2 = d[4 + c] - d[8 + c], t3 = d[c] - d[12 + c];
        d[c] = (int16_t)(t0 + t1);
        d[4 + c] = (int16_t)(t3 + t2);
        d[8 + c] = (int16_t)(t0 - t1);
        d[12 + c] = (int16_t)(t3 - t2);
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int t0 = d[4 * r] + d[4 * r + 3] + 3, t1 = d[4 * r + 1] + d[4 * r + 2], t2 = d[4 * r + 1] - d[4 * r + 2],
                  t3 = d[4 * r] - d[4 * r + 3] + 3;
        o[4 * r + 0] = (int16_t)((t0 + t1) >> 3);
        o[4 * r + 1] = (int16_t)((t3 + t2) >> 3);
        o[4 * r + 2] = (int16_t)((t0 - t1) >> 3);
        o[4 * r + 3] = (int16_t)((t3 - t2) >> 3);
    }
}

__device__ __forceinline__ int vp8_mul20091(int a) { return ((a * 20091) >> 16) + a; }
__device__ __forceinline__ int vp8_mul35468(int a) { return (a * 35468) >> 16; }

/* what vp8_idct_add_c adds for the coefficients c[]: z[4 r + col]; the first pass (down the columns) keeps the reference's int16 tmp[] */
__device__ __forceinline__ void vp8_idct16(const int16_t (&c)[16], int (&z)[16])
{
    int16_t tmp[16];
#pragma unroll
    for (int col = 0; col < 4; col++) {
        const int t0 = c[col] + c[8 + col], t1 = c[col] - c[8 + col];
        const int t2 = vp8_mul35468(c[4 + col]) - vp8_mul20091(c[12 + col]), t3 = vp8_mul20091(c[4 + col]) + vp8_mul35468(c[12 + col]);
        tmp[4 * col + 0] = (int16_t)(t0 + t3);
        tmp[4 * col + 1] = (int16_t)(t1 + t2);
        tmp[4 * col + 2] = (int16_t)(t1 - t2);
        tmp[4 * col + 3] = (int16_t)(t0 - t3);
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int t0 = tmp[r] + tmp[8 + r], t1 = tmp[r] - tmp[8 + r];
        const int t2 = vp8_mul35468(tmp[4 + r]) - vp8_mul20091(tmp[12 + r]), t3 = vp8_mul20091(tmp[4 + r]) + vp8_mul35468(tmp[12 + r]);
        z[4 * r + 0] = (t0 + t3 + 4) >> 3;
        z[4 * r + 1] = (t1 + t2 + 4) >> 3;
        z[4 * r + 2] = (t1 - t2 + 4) >> 3;
        z[4 * r + 3] = (t0 - t3 + 4) >> 3;
    }
}
#endif

#endif
