/*
 * vp8_dsp.hip — VP8DSPContext's transforms, MC and loop-filter members on the device (libavcodec/vp8dsp.c, 8 bits): the batch faces
 * ffhip_vp8_luma_dc_wht_batch_dev / ffhip_vp8_idct_add_batch_dev / ffhip_vp8_mc_batch_dev and the per-call edges of the host-pointer
 * loop filters (shims_vp8.hip).
 *
 *  - WHT: one lane per macroblock record, the 16 DCs in registers.  The first pass stores into the int16 dc[] as the reference does,
 *    so its sums wrap to 16 bits the same way, and so do the int16 outputs.
 *  - IDCT: one lane per 4x4 block; the first pass (down the columns) keeps the reference's int16 tmp[].  Dword rows when the block is
 *    4-byte aligned, bytes otherwise.
 *  - MC: one wave per record, four records per 256-lane workgroup.  A 2-D call filters rows into a uint8 LDS temporary first (clipped,
 *    as the reference's tmp_array), then columns; a 1-D or copy call goes straight from src.  Only what the record's slot reads of
 *    src is read.
 *  - loop-filter edges: one lane per line (vp8_lf_line, vp8_kernels.h).
 */
#include "common.h"
#include "vp8_kernels.h"

static_assert(sizeof(FFHipVp8WhtRec) == 12, "FFHipVp8WhtRec is a 12-byte record");
static_assert(sizeof(FFHipVp8IdctRec) == 12, "FFHipVp8IdctRec is a 12-byte record");
static_assert(sizeof(FFHipVp8McRec) == 16, "FFHipVp8McRec is a 16-byte record");

__global__ __launch_bounds__(256) void k_vp8_wht(uint8_t *base, const FFHipVp8WhtRec *recs, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n)
        return;
    const FFHipVp8WhtRec R = recs[i];
    if (((R.dc_offset | R.block_offset) & 1) || R.dc_only > 1)
        return;
    int16_t *dc = reinterpret_cast<int16_t *>(base + R.dc_offset), *blk = reinterpret_cast<int16_t *>(base + R.block_offset);
    if (R.dc_only) {
        const int16_t val = (int16_t)((dc[0] + 3) >> 3);
        dc[0] = 0;
        for (int k = 0; k < 16; k++)
            blk[16 * k] = val;
        return;
    }
    int16_t d[16], o[16];
#pragma unroll
    for (int k = 0; k < 16; k++)
        d[k] = dc[k];
    vp8_wht16(d, o);
#pragma unroll
    for (int k = 0; k < 16; k++)
        blk[k * 16] = o[k];
#pragma unroll
    for (int k = 0; k < 16; k++)
        dc[k] = 0;
}

__global__ __launch_bounds__(256) void k_vp8_idct(uint8_t *dst, ptrdiff_t stride, uint8_t *cbase, const FFHipVp8IdctRec *recs, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n)
        return;
    const FFHipVp8IdctRec R = recs[i];
    if ((R.coeff_offset & 1) || R.dc_only > 1)
        return;
    int16_t *b = reinterpret_cast<int16_t *>(cbase + R.coeff_offset);
    uint8_t *d = dst + R.dst_offset;
    int z[16]; /* z[4 r + c]: what row r, column c adds */
    if (R.dc_only) {
        const int dc = (b[0] + 4) >> 3;
        b[0] = 0;
#pragma unroll
        for (int k = 0; k < 16; k++)
            z[k] = dc;
    } else {
        int16_t c[16];
#pragma unroll
        for (int k = 0; k < 16; k++)
            c[k] = b[k];
#pragma unroll
        for (int k = 0; k < 16; k++)
            b[k] = 0;
        vp8_idct16(c, z);
    }
    const bool aligned = !((reinterpret_cast<uintptr_t>(d) | (uintptr_t)stride) & 3);
#pragma unroll
    for (int r = 0; r < 4; r++) {
        uint8_t *row = d + r * stride;
        if (aligned) {
            const uint32_t p = *reinterpret_cast<const uint32_t *>(row);
            *reinterpret_cast<uint32_t *>(row) = pack4(clip_u8((int)(p & 0xFF) + z[4 * r]), clip_u8((int)((p >> 8) & 0xFF) + z[4 * r + 1]),
                                                       clip_u8((int)((p >> 16) & 0xFF) + z[4 * r + 2]), clip_u8((int)(p >> 24) + z[4 * r + 3]));
        } else {
#pragma unroll
            for (int c = 0; c < 4; c++)
                row[c] = (uint8_t)clip_u8((int)row[c] + z[4 * r + c]);
        }
    }
}

/* one tap sum of the 6-tap (T 6) or 4-tap (T 4) form around s[0], samples `step` apart */
__device__ __forceinline__ int vp8_epel(const uint8_t *s, ptrdiff_t step, const uint8_t *F, int taps)
{
    int sum = F[2] * s[0] - F[1] * s[-step] + F[3] * s[step] - F[4] * s[2 * step];
    if (taps == 2)
        sum += F[0] * s[-2 * step] + F[5] * s[3 * step];
    return vp8_u8((sum + 64) >> 7);
}

#define VP8_MC_TMP ((2 * 16 + 5) * 16) /* the reference's tmp_array at width 16, 6-tap */
__global__ __launch_bounds__(256) void k_vp8_mc(uint8_t *dst, ptrdiff_t ds, const uint8_t *src, ptrdiff_t ss, const FFHipVp8McRec *recs, int n)
{
    __shared__ uint8_t tmp_all[4][VP8_MC_TMP];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = blockIdx.x * 4 + wave;
    if (i >= n)
        return;
    const FFHipVp8McRec R = recs[i];
    const int W = R.width, h = R.h, ht = R.htaps, vt = R.vtaps, bil = R.bilinear, mx = R.mx, my = R.my;
    const int lo = bil ? 0 : 1;
    if ((W != 16 && W != 8 && W != 4) || h < 1 || h > 2 * W || ht > 2 || vt > 2 || bil > 1 || (ht && (mx < lo || mx > 7)) ||
        (vt && (my < lo || my > 7)))
        return;
    uint8_t *d = dst + R.dst_offset;
    const uint8_t *s = src + R.src_offset;
    const int lw = W == 16 ? 4 : W == 8 ? 3 : 2;
    if (!ht && !vt) { /* put_vp8_pixels */
        for (int k = lane; k < h * W; k += 64) {
            const int y = k >> lw, x = k & (W - 1);
            d[y * ds + x] = s[y * ss + x];
        }
        return;
    }
    if (bil) {
        const int a = 8 - mx, b = mx, c = 8 - my, e = my;
        if (ht && vt) {
            uint8_t *t = tmp_all[wave];
            for (int k = lane; k < (h + 1) * W; k += 64) {
                const int y = k >> lw, x = k & (W - 1);
                t[k] = (uint8_t)((a * s[y * ss + x] + b * s[y * ss + x + 1] + 4) >> 3);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            for (int k = lane; k < h * W; k += 64) {
                const int y = k >> lw, x = k & (W - 1);
                d[y * ds + x] = (uint8_t)((c * t[k] + e * t[k + W] + 4) >> 3);
            }
        } else {
            const ptrdiff_t step = ht ? 1 : ss;
            const int p = ht ? a : c, q = ht ? b : e;
            for (int k = lane; k < h * W; k += 64) {
                const int y = k >> lw, x = k & (W - 1);
                const uint8_t *o = s + y * ss + x;
                d[y * ds + x] = (uint8_t)((p * o[0] + q * o[step] + 4) >> 3);
            }
        }
        return;
    }
    const uint8_t *FH = c_vp8_subpel[(ht ? mx : 1) - 1], *FV = c_vp8_subpel[(vt ? my : 1) - 1];
    if (ht && vt) {
        uint8_t *t = tmp_all[wave];
        const int before = vt == 2 ? 2 : 1, rows = h + (vt == 2 ? 5 : 3);
        for (int k = lane; k < rows * W; k += 64) {
            const int y = k >> lw, x = k & (W - 1);
            t[k] = (uint8_t)vp8_epel(s + (y - before) * ss + x, 1, FH, ht);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int k = lane; k < h * W; k += 64) {
            const int y = k >> lw, x = k & (W - 1);
            int v;
            { /* the column filter over t, rows y + before - 2 .. y + before + 3 */
                const uint8_t *o = t + (y + before) * W + x;
                int sum = FV[2] * o[0] - FV[1] * o[-W] + FV[3] * o[W] - FV[4] * o[2 * W];
                if (vt == 2)
                    sum += FV[0] * o[-2 * W] + FV[5] * o[3 * W];
                v = vp8_u8((sum + 64) >> 7);
            }
            d[y * ds + x] = (uint8_t)v;
        }
        return;
    }
    const ptrdiff_t step = ht ? 1 : ss;
    const uint8_t *F = ht ? FH : FV;
    const int taps = ht ? ht : vt;
    for (int k = lane; k < h * W; k += 64) {
        const int y = k >> lw, x = k & (W - 1);
        d[y * ds + x] = (uint8_t)vp8_epel(s + y * ss + x, step, F, taps);
    }
}

__global__ __launch_bounds__(256) void k_vp8_lf_edges(uint8_t *base, ptrdiff_t stride, const Vp8LfEdge *edges, int n)
{
    const int t = blockIdx.x * 256 + threadIdx.x, e = t >> 4, l = t & 15;
    if (e >= n)
        return;
    const Vp8LfEdge R = edges[e];
    if (l >= R.lines)
        return;
    const ptrdiff_t step = R.dir ? stride : 1;
    uint8_t *p = base + R.offset + (R.dir ? l : l * stride);
    int v[8];
#pragma unroll
    for (int k = 0; k < 8; k++)
        v[k] = p[(k - 4) * step];
    vp8_lf_line(v, R.kind, R.E, R.I, R.H);
#pragma unroll
    for (int k = 1; k < 7; k++)
        p[(k - 4) * step] = (uint8_t)v[k];
}

#define VP8_LAUNCH(...)                                                                            \
    do {                                                                                           \
        if (n == 0)                                                                                \
            return 0;                                                                              \
        hipLaunchKernelGGL(__VA_ARGS__);                                                           \
        LAUNCH_CHECK();                                                                            \
        return 0;                                                                                  \
    } while (0)

int ffhip_launch_vp8_wht(int16_t *coeffs, const FFHipVp8WhtRec *recs, int n, hipStream_t stream)
{
    VP8_LAUNCH(k_vp8_wht, dim3(cdiv(n, 256)), dim3(256), 0, stream, reinterpret_cast<uint8_t *>(coeffs), recs, n);
}

int ffhip_launch_vp8_idct(uint8_t *dst, ptrdiff_t stride, int16_t *coeffs, const FFHipVp8IdctRec *recs, int n, hipStream_t stream)
{
    VP8_LAUNCH(k_vp8_idct, dim3(cdiv(n, 256)), dim3(256), 0, stream, dst, stride, reinterpret_cast<uint8_t *>(coeffs), recs, n);
}

int ffhip_launch_vp8_mc(uint8_t *dst, ptrdiff_t dststride, const uint8_t *src, ptrdiff_t srcstride, const FFHipVp8McRec *recs, int n,
                        hipStream_t stream)
{
    VP8_LAUNCH(k_vp8_mc, dim3(cdiv(n, 4)), dim3(256), 0, stream, dst, dststride, src, srcstride, recs, n);
}

int ffhip_launch_vp8_lf_edges(uint8_t *base, ptrdiff_t stride, const Vp8LfEdge *edges, int n, hipStream_t stream)
{
    VP8_LAUNCH(k_vp8_lf_edges, dim3(cdiv(n, 16)), dim3(256), 0, stream, base, stride, edges, n);
}
