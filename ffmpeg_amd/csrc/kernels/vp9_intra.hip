/*
 * vp9_intra.hip — VP9 intra prediction, 8 / 10 / 12 bits (PIX = uint8_t / uint16_t; offsets and strides in bytes), batched: VP9DSPContext.intra_pred[tx][mode]
 * (libavcodec/vp9dsp_template.c:33-1153; enum IntraPredMode, libavcodec/vp9.h:45-62).
 * A block's neighbours arrive as its "edge line" e[] = left[0..N-1] (bottom to top, as the reference's left[]), the corner, then
 * top[0..] — the samples met walking up the left column, round the corner and along the top; each mode is its per-sample rule
 * over that line (the rules live in vp9_intra_rules.h).  One thread per 4 samples of a row, no block-level state: prediction is a
 * gather.  Blocks of a launch are independent (their edges are inputs); a decoder orders launches by its reconstruction wavefront.
 */
#include "common.h"
#include "h264_kernels.h"
#include "vp9_intra_rules.h"

static_assert(sizeof(FFHipVp9Intra) == 12, "FFHipVp9Intra is a 12-byte record");

template <int LOG2, typename PIX>
__global__ __launch_bounds__(256) void k_vp9_intra(uint8_t *dst, ptrdiff_t stride, const uint8_t *edges, const FFHipVp9Intra *blocks, int n, int bd)
{
    constexpr int N = 1 << LOG2, ITEMS = N * N / 4, QW = N / 4;
    const int gid = blockIdx.x * 256 + threadIdx.x, b = gid / ITEMS, it = gid % ITEMS;
    if (b >= n)
        return;
    const FFHipVp9Intra k = blocks[b];
    const PIX *e = reinterpret_cast<const PIX *>(edges + k.edge_offset);
    const int maxv = (1 << bd) - 1;
    const int mode = k.mode, y = it / QW, x0 = 4 * (it % QW);
    const int dc = vi_dc<LOG2>(mode, e, bd);
    int v[4];
#pragma unroll
    for (int j = 0; j < 4; j++)
        v[j] = vi_sample<LOG2, PIX>(mode, e, x0 + j, y, dc, maxv);
    if (sizeof(PIX) == 2) {
        uint16_t *d16 = reinterpret_cast<uint16_t *>(dst + k.dst_offset + (ptrdiff_t)y * stride) + x0;
        if (!(reinterpret_cast<uintptr_t>(d16) & 7)) {
            *reinterpret_cast<uint2 *>(d16) = make_uint2((uint32_t)v[0] | (uint32_t)v[1] << 16, (uint32_t)v[2] | (uint32_t)v[3] << 16);
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                d16[j] = (uint16_t)v[j];
        }
        return;
    }
    uint8_t *d = dst + k.dst_offset + (ptrdiff_t)y * stride + x0;
    if (!(reinterpret_cast<uintptr_t>(d) & 3)) {
        *reinterpret_cast<uint32_t *>(d) = (uint32_t)v[0] | (uint32_t)v[1] << 8 | (uint32_t)v[2] << 16 | (uint32_t)v[3] << 24;
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
            d[j] = (uint8_t)v[j];
    }
}

int ffhip_launch_vp9_intra(int tx, uint8_t *dst, ptrdiff_t stride, const uint8_t *edges, const FFHipVp9Intra *blocks, int n, hipStream_t stream)
{
    return ffhip_launch_vp9_intra_bd(8, tx, dst, stride, edges, blocks, n, stream);
}

int ffhip_launch_vp9_intra_bd(int bd, int tx, uint8_t *dst, ptrdiff_t stride, const uint8_t *edges, const FFHipVp9Intra *blocks, int n,
                              hipStream_t stream)
{
    if (n <= 0)
        return 0;
    if (tx < 0 || tx > 3) {
        ffhip_set_error("ffhip_vp9_intra: tx %d outside 0..3", tx);
        return FFHIP_EINVAL;
    }
    if (bd != 8 && !((bd == 10 || bd == 12) && !(((uintptr_t)dst | (uintptr_t)edges | (size_t)stride) & 1))) {
        ffhip_set_error("ffhip_vp9_intra: bit depth %d (8, 10, 12) / 16-bit planes must be 2-byte aligned", bd);
        return FFHIP_EINVAL;
    }
    const int items = (16 << (2 * tx)) / 4;
    const dim3 grid(cdiv((int)(((long long)n * items + 255) / 256), 1)), block(256);
#define VI_CASE(T, LG) case T: if (bd == 8) hipLaunchKernelGGL((k_vp9_intra<LG, uint8_t>), grid, block, 0, stream, dst, stride, edges, blocks, n, 8); \
                               else hipLaunchKernelGGL((k_vp9_intra<LG, uint16_t>), grid, block, 0, stream, dst, stride, edges, blocks, n, bd); break;
    switch (tx) {
    VI_CASE(0, 2) VI_CASE(1, 3) VI_CASE(2, 4)
    default:
    VI_CASE(3, 5)
    }
#undef VI_CASE
    LAUNCH_CHECK();
    return 0;
}
