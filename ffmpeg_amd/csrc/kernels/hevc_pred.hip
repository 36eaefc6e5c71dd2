/*
 * hevc_pred.hip — HEVC intra prediction, 8 / 10 / 12 bits (PIX = uint8_t / uint16_t; offsets and strides in bytes), batched:
 * HEVCPredContext.pred_planar / pred_dc / pred_angular (libavcodec/hevc/pred_template.c) and, for records that ask for it, the
 * reference-sample preparation of its intra_pred(): substitution of unavailable samples (H.265 8.4.4.2.2) and filtering
 * (8.4.4.2.3, strong bi-linear smoothing included).
 *
 * The reference line's layout and the per-sample rules are in hevc_intra_rules.h, shared with the picture wavefront
 * (hevc_intra_pic.hip).
 *
 * One wave per record (a batch mixes sizes, and the host cannot read device records): the wave brings the line into LDS
 * (substituting as it reads when the line is raw), filters it into a second LDS copy, then each lane predicts 4 samples of one row
 * from that copy and stores them with one dword-or-wider store where the row's alignment allows.  Blocks of a launch are
 * independent (their lines are inputs); a decoder orders launches by its reconstruction wavefront.
 */
#include "hevc_intra_rules.h"

static_assert(sizeof(FFHipHevcIntra) == 16, "FFHipHevcIntra is a 16-byte record");

template <typename PIX>
__global__ __launch_bounds__(256) void k_hevc_intra(uint8_t *dst, ptrdiff_t stride, const uint8_t *edges, const FFHipHevcIntra *blocks, int n, int bd)
{
    __shared__ int sl[4][2][HI_LINE];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + w);
    FFHipHevcIntra k = {};
    if (b < n)
        k = blocks[b];
    const int log2 = k.log2_size, mode = k.mode, cidx = k.c_idx_unit & 3, luh = (k.c_idx_unit >> 2) & 3, luv = (k.c_idx_unit >> 4) & 3;
    const int N = 1 << (log2 & 7), n2 = 2 * N, LL = 4 * N + 1;
    const bool raw = k.flags & FFHIP_HEVC_INTRA_RAW;
    bool live = b < n && log2 >= 2 && log2 <= 5 && mode <= 34;
    if (raw && ((n2 >> luv) > 16 || (n2 >> luh) > 16 || luv > 2 || luh > 2))
        live = false;
    int *S0 = sl[w][0], *S1 = sl[w][1];
    const int maxv = (1 << bd) - 1;

    /* 1. the line into LDS, substituted when raw */
    if (live) {
        const PIX *e = reinterpret_cast<const PIX *>(edges + k.edge_offset);
        uint64_t m = 0;
        int nl = 0;
        if (raw)
            m = hi_unit_mask(k.avail_left, k.avail_top, k.flags & FFHIP_HEVC_INTRA_CORNER, n2, luv, luh, &nl);
        for (int i = lane; i < LL; i += 64) {
            int src = i;
            if (raw)
                src = hi_subst_src(i, m, n2, nl, luv, luh);
            S0[i] = src < 0 ? 1 << (bd - 1) : (int)e[src];
        }
    }
    __syncthreads();

    /* 2. filtering (8.4.4.2.3) into the second copy; prepared lines are copied as they are */
    if (live)
        hi_filter_line(S0, S1, lane, N, log2, mode, cidx, raw, k.flags, bd);
    __syncthreads();
    if (!live)
        return;

    /* 3. prediction: lane = 4 samples of one row */
    const int dc = mode == 1 ? hi_dc(S1, N, log2) : 0;
    const int qw = N >> 2, items = N * qw;
    for (int it = lane; it < items; it += 64) {
        const int y = it / qw, x0 = 4 * (it - y * qw);
        int v[4];
#pragma unroll
        for (int j = 0; j < 4; j++)
            v[j] = hi_sample<PIX>(S1, N, log2, mode, cidx, x0 + j, y, dc, maxv);
        uint8_t *row = dst + k.dst_offset + (ptrdiff_t)y * stride + x0 * (int)sizeof(PIX);
        const uintptr_t al = reinterpret_cast<uintptr_t>(row);
        if (sizeof(PIX) == 2) {
            uint16_t *d16 = reinterpret_cast<uint16_t *>(row);
            const uint32_t lo = (uint32_t)v[0] | (uint32_t)v[1] << 16, hi = (uint32_t)v[2] | (uint32_t)v[3] << 16;
            if (!(al & 7)) {
                *reinterpret_cast<uint2 *>(d16) = make_uint2(lo, hi);
            } else if (!(al & 3)) {
                reinterpret_cast<uint32_t *>(d16)[0] = lo;
                reinterpret_cast<uint32_t *>(d16)[1] = hi;
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++)
                    d16[j] = (uint16_t)v[j];
            }
        } else {
            if (!(al & 3)) {
                *reinterpret_cast<uint32_t *>(row) = (uint32_t)v[0] | (uint32_t)v[1] << 8 | (uint32_t)v[2] << 16 | (uint32_t)v[3] << 24;
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++)
                    row[j] = (uint8_t)v[j];
            }
        }
    }
}

int ffhip_launch_hevc_intra(int bd, uint8_t *dst, ptrdiff_t stride, const uint8_t *edges, const FFHipHevcIntra *blocks, int n, hipStream_t stream)
{
    if (n <= 0)
        return 0;
    const dim3 grid(cdiv(n, 4)), block(256);
    if (bd == 8)
        hipLaunchKernelGGL(k_hevc_intra<uint8_t>, grid, block, 0, stream, dst, stride, edges, blocks, n, 8);
    else
        hipLaunchKernelGGL(k_hevc_intra<uint16_t>, grid, block, 0, stream, dst, stride, edges, blocks, n, bd);
    LAUNCH_CHECK();
    return 0;
}
