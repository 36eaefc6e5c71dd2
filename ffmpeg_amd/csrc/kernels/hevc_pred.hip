/*
 * hevc_pred.hip — HEVC intra prediction, 8 / 10 / 12 bits (PIX = uint8_t / uint16_t; offsets and strides in bytes), batched:
 * HEVCPredContext.pred_planar / pred_dc / pred_angular (libavcodec/hevc/pred_template.c) and, for records that ask for it, the
 * reference-sample preparation of its intra_pred(): substitution of unavailable samples (H.265 8.4.4.2.2) and filtering
 * (8.4.4.2.3, strong bi-linear smoothing included).
 *
 * A block's reference line runs bottom-left to top-right: line[k] = left[2N-1-k] (k < 2N), line[2N] = the corner, line[2N+1+x] =
 * top[x].  So left(y) = line[2N-1-y] and top(x) = line[2N+1+x] for x, y in -1..2N-1, and the angular modes' projected reference
 * row is ref(i) = line[2N + s*i] (s = +1 from the top, -1 from the left) for i >= 0.
 *
 * One wave per record (a batch mixes sizes, and the host cannot read device records): the wave brings the line into LDS
 * (substituting as it reads when the line is raw), filters it into a second LDS copy, then each lane predicts 4 samples of one row
 * from that copy and stores them with one dword-or-wider store where the row's alignment allows.  Blocks of a launch are
 * independent (their lines are inputs); a decoder orders launches by its reconstruction wavefront.
 */
#include "common.h"
#include "h264_kernels.h"

static_assert(sizeof(FFHipHevcIntra) == 16, "FFHipHevcIntra is a 16-byte record");

#define HI_LINE 132 /* 4 * 32 + 1 samples, rounded up */

__constant__ int8_t hi_angle[33] = { 32, 26, 21, 17, 13, 9, 5, 2, 0, -2, -5, -9, -13, -17, -21, -26, -32,
                                     -26, -21, -17, -13, -9, -5, -2, 0, 2, 5, 9, 13, 17, 21, 26, 32 };
__constant__ int16_t hi_inv_angle[15] = { -4096, -1638, -910, -630, -482, -390, -315, -256, -315, -390, -482, -630, -910, -1638, -4096 };

/* the sample substitution takes for line[k] when k is unavailable: the nearest available sample below it, or, when there is none
 * below, the first available one.  m: one bit per availability unit along the line (nl left units bottom-up, the corner, the top
 * units); -1 when nothing is available. */
__device__ __forceinline__ int hi_subst_src(int k, uint64_t m, int n2, int nl, int luv, int luh)
{
    if (!m)
        return -1;
    const int u = k < n2 ? k >> luv : k == n2 ? nl : nl + 1 + ((k - n2 - 1) >> luh);
    if ((m >> u) & 1)
        return k;
    const uint64_t below = m & ((1ull << u) - 1);
    if (below) {
        const int j = 63 - __builtin_clzll(below); /* its last sample */
        return j < nl ? ((j + 1) << luv) - 1 : j == nl ? n2 : n2 + ((j - nl) << luh);
    }
    const int j = __builtin_ctzll(m); /* its first sample */
    return j < nl ? j << luv : j == nl ? n2 : n2 + 1 + ((j - nl - 1) << luh);
}

template <typename PIX>
__device__ __forceinline__ int hi_sample(const int *L, int N, int log2, int mode, int cidx, int x, int y, int dc, int maxv)
{
    const int n2 = 2 * N, c = L[n2];
    if (mode == 0)
        return ((N - 1 - x) * L[n2 - 1 - y] + (x + 1) * L[n2 + 1 + N] + (N - 1 - y) * L[n2 + 1 + x] + (y + 1) * L[n2 - 1 - N] + N) >> (log2 + 1);
    if (mode == 1) {
        if (cidx == 0 && N < 32) {
            if (x == 0 && y == 0)
                return (L[n2 - 1] + 2 * dc + L[n2 + 1] + 2) >> 2;
            if (y == 0)
                return (L[n2 + 1 + x] + 3 * dc + 2) >> 2;
            if (x == 0)
                return (L[n2 - 1 - y] + 3 * dc + 2) >> 2;
        }
        return dc;
    }
    if (cidx == 0 && N < 32) { /* boundary filters of the pure vertical / horizontal modes */
        if (mode == 26 && x == 0)
            return min(max(L[n2 + 1] + ((L[n2 - 1 - y] - c) >> 1), 0), maxv);
        if (mode == 10 && y == 0)
            return min(max(L[n2 - 1] + ((L[n2 + 1 + x] - c) >> 1), 0), maxv);
    }
    const bool vert = mode >= 18;
    const int s = vert ? 1 : -1, u = vert ? x : y, v = vert ? y : x;
    const int angle = hi_angle[mode - 2], inv = (mode >= 11 && mode <= 25) ? hi_inv_angle[mode - 11] : 0;
    const int idx = ((v + 1) * angle) >> 5, f = ((v + 1) * angle) & 31;
    const int i0 = u + idx + 1;
    /* ref(i) for i < 0 projects onto the other side (only reached when angle < 0 and (N * angle >> 5) < -1) */
    const int a = L[i0 >= 0 ? n2 + s * i0 : n2 - s * ((i0 * inv + 128) >> 8)];
    if (!f)
        return a;
    const int i1 = i0 + 1;
    const int b = L[i1 >= 0 ? n2 + s * i1 : n2 - s * ((i1 * inv + 128) >> 8)];
    return ((32 - f) * a + f * b + 16) >> 5;
}

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
        if (raw) {
            nl = n2 >> luv;
            const int nt = n2 >> luh;
            m = (uint64_t)(__builtin_bitreverse32((uint32_t)k.avail_left) >> (32 - nl)) |
                (uint64_t)((k.flags & FFHIP_HEVC_INTRA_CORNER) ? 1 : 0) << nl | (uint64_t)(k.avail_top & ((1u << nt) - 1)) << (nl + 1);
        }
        for (int i = lane; i < LL; i += 64) {
            int src = i;
            if (raw)
                src = hi_subst_src(i, m, n2, nl, luv, luh);
            S0[i] = src < 0 ? 1 << (bd - 1) : (int)e[src];
        }
    }
    __syncthreads();

    /* 2. filtering (8.4.4.2.3) into the second copy; prepared lines are copied as they are */
    if (live) {
        const int dist = min(abs(mode - 26), abs(mode - 10)), thresh = log2 == 3 ? 7 : log2 == 4 ? 1 : 0;
        const bool filt = raw && !(k.flags & FFHIP_HEVC_INTRA_NO_SMOOTH) && (cidx == 0 || (k.flags & FFHIP_HEVC_INTRA_CHROMA444)) && mode != 1 &&
                          N != 4 && dist > thresh;
        const int c = S0[n2], thr = 1 << (bd - 5);
        const bool strong = filt && (k.flags & FFHIP_HEVC_INTRA_STRONG) && cidx == 0 && N == 32 && abs(c + S0[128] - 2 * S0[96]) < thr &&
                            abs(c + S0[0] - 2 * S0[32]) < thr;
        for (int i = lane; i < LL; i += 64) {
            int v = S0[i];
            if (strong) {
                if (i > n2 && i < 4 * N)
                    v = ((63 - (i - n2 - 1)) * c + (i - n2) * S0[128] + 32) >> 6;
                else if (i > 0 && i < n2)
                    v = ((63 - (n2 - 1 - i)) * c + (n2 - i) * S0[0] + 32) >> 6;
            } else if (filt && i > 0 && i < 4 * N) {
                v = (S0[i - 1] + 2 * v + S0[i + 1] + 2) >> 2;
            }
            S1[i] = v;
        }
    }
    __syncthreads();
    if (!live)
        return;

    /* 3. prediction: lane = 4 samples of one row */
    int dc = 0;
    if (mode == 1) {
        for (int i = 0; i < N; i++)
            dc += S1[n2 + 1 + i] + S1[n2 - 1 - i];
        dc = (dc + N) >> (log2 + 1);
    }
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
