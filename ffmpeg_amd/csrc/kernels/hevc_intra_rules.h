/*
 * hevc_intra_rules.h — the per-sample rules of HEVC intra prediction (H.265 8.4.4.2), shared by the batch kernel on prepared or
 * raw lines (k_hevc_intra, hevc_pred.hip) and the picture wavefront that gathers its lines from the picture (k_hevc_intra_pic,
 * hevc_intra_pic.hip).
 *
 * A block's reference line runs bottom-left to top-right: line[k] = left[2N-1-k] (k < 2N), line[2N] = the corner, line[2N+1+x] =
 * top[x].  So left(y) = line[2N-1-y] and top(x) = line[2N+1+x] for x, y in -1..2N-1, and the angular modes' projected reference
 * row is ref(i) = line[2N + s*i] (s = +1 from the top, -1 from the left) for i >= 0.
 */
#ifndef FFHIP_HEVC_INTRA_RULES_H
#define FFHIP_HEVC_INTRA_RULES_H

#include <stdint.h>

#include "common.h"
#include "h264_kernels.h"

#define HI_LINE 132 /* 4 * 32 + 1 samples, rounded up */

static __constant__ int8_t hi_angle[33] = { 32, 26, 21, 17, 13, 9, 5, 2, 0, -2, -5, -9, -13, -17, -21, -26, -32,
                                            -26, -21, -17, -13, -9, -5, -2, 0, 2, 5, 9, 13, 17, 21, 26, 32 };
static __constant__ int16_t hi_inv_angle[15] = { -4096, -1638, -910, -630, -482, -390, -315, -256, -315, -390, -482, -630, -910, -1638, -4096 };

/* the substitution mask of a raw line: one bit per availability unit along the line (nl = 2N >> luv left units bottom-up, the
 * corner, the 2N >> luh top units) out of the record's avail_left (counted from the top) and avail_top */
__device__ __forceinline__ uint64_t hi_unit_mask(int avail_left, int avail_top, bool corner, int n2, int luv, int luh, int *nl_out)
{
    const int nl = n2 >> luv, nt = n2 >> luh;
    *nl_out = nl;
    return (uint64_t)(__builtin_bitreverse32((uint32_t)avail_left) >> (32 - nl)) | (uint64_t)(corner ? 1 : 0) << nl |
           (uint64_t)(avail_top & ((1u << nt) - 1)) << (nl + 1);
}

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

/* 8.4.4.2.3: the filtered (or, where no filter applies, copied) line S1 out of the substituted line S0, lanes striding by 64.
 * raw: the line was substituted here (prepared lines are copied as they are); flags: FFHIP_HEVC_INTRA_*. */
__device__ __forceinline__ void hi_filter_line(const int *S0, int *S1, int lane, int N, int log2, int mode, int cidx, bool raw, int flags, int bd)
{
    const int n2 = 2 * N, LL = 4 * N + 1;
    const int dist = min(abs(mode - 26), abs(mode - 10)), thresh = log2 == 3 ? 7 : log2 == 4 ? 1 : 0;
    const bool filt = raw && !(flags & FFHIP_HEVC_INTRA_NO_SMOOTH) && (cidx == 0 || (flags & FFHIP_HEVC_INTRA_CHROMA444)) && mode != 1 &&
                      N != 4 && dist > thresh;
    const int c = S0[n2], thr = 1 << (bd - 5);
    const bool strong = filt && (flags & FFHIP_HEVC_INTRA_STRONG) && cidx == 0 && N == 32 && abs(c + S0[128] - 2 * S0[96]) < thr &&
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

/* the DC value of mode 1 out of a prepared line (uniform across the wave) */
__device__ __forceinline__ int hi_dc(const int *L, int N, int log2)
{
    const int n2 = 2 * N;
    int dc = 0;
    for (int i = 0; i < N; i++)
        dc += L[n2 + 1 + i] + L[n2 - 1 - i];
    return (dc + N) >> (log2 + 1);
}

/* 8.4.4.2.4 - 8.4.4.2.6: sample (x, y) of the block predicted from the prepared line L (dc: hi_dc() when mode == 1) */
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

#endif
