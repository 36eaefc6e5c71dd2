/*
 * vp9_intra_rules.h — the per-sample rules of VP9 intra prediction (libavcodec/vp9dsp_template.c:33-1153; enum IntraPredMode,
 * libavcodec/vp9.h:45-62) over a block's "edge line" e[] = left[0..N-1] (bottom to top, as the reference's left[]; top to bottom for
 * HOR_UP, whose left[] check_intra_mode fills inverted), the corner, then top[0..]: the samples met walking up the left column, round
 * the corner and along the top.  Shared by k_vp9_intra (vp9_intra.hip, edges as inputs) and k_vp9_intra_frame (vp9_intra_frame.hip,
 * edges gathered from the frame being reconstructed).
 */
#ifndef FFHIP_VP9_INTRA_RULES_H
#define FFHIP_VP9_INTRA_RULES_H

#include "common.h"

__device__ __forceinline__ int vi_a2(int a, int b) { return (a + b + 1) >> 1; }
__device__ __forceinline__ int vi_a3(int a, int b, int c) { return (a + 2 * b + c + 2) >> 2; }

template <int LOG2, typename PIX>
__device__ __forceinline__ int vi_sample(int mode, const PIX *e, int x, int y, int dc, int maxv)
{
    constexpr int n = 1 << LOG2;
    const PIX *T = e + n + 1; /* T[-1] = the corner */
    switch (mode) {
    case 0: return T[x];                                                       /* VERT */
    case 1: return e[n - 1 - y];                                               /* HOR */
    case 3: {                                                                  /* DIAG_DOWN_LEFT */
        const int i = x + y;
        if (LOG2 == 2)
            return i < 6 ? vi_a3(T[i], T[i + 1], T[i + 2]) : T[7];
        return i < n - 2 ? vi_a3(T[i], T[i + 1], T[i + 2]) : i == n - 2 ? (T[n - 2] + 3 * T[n - 1] + 2) >> 2 : T[n - 1];
    }
    case 4: {                                                                  /* DIAG_DOWN_RIGHT */
        const int i = n - 1 - y + x;
        return vi_a3(e[i], e[i + 1], e[i + 2]);
    }
    case 5: {                                                                  /* VERT_RIGHT */
        const int i = n / 2 - 1 - (y >> 1) + x;
        if (i >= n / 2 - 1) {
            const int k = n + i - (n / 2 - 1);
            return (y & 1) ? vi_a3(e[k - 1], e[k], e[k + 1]) : vi_a2(e[k], e[k + 1]);
        }
        return (y & 1) ? vi_a3(e[2 * i + 3], e[2 * i + 2], e[2 * i + 1]) : vi_a3(e[2 * i + 4], e[2 * i + 3], e[2 * i + 2]);
    }
    case 6: {                                                                  /* HOR_DOWN */
        const int i = 2 * n - 2 - 2 * y + x;
        if (i >= 2 * n)
            return vi_a3(e[i - n], e[i - n + 1], e[i - n + 2]);
        return (i & 1) ? vi_a3(e[(i >> 1) + 2], e[(i >> 1) + 1], e[i >> 1]) : vi_a2(e[(i >> 1) + 1], e[i >> 1]);
    }
    case 7: {                                                                  /* VERT_LEFT */
        const int i = (y >> 1) + x;
        if (LOG2 == 2)
            return (y & 1) ? vi_a3(T[i], T[i + 1], T[i + 2]) : vi_a2(T[i], T[i + 1]);
        if (i >= n - 1)
            return T[n - 1];
        if (y & 1)
            return i < n - 2 ? vi_a3(T[i], T[i + 1], T[i + 2]) : (T[n - 2] + 3 * T[n - 1] + 2) >> 2;
        return vi_a2(T[i], T[i + 1]);
    }
    case 8: {                                                                  /* HOR_UP */
        const int i = 2 * y + x;
        if (i >= 2 * n - 2)
            return e[n - 1];
        if (i == 2 * n - 3)
            return (e[n - 2] + 3 * e[n - 1] + 2) >> 2;
        return (i & 1) ? vi_a3(e[i >> 1], e[(i >> 1) + 1], e[(i >> 1) + 2]) : vi_a2(e[i >> 1], e[(i >> 1) + 1]);
    }
    case 9: return min(max(T[x] + e[n - 1 - y] - T[-1], 0), maxv);              /* TM */
    default: return dc;                                                        /* the DC family */
    }
}

/* the DC family's value: DC (2), LEFT_DC (10), TOP_DC (11) from the edge line, DC_128 / DC_127 / DC_129 (12 / 13 / 14) constant */
template <int LOG2, typename E>
__device__ __forceinline__ int vi_dc(int mode, const E *e, int bd)
{
    constexpr int N = 1 << LOG2;
    if (mode == 2 || mode == 10 || mode == 11) {
        int sl = 0, st = 0;
        for (int i = 0; i < N; i++) {
            sl += e[i];
            st += e[N + 1 + i];
        }
        return mode == 2 ? (sl + st + N) >> (LOG2 + 1) : ((mode == 10 ? sl : st) + N / 2) >> LOG2;
    }
    if (mode >= 12)
        return (128 << (bd - 8)) + (mode == 12 ? 0 : mode == 13 ? -1 : 1);
    return 0;
}

#endif
