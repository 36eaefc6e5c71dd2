/*
 * hevc_tx_rules.h — the arithmetic of the HEVC inverse transforms, shared by the batch kernels of hevc_idct.hip and the residual
 * picture kernel (hevc_res_pic.hip): the core-matrix tables, the 1-D partial-butterfly pass of idct_{4,8,16,32} as v_dot2 products
 * (hevc_pass<N>), the 4x4 DST pass (hevc_dst4) and the 32x32 transform on the matrix cores (hevc_idct32_mfma_lds), restating
 * libavcodec/hevc/dsp_template.c:155-300.
 *
 * Everything here has internal linkage.  Each file that includes it defines its own __constant__ uint32_t[352] table image (a
 * device symbol of its code object), passes it to hevc_pass and uploads it with hevc_pk_upload; hm_tab_init gives each code object
 * its own per-device MFMA operand tables.
 */
#ifndef FFHIP_HEVC_TX_RULES_H
#define FFHIP_HEVC_TX_RULES_H

#include <mutex>
#include <stdint.h>

#include "common.h"

/* |64 sqrt2 cos(m pi / 64)| as the standard rounds it; T32[k][i] = +-g[fold((2i+1)k mod 128)] */
static int8_t hevc_t32_host[32][32];
static std::once_flag hevc_tab_once;
/* the same matrix as int16 PAIRS for v_dot2_i32_i16, per transform size N (offset hevc_pk_off(N)): entry [j][q][0] =
 * (T_N[4q][j], T_N[4q+2][j]) (even basis functions), [j][q][1] = (T_N[4q+1][j], T_N[4q+3][j]) (odd), j < N/2, q < N/4 */
static uint32_t hevc_pk_host[352];
__host__ __device__ constexpr int hevc_pk_off(int n) { return n == 4 ? 0 : n == 8 ? 4 : n == 16 ? 4 + 16 : 4 + 16 + 64; }

static void hevc_build_table()
{
    static const int g[32] = { 64, 90, 90, 90, 89, 88, 87, 85, 83, 82, 80, 78, 75, 73, 70, 67,
                               64, 61, 57, 54, 50, 46, 43, 38, 36, 31, 25, 22, 18, 13, 9, 4 };
    for (int k = 0; k < 32; k++)
        for (int i = 0; i < 32; i++) {
            const int m = ((2 * i + 1) * k) & 127;
            int v;
            if (k == 0) v = 64;
            else if (m < 32) v = g[m];
            else if (m == 32 || m == 96) v = 0;
            else if (m < 64) v = -g[64 - m];
            else if (m < 96) v = -g[m - 64];
            else v = g[128 - m];
            hevc_t32_host[k][i] = (int8_t)v;
        }
    for (int n = 4; n <= 32; n *= 2) {
        const int sc = 32 / n;
        uint32_t *t = hevc_pk_host + hevc_pk_off(n);
        for (int j = 0; j < n / 2; j++)
            for (int q = 0; q < n / 4; q++)
                for (int odd = 0; odd < 2; odd++) {
                    const int a = hevc_t32_host[(4 * q + odd) * sc][j], b = hevc_t32_host[(4 * q + 2 + odd) * sc][j];
                    t[(j * (n / 4) + q) * 2 + odd] = (uint32_t)(a & 0xFFFF) | ((uint32_t)b << 16);
                }
    }
}

__device__ __forceinline__ int hevc_clip16(int v) { return min(max(v, -32768), 32767); }

/* one 1-D pass over the vector at src (stride sstep int16) into dst (stride dstep): N outputs; pk: the includer's table image */
template <int N>
__device__ __forceinline__ void hevc_pass(int16_t *dst, int dstep, const int16_t *src, int sstep, int end, int shift, const uint32_t *pk)
{
    constexpr int SC = 32 / N;
    int s[N];
#pragma unroll
    for (int k = 0; k < N; k++) {
        bool keep = true;
        if (N > 4) {
            if (k & 1) keep = k < end;
            else if (N == 32 && (k & 3) == 2) keep = (k >> 1) < (end >> 1);
        }
        const int v = src[k * sstep];
        s[k] = keep ? v : 0;
    }
    const int add = 1 << (shift - 1);
    /* inputs as int16 pairs (s[4q], s[4q+2]) and (s[4q+1], s[4q+3]): two multiply-adds per v_dot2_i32_i16 against the
     * wave-uniform coefficient pairs */
    typedef short hv_s2 __attribute__((ext_vector_type(2)));
    hv_s2 pe[N / 4], po[N / 4];
#pragma unroll
    for (int q = 0; q < N / 4; q++) {
        pe[q] = hv_s2{ (short)s[4 * q], (short)s[4 * q + 2] };
        po[q] = hv_s2{ (short)s[4 * q + 1], (short)s[4 * q + 3] };
    }
    const uint32_t *tab = pk + hevc_pk_off(N);
    (void)SC;
#pragma unroll
    for (int j = 0; j < N / 2; j++) {
        int e = 0, o = 0;
#pragma unroll
        for (int q = 0; q < N / 4; q++) {
            e = __builtin_amdgcn_sdot2(pe[q], __builtin_bit_cast(hv_s2, tab[(j * (N / 4) + q) * 2]), e, false);
            o = __builtin_amdgcn_sdot2(po[q], __builtin_bit_cast(hv_s2, tab[(j * (N / 4) + q) * 2 + 1]), o, false);
        }
        dst[j * dstep] = (int16_t)hevc_clip16((e + o + add) >> shift);
        dst[(N - 1 - j) * dstep] = (int16_t)hevc_clip16((e - o + add) >> shift);
    }
}

__device__ __forceinline__ void hevc_dst4(int16_t *dst, const int16_t *src, int step, int shift)
{
    const int add = 1 << (shift - 1);
    const int s0 = src[0], s1 = src[step], s2 = src[2 * step], s3 = src[3 * step];
    const int c0 = s0 + s2, c1 = s2 + s3, c2 = s0 - s3, c3 = 74 * s1;
    dst[0]        = (int16_t)hevc_clip16((29 * c0 + 55 * c1 + c3 + add) >> shift);
    dst[step]     = (int16_t)hevc_clip16((55 * c2 - 29 * c1 + c3 + add) >> shift);
    dst[2 * step] = (int16_t)hevc_clip16((74 * (s0 - s2 + s3) + add) >> shift);
    dst[3 * step] = (int16_t)hevc_clip16((55 * c0 + 29 * c2 - c3 + add) >> shift);
}

typedef int hm_i4 __attribute__((ext_vector_type(4)));
typedef int hm_i16 __attribute__((ext_vector_type(16)));
struct HevcMfmaTab { int8_t b1[64][16], b2[64][16]; int32_t sum[32]; }; /* sum[j] = 128 * sum_k T[k][j] */
static std::once_flag hm_once;

__device__ __forceinline__ bool hm_keep(int k, int end) /* hevc_pass<32>'s rule */
{
    return (k & 1) ? k < end : ((k & 3) == 2 ? (k >> 1) < (end >> 1) : true);
}
/* 16 int16 values -> the high-byte plane and the (low byte - 128) plane, 4 bytes per dword in order */
__device__ __forceinline__ void hm_split(const int (&v)[16], hm_i4 &hi, hm_i4 &lo)
{
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint32_t p01 = ((uint32_t)v[4 * q] & 0xFFFFu) | ((uint32_t)v[4 * q + 1] << 16);
        const uint32_t p23 = ((uint32_t)v[4 * q + 2] & 0xFFFFu) | ((uint32_t)v[4 * q + 3] << 16);
        hi[q] = (int)__builtin_amdgcn_perm(p23, p01, 0x07050301u);
        lo[q] = (int)(__builtin_amdgcn_perm(p23, p01, 0x06040200u) ^ 0x80808080u);
    }
}

/* the 32x32 inverse transform of one unit on the matrix cores (k_hevc_idct32_mfma in hevc_idct.hip describes the layout):
 * lds[wave] is the wave's block holding the coefficients row-major, visible to the wave; on return it holds the residual row-major,
 * visible to the wave.  All 64 lanes take part. */
__device__ __forceinline__ void hevc_idct32_mfma_lds(int16_t (*lds)[1024], int wave, int col_limit, int bd, const HevcMfmaTab *tab, int lane)
{
    int16_t *L = lds[wave];
    const int c = lane & 31, g = lane >> 5;
    const hm_i4 B1 = reinterpret_cast<const hm_i4 *>(tab->b1)[lane], B2 = reinterpret_cast<const hm_i4 *>(tab->b2)[lane];
    const int sum_t = tab->sum[c];
    /* ---- pass 1: my column c, rows 16 g .. 16 g + 15; limit2 has shrunk by 4 for every column 4, 8, ... before mine ---- */
    int limit2 = min(col_limit + 4, 32);
    for (int q = 4; q < c; q += 4)
        if (limit2 < 32)
            limit2 -= 4;
    int v[16];
#pragma unroll
    for (int s = 0; s < 16; s++) {
        const int k = 16 * g + s, x = L[k * 32 + c];
        v[s] = hm_keep(k, limit2) ? x : 0;
    }
    hm_i4 ahi, alo;
    hm_split(v, ahi, alo);
    hm_i16 acc = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(ahi, B1, acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; r++)
        acc[r] = (int)(((uint32_t)acc[r] << 8) + (uint32_t)(sum_t + 64));
    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(alo, B1, acc, 0, 0, 0);
    /* ---- Y[j = c][cc], cc = (r & 3) + 8 (r >> 2) + 4 g: >> 7, clip, the second pass's limit ---- */
    const int limit = min(col_limit, 32);
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int cc = (r & 3) + 8 * (r >> 2) + 4 * g;
        const int y = hevc_clip16(acc[r] >> 7);
        v[r] = hm_keep(cc, limit) ? y : 0;
    }
    hm_split(v, ahi, alo);
    const int shift2 = 20 - bd;
#pragma unroll
    for (int r = 0; r < 16; r++)
        acc[r] = 0;
    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(ahi, B2, acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; r++)
        acc[r] = (int)(((uint32_t)acc[r] << 8) + (uint32_t)(sum_t + (1 << (shift2 - 1))));
    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(alo, B2, acc, 0, 0, 0);
    /* ---- Z[j][m = c], j = (r & 3) + 8 (r >> 2) + 4 g: back through LDS into rows; residual in place, picture += residual ---- */
    ffhip_wave_sync(); /* every lane has read its inputs */
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int j = (r & 3) + 8 * (r >> 2) + 4 * g;
        L[j * 32 + c] = (int16_t)hevc_clip16(acc[r] >> shift2);
    }
    ffhip_wave_sync();
}

/* the host tables are built once; their device copies (the includer's __constant__ table image and the two MFMA operand tables)
 * exist per device, uploaded when a device first runs a transform */
static HevcMfmaTab *g_hm_tab16_dev[64];
static HevcMfmaTab *g_hm_tab_dev[64];
static HevcMfmaTab hm_host, hm_host16;
static FFHipPerDeviceOnce hevc_pk_dev_once, hm_dev_once;

/* pk_symbol: HIP_SYMBOL() of the includer's __constant__ uint32_t[352]; who: the entry point named in an error */
static int hevc_pk_upload(const void *pk_symbol, const char *who)
{
    std::call_once(hevc_tab_once, [] { hevc_build_table(); });
    if (hevc_pk_dev_once.enter()) {
        const hipError_t e = hipMemcpyToSymbol(pk_symbol, hevc_pk_host, sizeof(hevc_pk_host));
        hevc_pk_dev_once.leave(e == hipSuccess);
        if (e != hipSuccess) {
            ffhip_set_error("%s: coefficient table upload failed: %s", who, hipGetErrorString(e));
            return FFHIP_EIO;
        }
    }
    return 0;
}

static int hm_tab_init(const char *who)
{
    std::call_once(hevc_tab_once, [] { hevc_build_table(); });
    std::call_once(hm_once, [] {
        HevcMfmaTab &h = hm_host;
        for (int l = 0; l < 64; l++) {
            const int j = l & 31, g = l >> 5;
            for (int s = 0; s < 16; s++) {
                h.b1[l][s] = hevc_t32_host[16 * g + s][j];                              /* T[k = 16 g + s][j]               */
                h.b2[l][s] = hevc_t32_host[(s & 3) + 8 * (s >> 2) + 4 * g][j];        /* T[c = the D row of register s][m] */
            }
        }
        for (int j = 0; j < 32; j++) {
            int t = 0;
            for (int k = 0; k < 32; k++)
                t += hevc_t32_host[k][j];
            h.sum[j] = 128 * t;
        }
        /* the block-diagonal pair of 16-point matrices (T16[k][j] = T32[2 k][j]): slot s of group g belongs to unit s >> 3 and is
         * row 8 g + (s & 7) of T16 in pass 1, row (s & 3) + 8 ((s >> 2) & 1) + 4 g in pass 2 */
        HevcMfmaTab &h16 = hm_host16;
        for (int l = 0; l < 64; l++) {
            const int jp = l & 31, g = l >> 5, j = jp & 15;
            for (int sl = 0; sl < 16; sl++) {
                const bool mine = (sl >> 3) == (jp >> 4);
                h16.b1[l][sl] = mine ? hevc_t32_host[2 * (8 * g + (sl & 7))][j] : 0;
                h16.b2[l][sl] = mine ? hevc_t32_host[2 * ((sl & 3) + 8 * ((sl >> 2) & 1) + 4 * g)][j] : 0;
            }
        }
        for (int jp = 0; jp < 32; jp++) {
            int t = 0;
            for (int k = 0; k < 16; k++)
                t += hevc_t32_host[2 * k][jp & 15];
            h16.sum[jp] = 128 * t;
        }
    });
    if (hm_dev_once.enter()) {
        const int d = ffhip_current_device();
        HevcMfmaTab *t32 = nullptr, *t16 = nullptr;
        const bool ok = hipMalloc(reinterpret_cast<void **>(&t32), sizeof(HevcMfmaTab)) == hipSuccess &&
                        hipMalloc(reinterpret_cast<void **>(&t16), sizeof(HevcMfmaTab)) == hipSuccess &&
                        hipMemcpy(t32, &hm_host, sizeof(HevcMfmaTab), hipMemcpyHostToDevice) == hipSuccess &&
                        hipMemcpy(t16, &hm_host16, sizeof(HevcMfmaTab), hipMemcpyHostToDevice) == hipSuccess;
        if (ok) {
            g_hm_tab_dev[d] = t32;
            g_hm_tab16_dev[d] = t16;
        } else {
            (void)hipFree(t32);
            (void)hipFree(t16);
        }
        hm_dev_once.leave(ok);
        if (!ok) {
            ffhip_set_error("%s: table upload failed", who);
            return FFHIP_EIO;
        }
    }
    return 0;
}

#endif
