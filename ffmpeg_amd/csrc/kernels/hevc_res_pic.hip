/*
 * hevc_res_pic.hip — HEVC residuals of whole pictures in one launch (ffhip_hevc_residual_pictures_dev), 8 / 10 / 12 bits.
 *
 * Every transform unit of up to 16 pictures goes from its scaled coefficients to its final residual: rotation, the kind's operation
 * (idct / idct_dc / transform_4x4_luma / dequant / bypass / zero), RDPCM, then cross-component prediction, with the arithmetic of
 * the batch kernels (hevc_tx_rules.h: hevc_pass<N>, hevc_dst4, the 32x32 matrix-core transform).
 *
 * The grid is a concatenation of segments, one per (picture, plane, log2 size) with records, each a run of workgroups over that
 * group of records; the host builds the segment table and stages it in a progress-pool slot, the way the inter face stages its
 * pictures.  A workgroup therefore has one size and a uniform code path; kinds may mix within a wave.  Per size the layout is that
 * of k_hevc_idct: a unit is N lanes (64 / N units per wave) staged in wave-private LDS with 16-byte accesses, lane i of a unit
 * transforms column i then row i.  32x32 units take a whole wave each, so that the DCT runs on the matrix cores
 * (hevc_idct32_mfma_lds) and the other kinds use lanes 0..31.
 *
 * A _CROSS record recomputes its luma record's final residual in a second LDS block of the same wave (4:4:4 chroma TUs have the
 * luma TU's size), so nothing depends on record order or on which workgroup runs first.  Records are checked before anything is
 * read (include/ffhip.h lists what is malformed); a malformed record reads and writes nothing.
 */
#include <stddef.h>

#include "common.h"
#include "h264_kernels.h"
#include "hevc_tx_rules.h"

static_assert(sizeof(FFHipHevcResTU) == 16, "FFHipHevcResTU is a 16-byte record");
static_assert(sizeof(FFHipHevcResPlane) == 56, "FFHipHevcResPlane is 56 bytes");

__constant__ uint32_t hevc_res_pk[352]; /* hevc_tx_rules.h's table image for this code object */

#define HRP_PICS 16 /* pictures per launch */

namespace {
/* one (picture, plane, size) group of records and the plane-0 records its _CROSS records may name */
struct HrpSeg {
    const int16_t *coeffs;
    int16_t *res;
    const FFHipHevcResTU *tus;
    const int16_t *lcoeffs;         /* plane 0 of the same picture */
    const FFHipHevcResTU *ltus;
    int32_t ncoeffs, nres, lncoeffs, lnres;
    int32_t tu0, ntus;              /* tus[tu0 .. tu0 + ntus) */
    int32_t l_lo, l_hi;             /* plane 0's records of this size: a _CROSS record's `luma` lies in [l_lo, l_hi) */
    int32_t blk0;                   /* the segment's first workgroup */
    int32_t log2, cross_ok;         /* cross_ok: plane 1 or 2 of chroma format 3 */
    int32_t pad;
};
static_assert(sizeof(HrpSeg) % 8 == 0, "HrpSeg is staged as an array");
constexpr int HRP_MAX_SEGS = HRP_PICS * 3 * 4;
static_assert(HRP_MAX_SEGS * sizeof(HrpSeg) <= FFHIP_PROGRESS_SLOT_INTS * sizeof(int), "a launch's segments fit one slot");

/* the checks of include/ffhip.h that one record can fail by itself, against the plane lengths */
__device__ __forceinline__ bool hrp_record_ok(const FFHipHevcResTU &t, int log2, int ncoeffs, int nres, bool cross_ok)
{
    const int kf = t.kind_flags, kind = kf & FFHIP_HEVC_RES_KIND, nn = 1 << (2 * log2);
    const bool skipish = kind == FFHIP_HEVC_RES_SKIP || kind == FFHIP_HEVC_RES_BYPASS;
    if (t.log2_size != log2 || kind > FFHIP_HEVC_RES_ZERO || (kf & 0x80))
        return false;
    if (kind == FFHIP_HEVC_RES_DST && log2 != 2)
        return false;
    if ((kf & FFHIP_HEVC_RES_ROTATE) && (log2 != 2 || !skipish))
        return false;
    if ((kf & (FFHIP_HEVC_RES_RDPCM_H | FFHIP_HEVC_RES_RDPCM_V)) &&
        (!skipish || (kf & (FFHIP_HEVC_RES_RDPCM_H | FFHIP_HEVC_RES_RDPCM_V)) == (FFHIP_HEVC_RES_RDPCM_H | FFHIP_HEVC_RES_RDPCM_V)))
        return false;
    if (kf & FFHIP_HEVC_RES_CROSS) {
        const int s = t.res_scale_val, a = s < 0 ? -s : s;
        if (!cross_ok || (a != 0 && a != 1 && a != 2 && a != 4 && a != 8))
            return false;
    }
    return !(t.coeff_offset & 15) && !(t.res_offset & 15) && t.coeff_offset >= 0 && t.res_offset >= 0 && t.coeff_offset <= ncoeffs - nn &&
           t.res_offset <= nres - nn;
}

/* rotate -> the kind's operation -> RDPCM on the unit at `mine` (N*N int16, row-major, in LDS), lane i of the unit; `act`: the lane
 * is one of the unit's N (always, below 32x32).  Kinds may differ between the units of a wave; every lane of a unit takes the same
 * branches.  The 32x32 DCT is the matrix-core pass and needs the whole wave: the caller runs it (the kind is wave-uniform there). */
template <int N>
__device__ __forceinline__ void hrp_unit(int16_t *mine, int i, bool act, int kind, int kf, int col_limit, int bd)
{
    if (N == 4 && act && (kf & FFHIP_HEVC_RES_ROTATE)) { /* c[k] <-> c[15 - k]: row i is row 3 - i reversed */
        int r[4];
#pragma unroll
        for (int x = 0; x < 4; x++)
            r[x] = mine[(3 - i) * 4 + 3 - x];
        ffhip_wave_sync();
#pragma unroll
        for (int x = 0; x < 4; x++)
            mine[i * 4 + x] = (int16_t)r[x];
    }
    ffhip_wave_sync();
    if (N < 32 && act && kind == FFHIP_HEVC_RES_DCT) {
        const int limit = min(col_limit, N);
        int limit2 = min(col_limit + 4, N); /* shrunk by 4 for every column 4, 8, ... before mine while it was < N */
        for (int c = 4; c < i; c += 4)
            if (limit2 < N)
                limit2 -= 4;
        hevc_pass<N < 32 ? N : 16>(mine + i, N, mine + i, N, limit2, 7, hevc_res_pk);
        ffhip_wave_sync();
        hevc_pass<N < 32 ? N : 16>(mine + i * N, 1, mine + i * N, 1, limit, 20 - bd, hevc_res_pk);
    } else if (act && kind == FFHIP_HEVC_RES_DC) {
        const int v = ((((int)mine[0] + 1) >> 1) + (1 << (13 - bd))) >> (14 - bd);
        ffhip_wave_sync();
#pragma unroll
        for (int k = 0; k < N; k++)
            mine[i * N + k] = (int16_t)v;
    } else if (N == 4 && act && kind == FFHIP_HEVC_RES_DST) {
        hevc_dst4(mine + i, mine + i, 4, 7);
        ffhip_wave_sync();
        hevc_dst4(mine + 4 * i, mine + 4 * i, 1, 20 - bd);
    } else if (act && kind == FFHIP_HEVC_RES_SKIP) {
        /* dequant (hevc/dsp_template.c:110-143), row i: as k_hevc_idct's DEQUANT */
        const int shift = 15 - bd - (N == 4 ? 2 : N == 8 ? 3 : N == 16 ? 4 : 5);
#pragma unroll
        for (int k = 0; k < N; k++) {
            const int c = mine[i * N + k];
            mine[i * N + k] = (int16_t)(shift > 0 ? (c + (1 << (shift - 1))) >> shift : shift < 0 ? (int)((uint32_t)(uint16_t)c << -shift) : c);
        }
    }
    ffhip_wave_sync();
    if (act && (kf & (FFHIP_HEVC_RES_RDPCM_H | FFHIP_HEVC_RES_RDPCM_V))) {
        /* transform_rdpcm (hevc/dsp_template.c:85-105): running sums in int16 along row i (mode 0) or down column i (mode 1) */
        const bool h = kf & FFHIP_HEVC_RES_RDPCM_H;
        const int step = h ? 1 : N;
        int16_t *v = mine + (h ? i * N : i);
        int acc = v[0];
#pragma unroll
        for (int k = 1; k < N; k++) {
            acc = (int16_t)(acc + v[k * step]);
            v[k * step] = (int16_t)acc;
        }
    }
    ffhip_wave_sync();
}

/* the wave's units of one segment: UPW units of N lanes (one unit of 64 lanes at 32x32) */
template <int LOG2>
__device__ __forceinline__ void hrp_wave(const HrpSeg &S, int unit0, int16_t (*lds)[1024], int16_t (*ldsl)[1024], int wave, int lane, int bd,
                                         const HevcMfmaTab *tab)
{
    constexpr int N = 1 << LOG2, UPW = N == 32 ? 1 : 64 / N, LPU = 64 / UPW; /* units per wave, lanes per unit */
    constexpr int Q4 = N * N / 8, ITER = (UPW * Q4 + 63) / 64;                  /* 16-byte pieces per unit, per lane */
    const int ul = lane / LPU, i = (lane % LPU) & (N - 1);
    const bool act = (lane % LPU) < N;
    const int u = unit0 + ul;
    /* ---- my unit's record, and its luma record for _CROSS ---- */
    bool ok = false, cross = false;
    FFHipHevcResTU t = {}, lt = {};
    if (u < S.ntus) {
        t = S.tus[S.tu0 + u];
        ok = hrp_record_ok(t, LOG2, S.ncoeffs, S.nres, S.cross_ok);
        if (ok && (t.kind_flags & FFHIP_HEVC_RES_CROSS)) {
            cross = true;
            const int li = t.luma;
            ok = li >= S.l_lo && li < S.l_hi;
            if (ok) {
                lt = S.ltus[li];
                ok = hrp_record_ok(lt, LOG2, S.lncoeffs, S.lnres, false);
            }
        }
    }
    const int kind = t.kind_flags & FFHIP_HEVC_RES_KIND, lkind = lt.kind_flags & FFHIP_HEVC_RES_KIND;
    const bool any_cross = __any(ok && cross);
    int16_t *blk = lds[wave], *blkl = ldsl[wave];
    /* ---- stage the coefficients (zeros for ZERO records and malformed units); every lane takes part in the shuffles ---- */
    for (int it = 0; it < ITER; it++) {
        const int q = lane + 64 * it, b = min(q / Q4, UPW - 1), w = q % Q4;
        const int bok = __shfl(ok ? 1 : 0, b * LPU, 64), bkind = __shfl(kind, b * LPU, 64), boff = __shfl(t.coeff_offset, b * LPU, 64);
        uint4 v = make_uint4(0, 0, 0, 0);
        if (q < UPW * Q4 && bok && bkind != FFHIP_HEVC_RES_ZERO)
            v = reinterpret_cast<const uint4 *>(S.coeffs + boff)[w];
        if (q < UPW * Q4)
            reinterpret_cast<uint4 *>(blk)[q] = v;
        if (any_cross) {
            const int bc = __shfl(cross ? 1 : 0, b * LPU, 64), blkind = __shfl(lkind, b * LPU, 64), bloff = __shfl(lt.coeff_offset, b * LPU, 64);
            uint4 lv = make_uint4(0, 0, 0, 0);
            if (q < UPW * Q4 && bok && bc && blkind != FFHIP_HEVC_RES_ZERO)
                lv = reinterpret_cast<const uint4 *>(S.lcoeffs + bloff)[w];
            if (q < UPW * Q4)
                reinterpret_cast<uint4 *>(blkl)[q] = lv;
        }
    }
    ffhip_wave_sync();
    int16_t *mine = blk + ul * N * N, *lmine = blkl + ul * N * N;
    if (N == 32) { /* one unit per wave: the record is wave-uniform */
        if (__builtin_amdgcn_readfirstlane(ok ? kind : -1) == FFHIP_HEVC_RES_DCT)
            hevc_idct32_mfma_lds(lds, wave, __builtin_amdgcn_readfirstlane((int)t.col_limit), bd, tab, lane);
        if (__builtin_amdgcn_readfirstlane(ok && cross ? lkind : -1) == FFHIP_HEVC_RES_DCT)
            hevc_idct32_mfma_lds(ldsl, wave, __builtin_amdgcn_readfirstlane((int)lt.col_limit), bd, tab, lane);
    }
    hrp_unit<N>(mine, i, act && ok, kind, t.kind_flags, t.col_limit, bd);
    if (any_cross)
        hrp_unit<N>(lmine, i, act && ok && cross, lkind, lt.kind_flags, lt.col_limit, bd);
    /* ---- cross-component (H.265 8.6.6), row i ---- */
    if (act && ok && cross) {
        const int sc = t.res_scale_val;
#pragma unroll
        for (int k = 0; k < N; k++)
            mine[i * N + k] = (int16_t)(mine[i * N + k] + ((sc * (int)lmine[i * N + k]) >> 3));
    }
    ffhip_wave_sync();
    /* ---- the residuals of the well-formed units ---- */
    for (int it = 0; it < ITER; it++) {
        const int q = lane + 64 * it, b = min(q / Q4, UPW - 1), w = q % Q4;
        const int bok = __shfl(ok ? 1 : 0, b * LPU, 64), boff = __shfl(t.res_offset, b * LPU, 64);
        if (q < UPW * Q4 && bok)
            reinterpret_cast<uint4 *>(S.res + boff)[w] = reinterpret_cast<const uint4 *>(blk)[q];
    }
}

__global__ __launch_bounds__(256) void k_hevc_res_pic(const HrpSeg *segs, int nsegs, int bd, const HevcMfmaTab *tab)
{
    __shared__ __align__(16) int16_t lds[4][1024], ldsl[4][1024];
    /* my segment: the last one that starts at or before my workgroup (wave-uniform binary search) */
    const int bx = blockIdx.x;
    int lo = 0, hi = nsegs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (segs[mid].blk0 <= bx)
            lo = mid;
        else
            hi = mid - 1;
    }
    const HrpSeg &S = segs[lo];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int log2 = S.log2, wl = (bx - S.blk0) * 4 + wave; /* my wave within the segment */
    switch (log2) {
    case 2: hrp_wave<2>(S, wl * 16, lds, ldsl, wave, lane, bd, tab); break;
    case 3: hrp_wave<3>(S, wl * 8, lds, ldsl, wave, lane, bd, tab); break;
    case 4: hrp_wave<4>(S, wl * 4, lds, ldsl, wave, lane, bd, tab); break;
    default: hrp_wave<5>(S, wl, lds, ldsl, wave, lane, bd, tab); break;
    }
}
} // namespace

int ffhip_launch_hevc_residual_pictures(int bd, int cfi, int npics, const FFHipHevcResPic *pics, hipStream_t stream)
{
    {
        int r = hevc_pk_upload(HIP_SYMBOL(hevc_res_pk), "ffhip_hevc_residual_pictures_dev");
        if (r >= 0)
            r = hm_tab_init("ffhip_hevc_residual_pictures_dev");
        if (r < 0)
            return r;
    }
    const HevcMfmaTab *tab = g_hm_tab_dev[ffhip_current_device()];
    const int nplanes = cfi ? 3 : 1;
    HrpSeg segs[HRP_MAX_SEGS];
    for (int p0 = 0; p0 < npics; p0 += HRP_PICS) {
        const int n = npics - p0 < HRP_PICS ? npics - p0 : HRP_PICS;
        int nsegs = 0;
        long long blocks = 0;
        for (int k = 0; k < n; k++) {
            const FFHipHevcResPic &P = pics[p0 + k];
            const FFHipHevcResPlane &Y = P.plane[0];
            for (int p = 0; p < nplanes; p++) {
                const FFHipHevcResPlane &D = P.plane[p];
                for (int s = 0; s < 4; s++) {
                    const int cnt = D.size_start[s + 1] - D.size_start[s];
                    if (cnt <= 0)
                        continue;
                    const int upb = 4 * (s == 3 ? 1 : 64 >> (s + 2)); /* units per workgroup */
                    HrpSeg &S = segs[nsegs++];
                    S = HrpSeg{};
                    S.coeffs = D.coeffs; S.res = D.res; S.tus = D.tus;
                    S.lcoeffs = Y.coeffs; S.ltus = Y.tus; S.lncoeffs = Y.ncoeffs; S.lnres = Y.nres;
                    S.ncoeffs = D.ncoeffs; S.nres = D.nres;
                    S.tu0 = D.size_start[s]; S.ntus = cnt;
                    S.l_lo = Y.size_start[s]; S.l_hi = Y.size_start[s + 1];
                    S.blk0 = (int32_t)blocks;
                    S.log2 = s + 2;
                    S.cross_ok = cfi == 3 && p > 0;
                    blocks += cdiv(cnt, upb);
                }
            }
        }
        if (!nsegs)
            continue;
        if (blocks > 0x7FFFFFFF) {
            ffhip_set_error("ffhip_hevc_residual_pictures_dev: %lld workgroups in one launch", blocks);
            return FFHIP_EINVAL;
        }
        const int r = ffhip_progress_launch_table(stream, "ffhip_hevc_residual_pictures_dev: copy or launch", segs, nsegs, [&](HrpSeg *dsegs) {
            hipLaunchKernelGGL(k_hevc_res_pic, dim3((unsigned)blocks), dim3(256), 0, stream, dsegs, nsegs, bd, tab);
        });
        if (r < 0)
            return r;
    }
    return 0;
}
