/*
 * h264_res_pic.hip — the residual of every inter macroblock of whole H.264 pictures in one launch (ffhip_h264_residual_pictures_dev,
 * ffhip_h264_residual_pictures_fmt_dev):
 * idct_add16 / idct8_add4, chroma_dc_dequant_idct and idct_add8 of all planes from the macroblock array of the inter and the
 * edge-parameter faces plus one FFHipH264ResMb per macroblock, with no list sorted by transform size on the host.
 *
 * 32 lanes per macroblock, 8 macroblocks per workgroup of 4 waves, macroblocks in raster order along blockIdx.x.  Lane r of a
 * macroblock: r < 16 is luma block r of the decoder's order, 16 .. 19 the Cb blocks, 20 .. 23 the Cr blocks, 24 .. 31 idle.  The chroma
 * format is a template parameter FMT.  FMT 2 (4:2:2): 16 luma + 8 Cb + 8 Cr blocks are exactly the 32 lanes (16 .. 23 Cb, 24 .. 31 Cr);
 * the eight DCs of a plane meet among the plane's eight lanes, two quads of one DPP row, by quad_perm and row_half_mirror.  FMT 3
 * (4:4:4): the 16 luma lanes walk the three planes one after the other, each with the plane's own bits, which keeps the registers of
 * the 8x8 quad path where they are; lanes 16 .. 31 stay idle (a macroblock's planes on separate lanes would need a second set of 16
 * coefficients per lane or a third of the macroblocks per workgroup).  Every lane
 * reads the two records of its macroblock (32 lanes on the same words: one request) and resolves them with h264res_plan(); a lane
 * whose block is not coded leaves before it touches a coefficient.  Luma and chroma 4x4 blocks run through one code path, a lane per
 * block from end to end: the coefficients come in 16-byte loads (2 per block at 8 bits, 4 above), both passes run in registers, and
 * the destination rows are read, added to and written as one dword (8 bits) or 8 bytes (above) per 4 samples.  The DC values of a
 * chroma plane meet among the plane's four lanes, which are a quad, by DPP.  With the 8x8 transform the quad of lanes 4k .. 4k + 3
 * shares 8x8 block k: 16 coefficients a lane and a 4 x 4 transpose over the quad before each pass (idct8_add_quad), where one lane per
 * block would hold 64 coefficients (154 VGPRs for the kernel against 42, docs/KERNELS.md 5.5h-6).  Nothing goes through LDS,
 * nothing is shared between waves and there is no barrier.
 */
#include <stddef.h>

#include "common.h"
#include "h264_kernels.h"
#include "h264_res_rules.h"

static_assert(sizeof(FFHipH264BsMb) == 8, "the macroblock record of the edge-parameter face");
static_assert(sizeof(FFHipH264ResMb) == 16, "FFHipH264ResMb is a 16-byte record");
static_assert(sizeof(FFHipH264ResPic) == 80, "FFHipH264ResPic is staged as an array");

#define H4R_PICS 16 /* pictures per launch: their FFHipH264ResPic structs travel in one progress-pool slot */
#define H4R_MBS 8   /* macroblocks per workgroup */
static_assert(H4R_PICS * sizeof(FFHipH264ResPic) <= FFHIP_PROGRESS_SLOT_INTS * sizeof(int), "a launch's pictures fit one slot");

namespace {
/* N coefficients from 16-byte aligned c, as ints */
template <int N>
__device__ __forceinline__ void load_coefs(const int16_t *c, int (&v)[N])
{
#pragma unroll
    for (int k = 0; k < N / 8; k++) {
        const uint4 w = reinterpret_cast<const uint4 *>(c)[k];
        const uint32_t d[4] = { w.x, w.y, w.z, w.w };
#pragma unroll
        for (int i = 0; i < 4; i++) {
            v[8 * k + 2 * i] = (int16_t)(d[i] & 0xFFFF);
            v[8 * k + 2 * i + 1] = (int16_t)(d[i] >> 16);
        }
    }
}
template <int N>
__device__ __forceinline__ void load_coefs(const int32_t *c, int (&v)[N])
{
#pragma unroll
    for (int k = 0; k < N / 4; k++) {
        const uint4 w = reinterpret_cast<const uint4 *>(c)[k];
        v[4 * k] = (int)w.x; v[4 * k + 1] = (int)w.y; v[4 * k + 2] = (int)w.z; v[4 * k + 3] = (int)w.w;
    }
}

/* 4 samples of a row at p (4-sample aligned) += d0 .. d3, clipped */
__device__ __forceinline__ void add_row4(uint8_t *p, uint8_t, int d0, int d1, int d2, int d3, int maxv)
{
    const uint32_t w = *reinterpret_cast<const uint32_t *>(p);
    *reinterpret_cast<uint32_t *>(p) = pack4(h264tx_clip((int)(w & 0xFF) + d0, maxv), h264tx_clip((int)((w >> 8) & 0xFF) + d1, maxv),
                                             h264tx_clip((int)((w >> 16) & 0xFF) + d2, maxv), h264tx_clip((int)(w >> 24) + d3, maxv));
}
__device__ __forceinline__ void add_row4(uint8_t *p, uint16_t, int d0, int d1, int d2, int d3, int maxv)
{
    const uint2 w = *reinterpret_cast<const uint2 *>(p);
    const uint32_t a = (uint32_t)h264tx_clip((int)(w.x & 0xFFFF) + d0, maxv) | (uint32_t)h264tx_clip((int)(w.x >> 16) + d1, maxv) << 16;
    const uint32_t b = (uint32_t)h264tx_clip((int)(w.y & 0xFFFF) + d2, maxv) | (uint32_t)h264tx_clip((int)(w.y >> 16) + d3, maxv) << 16;
    *reinterpret_cast<uint2 *>(p) = make_uint2(a, b);
}

/* the value of lane (lane ^ 1), (lane ^ 2) and of lane N of the quad; every lane of the quad must be active */
__device__ __forceinline__ int quad_xor1(int v) { return __builtin_amdgcn_mov_dpp(v, 0xB1, 0xf, 0xf, true); }   /* quad_perm [1,0,3,2] */
__device__ __forceinline__ int quad_xor2(int v) { return __builtin_amdgcn_mov_dpp(v, 0x4E, 0xf, 0xf, true); }   /* quad_perm [2,3,0,1] */
template <int N>
__device__ __forceinline__ int quad_lane(int v) { return __builtin_amdgcn_mov_dpp(v, N * 0x55, 0xf, 0xf, true); }  /* quad_perm [N,N,N,N] */
/* the value of lane (lane ^ 7) of an aligned group of eight lanes (row_half_mirror); every lane of the group must be active */
__device__ __forceinline__ int oct_mirror(int v) { return __builtin_amdgcn_mov_dpp(v, 0x141, 0xf, 0xf, true); }

/* the 4 x 4 transpose over a quad: w[p] of lane q becomes w[q] of lane p */
__device__ __forceinline__ void quad_transpose(int &w0, int &w1, int &w2, int &w3, int q)
{
    const bool odd = q & 1, high = q & 2;
    int s0 = quad_xor1(odd ? w0 : w1), s1 = quad_xor1(odd ? w2 : w3);
    if (odd) { w0 = s0; w2 = s1; } else { w1 = s0; w3 = s1; }
    s0 = quad_xor2(high ? w0 : w2);
    s1 = quad_xor2(high ? w1 : w3);
    if (high) { w0 = s0; w1 = s1; } else { w2 = s0; w3 = s1; }
}
/* a[8 * j + 2 * p + c] of lane q <-> a[8 * c + 2 * q + j] of lane p (j, c = 0, 1): two rows of eight per lane become two columns of
 * eight per lane, and back */
__device__ __forceinline__ void quad_rows_to_columns(const int (&a)[16], int (&b)[16], int q)
{
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
        for (int c = 0; c < 2; c++) {
            int w0 = a[8 * j + c], w1 = a[8 * j + 2 + c], w2 = a[8 * j + 4 + c], w3 = a[8 * j + 6 + c];
            quad_transpose(w0, w1, w2, w3, q);
            b[8 * c + j] = w0; b[8 * c + 2 + j] = w1; b[8 * c + 4 + j] = w2; b[8 * c + 6 + j] = w3;
        }
}

/* One 8x8 block on the four lanes q = 0 .. 3 of a quad (rule 5): lane q loads rows 2q and 2q + 1 of the stored block (16 coefficients,
 * 16-byte loads), the quad transposes so that it holds columns 2q and 2q + 1 for the first pass, transposes back for the second, and
 * after an exchange with lane q ^ 1 adds rows 4 (q & 1) .. + 3 of columns 4 (q >> 1) .. + 3 as whole 4-sample rows.  c: the block's 64
 * coefficients; dst: its top-left sample. */
template <typename PIX, typename CF>
__device__ __forceinline__ void idct8_add_quad(const CF *c, uint8_t *dst, ptrdiff_t stride, int q, int maxv)
{
    int a[16], b[16], d[16];
    load_coefs(c + 16 * q, a);
    int ac = q ? a[0] : 0;
#pragma unroll
    for (int i = 1; i < 16; i++)
        ac |= a[i];
    ac |= quad_xor1(ac);
    ac |= quad_xor2(ac);
    const int first = quad_lane<0>(a[0]);
    if (!ac) {  /* nothing but the DC (h264tx_flat over the quad): the *_dc_add form; uniform over the quad */
        const int dc = h264tx_dc(first);
#pragma unroll
        for (int i = 0; i < 16; i++)
            d[i] = dc;
    } else {
        if (q == 0)
            a[0] = (CF)((uint32_t)a[0] + 32u);
        quad_rows_to_columns(a, b, q);      /* b[8 c + k] = block[2q + c + 8k] */
#pragma unroll
        for (int n = 0; n < 2; n++) {
            uint32_t o[8];
            h264tx_idct8_1d<1>(b + 8 * n, o);
#pragma unroll
            for (int k = 0; k < 8; k++)
                b[8 * n + k] = (CF)o[k];
        }
        quad_rows_to_columns(b, a, q);      /* a[8 j + k] = block[8 (2q + j) + k] after the first pass */
#pragma unroll
        for (int n = 0; n < 2; n++) {
            uint32_t o[8];
            h264tx_idct8_1d<1>(a + 8 * n, o);
#pragma unroll
            for (int k = 0; k < 8; k++)
                a[8 * n + k] = (int)o[k] >> 6;  /* row k, column 2q + n */
        }
        /* lanes q and q ^ 1 hold columns 4 (q >> 1) .. + 3 between them: the even lane takes rows 0 .. 3, the odd one rows 4 .. 7 */
        const bool odd = q & 1;
#pragma unroll
        for (int n = 0; n < 2; n++)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int got = quad_xor1(odd ? a[8 * n + k] : a[8 * n + 4 + k]), mine = odd ? a[8 * n + 4 + k] : a[8 * n + k];
                d[4 * k + n] = odd ? got : mine;
                d[4 * k + 2 + n] = odd ? mine : got;
            }
    }
    uint8_t *at = dst + (ptrdiff_t)(4 * (q & 1)) * stride + (size_t)(4 * (q >> 1)) * sizeof(PIX);
#pragma unroll
    for (int k = 0; k < 4; k++)
        add_row4(at + k * stride, PIX(), d[4 * k], d[4 * k + 1], d[4 * k + 2], d[4 * k + 3], maxv);
}

template <typename PIX, typename CF, int FMT>
__global__ __launch_bounds__(32 * H4R_MBS) void k_h264_res_pic(const FFHipH264ResPic *pics, int mb_w, int nmb, int bd, int chroma)
{
    const FFHipH264ResPic &P = pics[blockIdx.z];
    const int r = threadIdx.x & 31;
    const int m = (int)blockIdx.x * H4R_MBS + ((int)threadIdx.x >> 5);      /* nmb <= 4096 * 4096 */
    if (m >= nmb || r >= (FMT == 2 ? 32 : FMT == 3 ? 16 : 24))
        return;
    const FFHipH264BsMb mb = P.mb[m];
    if (mb.flags & 1)
        return;
    const FFHipH264ResMb R = P.res[m];
    const H264ResPlan plan = h264res_plan(mb, R, chroma && P.dst[1], P.ncoeffs, FMT);
    if (!plan.need)
        return;
    const int mx = m % mb_w, my = m / mb_w, maxv = (1 << bd) - 1;
    if constexpr (FMT == 3) {   /* rule 15: three luma planes, one after the other on the 16 luma lanes */
        const int np = plan.need == 768 ? 3 : 1, j = r & 3;
#pragma unroll 1
        for (int pl = 0; pl < np; pl++) {
            const CF *c = reinterpret_cast<const CF *>(P.coeffs) + plan.off + 256 * pl + 16 * r;
            const ptrdiff_t s = P.dst_stride[pl];
            uint8_t *dst = P.dst[pl] + (ptrdiff_t)(my * 16 + 4 * h264res_y4(r)) * s + (size_t)(mx * 16 + 4 * h264res_x4(r)) * sizeof(PIX);
            if (plan.t8) {      /* uniform over the quad */
                if (h264res_luma8_on(plan, r >> 2, pl))
                    idct8_add_quad<PIX, CF>(c - 16 * j, dst - (ptrdiff_t)(4 * h264res_y4(j)) * s - (size_t)(4 * h264res_x4(j)) * sizeof(PIX), s, j, maxv);
                continue;
            }
            if (!h264res_luma4_on(plan, r, pl))
                continue;
            int v[16];
            load_coefs(c, v);
            h264res_luma<CF, 16>(v);
#pragma unroll
            for (int k = 0; k < 4; k++)
                add_row4(dst + k * s, PIX(), v[k], v[4 + k], v[8 + k], v[12 + k], maxv);
        }
        return;
    }
    constexpr int NC = FMT == 2 ? 8 : 4;                                    /* 4x4 blocks of a chroma plane */
    const bool luma = r < 16;
    const int pl = luma ? 0 : 1 + ((r - 16) >> (FMT == 2 ? 3 : 2)), j = r & (NC - 1);         /* the plane; a chroma lane's block x + 2 * y */
    /* the lane's 4x4 block: its coefficients, its top-left sample */
    const CF *c = reinterpret_cast<const CF *>(P.coeffs) + plan.off + (luma ? 16 * r : 256 * pl + 16 * j);
    const int bx = luma ? mx * 16 + 4 * h264res_x4(r) : mx * 8 + 4 * (j & 1), by = luma ? my * 16 + 4 * h264res_y4(r) : my * (2 * NC) + 4 * (j >> 1);
    const ptrdiff_t s = pl == 0 ? P.dst_stride[0] : pl == 1 ? P.dst_stride[1] : P.dst_stride[2];
    uint8_t *dst = (pl == 0 ? P.dst[0] : pl == 1 ? P.dst[1] : P.dst[2]) + (ptrdiff_t)by * s + (size_t)bx * sizeof(PIX);
    if (luma && plan.t8) {  /* lanes 4k .. 4k + 3 share 8x8 block k, whose coefficients and top-left sample are lane 4k's */
        const int q = r & 3;
        if (h264res_luma8_on(plan, r >> 2))
            idct8_add_quad<PIX, CF>(c - 16 * q, dst - (ptrdiff_t)(4 * h264res_y4(q)) * s - (size_t)(4 * h264res_x4(q)) * sizeof(PIX), s, q, maxv);
        return;
    }
    /* luma and chroma 4x4 blocks take one path: rules 4, 6 and 7 */
    const bool dc_on = !luma && ((plan.chroma_dc >> (pl - 1)) & 1);
    const bool ac_on = luma ? h264res_luma4_on(plan, r) : h264res_chroma_on(plan, pl - 1, j);
    if (!dc_on && !ac_on)
        return;
    int v[16];
    if (ac_on) {
        load_coefs(c, v);
    } else {    /* rule 8: of a block without its bit only the DC is read, in the 16 bytes that hold it */
        const uint4 w = *reinterpret_cast<const uint4 *>(c);
        v[0] = sizeof(CF) == 2 ? (int)(int16_t)(w.x & 0xFFFF) : (int)w.x;
    }
    if (dc_on) {    /* uniform over the plane's lanes, which are all here */
        const int qm = pl == 1 ? R.qmul[0] : R.qmul[1];
        if constexpr (FMT == 2) {   /* rule 14: the plane's eight lanes, quads 0 (blocks 0 .. 3) and 1 (blocks 4 .. 7) */
            const int o = oct_mirror(v[0]);     /* block 7 - j's */
            const int mine[4] = { quad_lane<0>(v[0]), quad_lane<1>(v[0]), quad_lane<2>(v[0]), quad_lane<3>(v[0]) };
            const int other[4] = { quad_lane<3>(o), quad_lane<2>(o), quad_lane<1>(o), quad_lane<0>(o) };   /* the other quad's, in its order */
            const bool hi = j & 4;
            int dc[8];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                dc[i] = hi ? other[i] : mine[i];
                dc[4 + i] = hi ? mine[i] : other[i];
            }
            h264tx_chroma422_dc<CF>(dc, qm);
            int d = dc[0];
#pragma unroll
            for (int i = 1; i < 8; i++)
                d = j == i ? dc[i] : d;
            v[0] = d;
        } else {
            int dc[4] = { quad_lane<0>(v[0]), quad_lane<1>(v[0]), quad_lane<2>(v[0]), quad_lane<3>(v[0]) };
            h264tx_chroma_dc<CF>(dc, qm);
            v[0] = j == 0 ? dc[0] : j == 1 ? dc[1] : j == 2 ? dc[2] : dc[3];
        }
    }
    if (luma ? h264tx_flat(v) : !ac_on) {  /* rule 9: the *_dc_add form */
        const int d = h264tx_dc(v[0]);
#pragma unroll
        for (int i = 0; i < 16; i++)
            v[i] = d;
    } else {
        h264tx_idct4<CF>(v);
    }
#pragma unroll
    for (int k = 0; k < 4; k++)
        add_row4(dst + k * s, PIX(), v[k], v[4 + k], v[8 + k], v[12 + k], maxv);
}

template <typename PIX, typename CF>
void launch(int fmt, dim3 grid, hipStream_t stream, const FFHipH264ResPic *dpics, int mb_w, int nmb, int bd)
{
    if (fmt == 3)
        hipLaunchKernelGGL((k_h264_res_pic<PIX, CF, 3>), grid, dim3(32 * H4R_MBS), 0, stream, dpics, mb_w, nmb, bd, 1);
    else if (fmt == 2)
        hipLaunchKernelGGL((k_h264_res_pic<PIX, CF, 2>), grid, dim3(32 * H4R_MBS), 0, stream, dpics, mb_w, nmb, bd, 1);
    else
        hipLaunchKernelGGL((k_h264_res_pic<PIX, CF, 1>), grid, dim3(32 * H4R_MBS), 0, stream, dpics, mb_w, nmb, bd, fmt);
}
} // namespace

int ffhip_launch_h264_residual_pictures(int bd, int chroma_format_idc, int mb_w, int mb_h, int npics, const FFHipH264ResPic *pics, hipStream_t stream)
{
    const int nmb = mb_w * mb_h;
    for (int p0 = 0; p0 < npics; p0 += H4R_PICS) {
        const int n = npics - p0 < H4R_PICS ? npics - p0 : H4R_PICS;
        const int r = ffhip_progress_launch_table(stream, "ffhip_h264_residual_pictures_dev: copy or launch", pics + p0, n,
                                                  [&](FFHipH264ResPic *dpics) {
            const dim3 grid((nmb + H4R_MBS - 1) / H4R_MBS, 1, n);   /* at most 2^21 x 1 x 16 */
            if (bd > 8)
                launch<uint16_t, int32_t>(chroma_format_idc, grid, stream, dpics, mb_w, nmb, bd);
            else
                launch<uint8_t, int16_t>(chroma_format_idc, grid, stream, dpics, mb_w, nmb, bd);
        });
        if (r < 0)
            return r;
    }
    return 0;
}
