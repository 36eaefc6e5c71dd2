/*
 * h264_hbd.hip — the H.264 DSP tables above 8 bits (9 / 10 / 12 / 14: every depth the reference instantiates, libavcodec/h264dsp.c:
 * 135-147, h264qpel.c:87-103, h264chroma.c:38-52) and the members the 8-bit kernels do not cover at any depth: the MBAFF loop
 * filters, the 4:2:2 chroma forms (h_loop_filter_chroma422*, idct_add8_422, chroma422_dc_dequant_idct).
 *
 * Bit-exact restatement of the reference's templates with the depth as a kernel argument (libavcodec/bit_depth_template.c: pixel =
 * uint16_t, dctcoef = int32_t above 8 bits; strides and offsets stay in BYTES; av_clip_pixel clips to (1 << depth) - 1):
 *   h264idct_template.c:33-175, h264addpx_template.c:30-74           idct_add / idct8_add / *_dc_add / add_pixels{4,8}_clear
 *   h264idct_template.c:264-352                                      luma / chroma / chroma422 dc_dequant_idct
 *   h264dsp_template.c:104-330                                       the loop-filter family (one generic line filter)
 *   h264qpel_template.c:77-465                                       put / avg x 16 / 8 / 4 x 16 quarter-pel positions
 *   h264chroma_template.c:28-190, h264dsp_template.c:30-98           chroma MC, explicit weighted prediction
 * Templates on the sample type, so the 8-bit instantiation serves the MBAFF / 4:2:2 members of 8-bit streams.
 *
 * Shape: block lists as in the 8-bit faces.  IDCT: one lane per block, both passes in registers, 16-byte coefficient loads
 * (a 4x4 block of int32 is four of them) and 8-byte picture rows.  Loop filter: 16 lanes per edge, a lane per sample line.
 * Motion compensation / weighting: a lane per output sample row segment of 4, taps from global memory (the reference rows of a
 * block are re-read by its lanes through L1/L2; the 8-bit kernels' LDS staging is not repeated here: the high-depth path is
 * bandwidth-light next to its arithmetic).
 */
#include "common.h"
#include "h264_kernels.h"
#include "h264_lf_line.h"
#include "h264_mc_rules.h"
#include "h264_tx_rules.h"

namespace {

__device__ __forceinline__ int hclip(int v, int maxv) { return min(max(v, 0), maxv); }

/* ---- IDCT ------------------------------------------------------------------------------------------------------------------ */
/* one block: kind FFHIP_H264_IDCT4 .. ADD_PIXELS8_CLEAR; c = its N*N coefficients (cleared as the reference clears them) */
template <typename P, int N>
__device__ __forceinline__ void hbd_block(int kind, P *dst, ptrdiff_t s, typename H264Coef<P>::T *c, int maxv)
{
    typedef typename H264Coef<P>::T CF;
    if (kind == FFHIP_H264_IDCT4_DC || kind == FFHIP_H264_IDCT8_DC) {
        const int dc = h264tx_dc(c[0]);
        c[0] = 0;
#pragma unroll
        for (int y = 0; y < N; y++)
#pragma unroll
            for (int x = 0; x < N; x++)
                dst[y * s + x] = (P)hclip((int)dst[y * s + x] + dc, maxv);
        return;
    }
    int v[N * N]; /* block[], the layout of h264tx_idct4 / h264tx_idct8 */
#pragma unroll
    for (int i = 0; i < N * N; i++)
        v[i] = (int)c[i];
#pragma unroll
    for (int i = 0; i < N * N; i++)
        c[i] = 0;
    if (kind == FFHIP_H264_ADD_PIXELS4_CLEAR || kind == FFHIP_H264_ADD_PIXELS8_CLEAR) {
#pragma unroll
        for (int y = 0; y < N; y++)
#pragma unroll
            for (int x = 0; x < N; x++)
                dst[y * s + x] = (P)((unsigned)dst[y * s + x] + (unsigned)v[y * N + x]); /* the sample type's wrap-around, no clip */
        return;
    }
    if constexpr (N == 4) {
        h264tx_idct4<CF>(v);
#pragma unroll
        for (int i = 0; i < 4; i++)     /* v[4 * i + k] goes DOWN column i of dst */
#pragma unroll
            for (int k = 0; k < 4; k++)
                dst[i + k * s] = (P)hclip((int)dst[i + k * s] + v[4 * i + k], maxv);
    } else {
        h264tx_idct8_first<CF>(v);
#pragma unroll
        for (int i = 0; i < 8; i++) {   /* column i is added as it comes: all 64 results at once cost an occupancy step at 8 bits */
            uint32_t o[8];
            h264tx_idct8_1d<1>(v + 8 * i, o);
#pragma unroll
            for (int k = 0; k < 8; k++)
                dst[i + k * s] = (P)hclip((int)dst[i + k * s] + ((int)o[k] >> 6), maxv);
        }
    }
}

template <typename P>
__global__ __launch_bounds__(64) void k_h264_idct_hbd(int kind, uint8_t *dst_base, ptrdiff_t stride, const int32_t *dst_offset, int16_t *blocks,
                                                     int n, int bd)
{
    typedef typename H264Coef<P>::T CF;
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n)
        return;
    P *dst = reinterpret_cast<P *>(dst_base + dst_offset[i]);
    const ptrdiff_t s = stride / (ptrdiff_t)sizeof(P);
    const int maxv = (1 << bd) - 1;
    const bool is8 = kind == FFHIP_H264_IDCT8 || kind == FFHIP_H264_IDCT8_DC || kind == FFHIP_H264_ADD_PIXELS8_CLEAR;
    CF *c = reinterpret_cast<CF *>(blocks) + (size_t)i * (is8 ? 64 : 16);
    if (is8)
        hbd_block<P, 8>(kind, dst, s, c, maxv);
    else
        hbd_block<P, 4>(kind, dst, s, c, maxv);
}

/* the macroblock dispatchers (h264idct_template.c:177-262) over nmb macroblocks: lane = (macroblock, block).
 * which 0 idct_add16, 1 idct8_add4, 2 idct_add16intra, 3 idct_add8 (4:2:0: blocks 16..19 / 32..35), 4 idct_add8_422 (+ 20..23 / 36..39
 * whose offsets / nnz entries sit four slots later).  For 3 / 4 `dst_base` is Cb and `dst2` Cr. */
__constant__ uint8_t hbd_scan8[48] = {
    4 + 1 * 8, 5 + 1 * 8, 4 + 2 * 8, 5 + 2 * 8, 6 + 1 * 8, 7 + 1 * 8, 6 + 2 * 8, 7 + 2 * 8,
    4 + 3 * 8, 5 + 3 * 8, 4 + 4 * 8, 5 + 4 * 8, 6 + 3 * 8, 7 + 3 * 8, 6 + 4 * 8, 7 + 4 * 8,
    4 + 6 * 8, 5 + 6 * 8, 4 + 7 * 8, 5 + 7 * 8, 6 + 6 * 8, 7 + 6 * 8, 6 + 7 * 8, 7 + 7 * 8,
    4 + 8 * 8, 5 + 8 * 8, 4 + 9 * 8, 5 + 9 * 8, 6 + 8 * 8, 7 + 8 * 8, 6 + 9 * 8, 7 + 9 * 8,
    4 + 11 * 8, 5 + 11 * 8, 4 + 12 * 8, 5 + 12 * 8, 6 + 11 * 8, 7 + 11 * 8, 6 + 12 * 8, 7 + 12 * 8,
    4 + 13 * 8, 5 + 13 * 8, 4 + 14 * 8, 5 + 14 * 8, 6 + 13 * 8, 7 + 13 * 8, 6 + 14 * 8, 7 + 14 * 8,
};

template <typename P>
__global__ __launch_bounds__(64) void k_h264_idct_mb_hbd(int which, uint8_t *dst_base, uint8_t *dst2, ptrdiff_t stride, const int32_t *mb_offset,
                                                        const int32_t *blockoffset, int16_t *blocks, const uint8_t *nnzc, int nmb, int bd)
{
    typedef typename H264Coef<P>::T CF;
    const int per = which == 1 ? 4 : which == 3 ? 8 : 16; /* lanes per macroblock */
    const int t = blockIdx.x * 64 + threadIdx.x, m = t / per, k = t % per;
    if (m >= nmb)
        return;
    const int ncoef = which >= 3 ? 768 : 256, nnz_rows = which >= 3 ? 120 : 40;
    const uint8_t *nn = nnzc + (size_t)m * nnz_rows;
    CF *mbc = reinterpret_cast<CF *>(blocks) + (size_t)m * ncoef;
    const ptrdiff_t s = stride / (ptrdiff_t)sizeof(P);
    const int maxv = (1 << bd) - 1;
    uint8_t *base = dst_base;
    int blk, slot; /* coefficient block index, index into blockoffset / scan8 */
    if (which == 1) { blk = slot = 4 * k; }
    else if (which < 3) { blk = slot = k; }
    else {
        const int j = which == 3 ? k >> 2 : k >> 3, r = which == 3 ? k & 3 : k & 7; /* plane, block of the plane */
        base = j ? dst2 : dst_base;
        blk = 16 * (j + 1) + r;
        slot = blk + (r >= 4 ? 4 : 0);
    }
    const int nnz = nn[hbd_scan8[slot]];
    CF *c = mbc + blk * 16;
    P *dst = reinterpret_cast<P *>(base + mb_offset[m] + blockoffset[slot]);
    if (which == 1) {
        if (nnz) {
            if (nnz == 1 && c[0]) hbd_block<P, 8>(FFHIP_H264_IDCT8_DC, dst, s, c, maxv);
            else hbd_block<P, 8>(FFHIP_H264_IDCT8, dst, s, c, maxv);
        }
    } else if (which == 0) {
        if (nnz) {
            if (nnz == 1 && c[0]) hbd_block<P, 4>(FFHIP_H264_IDCT4_DC, dst, s, c, maxv);
            else hbd_block<P, 4>(FFHIP_H264_IDCT4, dst, s, c, maxv);
        }
    } else {
        if (nnz) hbd_block<P, 4>(FFHIP_H264_IDCT4, dst, s, c, maxv);
        else if (c[0]) hbd_block<P, 4>(FFHIP_H264_IDCT4_DC, dst, s, c, maxv);
    }
}

/* DC transforms: which 0 luma (16 values of input + m*in_pitch -> the DC positions of output + m*out_pitch), 1 chroma 4:2:0,
 * 2 chroma 4:2:2 (in place on blocks + block_offset[m]).  Pitches / offsets in coefficients. */
template <typename CF>
__global__ __launch_bounds__(64) void k_h264_dc_dequant_hbd(int which, CF *output, size_t out_pitch, const CF *input, size_t in_pitch,
                                                           const int32_t *block_offset, const int32_t *qmul, int n)
{
    const int m = blockIdx.x * 64 + threadIdx.x;
    if (m >= n)
        return;
    if (which == 0) {
        const CF *in = input + (size_t)m * in_pitch;
        CF *out = output + (size_t)m * out_pitch;
        int dc[16];
#pragma unroll
        for (int i = 0; i < 16; i++)
            dc[i] = (int)in[i];
        h264tx_luma_dc<CF>(dc, qmul[m]);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int o = i == 0 ? 0 : i == 1 ? 32 : i == 2 ? 128 : 160;
            out[o] = (CF)dc[4 * i];
            out[16 + o] = (CF)dc[4 * i + 1];
            out[64 + o] = (CF)dc[4 * i + 2];
            out[80 + o] = (CF)dc[4 * i + 3];
        }
        return;
    }
    CF *b = output + block_offset[m];
    if (which == 1) {
        int dc[4] = { (int)b[0], (int)b[16], (int)b[32], (int)b[48] };
        h264tx_chroma_dc<CF>(dc, qmul[m]);
#pragma unroll
        for (int j = 0; j < 4; j++)
            b[16 * j] = (CF)dc[j];
        return;
    }
    int dc[8];
#pragma unroll
    for (int j = 0; j < 8; j++)
        dc[j] = (int)b[16 * j];
    h264tx_chroma422_dc<CF>(dc, qmul[m]);
#pragma unroll
    for (int j = 0; j < 8; j++)
        b[16 * j] = (CF)dc[j];
}

/* ---- loop filter: 16 lanes per edge, lane = sample line.  FFHipH264Edge.pad = lines per tc0 entry (0: luma 4, chroma 2) ------------ */
template <typename P>
__global__ __launch_bounds__(256) void k_h264_loop_filter_hbd(uint8_t *base, ptrdiff_t stride, const FFHipH264Edge *edges, int n, int bd,
                                                             const int32_t *ab)
{
    const int e = (blockIdx.x * 256 + threadIdx.x) >> 4, d = threadIdx.x & 15;
    if (e >= n)
        return;
    const FFHipH264Edge ed = edges[e];
    const int kind = ed.kind & 7;
    const bool chroma = kind & 2, intra = kind & 4, vert_edge = kind & 1;
    const int inner = ed.pad ? ed.pad : chroma ? 2 : 4;
    if (d >= 4 * inner)
        return;
    const ptrdiff_t s = stride / (ptrdiff_t)sizeof(P);
    const ptrdiff_t xs = vert_edge ? 1 : s, ys = vert_edge ? s : 1;
    P *pix = reinterpret_cast<P *>(base + ed.offset) + d * ys;
    const int maxv = (1 << bd) - 1, sh = bd - 8;
    /* the record holds alpha / beta as the decoder's tables do (bytes); the host faces pass the caller's ints through `ab`, whatever
     * they are (checkasm hands the functions values far outside the tables' range) */
    const int cls = (chroma ? 1 : 0) + (intra ? 2 : 0);
    const LfDepth D = lf_depth(cls, ab ? ab[2 * e] : (int)ed.alpha, ab ? ab[2 * e + 1] : (int)ed.beta, intra ? 0 : ed.tc0[d / inner], sh);
    lf_apply<P, true>(pix, xs, cls, D.alpha, D.beta, D.tc0, maxv);
}

/* ---- luma qpel: a lane per output sample (16 lanes per row of a 16-wide block); the arithmetic is h264_mc_rules.h's -------------- */
/* The reference samples around one output sample: at(dx, dy).  A record flagged FFHIP_MC_EMU (include/ffhip.h; h264_mb.c:229-247,
 * 297-317 -> videodsp_template.c:24-100) reads them at clamped coordinates of the reference picture whose (0, 0) is `p`. */
template <typename P>
struct HbdSrc {
    const P *p;      /* plain: the sample under the output sample; emu: the picture's (0, 0) */
    ptrdiff_t s;     /* row pitch in samples */
    int x, y, pw, ph;
    bool emu;
    __device__ __forceinline__ int at(int dx, int dy) const
    {
        if (emu)
            return (int)p[(ptrdiff_t)min(max(y + dy, 0), ph - 1) * s + min(max(x + dx, 0), pw - 1)];
        return (int)p[dy * s + dx];
    }
};

template <typename P>
__global__ __launch_bounds__(256) void k_h264_qpel_hbd(uint8_t *dst_base, const uint8_t *src_base, ptrdiff_t stride, const FFHipQpelBlock *blocks, int n,
                                                      int bd, int pic_w, int pic_h)
{
    const int b = blockIdx.x, t = threadIdx.x; /* one workgroup per block, 256 lanes = 16 x 16 samples */
    if (b >= n)
        return;
    const FFHipQpelBlock bl = blocks[b];
    const int sz = 16 >> bl.size_idx, x = t & 15, y = t >> 4;
    if (x >= sz || y >= sz)
        return;
    const ptrdiff_t s = stride / (ptrdiff_t)sizeof(P);
    HbdSrc<P> S;
    S.s = s; S.pw = pic_w; S.ph = pic_h;
    S.emu = pic_w > 0 && (bl.flags & FFHIP_MC_EMU);
    S.x = bl.src_x + x; S.y = bl.src_y + y;
    S.p = reinterpret_cast<const P *>(src_base + bl.src_offset) + (S.emu ? 0 : y * s + x);
    P *dst = reinterpret_cast<P *>(dst_base + bl.dst_offset) + y * s + x;
    const int mc = bl.mcxy & 15;
    int v;
    H264MC_LUMA(v, S, mc & 3, mc >> 2, (1 << bd) - 1);
    dst[0] = (P)(bl.avg ? h264mc_avg((int)dst[0], v) : v);
}

/* ---- chroma MC and explicit weighting: a lane per output sample ---------------------------------------------------------------- */
template <typename P>
__global__ __launch_bounds__(128) void k_h264_chroma_mc_hbd(uint8_t *dst_base, const uint8_t *src_base, ptrdiff_t stride, const FFHipChromaBlock *blocks,
                                                           int n, int pic_w, int pic_h)
{
    const int b = blockIdx.x, t = threadIdx.x; /* up to 8 wide x 16 rows */
    if (b >= n)
        return;
    const FFHipChromaBlock bl = blocks[b];
    const int w = 8 >> bl.w_idx, x = t & 7, y = t >> 3;
    if (x >= w || y >= bl.h)
        return;
    const ptrdiff_t s = stride / (ptrdiff_t)sizeof(P);
    HbdSrc<P> S;
    S.s = s; S.pw = pic_w; S.ph = pic_h;
    S.emu = pic_w > 0 && (bl.flags & FFHIP_MC_EMU);
    S.x = bl.src_x + x; S.y = bl.src_y + y;
    S.p = reinterpret_cast<const P *>(src_base + bl.src_offset) + (S.emu ? 0 : y * s + x);
    P *dst = reinterpret_cast<P *>(dst_base + bl.dst_offset) + y * s + x;
    const int v = h264mc_chroma(S, bl.x, bl.y);
    dst[0] = (P)(bl.avg ? h264mc_avg((int)dst[0], v) : v);
}

template <typename P>
__global__ __launch_bounds__(256) void k_h264_weight_hbd(uint8_t *dst_base, const uint8_t *src_base, ptrdiff_t stride, const FFHipWeightBlock *blocks, int n,
                                                        int bd)
{
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= n)
        return;
    const FFHipWeightBlock bl = blocks[b];
    const int w = 16 >> bl.w_idx, x = t & 15, y = t >> 4;
    if (x >= w || y >= bl.height)
        return;
    const ptrdiff_t s = stride / (ptrdiff_t)sizeof(P);
    P *dst = reinterpret_cast<P *>(dst_base + bl.dst_offset) + y * s + x;
    if (!bl.bi) {
        dst[0] = (P)h264mc_weight((int)dst[0], bd, bl.log2_denom, bl.weightd, bl.offset);
    } else {
        const P *src = reinterpret_cast<const P *>(src_base + bl.src_offset) + y * s + x;
        dst[0] = (P)h264mc_biweight((int)dst[0], (int)src[0], bd, bl.log2_denom, bl.weightd, bl.weights, bl.offset);
    }
}

bool hbd_depth_ok(int bd) { return bd == 8 || bd == 9 || bd == 10 || bd == 12 || bd == 14; }

} // namespace

#define HBD_CHECK(bd)                                                                                            \
    do {                                                                                                         \
        if (!hbd_depth_ok(bd)) {                                                                                 \
            ffhip_set_error("ffhip_h264: bit depth %d (8, 9, 10, 12 and 14 are the depths H.264 defines)", bd);  \
            return FFHIP_EINVAL;                                                                                 \
        }                                                                                                        \
        if (bd > 8 && (stride & 1)) {                                                                            \
            ffhip_set_error("ffhip_h264: odd byte stride %td with 16-bit samples", (ptrdiff_t)stride);           \
            return FFHIP_EINVAL;                                                                                 \
        }                                                                                                        \
    } while (0)

int ffhip_launch_h264_idct_add_bd(int bd, int kind, uint8_t *dst_base, ptrdiff_t stride, const int32_t *dst_offset, int16_t *blocks, int n,
                                  hipStream_t stream)
{
    if (n <= 0)
        return 0;
    HBD_CHECK(bd);
    if (kind < FFHIP_H264_IDCT4 || kind > FFHIP_H264_ADD_PIXELS8_CLEAR)
        return FFHIP_EINVAL;
    if (bd > 8)
        hipLaunchKernelGGL(k_h264_idct_hbd<uint16_t>, dim3(cdiv(n, 64)), dim3(64), 0, stream, kind, dst_base, stride, dst_offset, blocks, n, bd);
    else
        hipLaunchKernelGGL(k_h264_idct_hbd<uint8_t>, dim3(cdiv(n, 64)), dim3(64), 0, stream, kind, dst_base, stride, dst_offset, blocks, n, bd);
    LAUNCH_CHECK();
    return 0;
}

int ffhip_launch_h264_idct_mb_bd(int bd, int which, uint8_t *dst_base, uint8_t *dst2, ptrdiff_t stride, const int32_t *mb_offset,
                                 const int32_t *blockoffset, int16_t *blocks, const uint8_t *nnzc, int nmb, hipStream_t stream)
{
    if (nmb <= 0)
        return 0;
    HBD_CHECK(bd);
    if (which < 0 || which > 4)
        return FFHIP_EINVAL;
    const int per = which == 1 ? 4 : which == 3 ? 8 : 16;
    const dim3 g(cdiv(nmb * per, 64)), t(64);
    if (bd > 8)
        hipLaunchKernelGGL(k_h264_idct_mb_hbd<uint16_t>, g, t, 0, stream, which, dst_base, dst2, stride, mb_offset, blockoffset, blocks, nnzc, nmb, bd);
    else
        hipLaunchKernelGGL(k_h264_idct_mb_hbd<uint8_t>, g, t, 0, stream, which, dst_base, dst2, stride, mb_offset, blockoffset, blocks, nnzc, nmb, bd);
    LAUNCH_CHECK();
    return 0;
}

int ffhip_launch_h264_dc_dequant_bd(int bd, int which, int16_t *output, size_t out_pitch, const int16_t *input, size_t in_pitch,
                                    const int32_t *block_offset, const int32_t *qmul, int n, hipStream_t stream)
{
    if (n <= 0)
        return 0;
    const ptrdiff_t stride = 0;
    HBD_CHECK(bd);
    if (which < 0 || which > 2)
        return FFHIP_EINVAL;
    if (bd > 8)
        hipLaunchKernelGGL(k_h264_dc_dequant_hbd<int32_t>, dim3(cdiv(n, 64)), dim3(64), 0, stream, which, reinterpret_cast<int32_t *>(output), out_pitch,
                           reinterpret_cast<const int32_t *>(input), in_pitch, block_offset, qmul, n);
    else
        hipLaunchKernelGGL(k_h264_dc_dequant_hbd<int16_t>, dim3(cdiv(n, 64)), dim3(64), 0, stream, which, output, out_pitch, input, in_pitch,
                           block_offset, qmul, n);
    LAUNCH_CHECK();
    return 0;
}

int ffhip_launch_h264_loop_filter_bd(int bd, uint8_t *base, ptrdiff_t stride, const FFHipH264Edge *edges, int n, hipStream_t stream,
                                     const int32_t *alpha_beta)
{
    if (n <= 0)
        return 0;
    HBD_CHECK(bd);
    if (bd > 8)
        hipLaunchKernelGGL(k_h264_loop_filter_hbd<uint16_t>, dim3(cdiv(n, 16)), dim3(256), 0, stream, base, stride, edges, n, bd, alpha_beta);
    else
        hipLaunchKernelGGL(k_h264_loop_filter_hbd<uint8_t>, dim3(cdiv(n, 16)), dim3(256), 0, stream, base, stride, edges, n, bd, alpha_beta);
    LAUNCH_CHECK();
    return 0;
}

int ffhip_launch_h264_qpel_bd(int bd, uint8_t *dst, const uint8_t *src, ptrdiff_t stride, const FFHipQpelBlock *blocks, int n, hipStream_t stream,
                              int pic_w, int pic_h)
{
    if (n <= 0)
        return 0;
    HBD_CHECK(bd);
    if (bd > 8)
        hipLaunchKernelGGL(k_h264_qpel_hbd<uint16_t>, dim3(n), dim3(256), 0, stream, dst, src, stride, blocks, n, bd, pic_w, pic_h);
    else
        hipLaunchKernelGGL(k_h264_qpel_hbd<uint8_t>, dim3(n), dim3(256), 0, stream, dst, src, stride, blocks, n, bd, pic_w, pic_h);
    LAUNCH_CHECK();
    return 0;
}

int ffhip_launch_h264_chroma_mc_bd(int bd, uint8_t *dst, const uint8_t *src, ptrdiff_t stride, const FFHipChromaBlock *blocks, int n,
                                   hipStream_t stream, int pic_w, int pic_h)
{
    if (n <= 0)
        return 0;
    HBD_CHECK(bd);
    if (bd > 8)
        hipLaunchKernelGGL(k_h264_chroma_mc_hbd<uint16_t>, dim3(n), dim3(128), 0, stream, dst, src, stride, blocks, n, pic_w, pic_h);
    else
        hipLaunchKernelGGL(k_h264_chroma_mc_hbd<uint8_t>, dim3(n), dim3(128), 0, stream, dst, src, stride, blocks, n, pic_w, pic_h);
    LAUNCH_CHECK();
    return 0;
}

int ffhip_launch_h264_weight_bd(int bd, uint8_t *dst, const uint8_t *src, ptrdiff_t stride, const FFHipWeightBlock *blocks, int n,
                                hipStream_t stream)
{
    if (n <= 0)
        return 0;
    HBD_CHECK(bd);
    if (bd > 8)
        hipLaunchKernelGGL(k_h264_weight_hbd<uint16_t>, dim3(n), dim3(256), 0, stream, dst, src, stride, blocks, n, bd);
    else
        hipLaunchKernelGGL(k_h264_weight_hbd<uint8_t>, dim3(n), dim3(256), 0, stream, dst, src, stride, blocks, n, bd);
    LAUNCH_CHECK();
    return 0;
}
