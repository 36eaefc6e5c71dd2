/*
 * hevc_lf_pic.hip — HEVC in-loop filtering of whole pictures in one launch (ffhip_hevc_loop_filter_pictures_dev), 8 / 10 / 12 bits:
 * deblocking (H.265 8.7.2) and SAO (8.7.3) from the reconstructed planes (src) into the DPB planes (dst).
 *
 * Out of place, the geometry makes one workgroup per (picture, CTB) exact with no hand-offs.  A deblocking edge changes at most 3
 * samples on each side and reads at most 4, and edges lie 8 apart, so per plane the workgroup
 *   1. loads its CTB plus a 4-sample halo on every side (clipped to the picture) from src into an LDS tile of uint16 samples;
 *   2. filters every vertical edge of the tile's columns x0 .. x_end on every tile row, halo rows included; after a barrier, every
 *      horizontal edge of rows y0 .. y_end on every tile column, halo columns included.  The CTB and its 1-sample ring are then
 *      deblocked exactly as the whole picture would be: edges on the CTB's border are filtered by both neighbouring workgroups with
 *      the same inputs.  Each segment takes its bS, QPs and bypass flags from the maps and its offsets from the CTB holding q0,0;
 *   3. after a barrier, applies SAO to its CTB from the tile (the edge filter's neighbours are deblocked samples of the tile), the
 *      sao_edge_restore rules and the bypass copy-back per sample, and stores the CTB a quad of samples per item.
 * Nothing but the CTB's own samples is stored, so every dst sample inside the picture is written once and the padding never is.
 *
 * Per-line and per-sample rules are hevc_lf_rules.h's, shared with the batch faces.  A lane takes one 4-line segment of an edge:
 * its decisions read its own lines 0 and 3.  Tile rows are 72 samples (144 bytes, a multiple of 16): a vertical edge's line p3..q3
 * is one 16-byte LDS read, a horizontal edge's 4 columns one 8-byte read per row.
 */
#include <stddef.h>

#include "common.h"
#include "h264_kernels.h"
#include "hevc_lf_rules.h"

static_assert(sizeof(FFHipHevcLfCtb) == 44, "FFHipHevcLfCtb is a 44-byte record");
static_assert(sizeof(FFHipHevcLfPic) % 8 == 0, "FFHipHevcLfPic is staged as an array");

#define HLP_PICS 16 /* pictures per launch: their FFHipHevcLfPic structs travel in one progress-pool slot */
static_assert(HLP_PICS * sizeof(FFHipHevcLfPic) <= FFHIP_PROGRESS_SLOT_INTS * sizeof(int), "a launch's pictures fit one slot");

namespace {
/* H.265 Table 8-12 (beta', tC') and Table 8-10 (QpC for qPi 30..43, chroma format 1): filter.c's betatable / tctable / qp_c */
__constant__ uint8_t hlp_beta[52] = { 0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  6,  7,  8,  9,  10, 11, 12, 13, 14, 15,
                                      16, 17, 18, 20, 22, 24, 26, 28, 30, 32, 34, 36, 38, 40, 42, 44, 46, 48, 50, 52, 54, 56, 58, 60, 62, 64 };
__constant__ uint8_t hlp_tc[54] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1,  1,  1,  1,  1,  1,  1,  1,  1,
                                    2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 5, 5, 6, 6, 7, 8, 9, 10, 11, 13, 14, 16, 18, 20, 22, 24 };
__constant__ uint8_t hlp_qpc[14] = { 29, 30, 31, 32, 33, 33, 34, 34, 35, 35, 36, 36, 37, 37 };

constexpr int HALO = 4;
constexpr int PITCH = 64 + 2 * HALO; /* tile row, samples */
constexpr int ROWS = 64 + 2 * HALO;

/* what a workgroup knows of its picture and plane */
struct Geo {
    const FFHipHevcLfPic *P;
    int lctb, lmc, ctb_w, sx, sy, pw, ph, maxv, bd, cfi, plane;
    int tx0, ty0; /* the tile's origin in plane samples: x0 - HALO, y0 - HALO */
};

/* bS, tC (scaled), beta (scaled), no_p, no_q of the 4-line segment whose q0,0 is plane sample (X, Y), across the edge direction
 * (vertical: p is X - 1; horizontal: p is Y - 1).  Returns false when the segment is not filtered. */
__device__ __forceinline__ bool hlp_segment(const Geo &g, int X, int Y, bool vertical, int &tc, int &beta, bool &no_p, bool &no_q)
{
    const FFHipHevcLfPic &P = *g.P;
    const int xl = X << g.sx, yl = Y << g.sy, xp = vertical ? xl - 1 : xl, yp = vertical ? yl : yl - 1;
    const int bs = (vertical ? P.bs_ver : P.bs_hor)[(ptrdiff_t)(yl >> 2) * P.bs_stride + (xl >> 2)];
    if (g.plane ? bs != 2 : (bs < 1 || bs > 2))
        return false;
    const ptrdiff_t iq = (ptrdiff_t)(yl >> g.lmc) * P.cb_stride + (xl >> g.lmc), ip = (ptrdiff_t)(yp >> g.lmc) * P.cb_stride + (xp >> g.lmc);
    const int qpl = (P.qp_y[ip] + P.qp_y[iq] + 1) >> 1;
    const FFHipHevcLfCtb &R = P.ctbs[(yl >> g.lctb) * g.ctb_w + (xl >> g.lctb)];
    const int tco = R.tc_offset;
    if (g.plane) {
        const int qpi = clip3(qpl + (g.plane == 1 ? P.cb_qp_offset : P.cr_qp_offset), 0, 57);
        const int qpc = g.cfi == 1 ? (qpi < 30 ? qpi : qpi > 43 ? qpi - 6 : hlp_qpc[qpi - 30]) : min(qpi, 51);
        tc = hlp_tc[clip3(qpc + 2 + tco, 0, 53)] << (g.bd - 8);
        beta = 0;
    } else {
        tc = hlp_tc[clip3(qpl + 2 * (bs - 1) + (tco & -2), 0, 53)] << (g.bd - 8);
        beta = hlp_beta[clip3(qpl + R.beta_offset, 0, 51)] << (g.bd - 8);
    }
    no_p = P.bypass && P.bypass[ip];
    no_q = P.bypass && P.bypass[iq];
    return true;
}

/* one 4-line segment of an edge in the tile.  l0: the tile index of line 0's q0; xs: the step across the edge, ys: between lines */
__device__ __forceinline__ void hlp_filter(uint16_t *tile, int l0, int xs, int ys, bool chroma, int tc, int beta, bool no_p, bool no_q,
                                           int maxv)
{
    if (chroma) {
        if (tc <= 0)
            return;
#pragma unroll
        for (int d = 0; d < 4; d++) {
            uint16_t *q = tile + l0 + d * ys;
            int p0 = q[-xs], q0 = q[0];
            hevc_lf_chroma(q[-2 * xs], p0, q0, q[xs], tc, no_p, no_q, maxv);
            q[-xs] = (uint16_t)p0;
            q[0] = (uint16_t)q0;
        }
        return;
    }
    int v[4][8];
    if (xs == 1) { /* vertical edge: a line is 16 contiguous, 16-byte aligned bytes */
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const uint4 w = *reinterpret_cast<const uint4 *>(tile + l0 + d * ys - 4);
            const uint32_t u[4] = { w.x, w.y, w.z, w.w };
#pragma unroll
            for (int k = 0; k < 4; k++) {
                v[d][2 * k] = u[k] & 0xFFFF;
                v[d][2 * k + 1] = u[k] >> 16;
            }
        }
    } else { /* horizontal edge: the 4 lines are 4 contiguous samples (8 aligned bytes) of each row */
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint2 w = *reinterpret_cast<const uint2 *>(tile + l0 + (k - 4) * xs);
            v[0][k] = w.x & 0xFFFF; v[1][k] = w.x >> 16; v[2][k] = w.y & 0xFFFF; v[3][k] = w.y >> 16;
        }
    }
    auto dp = [&](int d) { return hv_abs(v[d][1] - 2 * v[d][2] + v[d][3]); };
    auto dq = [&](int d) { return hv_abs(v[d][6] - 2 * v[d][5] + v[d][4]); };
    auto flat = [&](int d) { return hv_abs(v[d][0] - v[d][3]) + hv_abs(v[d][7] - v[d][4]); };
    auto step = [&](int d) { return hv_abs(v[d][3] - v[d][4]); };
    int nd_p = 1, nd_q = 1;
    const int mode = hevc_lf_decide(dp(0), dq(0), dp(3), dq(3), flat(0), flat(3), step(0), step(3), beta, tc, nd_p, nd_q);
    if (mode == HLF_NONE)
        return;
    unsigned ch = 0;
#pragma unroll
    for (int d = 0; d < 4; d++)
        ch |= mode == HLF_STRONG ? hevc_lf_strong(v[d], tc, no_p, no_q) : hevc_lf_weak(v[d], tc, nd_p, nd_q, no_p, no_q, maxv);
    if (!ch)
        return;
    if (xs == 1) {
#pragma unroll
        for (int d = 0; d < 4; d++) {
            uint32_t u[4];
#pragma unroll
            for (int k = 0; k < 4; k++)
                u[k] = (uint32_t)v[d][2 * k] | (uint32_t)v[d][2 * k + 1] << 16;
            *reinterpret_cast<uint4 *>(tile + l0 + d * ys - 4) = make_uint4(u[0], u[1], u[2], u[3]);
        }
    } else {
#pragma unroll
        for (int k = 1; k < 7; k++)
            if (ch >> k & 1)
                *reinterpret_cast<uint2 *>(tile + l0 + (k - 4) * xs) =
                    make_uint2((uint32_t)v[0][k] | (uint32_t)v[1][k] << 16, (uint32_t)v[2][k] | (uint32_t)v[3][k] << 16);
    }
}

template <typename PIX>
__global__ __launch_bounds__(256) void k_hevc_lf_pic(const FFHipHevcLfPic *pics, int cfi, int width, int height, int lctb, int lmc, int ctb_w,
                                                     int ctb_h, int bd)
{
    constexpr int PS = (int)sizeof(PIX);
    __shared__ __attribute__((aligned(16))) uint16_t tile[ROWS * PITCH];
    const int tid = threadIdx.x, a = blockIdx.x, cy = a / ctb_w, cx = a - cy * ctb_w;
    const FFHipHevcLfPic &P = pics[blockIdx.y];
    const FFHipHevcLfCtb &R = P.ctbs[a];
    const unsigned borders = (cx == 0 ? 1u : 0u) | (cy == 0 ? 2u : 0u) | (cx == ctb_w - 1 ? 4u : 0u) | (cy == ctb_h - 1 ? 8u : 0u);
    const int nplanes = cfi ? 3 : 1;
    for (int p = 0; p < nplanes; p++) {
        Geo g;
        g.P = &P;
        g.lctb = lctb; g.lmc = lmc; g.ctb_w = ctb_w; g.bd = bd; g.cfi = cfi; g.plane = p;
        g.sx = p && cfi != 3 ? 1 : 0;
        g.sy = p && cfi == 1 ? 1 : 0;
        g.pw = width >> g.sx;
        g.ph = height >> g.sy;
        g.maxv = (1 << bd) - 1;
        const int cw = (1 << lctb) >> g.sx, ch = (1 << lctb) >> g.sy;
        const int x0 = cx * cw, y0 = cy * ch;
        const int w = min(cw, g.pw - x0), h = min(ch, g.ph - y0); /* the CTB clipped to the picture (multiples of 4) */
        g.tx0 = x0 - HALO;
        g.ty0 = y0 - HALO;
        const FFHipHevcLfPlane &D = P.plane[p];

        /* ---- 1. CTB + halo from src, a quad of samples per item ---- */
        const int lx0 = max(g.tx0, 0), lx1 = min(x0 + cw + HALO, g.pw), ly0 = max(g.ty0, 0), ly1 = min(y0 + ch + HALO, g.ph);
        const int nq = (lx1 - lx0) >> 2, nrow = ly1 - ly0;
        for (int i = tid; i < nq * nrow; i += 256) {
            const int r = i / nq, c = lx0 + ((i - r * nq) << 2), Y = ly0 + r;
            const PIX *s = reinterpret_cast<const PIX *>(D.src + (ptrdiff_t)Y * D.src_stride) + c;
            uint2 u;
            if (PS == 1) {
                const uint32_t q = *reinterpret_cast<const uint32_t *>(s);
                u = make_uint2((q & 0xFF) | (q & 0xFF00) << 8, (q >> 16 & 0xFF) | (q >> 8 & 0xFF0000));
            } else {
                u = *reinterpret_cast<const uint2 *>(s);
            }
            *reinterpret_cast<uint2 *>(tile + (Y - g.ty0) * PITCH + (c - g.tx0)) = u;
        }
        __syncthreads();

        /* ---- 2. deblocking: vertical edges x0, x0 + 8, .., x0 + cw on the 4-line groups of every tile row, then horizontal ones ---- */
        const bool chroma = p != 0;
        const int ne_v = (cw >> 3) + 1, ng_v = (ch >> 2) + 2;
        for (int i = tid; i < ne_v * ng_v; i += 256) {
            const int e = i / ng_v, X = x0 + 8 * e, Y = g.ty0 + 4 * (i - e * ng_v);
            int tc, beta;
            bool no_p, no_q;
            if (X <= 0 || X >= g.pw || Y < 0 || Y >= g.ph || !hlp_segment(g, X, Y, true, tc, beta, no_p, no_q))
                continue;
            hlp_filter(tile, (Y - g.ty0) * PITCH + (X - g.tx0), 1, PITCH, chroma, tc, beta, no_p, no_q, g.maxv);
        }
        __syncthreads();
        const int ne_h = (ch >> 3) + 1, ng_h = (cw >> 2) + 2;
        for (int i = tid; i < ne_h * ng_h; i += 256) {
            const int e = i / ng_h, Y = y0 + 8 * e, X = g.tx0 + 4 * (i - e * ng_h);
            int tc, beta;
            bool no_p, no_q;
            if (Y <= 0 || Y >= g.ph || X < 0 || X >= g.pw || !hlp_segment(g, X, Y, false, tc, beta, no_p, no_q))
                continue;
            hlp_filter(tile, (Y - g.ty0) * PITCH + (X - g.tx0), PITCH, 1, chroma, tc, beta, no_p, no_q, g.maxv);
        }
        __syncthreads();

        /* ---- 3. SAO, the restore rules and the bypass copy-back from the tile; the CTB to dst a quad per item ---- */
        const int type = R.sao_type[p], cls = R.sao_class[p];
        const bool band = type == 1 && cls < 32, edge = type == 2 && cls < 4;
        const int o0 = R.sao_offset_val[p][0], o1 = R.sao_offset_val[p][1], o2 = R.sao_offset_val[p][2], o3 = R.sao_offset_val[p][3],
                  o4 = R.sao_offset_val[p][4];
        static const int8_t dxs[4][2] = { { -1, 1 }, { 0, 0 }, { -1, 1 }, { 1, -1 } }, dys[4][2] = { { 0, 0 }, { -1, 1 }, { -1, 1 }, { -1, 1 } };
        const int eo = cls & 3, da = dxs[eo][0] + dys[eo][0] * PITCH, db = dxs[eo][1] + dys[eo][1] * PITCH;
        const int wq = w >> 2;
        for (int i = tid; i < wq * h; i += 256) {
            const int r = i / wq, c = (i - r * wq) << 2, Y = y0 + r;
            const uint16_t *t = tile + (r + HALO) * PITCH + c + HALO;
            int out[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int v = t[j];
                int o = v;
                if (band) {
                    o = min(max(v + hevc_sao_band_off(v, bd - 5, cls, o1, o2, o3, o4), 0), g.maxv);
                } else if (edge) {
                    const int kind = hevc_sao_restore_kind(c + j, r, w, h, eo, borders, R.vert_edge, R.horiz_edge, R.diag_edge, R.restore != 0);
                    if (kind == 1)
                        o = min(max(v + o0, 0), g.maxv);
                    else if (kind == 0) /* every neighbour is inside the picture and the tile here */
                        o = min(max(v + hevc_sao_edge_off(v, t[j + da], t[j + db], o0, o1, o2, o3, o4), 0), g.maxv);
                }
                if ((band || edge) && P.bypass) {
                    const int xl = (x0 + c + j) << g.sx, yl = Y << g.sy;
                    if (P.bypass[(ptrdiff_t)(yl >> lmc) * P.cb_stride + (xl >> lmc)])
                        o = v;
                }
                out[j] = o;
            }
            PIX *d = reinterpret_cast<PIX *>(D.dst + (ptrdiff_t)Y * D.dst_stride) + x0 + c; /* base and stride are 4-sample aligned */
            if (PS == 1)
                *reinterpret_cast<uint32_t *>(d) = (uint32_t)out[0] | (uint32_t)out[1] << 8 | (uint32_t)out[2] << 16 | (uint32_t)out[3] << 24;
            else
                *reinterpret_cast<uint2 *>(d) = make_uint2((uint32_t)out[0] | (uint32_t)out[1] << 16, (uint32_t)out[2] | (uint32_t)out[3] << 16);
        }
        __syncthreads(); /* the next plane reuses the tile */
    }
}
} // namespace

int ffhip_launch_hevc_loop_filter_pictures(int bd, int cfi, int width, int height, int log2_ctb, int log2_min_cb, int npics,
                                           const FFHipHevcLfPic *pics, hipStream_t stream)
{
    const int C = 1 << log2_ctb, ctb_w = (width + C - 1) / C, ctb_h = (height + C - 1) / C;
    for (int p0 = 0; p0 < npics; p0 += HLP_PICS) {
        const int n = npics - p0 < HLP_PICS ? npics - p0 : HLP_PICS;
        const int r = ffhip_progress_launch_table(stream, "ffhip_hevc_loop_filter_pictures_dev: copy or launch", pics + p0, n,
                                                  [&](FFHipHevcLfPic *dpics) {
            if (bd > 8)
                hipLaunchKernelGGL(k_hevc_lf_pic<uint16_t>, dim3(ctb_w * ctb_h, n), dim3(256), 0, stream, dpics, cfi, width, height, log2_ctb,
                                   log2_min_cb, ctb_w, ctb_h, bd);
            else
                hipLaunchKernelGGL(k_hevc_lf_pic<uint8_t>, dim3(ctb_w * ctb_h, n), dim3(256), 0, stream, dpics, cfi, width, height, log2_ctb,
                                   log2_min_cb, ctb_w, ctb_h, 8);
        });
        if (r < 0)
            return r;
    }
    return 0;
}
