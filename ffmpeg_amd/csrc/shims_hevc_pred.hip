/*
 * shims_hevc_pred.hip — HEVC intra prediction: the batch face ffhip_hevc_intra_batch_dev() and the host-pointer members of
 * HEVCPredContext (pred_planar[4], pred_dc, pred_angular[4]) that ff_hevc_pred_init_hip() installs.
 *
 * A host face builds the block's reference line from top[-1 .. 2N-1] and left[-1 .. 2N-1] (the layout of FFHipHevcIntra) and stages
 * it with the block in one Stage image (kernels/shim_arena.h) before anything is written, since the caller's top / left may point
 * into src; the kernel runs with n = 1 and a prepared line, and the block travels back.  A call that cannot run on the device is
 * answered by the C function the init displaced, as in shims.hip.
 *
 * ffhip_hevc_intra_pictures_dev(): the host checks (kernels/picture_check.h; no overlap check) and the launch of the intra
 * reconstruction wavefront (kernels/hevc_intra_pic.hip) on the caller's stream.
 */
#include <stdint.h>
#include <string.h>
#include <type_traits>

#include "kernels/common.h"
#include "kernels/h264_kernels.h"
#include "kernels/picture_check.h"
#include "kernels/shim_arena.h"

static bool hpred_bd_ok(int bd) { return bd == 8 || bd == 10 || bd == 12; }

extern "C" int ffhip_hevc_intra_record_size(void) { return (int)sizeof(FFHipHevcIntra); }

extern "C" int ffhip_hevc_intra_batch_dev(int bit_depth, uint8_t *dst, ptrdiff_t stride, const uint8_t *edges, const FFHipHevcIntra *blocks, int n,
                                          void *stream)
{
    if (!hpred_bd_ok(bit_depth)) {
        ffhip_set_error("ffhip_hevc_intra_batch_dev: bit depth %d (8, 10 or 12)", bit_depth);
        return FFHIP_EINVAL;
    }
    if (n < 0 || !dst || !edges || !blocks) {
        ffhip_set_error("ffhip_hevc_intra_batch_dev: n = %d, or a NULL plane / line / record pointer", n);
        return FFHIP_EINVAL;
    }
    if (bit_depth > 8 && (((uintptr_t)dst | (uintptr_t)edges | (size_t)stride) & 1)) {
        ffhip_set_error("ffhip_hevc_intra_batch_dev: 16-bit planes, lines and strides must be 2-byte aligned");
        return FFHIP_EINVAL;
    }
    if (!ffhip_have_device())
        return FFHIP_ENOSYS;
    return ffhip_launch_hevc_intra(bit_depth, dst, stride, edges, blocks, n, (hipStream_t)stream);
}

/* ---- whole pictures: the intra reconstruction wavefront (kernels/hevc_intra_pic.hip) ---------------------- */
extern "C" int ffhip_hevc_intra_tu_record_size(void) { return (int)sizeof(FFHipHevcIntraTU); }

extern "C" int ffhip_hevc_intra_pictures_dev(int bit_depth, int chroma_format_idc, int width, int height, int log2_ctb_size, int npics,
                                             const FFHipHevcIntraPic *pics, void *stream)
{
    static const char who[] = "ffhip_hevc_intra_pictures_dev";
    if (const int r = ffhip_check_hevc_pictures(who, bit_depth, chroma_format_idc, log2_ctb_size, width, height, npics, pics))
        return r;
    const FFHipPlaneGeom G = FFHipPlaneGeom::hevc(bit_depth, chroma_format_idc, width, height);
    const int nplanes = G.nplanes;
    for (int i = 0; i < npics; i++)
        for (int p = 0; p < nplanes; p++) {
            const FFHipHevcIntraPlane &P = pics[i].plane[p];
            if (!P.base || !P.tus || !P.ctb_start || !P.res) {
                ffhip_set_error("%s: picture %d plane %d: a NULL pointer", who, i, p);
                return FFHIP_EINVAL;
            }
            if (!ffhip_plane_ok(P.base, P.stride, G.amask, G.row_bytes(p))) {
                ffhip_set_error("%s: picture %d plane %d: base and stride must be %u-byte aligned, the stride at least the plane's width", who,
                                i, p, G.amask + 1);
                return FFHIP_EINVAL;
            }
        }
    const int ctb_h = (height + (1 << log2_ctb_size) - 1) >> log2_ctb_size;
    if (nplanes * ctb_h > FFHIP_PROGRESS_SLOT_INTS) {
        ffhip_set_error("%s: %d CTB rows exceed the progress pool", who, nplanes * ctb_h);
        return FFHIP_EINVAL;
    }
    if (!ffhip_have_device())
        return FFHIP_ENOSYS;
    return ffhip_launch_hevc_intra_pictures(bit_depth, chroma_format_idc, width, height, log2_ctb_size, npics, pics, (hipStream_t)stream);
}

/* ---- host-pointer faces ---------------------------------------------------------------------------------- */
static constexpr int hpred_bdi(int bd) { return bd == 8 ? 0 : bd == 10 ? 1 : 2; }
static FFHipHEVCPredContext g_fb_hpred[3]; /* the C functions ff_hevc_pred_init_hip() displaced, per depth */

/* corner: the copy of the corner sample the reference reads (top[-1] or left[-1]); the modes that read neither take top[-1] */
template <int BD>
static bool hpred_gpu(uint8_t *src, const uint8_t *top, const uint8_t *left, ptrdiff_t stride, int log2, int mode, int c_idx, bool corner_left)
{
    using PIX = typename std::conditional<BD == 8, uint8_t, uint16_t>::type;
    if (log2 < 2 || log2 > 5 || mode < 0 || mode > 34)
        return false;
    const int N = 1 << log2, PS = (int)sizeof(PIX);
    const PIX *t = reinterpret_cast<const PIX *>(top), *l = reinterpret_cast<const PIX *>(left);
    Stage S;
    const size_t ln = S.hole((size_t)(4 * N + 1) * PS);
    PIX *L = S.img<PIX>(ln);
    for (int i = 0; i < 2 * N; i++) {
        L[i] = l[2 * N - 1 - i];
        L[2 * N + 1 + i] = t[i];
    }
    L[2 * N] = corner_left ? l[-1] : t[-1];
    const size_t pix = S.put2d(src, stride, (size_t)N * PS, N, DP), hdr = S.hole(sizeof(FFHipHevcIntra));
    FFHipHevcIntra &k = *S.img<FFHipHevcIntra>(hdr);
    k.dst_offset = (int32_t)pix;
    k.edge_offset = (int32_t)ln;
    k.log2_size = (uint8_t)log2;
    k.mode = (uint8_t)mode;
    k.c_idx_unit = (uint8_t)(c_idx & 3);
    if (!S.up() || ffhip_launch_hevc_intra(BD, S.dev(0), DP, S.dev(0), S.dev<const FFHipHevcIntra>(hdr), 1, 0) < 0 || !S.down())
        return false;
    S.get2d(src, stride, pix, DP, (size_t)N * PS, N);
    return true;
}

template <int BD, int I>
static void s_hpred_planar(uint8_t *src, const uint8_t *top, const uint8_t *left, ptrdiff_t stride)
{
    if (!hpred_gpu<BD>(src, top, left, stride, I + 2, 0, 0, false))
        SHIM_FB(g_fb_hpred[hpred_bdi(BD)], pred_planar[I], src, top, left, stride);
}
template <int BD>
static void s_hpred_dc(uint8_t *src, const uint8_t *top, const uint8_t *left, ptrdiff_t stride, int log2_size, int c_idx)
{
    if (!hpred_gpu<BD>(src, top, left, stride, log2_size, 1, c_idx, false))
        SHIM_FB(g_fb_hpred[hpred_bdi(BD)], pred_dc, src, top, left, stride, log2_size, c_idx);
}
/* the angular modes read top[-1] from the top (mode >= 18) and in mode 10's boundary filter, left[-1] otherwise */
template <int BD, int I>
static void s_hpred_angular(uint8_t *src, const uint8_t *top, const uint8_t *left, ptrdiff_t stride, int c_idx, int mode)
{
    const bool corner_left = !((mode >= 18 && mode != 26) || mode == 10);
    if (mode < 2 || !hpred_gpu<BD>(src, top, left, stride, I + 2, mode, c_idx, corner_left))
        SHIM_FB(g_fb_hpred[hpred_bdi(BD)], pred_angular[I], src, top, left, stride, c_idx, mode);
}
template <int BD>
static void hpred_fill(FFHipHEVCPredContext &o)
{
    o.pred_planar[0] = s_hpred_planar<BD, 0>; o.pred_planar[1] = s_hpred_planar<BD, 1>;
    o.pred_planar[2] = s_hpred_planar<BD, 2>; o.pred_planar[3] = s_hpred_planar<BD, 3>;
    o.pred_dc = s_hpred_dc<BD>;
    o.pred_angular[0] = s_hpred_angular<BD, 0>; o.pred_angular[1] = s_hpred_angular<BD, 1>;
    o.pred_angular[2] = s_hpred_angular<BD, 2>; o.pred_angular[3] = s_hpred_angular<BD, 3>;
}

extern "C" int ff_hevc_pred_init_hip(FFHipHEVCPredContext *c, int bit_depth)
{
    if (!c || !hpred_bd_ok(bit_depth)) {
        ffhip_set_error("ff_hevc_pred_init_hip: bit depth %d (8, 10 or 12)", bit_depth);
        return FFHIP_EINVAL;
    }
    if (!ffhip_have_device())
        return FFHIP_ENOSYS;
    FFHipHEVCPredContext o = *c; /* intra_pred[] stays the caller's */
    if (bit_depth == 8)
        hpred_fill<8>(o);
    else if (bit_depth == 10)
        hpred_fill<10>(o);
    else
        hpred_fill<12>(o);
    fb_snapshot(g_fb_hpred[hpred_bdi(bit_depth)], *c, o);
    *c = o;
    return 0;
}
