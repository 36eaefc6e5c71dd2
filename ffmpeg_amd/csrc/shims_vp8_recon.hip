/*
 * shims_vp8_recon.hip — VP8 reconstruction of whole frames: the host checks of ffhip_vp8_recon_frames_dev() (kernels/picture_check.h; kernels in
 * kernels/vp8_recon_frame.hip) and the device-free faces ffhip_vp8_mb_preds() / ffhip_vp8_intra_modes(), which run the rules the
 * kernels run (kernels/vp8_recon_rules.h) on the host.
 */
#include "kernels/common.h"
#include "kernels/picture_check.h"
#include "kernels/vp8_kernels.h"
#include "kernels/vp8_recon_rules.h"

extern "C" int ffhip_vp8_mb_record_size(void) { return (int)sizeof(FFHipVp8Mb); }

extern "C" int ffhip_vp8_mb_preds(const FFHipVp8Mb *mb, int mb_x, int mb_y, int fullpel_chroma, FFHipVp8Pred out[24])
{
    if (!mb || !out || mb->ref_frame == 0 || mb->ref_frame > 3 || mb->partitioning > FFHIP_VP8_PART_4x4 || mb_x < 0 || mb_y < 0) {
        ffhip_set_error("ffhip_vp8_mb_preds: NULL, an intra record, or a reference / partitioning out of range");
        return FFHIP_EINVAL;
    }
    const int n = v8r_npreds(mb->partitioning);
    for (int i = 0; i < n; i++)
        v8r_pred(*mb, i, mb_x, mb_y, fullpel_chroma != 0, out[i]);
    return n;
}

extern "C" int ffhip_vp8_intra_modes(const FFHipVp8Mb *mb, int mb_x, int mb_y, FFHipVp8IntraModes *out)
{
    bool ok = mb && out && mb->ref_frame == 0 && mb->mode <= FFHIP_VP8_MODE_I4x4 && mb->chroma_mode <= FFHIP_VP8_PRED_TM && mb_x >= 0 && mb_y >= 0;
    if (ok && mb->mode == FFHIP_VP8_MODE_I4x4)
        for (int i = 0; i < 16; i++)
            ok = ok && mb->sub_mode[i] <= FFHIP_VP8_B_TM;
    if (!ok) {
        ffhip_set_error("ffhip_vp8_intra_modes: NULL, an inter record, or a mode out of range");
        return FFHIP_EINVAL;
    }
    v8r_intra_modes(*mb, mb_x, mb_y, *out);
    return 0;
}

extern "C" int ffhip_vp8_recon_frames_dev(int mb_w, int mb_h, int bilinear, int fullpel_chroma, int npics, const FFHipVp8ReconPic *pics,
                                          ptrdiff_t stride_y, ptrdiff_t stride_uv, void *stream)
{
    static const char who[] = "ffhip_vp8_recon_frames_dev";
    if ((bilinear & ~1) || (fullpel_chroma & ~1) || mb_w < 1 || mb_w > 1024 || mb_h < 1 || mb_h > 1024) {
        ffhip_set_error("%s: bilinear %d, fullpel_chroma %d (0 or 1 each), %d x %d macroblocks (1..1024)", who, bilinear, fullpel_chroma, mb_w,
                        mb_h);
        return FFHIP_EINVAL;
    }
    if (const int r = ffhip_check_count(who, npics, pics, "frame"))
        return r;
    if ((stride_y & 3) || stride_y < 16 * mb_w || (stride_uv & 3) || stride_uv < 8 * mb_w) {
        ffhip_set_error("%s: strides %td / %td must be multiples of 4 and at least the planes' widths", who, stride_y, stride_uv);
        return FFHIP_EINVAL;
    }
    auto span = [&](const uint8_t *b, int p) { return ffhip_plane_span(b, p ? stride_uv : stride_y, (p ? 8 : 16) * mb_w, (p ? 8 : 16) * mb_h); };
    FFHipSpanSet dsts;
    std::vector<FFHipSpan> refs;
    for (int i = 0; i < npics; i++) {
        const FFHipVp8ReconPic &P = pics[i];
        const uint8_t *const pl[3] = { P.y, P.u, P.v };
        if (!P.mbs || P.coeff_count < 0 || (!P.coeffs && P.coeff_count > 0)) {
            ffhip_set_error("%s: frame %d: a NULL record array, or coefficients counted but NULL", who, i);
            return FFHIP_EINVAL;
        }
        for (int p = 0; p < 3; p++) {
            if (!pl[p] || ((uintptr_t)pl[p] & 3)) {
                ffhip_set_error("%s: frame %d plane %d: NULL, or not 4-byte aligned", who, i, p);
                return FFHIP_EINVAL;
            }
            dsts.add(span(pl[p], p));
            for (int r = 0; r < 3; r++) {
                if (!P.ref[r][p])
                    continue;
                if ((uintptr_t)P.ref[r][p] & 3) {
                    ffhip_set_error("%s: frame %d reference %d plane %d: not 4-byte aligned", who, i, r + 1, p);
                    return FFHIP_EINVAL;
                }
                refs.push_back(span(P.ref[r][p], p));
            }
        }
    }
    /* the frames of a call are reconstructed side by side: no two destination planes may share a byte, and no frame may be read
     * as a reference while the call writes it */
    if (dsts.seal()) {
        ffhip_set_error("%s: two destination planes of the call overlap", who);
        return FFHIP_EINVAL;
    }
    for (const FFHipSpan &r : refs)
        if (dsts.hits(r)) {
            ffhip_set_error("%s: a reference plane overlaps a destination plane of the call", who);
            return FFHIP_EINVAL;
        }
    if (!ffhip_have_device())
        return FFHIP_ENOSYS;
    return ffhip_launch_vp8_recon_frames(mb_w, mb_h, bilinear, fullpel_chroma, npics, pics, stride_y, stride_uv, (hipStream_t)stream);
}
