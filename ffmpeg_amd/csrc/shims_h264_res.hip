/*
 * shims_h264_res.hip — ffhip_h264_residual_pictures_dev() and ffhip_h264_residual_pictures_fmt_dev() (chroma_format_idc 0 .. 3, the
 * planes sized by the format): the host checks (format, geometry, pointers, strides and alignment, the
 * row-wise overlap rule of the destination planes, inputs against destination spans, through kernels/picture_check.h) and the launch
 * of kernels/h264_res_pic.hip on the caller's stream; and the device-free faces: ffhip_h264_residual_pictures_host() and
 * ffhip_h264_residual_pictures_fmt_host(), the same checks and the same rules (kernels/h264_res_rules.h) on host arrays, and the
 * record sizes.
 */
#include <string.h>

#include "kernels/common.h"
#include "kernels/h264_kernels.h"
#include "kernels/h264_res_rules.h"
#include "kernels/picture_check.h"

extern "C" int ffhip_h264_res_mb_record_size(void) { return (int)sizeof(FFHipH264ResMb); }
extern "C" int ffhip_h264_res_pic_record_size(void) { return (int)sizeof(FFHipH264ResPic); }

namespace {
/* the argument checks of every face.  max_idc: 1 for the faces of 4:2:0 and monochrome, which name 2 and 3 in a refusal of their own;
 * 3 for the _fmt faces */
int check(const char *who, int max_idc, int bit_depth, int chroma_format_idc, int mb_w, int mb_h, int npics, const FFHipH264ResPic *pics)
{
    if (max_idc == 1 && (chroma_format_idc == 2 || chroma_format_idc == 3)) {
        ffhip_set_error("%s: chroma_format_idc %d: 4:2:2 and 4:4:4 are not implemented (0 or 1)", who, chroma_format_idc);
        return FFHIP_ENOSYS;
    }
    if ((bit_depth != 8 && bit_depth != 9 && bit_depth != 10 && bit_depth != 12 && bit_depth != 14) || chroma_format_idc < 0 ||
        chroma_format_idc > max_idc) {
        ffhip_set_error("%s: bit depth %d (8, 9, 10, 12 or 14), chroma_format_idc %d (%s)", who, bit_depth, chroma_format_idc,
                        max_idc == 1 ? "0 or 1" : "0..3");
        return FFHIP_EINVAL;
    }
    if (mb_w < 1 || mb_h < 1 || mb_w > 4096 || mb_h > 4096) {
        ffhip_set_error("%s: %d x %d macroblocks (1..4096 each)", who, mb_w, mb_h);
        return FFHIP_EINVAL;
    }
    if (const int r = ffhip_check_count(who, npics, pics, "picture"))
        return r;
    /* the planes' sizes by format: 4:2:0 8 mb_w x 8 mb_h, 4:2:2 8 mb_w x 16 mb_h, 4:4:4 16 mb_w x 16 mb_h */
    const FFHipPlaneGeom g = FFHipPlaneGeom::hevc(bit_depth, chroma_format_idc, 16 * mb_w, 16 * mb_h);
    const int ps = g.ps;
    const unsigned amask = g.amask;
    std::vector<FFHipRows> dst;
    dst.reserve((size_t)npics * 3);
    for (int i = 0; i < npics; i++) {
        const FFHipH264ResPic &P = pics[i];
        if (chroma_format_idc && !P.dst[1] != !P.dst[2]) {
            ffhip_set_error("%s: picture %d: one of Cb / Cr without the other", who, i);
            return FFHIP_EINVAL;
        }
        const bool has_c = chroma_format_idc && P.dst[1];
        for (int p = 0; p < (has_c ? 3 : 1); p++) {
            const ptrdiff_t row_bytes = g.row_bytes(p);
            if (!ffhip_plane_ok(P.dst[p], P.dst_stride[p], amask, row_bytes)) {
                ffhip_set_error("%s: picture %d: dst plane %d is NULL, its base or stride %td is not a multiple of 4 samples, or the stride "
                                "is below the plane's %d samples", who, i, p, P.dst_stride[p], g.pw[p]);
                return FFHIP_EINVAL;
            }
            dst.push_back(FFHipRows{ (uintptr_t)P.dst[p], P.dst_stride[p], row_bytes, g.ph[p] });
        }
        if (!P.mb || !P.res || !P.coeffs || ((uintptr_t)P.res & 3) || ((uintptr_t)P.coeffs & 15) || P.ncoeffs < 0) {
            ffhip_set_error("%s: picture %d: a NULL mb, res or coeffs, a res that is not 4-byte aligned, a coeffs that is not 16-byte aligned, "
                            "or ncoeffs %lld (>= 0)", who, i, (long long)P.ncoeffs);
            return FFHIP_EINVAL;
        }
    }
    /* workgroups of every picture of the call read while others write */
    FFHipSpanSet out;
    if (ffhip_any_rows_share(dst, out)) {
        ffhip_set_error("%s: a destination plane overlaps another destination plane of the call", who);
        return FFHIP_EINVAL;
    }
    const ptrdiff_t nmb = (ptrdiff_t)mb_w * mb_h;
    for (int i = 0; i < npics; i++) {
        const FFHipH264ResPic &P = pics[i];
        const FFHipSpan in[3] = { ffhip_plane_span(P.mb, 0, nmb * (ptrdiff_t)sizeof(FFHipH264BsMb), 1),
                                  ffhip_plane_span(P.res, 0, nmb * (ptrdiff_t)sizeof(FFHipH264ResMb), 1),
                                  /* no offset reaches past INT32_MAX + 768 coefficients */
                                  ffhip_plane_span(P.coeffs, 0, (ptrdiff_t)std::min<int64_t>(P.ncoeffs, (int64_t)INT32_MAX + 768) * (ps == 2 ? 4 : 2), 1) };
        for (int k = 0; k < 3; k++)
            if (out.hits(in[k])) {
                ffhip_set_error("%s: picture %d: mb, res or coeffs overlaps a destination plane of the call", who, i);
                return FFHIP_EINVAL;
            }
    }
    return 0;
}

/* v[N * i + k] added to row k, column i of the N x N block at dst */
template <typename PIX, int N>
void add_block(uint8_t *dst, ptrdiff_t stride, const int (&v)[N * N], int maxv)
{
    for (int k = 0; k < N; k++)
        for (int i = 0; i < N; i++) {
            PIX px;
            memcpy(&px, dst + k * stride + i * sizeof(PIX), sizeof(px));
            px = (PIX)h264tx_clip((int)px + v[N * i + k], maxv);
            memcpy(dst + k * stride + i * sizeof(PIX), &px, sizeof(px));
        }
}
template <typename CF, int N>
void load_coefs(const CF *c, int (&v)[N])
{
    for (int i = 0; i < N; i++)
        v[i] = c[i];
}

/* one macroblock at chroma_format_idc fmt: what the lanes of a macroblock do in k_h264_res_pic, block after block */
template <typename PIX, typename CF>
void residual_mb(const FFHipH264ResPic &P, int fmt, int mb_w, ptrdiff_t m, bool has_c, int maxv)
{
    const FFHipH264ResMb R = P.res[m];
    const H264ResPlan plan = h264res_plan(P.mb[m], R, has_c, P.ncoeffs, fmt);
    if (!plan.need)
        return;
    const int mx = (int)(m % mb_w), my = (int)(m / mb_w);
    const CF *c = static_cast<const CF *>(P.coeffs) + plan.off;
    for (int p = 0; p < (fmt == 3 && plan.need == 768 ? 3 : 1); p++)       /* the luma plane; rule 15: Cb and Cr as luma planes */
        for (int r = 0; r < 16; r++) {
            uint8_t *dst = P.dst[p] + (ptrdiff_t)(my * 16 + 4 * h264res_y4(r)) * P.dst_stride[p] + (size_t)(mx * 16 + 4 * h264res_x4(r)) * sizeof(PIX);
            if (h264res_luma4_on(plan, r, p)) {
                int v[16];
                load_coefs(c + 256 * p + 16 * r, v);
                h264res_luma<CF, 16>(v);
                add_block<PIX, 4>(dst, P.dst_stride[p], v, maxv);
            } else if (!(r & 3) && h264res_luma8_on(plan, r >> 2, p)) {
                int v[64];
                load_coefs(c + 256 * p + 16 * r, v);
                h264res_luma<CF, 64>(v);
                add_block<PIX, 8>(dst, P.dst_stride[p], v, maxv);
            }
        }
    if (fmt == 3)
        return;
    const int nc = h264res_chroma_blocks(fmt);
    for (int pl = 0; pl < 2; pl++) {
        const bool dc_on = (plan.chroma_dc >> pl) & 1;
        const CF *cp = c + 256 * (1 + pl);
        int dc[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
        if (dc_on) {
            for (int j = 0; j < nc; j++)
                dc[j] = cp[16 * j];
            if (fmt == 2) {
                h264tx_chroma422_dc<CF>(dc, R.qmul[pl]);
            } else {
                int d4[4] = { dc[0], dc[1], dc[2], dc[3] };
                h264tx_chroma_dc<CF>(d4, R.qmul[pl]);
                for (int j = 0; j < 4; j++)
                    dc[j] = d4[j];
            }
        }
        for (int j = 0; j < nc; j++) {
            const bool ac_on = h264res_chroma_on(plan, pl, j);
            if (!dc_on && !ac_on)
                continue;
            int v[16];
            if (ac_on) {
                load_coefs(cp + 16 * j, v);
                if (dc_on)
                    v[0] = dc[j];
                h264tx_idct4<CF>(v);
            } else {
                for (int i = 0; i < 16; i++)
                    v[i] = h264tx_dc(dc[j]);
            }
            add_block<PIX, 4>(P.dst[1 + pl] + (ptrdiff_t)(my * 2 * nc + 4 * (j >> 1)) * P.dst_stride[1 + pl] + (size_t)(mx * 8 + 4 * (j & 1)) * sizeof(PIX),
                              P.dst_stride[1 + pl], v, maxv);
        }
    }
}
} // namespace

extern "C" int ffhip_h264_residual_pictures_dev(int bit_depth, int chroma_format_idc, int mb_w, int mb_h, int npics, const FFHipH264ResPic *pics,
                                                void *stream)
{
    const int r = check("ffhip_h264_residual_pictures_dev", 1, bit_depth, chroma_format_idc, mb_w, mb_h, npics, pics);
    if (r < 0)
        return r;
    if (!ffhip_have_device())
        return FFHIP_ENOSYS;
    return ffhip_launch_h264_residual_pictures(bit_depth, chroma_format_idc, mb_w, mb_h, npics, pics, (hipStream_t)stream);
}

extern "C" int ffhip_h264_residual_pictures_fmt_dev(int bit_depth, int chroma_format_idc, int mb_w, int mb_h, int npics, const FFHipH264ResPic *pics,
                                                    void *stream)
{
    const int r = check("ffhip_h264_residual_pictures_fmt_dev", 3, bit_depth, chroma_format_idc, mb_w, mb_h, npics, pics);
    if (r < 0)
        return r;
    if (!ffhip_have_device())
        return FFHIP_ENOSYS;
    return ffhip_launch_h264_residual_pictures(bit_depth, chroma_format_idc, mb_w, mb_h, npics, pics, (hipStream_t)stream);
}

namespace {
int residual_host(const char *who, int max_idc, int bit_depth, int chroma_format_idc, int mb_w, int mb_h, int npics, const FFHipH264ResPic *pics)
{
    const int r = check(who, max_idc, bit_depth, chroma_format_idc, mb_w, mb_h, npics, pics);
    if (r < 0)
        return r;
    const int maxv = (1 << bit_depth) - 1;
    for (int i = 0; i < npics; i++) {
        const bool has_c = chroma_format_idc && pics[i].dst[1];
        for (ptrdiff_t m = 0; m < (ptrdiff_t)mb_w * mb_h; m++)
            if (bit_depth > 8)
                residual_mb<uint16_t, int32_t>(pics[i], chroma_format_idc, mb_w, m, has_c, maxv);
            else
                residual_mb<uint8_t, int16_t>(pics[i], chroma_format_idc, mb_w, m, has_c, maxv);
    }
    return 0;
}
} // namespace

extern "C" int ffhip_h264_residual_pictures_host(int bit_depth, int chroma_format_idc, int mb_w, int mb_h, int npics, const FFHipH264ResPic *pics)
{
    return residual_host("ffhip_h264_residual_pictures_host", 1, bit_depth, chroma_format_idc, mb_w, mb_h, npics, pics);
}

extern "C" int ffhip_h264_residual_pictures_fmt_host(int bit_depth, int chroma_format_idc, int mb_w, int mb_h, int npics, const FFHipH264ResPic *pics)
{
    return residual_host("ffhip_h264_residual_pictures_fmt_host", 3, bit_depth, chroma_format_idc, mb_w, mb_h, npics, pics);
}
