/*
 * shims_h264_lf.hip — ffhip_h264_deblock_pictures_fmt_dev(): frame-order deblocking of whole H.264 pictures at chroma_format_idc
 * 0 .. 3 from the tables of ffhip_h264_edge_params_pictures_fmt_dev() (shims_h264_bs.hip).  The argument checks and the dispatch to the
 * frame-order filters' launchers (kernels/h264_deblock.hip, kernels/h264_c422.hip); no kernel of its own.
 */
#include <vector>

#include "kernels/common.h"
#include "kernels/h264_kernels.h"
#include "kernels/picture_check.h"

extern "C" int ffhip_h264_lf_pic_record_size(void) { return (int)sizeof(FFHipH264LfPic); }

namespace {
/* the planes of one filter (chroma 0: the luma filter, 1: the 4:2:0 chroma one, 2: the 4:2:2 chroma one) and stride, with their tables */
struct LfGroup {
    std::vector<uint8_t *> planes;
    std::vector<const FFHipH264Edge *> edges;
};

int lf_run(int bd, int chroma, const LfGroup &G, ptrdiff_t stride, int mb_w, int mb_h, hipStream_t stream)
{
    const int n = (int)G.planes.size();
    if (!n)
        return 0;
    if (chroma == 2)
        return ffhip_launch_h264_deblock_c422_planes(bd, n, G.planes.data(), G.edges.data(), stride, mb_w, mb_h, stream);
    /* several planes in one launch where the skewed-rows kernel can address them by table, else plane by plane */
    uintptr_t al = (uintptr_t)stride, ale = 0;
    for (int i = 0; i < n; i++) {
        al |= (uintptr_t)G.planes[i];
        ale |= (uintptr_t)G.edges[i];
    }
    if (n > 1 && !(al & (chroma && bd == 8 ? 7 : 15)) && !(ale & 15))
        return ffhip_launch_h264_deblock_pictures_bd(bd, chroma, G.planes.data(), G.edges.data(), n, stride, mb_w, mb_h, stream);
    for (int i = 0; i < n; i++) {
        const int r = ffhip_launch_h264_deblock_frames_bd(bd, chroma, G.planes[i], 0, 1, stride, mb_w, mb_h, G.edges[i], stream);
        if (r < 0)
            return r;
    }
    return 0;
}
} // namespace

extern "C" int ffhip_h264_deblock_pictures_fmt_dev(int bit_depth, int chroma_format_idc, int mb_w, int mb_h, ptrdiff_t stride_y, ptrdiff_t stride_c,
                                                   int npics, const FFHipH264LfPic *pics, void *stream)
{
    const char *who = "ffhip_h264_deblock_pictures_fmt_dev";
    const int bd = bit_depth, fmt = chroma_format_idc;
    if ((bd != 8 && bd != 9 && bd != 10 && bd != 12 && bd != 14) || fmt < 0 || fmt > 3) {
        ffhip_set_error("%s: bit depth %d (8, 9, 10, 12 or 14), chroma_format_idc %d (0..3)", who, bd, fmt);
        return FFHIP_EINVAL;
    }
    if (mb_w < 1 || mb_h < 1 || mb_w > 4096 || mb_h > 4096) {
        ffhip_set_error("%s: %d x %d macroblocks (1..4096 each)", who, mb_w, mb_h);
        return FFHIP_EINVAL;
    }
    if (const int r = ffhip_check_count(who, npics, pics, "picture"))
        return r;
    /* what the launchers ask of a plane, its stride and its table: 8 bits 4 bytes each; above, 16 bytes each, and for the 4:2:2 chroma
     * filter 8 bytes for the plane and the stride and 4 for the table */
    const int nplanes = fmt ? 3 : 1;
    for (int p = 0; p < nplanes; p++) {
        const bool c422 = p && fmt == 2;
        const uintptr_t pmask = bd == 8 ? 3 : c422 ? 7 : 15, emask = bd == 8 || c422 ? 3 : 15;
        const ptrdiff_t stride = p ? stride_c : stride_y;
        bool used = false;
        for (int i = 0; i < npics; i++) {
            if (!pics[i].edges[p])
                continue;
            used = true;
            if (!pics[i].plane[p] || ((uintptr_t)pics[i].plane[p] & pmask) || ((uintptr_t)pics[i].edges[p] & emask)) {
                ffhip_set_error("%s: picture %d: plane %d is NULL, or it is not %d-byte or its edge table not %d-byte aligned (bit depth %d)", who, i,
                                p, (int)pmask + 1, (int)emask + 1, bd);
                return FFHIP_EINVAL;
            }
        }
        if (used && ((uintptr_t)stride & pmask)) {
            ffhip_set_error("%s: the stride %td of plane %d is not %d-byte aligned (bit depth %d)", who, stride, p, (int)pmask + 1, bd);
            return FFHIP_EINVAL;
        }
    }
    if (!ffhip_have_device())
        return FFHIP_ENOSYS;
    /* plane 0, and at 4:4:4 every plane, by the luma filter (Cb / Cr apart when their stride is another one); Cb / Cr of 4:2:0 and 4:2:2
     * by the filter of their format, all pictures side by side */
    LfGroup luma, chroma;
    for (int i = 0; i < npics; i++)
        for (int p = 0; p < nplanes; p++)
            if (pics[i].edges[p]) {
                LfGroup &G = p && !(fmt == 3 && stride_c == stride_y) ? chroma : luma;
                G.planes.push_back(pics[i].plane[p]);
                G.edges.push_back(pics[i].edges[p]);
            }
    const int r = lf_run(bd, 0, luma, stride_y, mb_w, mb_h, (hipStream_t)stream);
    return r < 0 ? r : lf_run(bd, fmt == 3 ? 0 : fmt, chroma, stride_c, mb_w, mb_h, (hipStream_t)stream);
}
