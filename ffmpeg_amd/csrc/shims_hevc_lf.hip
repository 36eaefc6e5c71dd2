/*
 * shims_hevc_lf.hip — ffhip_hevc_loop_filter_pictures_dev(): the host checks (kernels/picture_check.h, the maps, src / dst overlap)
 * and the launch of the in-loop filter (kernels/hevc_lf_pic.hip) on the caller's stream.  The maps and CTB records are device data
 * the kernel only uses to select table entries or to skip.
 */
#include "kernels/common.h"
#include "kernels/h264_kernels.h"
#include "kernels/picture_check.h"

extern "C" int ffhip_hevc_lf_ctb_record_size(void) { return (int)sizeof(FFHipHevcLfCtb); }

extern "C" int ffhip_hevc_loop_filter_pictures_dev(int bit_depth, int chroma_format_idc, int width, int height, int log2_ctb_size,
                                                   int log2_min_cb_size, int npics, const FFHipHevcLfPic *pics, void *stream)
{
    static const char who[] = "ffhip_hevc_loop_filter_pictures_dev";
    if (const int r = ffhip_check_hevc_pictures(who, bit_depth, chroma_format_idc, log2_ctb_size, width, height, npics, pics))
        return r;
    if (log2_min_cb_size < 3 || log2_min_cb_size > log2_ctb_size) {
        ffhip_set_error("%s: log2 min CB size %d (3..log2 CTB size %d)", who, log2_min_cb_size, log2_ctb_size);
        return FFHIP_EINVAL;
    }
    const FFHipPlaneGeom G = FFHipPlaneGeom::hevc(bit_depth, chroma_format_idc, width, height);
    const int bs_w = width >> 2, cb_w = (width + (1 << log2_min_cb_size) - 1) >> log2_min_cb_size;
    for (int i = 0; i < npics; i++) {
        const FFHipHevcLfPic &P = pics[i];
        if (!P.bs_ver || !P.bs_hor || !P.qp_y || !P.ctbs || P.bs_stride < bs_w || P.cb_stride < cb_w) {
            ffhip_set_error("%s: picture %d: a NULL map, bs_stride %d (>= %d) or cb_stride %d (>= %d)", who, i, P.bs_stride, bs_w, P.cb_stride,
                            cb_w);
            return FFHIP_EINVAL;
        }
        for (int p = 0; p < G.nplanes; p++) {
            const FFHipHevcLfPlane &D = P.plane[p];
            if (!ffhip_plane_ok(D.src, D.src_stride, G.amask, G.row_bytes(p)) || !ffhip_plane_ok(D.dst, D.dst_stride, G.amask, G.row_bytes(p))) {
                ffhip_set_error("%s: picture %d plane %d: NULL, or base and stride not %u-byte aligned, or a stride below the plane's width", who,
                                i, p, G.amask + 1);
                return FFHIP_EINVAL;
            }
        }
    }
    /* no src plane of the call may overlap a dst plane of the call: every workgroup reads its halo from src while others write dst
     * (dst planes that coincide are not refused) */
    FFHipSpanSet dst;
    dst.reserve((size_t)npics * G.nplanes);
    for (int i = 0; i < npics; i++)
        for (int p = 0; p < G.nplanes; p++)
            dst.add(G.span(pics[i].plane[p].dst, pics[i].plane[p].dst_stride, p));
    dst.seal();
    for (int j = 0; j < npics; j++)
        for (int q = 0; q < G.nplanes; q++)
            if (dst.hits(G.span(pics[j].plane[q].src, pics[j].plane[q].src_stride, q))) {
                ffhip_set_error("%s: picture %d plane %d: src overlaps a dst plane of the call", who, j, q);
                return FFHIP_EINVAL;
            }
    if (!ffhip_have_device())
        return FFHIP_ENOSYS;
    return ffhip_launch_hevc_loop_filter_pictures(bit_depth, chroma_format_idc, width, height, log2_ctb_size, log2_min_cb_size, npics, pics,
                                                  (hipStream_t)stream);
}
