/*
 * shims_hevc_lf.hip — ffhip_hevc_loop_filter_pictures_dev(): validates what the host can see of a picture set (geometry, planes,
 * map pointers and strides, src / dst overlap) and launches the in-loop filter (kernels/hevc_lf_pic.hip) on the caller's stream.
 * The maps and CTB records are device data the kernel only uses to select table entries or to skip.
 */
#include <algorithm>
#include <stdint.h>
#include <vector>

#include "kernels/common.h"
#include "kernels/h264_kernels.h"

extern "C" int ffhip_hevc_lf_ctb_record_size(void) { return (int)sizeof(FFHipHevcLfCtb); }

namespace {
struct Span { /* the bytes a plane occupies: [lo, hi) */
    uintptr_t lo, hi;
};
Span plane_span(const void *base, ptrdiff_t stride, int w_bytes, int rows)
{
    const uintptr_t b = (uintptr_t)base;
    return { b, b + (uintptr_t)((ptrdiff_t)(rows - 1) * stride + w_bytes) };
}
} // namespace

extern "C" int ffhip_hevc_loop_filter_pictures_dev(int bit_depth, int chroma_format_idc, int width, int height, int log2_ctb_size,
                                                   int log2_min_cb_size, int npics, const FFHipHevcLfPic *pics, void *stream)
{
    if ((bit_depth != 8 && bit_depth != 10 && bit_depth != 12) || chroma_format_idc < 0 || chroma_format_idc > 3 || log2_ctb_size < 4 ||
        log2_ctb_size > 6 || log2_min_cb_size < 3 || log2_min_cb_size > log2_ctb_size) {
        ffhip_set_error("ffhip_hevc_loop_filter_pictures_dev: bit depth %d (8, 10 or 12), chroma format %d (0..3), log2 CTB size %d (4..6), "
                        "log2 min CB size %d (3..log2 CTB size)", bit_depth, chroma_format_idc, log2_ctb_size, log2_min_cb_size);
        return FFHIP_EINVAL;
    }
    if (width <= 0 || height <= 0 || width > 65535 || height > 65535 || (width | height) & 7) {
        ffhip_set_error("ffhip_hevc_loop_filter_pictures_dev: picture size %d x %d (multiples of 8, at most 65535)", width, height);
        return FFHIP_EINVAL;
    }
    if (npics <= 0 || !pics) {
        ffhip_set_error("ffhip_hevc_loop_filter_pictures_dev: npics = %d, or a NULL picture array", npics);
        return FFHIP_EINVAL;
    }
    const int ps = bit_depth > 8 ? 2 : 1, nplanes = chroma_format_idc ? 3 : 1;
    const unsigned amask = 4u * ps - 1; /* four samples per access */
    const int bs_w = width >> 2, cb_w = (width + (1 << log2_min_cb_size) - 1) >> log2_min_cb_size;
    int pw[3], ph[3];
    for (int p = 0; p < 3; p++) {
        pw[p] = p && chroma_format_idc != 3 ? width >> 1 : width;
        ph[p] = p && chroma_format_idc == 1 ? height >> 1 : height;
    }
    for (int i = 0; i < npics; i++) {
        const FFHipHevcLfPic &P = pics[i];
        if (!P.bs_ver || !P.bs_hor || !P.qp_y || !P.ctbs || P.bs_stride < bs_w || P.cb_stride < cb_w) {
            ffhip_set_error("ffhip_hevc_loop_filter_pictures_dev: picture %d: a NULL map, bs_stride %d (>= %d) or cb_stride %d (>= %d)", i,
                            P.bs_stride, bs_w, P.cb_stride, cb_w);
            return FFHIP_EINVAL;
        }
        for (int p = 0; p < nplanes; p++) {
            const FFHipHevcLfPlane &D = P.plane[p];
            if (!D.src || !D.dst || (((uintptr_t)D.src | (size_t)D.src_stride | (uintptr_t)D.dst | (size_t)D.dst_stride) & amask) ||
                D.src_stride < (ptrdiff_t)pw[p] * ps || D.dst_stride < (ptrdiff_t)pw[p] * ps) {
                ffhip_set_error("ffhip_hevc_loop_filter_pictures_dev: picture %d plane %d: NULL, or base and stride not %u-byte aligned, or a "
                                "stride below the plane's width", i, p, amask + 1);
                return FFHIP_EINVAL;
            }
        }
    }
    /* no src plane of the call may overlap a dst plane of the call: every workgroup reads its halo from src while others write dst.
     * The dst spans are sorted by start with a running maximum of their ends, so each src span is one binary search */
    std::vector<Span> dst;
    dst.reserve((size_t)npics * nplanes);
    for (int i = 0; i < npics; i++)
        for (int p = 0; p < nplanes; p++)
            dst.push_back(plane_span(pics[i].plane[p].dst, pics[i].plane[p].dst_stride, pw[p] * ps, ph[p]));
    std::sort(dst.begin(), dst.end(), [](const Span &x, const Span &y) { return x.lo < y.lo; });
    std::vector<uintptr_t> hi_max(dst.size());
    for (size_t k = 0; k < dst.size(); k++)
        hi_max[k] = k ? std::max(hi_max[k - 1], dst[k].hi) : dst[k].hi;
    for (int j = 0; j < npics; j++)
        for (int q = 0; q < nplanes; q++) {
            const Span s = plane_span(pics[j].plane[q].src, pics[j].plane[q].src_stride, pw[q] * ps, ph[q]);
            const size_t n = (size_t)(std::lower_bound(dst.begin(), dst.end(), s.hi, [](const Span &x, uintptr_t v) { return x.lo < v; }) -
                                      dst.begin());
            if (n && hi_max[n - 1] > s.lo) {
                ffhip_set_error("ffhip_hevc_loop_filter_pictures_dev: picture %d plane %d: src overlaps a dst plane of the call", j, q);
                return FFHIP_EINVAL;
            }
        }
    if (!ffhip_have_device())
        return FFHIP_ENOSYS;
    return ffhip_launch_hevc_loop_filter_pictures(bit_depth, chroma_format_idc, width, height, log2_ctb_size, log2_min_cb_size, npics, pics,
                                                  (hipStream_t)stream);
}
