/*
 * shims_hevc_inter.hip — ffhip_hevc_inter_pictures_dev(): the host checks (kernels/picture_check.h, the DPB tables, reference /
 * destination overlap) and the launch of the inter reconstruction (kernels/hevc_inter_pic.hip) on the caller's stream.  The records
 * themselves are device data and are checked by the kernel.
 */
#include "kernels/common.h"
#include "kernels/h264_kernels.h"
#include "kernels/picture_check.h"

extern "C" int ffhip_hevc_inter_pu_record_size(void) { return (int)sizeof(FFHipHevcInterPU); }
extern "C" int ffhip_hevc_inter_tu_record_size(void) { return (int)sizeof(FFHipHevcInterTU); }
extern "C" int ffhip_hevc_inter_slice_record_size(void) { return (int)sizeof(FFHipHevcInterSlice); }

extern "C" int ffhip_hevc_inter_pictures_dev(int bit_depth, int chroma_format_idc, int width, int height, int log2_ctb_size, int npics,
                                             const FFHipHevcInterPic *pics, void *stream)
{
    static const char who[] = "ffhip_hevc_inter_pictures_dev";
    if (const int r = ffhip_check_hevc_pictures(who, bit_depth, chroma_format_idc, log2_ctb_size, width, height, npics, pics))
        return r;
    const FFHipPlaneGeom G = FFHipPlaneGeom::hevc(bit_depth, chroma_format_idc, width, height);
    for (int i = 0; i < npics; i++) {
        const FFHipHevcInterPic &P = pics[i];
        if (!P.pus || !P.pu_ctb_start || (P.nslices > 0 && !P.slices) || P.nslices < 0 || P.nrefs < 0 || P.nrefs > 16) {
            ffhip_set_error("%s: picture %d: NULL PU / slice tables, nslices = %d or nrefs = %d (0..16)", who, i, P.nslices, P.nrefs);
            return FFHIP_EINVAL;
        }
        for (int p = 0; p < G.nplanes; p++) {
            const FFHipHevcInterPlane &D = P.plane[p];
            if (!D.base || !D.tus || !D.tu_ctb_start || !D.res) {
                ffhip_set_error("%s: picture %d plane %d: a NULL pointer", who, i, p);
                return FFHIP_EINVAL;
            }
            if (!ffhip_plane_ok(D.base, D.stride, G.amask, G.row_bytes(p))) {
                ffhip_set_error("%s: picture %d plane %d: base and stride must be %u-byte aligned, the stride at least the plane's width", who,
                                i, p, G.amask + 1);
                return FFHIP_EINVAL;
            }
            for (int r = 0; r < P.nrefs; r++)
                if (!ffhip_plane_ok(P.ref[r].base[p], P.ref[r].stride[p], G.ps - 1, G.row_bytes(p))) {
                    ffhip_set_error("%s: picture %d reference %d plane %d: NULL, misaligned or a stride below the width", who, i, r, p);
                    return FFHIP_EINVAL;
                }
        }
    }
    /* no reference plane of the call may be a destination plane of the call: a launch's pictures are predicted side by side
     * (destination planes that coincide are not refused) */
    FFHipSpanSet dst;
    dst.reserve((size_t)npics * G.nplanes);
    for (int i = 0; i < npics; i++)
        for (int p = 0; p < G.nplanes; p++)
            dst.add(G.span(pics[i].plane[p].base, pics[i].plane[p].stride, p));
    dst.seal();
    for (int j = 0; j < npics; j++)
        for (int r = 0; r < pics[j].nrefs; r++)
            for (int q = 0; q < G.nplanes; q++)
                if (dst.hits(G.span(pics[j].ref[r].base[q], pics[j].ref[r].stride[q], q))) {
                    ffhip_set_error("%s: picture %d reference %d plane %d overlaps a plane the call writes", who, j, r, q);
                    return FFHIP_EINVAL;
                }
    if (!ffhip_have_device())
        return FFHIP_ENOSYS;
    return ffhip_launch_hevc_inter_pictures(bit_depth, chroma_format_idc, width, height, log2_ctb_size, npics, pics, (hipStream_t)stream);
}
