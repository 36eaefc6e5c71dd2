/*
 * shims_vp9_intra.hip — ffhip_vp9_intra_frames_dev(): the host checks (kernels/picture_check.h, tile columns, plane overlap) and the
 * launch of the intra reconstruction (kernels/vp9_intra_frame.hip) on the caller's stream.  The records themselves are device data
 * and are checked by the kernel.  Also ffhip_vp9_intra_block_records(), the device-free expansion of one decoded
 * block into its records in intra_recon's order (libavcodec/vp9recon.c).
 */
#include <algorithm>

#include "kernels/common.h"
#include "kernels/h264_kernels.h"
#include "kernels/picture_check.h"

extern "C" int ffhip_vp9_intra_record_size(void) { return (int)sizeof(FFHipVp9IntraRec); }

extern "C" int ffhip_vp9_intra_frames_dev(int bit_depth, int ss_h, int ss_v, int width, int height, int npics, const FFHipVp9IntraPic *pics,
                                          void *stream)
{
    static const char who[] = "ffhip_vp9_intra_frames_dev";
    if (const int r = ffhip_check_vp9_frames(who, bit_depth, ss_h, ss_v, width, height, npics, pics))
        return r;
    const FFHipPlaneGeom G = FFHipPlaneGeom::vp9(bit_depth, ss_h, ss_v, width, height);
    FFHipSpanSet planes;
    planes.reserve((size_t)npics * 3);
    for (int i = 0; i < npics; i++) {
        const FFHipVp9IntraPic &P = pics[i];
        if (P.log2_tile_cols < 0 || P.log2_tile_cols > 6) {
            ffhip_set_error("%s: frame %d: log2_tile_cols %d (0..6)", who, i, P.log2_tile_cols);
            return FFHIP_EINVAL;
        }
        for (int p = 0; p < 3; p++) {
            const FFHipVp9IntraPlane &D = P.plane[p];
            if (!D.base || !D.recs || !D.rec_sb_start || !D.coeffs) {
                ffhip_set_error("%s: frame %d plane %d: a NULL pointer", who, i, p);
                return FFHIP_EINVAL;
            }
            if (!ffhip_plane_ok(D.base, D.stride, G.amask, G.row_bytes(p))) {
                ffhip_set_error("%s: frame %d plane %d: base and stride must be %u-byte aligned, the stride at least the decoded width", who, i,
                                p, G.amask + 1);
                return FFHIP_EINVAL;
            }
            planes.add(G.span(D.base, D.stride, p));
        }
    }
    /* no two planes of the call may overlap: a launch's planes are reconstructed side by side */
    if (planes.seal()) {
        ffhip_set_error("%s: two planes of the call overlap", who);
        return FFHIP_EINVAL;
    }
    if (!ffhip_have_device())
        return FFHIP_ENOSYS;
    return ffhip_launch_vp9_intra_frames(bit_depth, ss_h, ss_v, width, height, npics, pics, (hipStream_t)stream);
}

extern "C" int ffhip_vp9_intra_block_records(FFHipVp9IntraRec *out, int plane, int bs, int tx, int row, int col, const uint8_t mode[4], int skip,
                                             const uint16_t *eob, int lossless, int cols, int rows, int ss_h, int ss_v)
{
    /* ff_vp9_bwh_tab[1] (libavcodec/vp9data.c) in 8-sample units: BS_64x64 .. BS_4x4 (sub-8x8 blocks count as 8x8) */
    static const uint8_t bw8[13] = { 8, 8, 4, 4, 4, 2, 2, 2, 1, 1, 1, 1, 1 };
    static const uint8_t bh8[13] = { 8, 4, 8, 4, 2, 4, 2, 1, 2, 1, 1, 1, 1 };
    if (!out || !mode || (!skip && !eob) || plane < 0 || plane > 2 || bs < 0 || bs > 12 || tx < 0 || tx > 3 || cols < 1 || cols > 8192 ||
        rows < 1 || rows > 8192 || row < 0 || row >= rows || col < 0 || col >= cols || (ss_h & ~1) || (ss_v & ~1)) {
        ffhip_set_error("ffhip_vp9_intra_block_records: plane %d (0..2), block size %d (0..12), tx %d (0..3), row %d / col %d inside %d x %d "
                        "blocks (1..8192), subsampling %d, %d, or a NULL pointer", plane, bs, tx, row, col, cols, rows, ss_h, ss_v);
        return FFHIP_EINVAL;
    }
    const int hs = plane ? ss_h : 0, vs = plane ? ss_v : 0;
    const int w4 = (bw8[bs] << 1) >> hs, h4 = (bh8[bs] << 1) >> vs; /* intra_recon's w4 (shifted for chroma), 4-sample units */
    const int end_x = std::min(2 * (cols - col), bw8[bs] << 1) >> hs, end_y = std::min(2 * (rows - row), bh8[bs] << 1) >> vs;
    const int step1d = 1 << tx, step = 1 << (2 * tx);
    /* the transform must fit the block in this plane (uvtx is at most what the chroma block allows) */
    if (4 * step1d > 4 * std::max(w4, 1) || 4 * step1d > 4 * std::max(h4, 1) || (lossless && tx)) {
        ffhip_set_error("ffhip_vp9_intra_block_records: tx %d does not fit block size %d in plane %d (or a lossless frame with tx > 0)", tx, bs,
                        plane);
        return FFHIP_EINVAL;
    }
    const int x0 = (col * 8) >> hs, y0 = (row * 8) >> vs;
    int k = 0, n = 0;
    for (int y = 0; y < end_y; y += step1d)
        for (int x = 0; x < end_x; x += step1d, n += step) {
            const int m = mode[plane == 0 && bs > 9 && tx == 0 ? y * 2 + x : 0]; /* b->bs > BS_8x8 && b->tx == TX_4X4 */
            const int e = skip ? 0 : eob[n];
            FFHipVp9IntraRec &R = out[k++];
            R.x = (uint16_t)(x0 + 4 * x);
            R.y = (uint16_t)(y0 + 4 * y);
            R.coeff_offset = 16 * n;
            R.tx = (uint8_t)(lossless ? 4 : tx);
            R.mode = (uint8_t)m;
            R.txtp = 0;
            if (plane == 0) { /* ff_vp9_intra_txfm_type[mode] */
                static const uint8_t intra_txfm_type[10] = { 2, 1, 0, 0, 3, 2, 1, 2, 1, 3 };
                R.txtp = m < 10 ? intra_txfm_type[m] : 0;
            }
            R.flags = (uint8_t)((e ? FFHIP_VP9_INTRA_RESIDUAL : 0) | (e == 1 ? FFHIP_VP9_INTRA_DC_ONLY : 0) |
                                (x < w4 - 1 ? FFHIP_VP9_INTRA_HAVE_RIGHT : 0));
        }
    return k;
}
