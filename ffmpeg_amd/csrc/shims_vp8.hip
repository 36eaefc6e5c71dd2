/*
 * shims_vp8.hip — vp8dsp: the signature-exact HOST-pointer table (ff_vp78dsp_init_hip / ff_vp8dsp_init_hip), the batch device faces
 * (ffhip_vp8_luma_dc_wht_batch_dev, ffhip_vp8_idct_add_batch_dev, ffhip_vp8_mc_batch_dev) and the whole-frame loop filter's
 * validation (ffhip_vp8_loopfilter_frames_dev).  The kernels are in kernels/vp8_dsp.hip and kernels/vp8_lf_frame.hip.
 *
 * The host faces follow shims.hip: one call = one Stage image sent in one copy, the same kernels as the batch faces with n = 1, the
 * image back in one copy and committed from there; a call that cannot run on the device (or an argument outside the reference's
 * range) is answered by the C function the init displaced (SHIM_FB).  Only what the reference reads of the caller's memory is staged.
 */
#include <stdint.h>
#include <string.h>

#include "kernels/common.h"
#include "kernels/picture_check.h"
#include "kernels/shim_arena.h"
#include "kernels/vp8_kernels.h"

static FFHipVP8DSPContext g_fb_vp8; /* the C functions the two inits displaced */

/* ---- transforms ---- */
static bool vp8_wht_single(int16_t block[4][4][16], int16_t dc[16], int dc_only)
{
    Stage S;
    const size_t co = S.put(dc, 32), bo = S.put(block, 512), hdr = S.hole(sizeof(FFHipVp8WhtRec));
    FFHipVp8WhtRec &k = *S.img<FFHipVp8WhtRec>(hdr);
    k.dc_offset = (int32_t)co;
    k.block_offset = (int32_t)bo;
    k.dc_only = (uint8_t)dc_only;
    if (!S.up() || ffhip_launch_vp8_wht(S.dev<int16_t>(0), S.dev<const FFHipVp8WhtRec>(hdr), 1, 0) < 0 || !S.down())
        return false;
    memcpy(dc, S.img(co), 32);
    /* only block[i][j][0] is written: the other coefficients may be changing elsewhere (they are the caller's) */
    int16_t *b = &block[0][0][0];
    const int16_t *r = S.img<int16_t>(bo);
    for (int i = 0; i < 16; i++)
        b[16 * i] = r[16 * i];
    return true;
}
static void s_wht(int16_t block[4][4][16], int16_t dc[16]) { if (!vp8_wht_single(block, dc, 0)) SHIM_FB(g_fb_vp8, vp8_luma_dc_wht, block, dc); }
static void s_wht_dc(int16_t block[4][4][16], int16_t dc[16]) { if (!vp8_wht_single(block, dc, 1)) SHIM_FB(g_fb_vp8, vp8_luma_dc_wht_dc, block, dc); }

/* nb 4x4 blocks at (bx[i], by[i]) samples from dst, coefficients block + 16 i; a w x h rectangle travels */
static bool vp8_idct_single(uint8_t *dst, ptrdiff_t stride, int16_t *block, int nb, const int *bx, const int *by, int dc_only, int w, int h)
{
    const Rect d = { dst, stride, 0, h - 1, 0, w - 1 };
    Stage S;
    const size_t co = S.put(block, (size_t)nb * 32), hdr = S.hole((size_t)nb * sizeof(FFHipVp8IdctRec));
    const ptrdiff_t pix = S.rect(d);
    FFHipVp8IdctRec *k = S.img<FFHipVp8IdctRec>(hdr);
    for (int i = 0; i < nb; i++) {
        k[i].dst_offset = (int32_t)(pix + by[i] * DP + bx[i]);
        k[i].coeff_offset = (int32_t)(co + 32 * i);
        k[i].dc_only = (uint8_t)dc_only;
    }
    if (!S.up() || ffhip_launch_vp8_idct(S.dev(0), DP, S.dev<int16_t>(0), S.dev<const FFHipVp8IdctRec>(hdr), nb, 0) < 0 || !S.down())
        return false;
    S.commit(d, pix);
    /* idct_add zeroes all 16, the dc forms block[i][0] only */
    const int16_t *r = S.img<int16_t>(co);
    for (int i = 0; i < nb; i++) {
        if (dc_only)
            block[16 * i] = r[16 * i];
        else
            memcpy(block + 16 * i, r + 16 * i, 32);
    }
    return true;
}
static const int k_x0[4] = { 0, 0, 0, 0 }, k_x4y[4] = { 0, 4, 8, 12 }, k_x4uv[4] = { 0, 4, 0, 4 }, k_y4uv[4] = { 0, 0, 4, 4 };
static void s_idct_add(uint8_t *d, int16_t b[16], ptrdiff_t s)
{ if (!vp8_idct_single(d, s, b, 1, k_x0, k_x0, 0, 4, 4)) SHIM_FB(g_fb_vp8, vp8_idct_add, d, b, s); }
static void s_idct_dc_add(uint8_t *d, int16_t b[16], ptrdiff_t s)
{ if (!vp8_idct_single(d, s, b, 1, k_x0, k_x0, 1, 4, 4)) SHIM_FB(g_fb_vp8, vp8_idct_dc_add, d, b, s); }
static void s_idct_dc_add4y(uint8_t *d, int16_t b[4][16], ptrdiff_t s)
{ if (!vp8_idct_single(d, s, &b[0][0], 4, k_x4y, k_x0, 1, 16, 4)) SHIM_FB(g_fb_vp8, vp8_idct_dc_add4y, d, b, s); }
static void s_idct_dc_add4uv(uint8_t *d, int16_t b[4][16], ptrdiff_t s)
{ if (!vp8_idct_single(d, s, &b[0][0], 4, k_x4uv, k_y4uv, 1, 8, 8)) SHIM_FB(g_fb_vp8, vp8_idct_dc_add4uv, d, b, s); }

/* ---- loop filters: the lines across the edge, 4 samples either side (2 for the simple filter, the only ones it reads) ---- */
static bool vp8_lf_single(int kind, int dir, int lines, uint8_t *const *planes, int nplanes, ptrdiff_t stride, int E, int I, int H)
{
    if (E < 0 || E > 255 || I < 0 || I > 255 || H < 0 || H > 255)
        return false; /* the record carries bytes; any other value is the C function's */
    const int r = kind == VP8_LF_SIMPLE ? 2 : 4;
    Stage S;
    const size_t hdr = S.hole((size_t)nplanes * sizeof(Vp8LfEdge));
    Rect d[2];
    ptrdiff_t org[2];
    for (int p = 0; p < nplanes; p++) {
        d[p] = dir ? Rect{ planes[p], stride, -r, r - 1, 0, lines - 1 } : Rect{ planes[p], stride, 0, lines - 1, -r, r - 1 };
        /* the staged area holds 4 samples either side (what the line function loads), zero where the reference reads nothing */
        const Rect a = dir ? Rect{ planes[p], stride, -4, 3, 0, lines - 1 } : Rect{ planes[p], stride, 0, lines - 1, -4, 3 };
        org[p] = S.area(a);
        S.fill(d[p], org[p]);
        Vp8LfEdge &k = S.img<Vp8LfEdge>(hdr)[p];
        k.offset = (int32_t)org[p];
        k.kind = (uint8_t)kind; k.dir = (uint8_t)dir; k.lines = (uint8_t)lines;
        k.E = (uint8_t)E; k.I = (uint8_t)I; k.H = (uint8_t)H;
    }
    if (!S.up() || ffhip_launch_vp8_lf_edges(S.dev(0), DP, S.dev<const Vp8LfEdge>(hdr), nplanes, 0) < 0 || !S.down())
        return false;
    for (int p = 0; p < nplanes; p++)
        S.commit(d[p], org[p]);
    return true;
}
template <int KIND, int DIR>
static void s_lf16(uint8_t *d, ptrdiff_t s, int E, int I, int H)
{
    uint8_t *pl[1] = { d };
    if (!vp8_lf_single(KIND, DIR, 16, pl, 1, s, E, I, H)) {
        if (KIND == VP8_LF_MBEDGE) {
            if (DIR) SHIM_FB(g_fb_vp8, vp8_v_loop_filter16y, d, s, E, I, H);
            else     SHIM_FB(g_fb_vp8, vp8_h_loop_filter16y, d, s, E, I, H);
        } else {
            if (DIR) SHIM_FB(g_fb_vp8, vp8_v_loop_filter16y_inner, d, s, E, I, H);
            else     SHIM_FB(g_fb_vp8, vp8_h_loop_filter16y_inner, d, s, E, I, H);
        }
    }
}
template <int KIND, int DIR>
static void s_lf8uv(uint8_t *u, uint8_t *v, ptrdiff_t s, int E, int I, int H)
{
    uint8_t *pl[2] = { u, v };
    if (!vp8_lf_single(KIND, DIR, 8, pl, 2, s, E, I, H)) {
        if (KIND == VP8_LF_MBEDGE) {
            if (DIR) SHIM_FB(g_fb_vp8, vp8_v_loop_filter8uv, u, v, s, E, I, H);
            else     SHIM_FB(g_fb_vp8, vp8_h_loop_filter8uv, u, v, s, E, I, H);
        } else {
            if (DIR) SHIM_FB(g_fb_vp8, vp8_v_loop_filter8uv_inner, u, v, s, E, I, H);
            else     SHIM_FB(g_fb_vp8, vp8_h_loop_filter8uv_inner, u, v, s, E, I, H);
        }
    }
}
template <int DIR>
static void s_lf_simple(uint8_t *d, ptrdiff_t s, int E)
{
    uint8_t *pl[1] = { d };
    if (!vp8_lf_single(VP8_LF_SIMPLE, DIR, 16, pl, 1, s, E, 0, 0)) {
        if (DIR) SHIM_FB(g_fb_vp8, vp8_v_loop_filter_simple, d, s, E);
        else     SHIM_FB(g_fb_vp8, vp8_h_loop_filter_simple, d, s, E);
    }
}

/* ---- MC: the source rows / columns the slot reads, at a pitch of 64, and the w x h destination at DP ---- */
static bool vp8_mc_single(int bil, int W, int vt, int ht, uint8_t *dst, ptrdiff_t ds, const uint8_t *src, ptrdiff_t ss, int h, int mx, int my)
{
    const int lo = bil ? 0 : 1;
    if (h < 1 || h > 2 * W || (ht && (mx < lo || mx > 7)) || (vt && (my < lo || my > 7)))
        return false; /* outside the reference's range (its temporary, subpel_filters[]): the C function's */
    auto before = [&](int t) { return !t || bil ? 0 : t == 2 ? 2 : 1; };
    auto after = [&](int t) { return !t ? 0 : bil ? 1 : t == 2 ? 3 : 2; };
    const int y0 = -before(vt), y1 = h - 1 + after(vt), x0 = -before(ht), x1 = W - 1 + after(ht);
    const int SP = 64;
    Stage S;
    const size_t hdr = S.hole(sizeof(FFHipVp8McRec)), sv = S.hole((size_t)(y1 - y0 + 1) * SP);
    const size_t dv = S.hole((size_t)h * DP);
    S.put2d_at(sv, SP, src + y0 * ss + x0, ss, (size_t)(x1 - x0 + 1), y1 - y0 + 1);
    FFHipVp8McRec &k = *S.img<FFHipVp8McRec>(hdr);
    k.dst_offset = (int32_t)dv;
    k.src_offset = (int32_t)(sv - (ptrdiff_t)y0 * SP - x0);
    k.width = (uint8_t)W; k.h = (uint8_t)h; k.mx = (uint8_t)(ht ? mx : 0); k.my = (uint8_t)(vt ? my : 0);
    k.htaps = (uint8_t)ht; k.vtaps = (uint8_t)vt; k.bilinear = (uint8_t)bil;
    if (!S.up() || ffhip_launch_vp8_mc(S.dev(0), DP, S.dev(0), SP, S.dev<const FFHipVp8McRec>(hdr), 1, 0) < 0 || !S.down())
        return false;
    S.get2d(dst, ds, dv, DP, (size_t)W, h);
    return true;
}
template <int BIL, int IDX, int V, int H>
static void s_mc(uint8_t *d, ptrdiff_t ds, const uint8_t *s, ptrdiff_t ss, int h, int mx, int my)
{
    constexpr int W = 16 >> IDX;
    /* the bilinear table's slots 1 and 2 are one function */
    if (!vp8_mc_single(BIL, W, BIL && V ? 1 : V, BIL && H ? 1 : H, d, ds, s, ss, h, mx, my)) {
        if (BIL) SHIM_FB(g_fb_vp8, put_vp8_bilinear_pixels_tab[IDX][V][H], d, ds, s, ss, h, mx, my);
        else     SHIM_FB(g_fb_vp8, put_vp8_epel_pixels_tab[IDX][V][H], d, ds, s, ss, h, mx, my);
    }
}
template <int BIL, int IDX>
static void vp8_mc_fill(ffhip_vp8_mc_func (&t)[3][3][3])
{
    t[IDX][0][0] = s_mc<BIL, IDX, 0, 0>; t[IDX][0][1] = s_mc<BIL, IDX, 0, 1>; t[IDX][0][2] = s_mc<BIL, IDX, 0, 2>;
    t[IDX][1][0] = s_mc<BIL, IDX, 1, 0>; t[IDX][1][1] = s_mc<BIL, IDX, 1, 1>; t[IDX][1][2] = s_mc<BIL, IDX, 1, 2>;
    t[IDX][2][0] = s_mc<BIL, IDX, 2, 0>; t[IDX][2][1] = s_mc<BIL, IDX, 2, 1>; t[IDX][2][2] = s_mc<BIL, IDX, 2, 2>;
}

extern "C" int ff_vp78dsp_init_hip(FFHipVP8DSPContext *c)
{
    if (!c)
        return FFHIP_EINVAL;
    if (!ffhip_have_device())
        return FFHIP_ENOSYS;
    FFHipVP8DSPContext o = *c;
    vp8_mc_fill<0, 0>(o.put_vp8_epel_pixels_tab); vp8_mc_fill<0, 1>(o.put_vp8_epel_pixels_tab); vp8_mc_fill<0, 2>(o.put_vp8_epel_pixels_tab);
    vp8_mc_fill<1, 0>(o.put_vp8_bilinear_pixels_tab); vp8_mc_fill<1, 1>(o.put_vp8_bilinear_pixels_tab);
    vp8_mc_fill<1, 2>(o.put_vp8_bilinear_pixels_tab);
    fb_snapshot(g_fb_vp8, *c, o);
    *c = o;
    return 0;
}

extern "C" int ff_vp8dsp_init_hip(FFHipVP8DSPContext *c)
{
    if (!c)
        return FFHIP_EINVAL;
    if (!ffhip_have_device())
        return FFHIP_ENOSYS;
    FFHipVP8DSPContext o = *c;
    o.vp8_luma_dc_wht = s_wht;
    o.vp8_luma_dc_wht_dc = s_wht_dc;
    o.vp8_idct_add = s_idct_add;
    o.vp8_idct_dc_add = s_idct_dc_add;
    o.vp8_idct_dc_add4y = s_idct_dc_add4y;
    o.vp8_idct_dc_add4uv = s_idct_dc_add4uv;
    o.vp8_v_loop_filter16y = s_lf16<VP8_LF_MBEDGE, 1>;
    o.vp8_h_loop_filter16y = s_lf16<VP8_LF_MBEDGE, 0>;
    o.vp8_v_loop_filter8uv = s_lf8uv<VP8_LF_MBEDGE, 1>;
    o.vp8_h_loop_filter8uv = s_lf8uv<VP8_LF_MBEDGE, 0>;
    o.vp8_v_loop_filter16y_inner = s_lf16<VP8_LF_INNER, 1>;
    o.vp8_h_loop_filter16y_inner = s_lf16<VP8_LF_INNER, 0>;
    o.vp8_v_loop_filter8uv_inner = s_lf8uv<VP8_LF_INNER, 1>;
    o.vp8_h_loop_filter8uv_inner = s_lf8uv<VP8_LF_INNER, 0>;
    o.vp8_v_loop_filter_simple = s_lf_simple<1>;
    o.vp8_h_loop_filter_simple = s_lf_simple<0>;
    fb_snapshot(g_fb_vp8, *c, o);
    *c = o;
    return 0;
}

/* ---- batch device faces ---- */
extern "C" int ffhip_vp8_wht_record_size(void) { return (int)sizeof(FFHipVp8WhtRec); }
extern "C" int ffhip_vp8_idct_record_size(void) { return (int)sizeof(FFHipVp8IdctRec); }
extern "C" int ffhip_vp8_mc_record_size(void) { return (int)sizeof(FFHipVp8McRec); }

static bool vp8_stride_ok(ptrdiff_t s) { return s != 0 && s <= (1 << 24) && s >= -(1 << 24); }

extern "C" int ffhip_vp8_luma_dc_wht_batch_dev(int16_t *coeffs, const FFHipVp8WhtRec *recs, int n, void *stream)
{
    if (!coeffs || !recs || n < 0 || ((uintptr_t)coeffs & 1)) {
        ffhip_set_error("ffhip_vp8_luma_dc_wht_batch_dev: NULL or odd pointer, or n = %d < 0", n);
        return FFHIP_EINVAL;
    }
    if (!ffhip_have_device())
        return FFHIP_ENOSYS;
    return ffhip_launch_vp8_wht(coeffs, recs, n, (hipStream_t)stream);
}

extern "C" int ffhip_vp8_idct_add_batch_dev(uint8_t *dst, ptrdiff_t stride, int16_t *coeffs, const FFHipVp8IdctRec *recs, int n, void *stream)
{
    if (!dst || !coeffs || !recs || n < 0 || ((uintptr_t)coeffs & 1) || !vp8_stride_ok(stride)) {
        ffhip_set_error("ffhip_vp8_idct_add_batch_dev: NULL or odd pointer, stride %td, or n = %d < 0", stride, n);
        return FFHIP_EINVAL;
    }
    if (!ffhip_have_device())
        return FFHIP_ENOSYS;
    return ffhip_launch_vp8_idct(dst, stride, coeffs, recs, n, (hipStream_t)stream);
}

extern "C" int ffhip_vp8_mc_batch_dev(uint8_t *dst, ptrdiff_t dststride, const uint8_t *src, ptrdiff_t srcstride, const FFHipVp8McRec *recs,
                                      int n, void *stream)
{
    if (!dst || !src || !recs || n < 0 || !vp8_stride_ok(dststride) || !vp8_stride_ok(srcstride)) {
        ffhip_set_error("ffhip_vp8_mc_batch_dev: NULL pointer, strides %td / %td, or n = %d < 0", dststride, srcstride, n);
        return FFHIP_EINVAL;
    }
    if (!ffhip_have_device())
        return FFHIP_ENOSYS;
    return ffhip_launch_vp8_mc(dst, dststride, src, srcstride, recs, n, (hipStream_t)stream);
}

/* ---- the whole-frame loop filter ---- */
extern "C" int ffhip_vp8_loopfilter_frames_dev(int filter_type, int keyframe, int mb_w, int mb_h, int npics, const FFHipVp8LfPic *pics,
                                               ptrdiff_t stride_y, ptrdiff_t stride_uv, void *stream)
{
    static const char who[] = "ffhip_vp8_loopfilter_frames_dev";
    if ((filter_type & ~1) || (keyframe & ~1) || mb_w < 1 || mb_w > 1024 || mb_h < 1 || mb_h > 1024) {
        ffhip_set_error("%s: filter type %d, keyframe %d (0 or 1 each), %d x %d macroblocks (1..1024)", who, filter_type, keyframe, mb_w, mb_h);
        return FFHIP_EINVAL;
    }
    if (const int r = ffhip_check_count(who, npics, pics, "frame"))
        return r;
    const bool normal = filter_type == 0;
    if ((stride_y & 3) || stride_y < 16 * mb_w || (normal && ((stride_uv & 3) || stride_uv < 8 * mb_w))) {
        ffhip_set_error("%s: strides %td / %td must be multiples of 4 and at least the planes' widths", who, stride_y, stride_uv);
        return FFHIP_EINVAL;
    }
    FFHipSpanSet planes;
    for (int i = 0; i < npics; i++) {
        const FFHipVp8LfPic &P = pics[i];
        uint8_t *const pl[3] = { P.y, P.u, P.v };
        if (!P.strength) {
            ffhip_set_error("%s: frame %d: a NULL record array", who, i);
            return FFHIP_EINVAL;
        }
        for (int p = 0; p < (normal ? 3 : 1); p++) {
            if (!pl[p] || ((uintptr_t)pl[p] & 3)) {
                ffhip_set_error("%s: frame %d plane %d: NULL, or not 4-byte aligned", who, i, p);
                return FFHIP_EINVAL;
            }
            planes.add(ffhip_plane_span(pl[p], p ? stride_uv : stride_y, (p ? 8 : 16) * mb_w, (p ? 8 : 16) * mb_h));
        }
    }
    /* the frames of a launch are filtered side by side: no two planes may share a byte */
    if (planes.seal()) {
        ffhip_set_error("%s: two planes of the call overlap", who);
        return FFHIP_EINVAL;
    }
    if (!ffhip_have_device())
        return FFHIP_ENOSYS;
    return ffhip_launch_vp8_lf_frames(filter_type, keyframe, mb_w, mb_h, npics, pics, stride_y, stride_uv, (hipStream_t)stream);
}
