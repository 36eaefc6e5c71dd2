/*
 * tools/h264_fmt_host_san.cpp — a stand-alone host program over ffhip_h264_inter_pictures_fmt_host() and
 * ffhip_h264_residual_pictures_fmt_host() and the argument checks of their _fmt_dev twins at chroma_format_idc 0 .. 3, for
 * AddressSanitizer and UBSan: well-formed random pictures and pictures whose records are random bytes throughout (slice indices,
 * ref_idx, num_ref, slots, denominators, vectors anywhere in int16_t, offsets negative, unaligned and past the end, chroma bits and
 * nnz444 of every value), with planes, maps and coeffs in heap blocks exactly as large as the geometry, the format and ncoeffs say,
 * so a read or write outside one of them is an error the sanitizer reports and a signed overflow or a bad shift one UBSan reports.
 * CPU only: nothing here touches a device.
 *
 * Build and run from the repository root (the two faces' files and this one, nothing else of the library):
 *   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
 *         --offload-arch=gfx950 -Iinclude -Iffmpeg_amd/csrc -Iffmpeg_amd/csrc/host ffmpeg_amd/csrc/shims_h264_inter.hip \
 *         ffmpeg_amd/csrc/shims_h264_res.hip tools/h264_fmt_host_san.cpp -o h264_fmt_host_san && ./h264_fmt_host_san
 * Prints a checksum of the planes per case and "ok"; the sanitizer aborts on the first finding.
 */
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ffhip.h"

/* what the two shim files take from the rest of the library */
static bool quiet;
extern "C" void ffhip_set_error(const char *fmt, ...)
{
    if (quiet)
        return;
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
}
int ffhip_have_device(void) { return 0; }
struct ihipStream_t;
int ffhip_launch_h264_inter_pictures(int, int, int, int, int, const FFHipH264InterPic *, ihipStream_t *) { return FFHIP_ENOSYS; }
int ffhip_launch_h264_residual_pictures(int, int, int, int, int, const FFHipH264ResPic *, ihipStream_t *) { return FFHIP_ENOSYS; }

static uint32_t rnd_state = 24680;
static uint32_t rnd(void)
{
    rnd_state = rnd_state * 1664525u + 1013904223u;
    return rnd_state >> 8;
}
static void noise(void *p, size_t n)
{
    for (size_t i = 0; i < n; i++)
        static_cast<uint8_t *>(p)[i] = (uint8_t)rnd();
}
/* n bytes on a 16-byte boundary, exactly: the byte after them is the sanitizer's */
static uint8_t *block(size_t n)
{
    void *p = nullptr;
    if (posix_memalign(&p, 16, n ? n : 1))
        abort();
    return static_cast<uint8_t *>(p);
}

/* the planes of a format: width and height of plane p in samples */
static int plane_w(int cfi, int mb_w, int p) { return mb_w * (p && cfi != 3 ? 8 : 16); }
static int plane_h(int cfi, int mb_h, int p) { return mb_h * (p && cfi < 2 ? 8 : 16); }

/* a plane of samples below 1 << bd whose last row ends with the block */
static uint8_t *plane(int bd, int w, int h, int pad, ptrdiff_t *stride, size_t *bytes)
{
    const int ps = bd > 8 ? 2 : 1;
    *stride = (ptrdiff_t)(w + 4 * pad) * ps;
    *bytes = (size_t)(h - 1) * *stride + (size_t)w * ps;
    uint8_t *b = block(*bytes);
    for (size_t i = 0; i < *bytes; i += ps) {
        const uint16_t v = (uint16_t)(rnd() & ((1u << bd) - 1));
        memcpy(b + i, &v, ps);
    }
    return b;
}
static int checksum(const char *what, int bd, int cfi, int mb_w, int mb_h, int wild, int rc, uint8_t *const *dst, const size_t *bytes)
{
    const int ps = bd > 8 ? 2 : 1;
    uint32_t sum = 0;
    int bad = rc != 0;
    for (int p = 0; p < 3; p++)
        for (size_t i = 0; dst[p] && i < bytes[p]; i += ps) {
            uint16_t v = 0;
            memcpy(&v, dst[p] + i, ps);
            sum = sum * 31 + v;
            bad |= v >> bd;                             /* every result is clipped, and the rest was drawn below the limit */
        }
    printf("%s: %d bits cfi %d %d x %d wild %d: rc %d checksum %08x\n", what, bd, cfi, mb_w, mb_h, wild, rc, sum);
    return bad;
}

static int run_inter(int bd, int cfi, int mb_w, int mb_h, int pad, bool wild, bool luma_only)
{
    const size_t nmb = (size_t)mb_w * mb_h;
    const bool has_c = cfi && !luma_only;
    const int nrefs = (int)(rnd() % 5), nslices = 1 + (int)(rnd() % 3), extra = (int)(rnd() % 3);
    FFHipH264InterPic pic;
    memset(&pic, 0, sizeof(pic));
    size_t bytes[3] = { 0, 0, 0 }, rb;
    uint8_t *refs[32][3] = {};
    for (int p = 0; p < (has_c ? 3 : 1); p++) {
        pic.dst[p] = plane(bd, plane_w(cfi, mb_w, p), plane_h(cfi, mb_h, p), pad, &pic.dst_stride[p], &bytes[p]);
        for (int k = 0; k < nrefs; k++)
            pic.ref[k].base[p] = refs[k][p] = plane(bd, plane_w(cfi, mb_w, p), plane_h(cfi, mb_h, p), (pad + k) % 3, &pic.ref[k].stride[p], &rb);
    }
    for (int k = 0; k < 32; k++)
        pic.ref[k].chroma_dy = (int8_t)rnd();
    FFHipH264BsMb *mb = reinterpret_cast<FFHipH264BsMb *>(block(nmb * sizeof(FFHipH264BsMb)));
    FFHipH264InterSlice *slices = reinterpret_cast<FFHipH264InterSlice *>(block((size_t)nslices * sizeof(FFHipH264InterSlice)));
    pic.mvf_stride = 4 * mb_w + extra;
    const size_t nmv = (size_t)(4 * mb_h - 1) * pic.mvf_stride + 4 * mb_w;     /* the last row ends with the picture */
    FFHipH264MvField *mvf = reinterpret_cast<FFHipH264MvField *>(block(nmv * sizeof(FFHipH264MvField)));
    noise(mb, nmb * sizeof(*mb));
    noise(slices, (size_t)nslices * sizeof(*slices));
    noise(mvf, nmv * sizeof(*mvf));
    if (!wild) {    /* well formed: every block predicts, from slots that exist, with weights of every kind */
        for (size_t i = 0; i < nmb; i++) {
            mb[i].flags = (uint8_t)(rnd() % 8 == 0);
            mb[i].slice = (uint16_t)(rnd() % nslices);
        }
        for (int s = 0; s < nslices; s++) {
            slices[s].use_weight = (uint8_t)(rnd() % 3);
            slices[s].luma_log2_denom = (uint8_t)(rnd() % 8);
            slices[s].chroma_log2_denom = (uint8_t)(rnd() % 8);
            for (int l = 0; l < 2; l++) {
                slices[s].num_ref[l] = (uint8_t)(1 + rnd() % 32);
                for (int r = 0; r < 32; r++)
                    slices[s].ref[l][r] = (uint8_t)(nrefs ? rnd() % nrefs : 0);
            }
        }
        for (size_t i = 0; i < nmv; i++)
            for (int l = 0; l < 2; l++) {
                mvf[i].ref_idx[l] = (int8_t)(rnd() % 3 ? rnd() % 4 : -1);
                if (rnd() % 4)
                    for (int c = 0; c < 2; c++)
                        mvf[i].mv[l][c] = (int16_t)((int)(rnd() % 257) - 128);
            }
    }
    pic.mb = mb; pic.mvf = mvf; pic.slices = slices; pic.nslices = nslices; pic.nrefs = nrefs;
    const int r = ffhip_h264_inter_pictures_fmt_host(bd, cfi, mb_w, mb_h, 1, &pic);
    const int bad = checksum("inter", bd, cfi, mb_w, mb_h, wild, r, pic.dst, bytes);
    for (int p = 0; p < 3; p++) {
        free(pic.dst[p]);
        for (int k = 0; k < nrefs; k++)
            free(refs[k][p]);
    }
    free(mb); free(slices); free(mvf);
    return bad;
}

static int run_res(int bd, int cfi, int mb_w, int mb_h, int pad, bool wild, bool luma_only)
{
    const size_t nmb = (size_t)mb_w * mb_h;
    const int cs = bd > 8 ? 4 : 2;
    const bool has_c = cfi && !luma_only;
    FFHipH264ResPic pic;
    memset(&pic, 0, sizeof(pic));
    size_t bytes[3] = { 0, 0, 0 };
    for (int p = 0; p < (has_c ? 3 : 1); p++)
        pic.dst[p] = plane(bd, plane_w(cfi, mb_w, p), plane_h(cfi, mb_h, p), pad, &pic.dst_stride[p], &bytes[p]);
    FFHipH264BsMb *mb = reinterpret_cast<FFHipH264BsMb *>(block(nmb * sizeof(FFHipH264BsMb)));
    FFHipH264ResMb *res = reinterpret_cast<FFHipH264ResMb *>(block(nmb * sizeof(FFHipH264ResMb)));
    noise(mb, nmb * sizeof(*mb));
    noise(res, nmb * sizeof(*res));
    int64_t ncoeffs = 0;
    for (size_t i = 0; i < nmb; i++) {
        if (rnd() % 4 == 0)
            mb[i].nnz = 0;
        if (rnd() % 3 == 0) {
            res[i].chroma = res[i].chroma_dc = res[i].chroma_lo422 = 0;
            if (cfi == 3)
                res[i].nnz444[0] = res[i].nnz444[1] = rnd() << 16;      /* only the high halves, which are not read */
        }
        if (wild) {
            if (rnd() % 2)
                res[i].coeff_offset = (int32_t)(rnd() % 4096) - 512;
            continue;
        }
        mb[i].flags = (uint8_t)(rnd() % 8 == 0) | (uint8_t)((rnd() % 3 == 0) << 1);
        const bool c = has_c && (cfi == 3 ? ((res[i].nnz444[0] | res[i].nnz444[1]) & 0xFFFF) != 0
                                          : (res[i].chroma | res[i].chroma_dc | (cfi == 2 ? res[i].chroma_lo422 : 0)) != 0);
        res[i].coeff_offset = (int32_t)ncoeffs;
        ncoeffs += c ? 768 : mb[i].nnz ? 256 : 0;       /* exactly what the rules say the macroblock needs */
    }
    if (wild)
        ncoeffs = 16 * (int64_t)(rnd() % 160);
    uint8_t *coeffs = block((size_t)ncoeffs * cs);
    noise(coeffs, (size_t)ncoeffs * cs);                /* every value of int16_t / int32_t */
    pic.mb = mb; pic.res = res; pic.coeffs = coeffs; pic.ncoeffs = ncoeffs;
    const int r = ffhip_h264_residual_pictures_fmt_host(bd, cfi, mb_w, mb_h, 1, &pic);
    const int bad = checksum("residual", bd, cfi, mb_w, mb_h, wild, r, pic.dst, bytes);
    for (int p = 0; p < 3; p++)
        free(pic.dst[p]);
    free(mb); free(res); free(coeffs);
    return bad;
}

/* the _fmt_dev faces' checks: pointers into one arena that is never dereferenced */
static int refusals(void)
{
    static uint8_t arena[1 << 22];
    static FFHipH264InterPic ip[2];
    FFHipH264ResPic rp[2];
    int bad = 0;
    auto fill = [&](int cfi, int mb_w, int mb_h, int ps) {
        uint8_t *at = arena;
        auto take = [&](size_t bytes) { uint8_t *p = at; at += (bytes + 63) & ~(size_t)63; return p; };
        memset(ip, 0, sizeof(ip));
        memset(rp, 0, sizeof(rp));
        for (int i = 0; i < 2; i++) {
            for (int p = 0; p < 3; p++) {
                const ptrdiff_t s = (ptrdiff_t)plane_w(cfi, mb_w, p) * ps;
                const size_t n = (size_t)s * plane_h(cfi, mb_h, p);
                ip[i].dst_stride[p] = rp[i].dst_stride[p] = ip[i].ref[0].stride[p] = s;
                ip[i].dst[p] = rp[i].dst[p] = take(n);
                ip[i].ref[0].base[p] = take(n);
            }
            ip[i].mb = rp[i].mb = reinterpret_cast<const FFHipH264BsMb *>(take(4096));
            ip[i].mvf = reinterpret_cast<const FFHipH264MvField *>(take(16384));
            ip[i].slices = reinterpret_cast<const FFHipH264InterSlice *>(take(4096));
            ip[i].mvf_stride = 4 * mb_w; ip[i].nslices = 1; ip[i].nrefs = 1;
            rp[i].res = reinterpret_cast<const FFHipH264ResMb *>(take(4096));
            rp[i].coeffs = take(16384);
            rp[i].ncoeffs = 16384 / (2 * ps);
        }
    };
    auto expect = [&](int want, int bd, int cfi, int w, int h, const char *what) {
        const int a = ffhip_h264_inter_pictures_fmt_dev(bd, cfi, w, h, 2, ip, nullptr);
        const int b = ffhip_h264_residual_pictures_fmt_dev(bd, cfi, w, h, 2, rp, nullptr);
        if (a != want || b != want) {
            printf("refusals: %s: rc %d / %d, expected %d\n", what, a, b, want);
            bad = 1;
        }
    };
    quiet = true;
    for (int cfi = 0; cfi < 4; cfi++) {
        fill(cfi, 3, 2, 1); expect(FFHIP_ENOSYS, 8, cfi, 3, 2, "two pictures");
        fill(cfi, 3, 2, 2); expect(FFHIP_ENOSYS, 14, cfi, 3, 2, "16-bit samples");
        fill(cfi, 3, 2, 1); expect(FFHIP_EINVAL, 11, cfi, 3, 2, "depth 11");
        fill(cfi, 3, 2, 1); expect(FFHIP_EINVAL, 8, cfi, 4097, 2, "mb_w 4097");
        if (!cfi)
            continue;
        fill(cfi, 3, 2, 1); ip[1].dst[2] = rp[1].dst[2] = nullptr; expect(FFHIP_EINVAL, 8, cfi, 3, 2, "Cr alone missing");
        fill(cfi, 3, 2, 1); ip[0].dst_stride[1] -= 4; rp[0].dst_stride[1] -= 4; expect(FFHIP_EINVAL, 8, cfi, 3, 2, "a Cb stride below the format's width");
        /* the last byte of the format's last Cb row of picture 0 is picture 1's Cr */
        fill(cfi, 3, 2, 1);
        ip[1].dst[2] = rp[1].dst[2] = ip[0].dst[1] + (ptrdiff_t)(plane_h(cfi, 2, 1) - 1) * ip[0].dst_stride[1] + plane_w(cfi, 3, 1) - 4;
        expect(FFHIP_EINVAL, 8, cfi, 3, 2, "a plane that begins inside another's last row");
    }
    fill(1, 3, 2, 1); expect(FFHIP_EINVAL, 8, -1, 3, 2, "chroma_format_idc -1");
    fill(1, 3, 2, 1); expect(FFHIP_EINVAL, 8, 4, 3, 2, "chroma_format_idc 4");
    fill(1, 3, 2, 1); expect(FFHIP_EINVAL, 8, 3, 3, 2, "4:2:0 planes handed to 4:4:4");
    quiet = false;
    return bad;
}

int main(void)
{
    static const int depths[5] = { 8, 9, 10, 12, 14 };
    int bad = 0;
    for (int k = 0; k < 64; k++) {
        const int mb_w = 1 + (int)(rnd() % 7), mb_h = 1 + (int)(rnd() % 5), pad = (int)(rnd() % 3);
        bad |= run_inter(depths[k % 5], k % 4, mb_w, mb_h, pad, k >= 24, k % 11 == 3);
        bad |= run_res(depths[k % 5], k % 4, mb_w, mb_h, pad, k >= 24, k % 11 == 3);
    }
    for (int cfi = 2; cfi < 4; cfi++) {
        bad |= run_inter(8, cfi, 30, 17, 0, false, false);
        bad |= run_res(10, cfi, 30, 17, 1, false, false);
        bad |= run_res(8, cfi, 30, 17, 0, true, false);
    }
    bad |= refusals();
    puts(bad ? "FAILED" : "ok");
    return bad;
}
