/*
 * tools/h264_res_host_san.cpp — a stand-alone host program over ffhip_h264_residual_pictures_host() and the argument checks of
 * ffhip_h264_residual_pictures_dev() for AddressSanitizer and UBSan: random and malformed pictures (every byte of the records random:
 * offsets negative, unaligned and past the end, chroma bits without chroma planes, coefficients and qmul of every value) in heap
 * blocks exactly as large as the geometry and ncoeffs say, so a read or write outside a plane, a map or coeffs is an error the
 * sanitizer reports, and a signed overflow in the arithmetic one UBSan reports; then the refusals and the row-overlap rule of the _dev
 * face on pointers it never follows.  CPU only: nothing here touches a device.
 *
 * Build and run from the repository root (the face's file and this one, nothing else of the library):
 *   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
 *         --offload-arch=gfx950 -Iinclude -Iffmpeg_amd/csrc -Iffmpeg_amd/csrc/host ffmpeg_amd/csrc/shims_h264_res.hip \
 *         tools/h264_res_host_san.cpp -o h264_res_host_san && ./h264_res_host_san
 * Prints a checksum of the planes per case and "ok"; the sanitizer aborts on the first finding.
 */
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ffhip.h"

/* what shims_h264_res.hip takes from the rest of the library */
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
int ffhip_launch_h264_residual_pictures(int, int, int, int, int, const FFHipH264ResPic *, ihipStream_t *) { return FFHIP_ENOSYS; }

static uint32_t rnd_state = 97531;
static uint32_t rnd(void)
{
    rnd_state = rnd_state * 1664525u + 1013904223u;
    return rnd_state >> 8;
}

/* n bytes on a 16-byte boundary, exactly: the byte after them is the sanitizer's */
static uint8_t *block(size_t n)
{
    void *p = nullptr;
    if (posix_memalign(&p, 16, n ? n : 1))
        abort();
    return static_cast<uint8_t *>(p);
}

static int run(int bd, int cfi, int mb_w, int mb_h, int pad, bool malformed, bool mono_by_null)
{
    const size_t nmb = (size_t)mb_w * mb_h;
    const int ps = bd > 8 ? 2 : 1, cs = 2 * ps;
    const bool has_c = cfi && !mono_by_null;
    FFHipH264ResPic pic;
    memset(&pic, 0, sizeof(pic));
    size_t bytes[3] = { 0, 0, 0 };
    for (int p = 0; p < (has_c ? 3 : 1); p++) {
        const int w = mb_w * (p ? 8 : 16), h = mb_h * (p ? 8 : 16);
        pic.dst_stride[p] = (ptrdiff_t)(w + 4 * pad) * ps;
        bytes[p] = (size_t)(h - 1) * pic.dst_stride[p] + (size_t)w * ps;     /* the last row ends with the picture */
        pic.dst[p] = block(bytes[p]);
        for (size_t i = 0; i < bytes[p]; i += ps) {
            const uint16_t v = (uint16_t)(rnd() & ((1u << bd) - 1));
            memcpy(pic.dst[p] + i, &v, ps);
        }
    }
    FFHipH264BsMb *mb = reinterpret_cast<FFHipH264BsMb *>(block(nmb * sizeof(FFHipH264BsMb)));
    FFHipH264ResMb *res = reinterpret_cast<FFHipH264ResMb *>(block(nmb * sizeof(FFHipH264ResMb)));
    /* well formed: every macroblock gets the space it needs, back to back; malformed: the records are noise over a small coeffs */
    int64_t ncoeffs = 0;
    for (size_t i = 0; i < nmb; i++) {
        uint8_t *raw = reinterpret_cast<uint8_t *>(&mb[i]);
        for (size_t k = 0; k < sizeof(mb[i]); k++)
            raw[k] = (uint8_t)rnd();
        raw = reinterpret_cast<uint8_t *>(&res[i]);
        for (size_t k = 0; k < sizeof(res[i]); k++)
            raw[k] = (uint8_t)rnd();
        if (rnd() % 4 == 0)
            mb[i].nnz = 0;
        if (rnd() % 3 == 0)
            res[i].chroma = res[i].chroma_dc = 0;
        if (malformed) {
            if (rnd() % 2)
                res[i].coeff_offset = (int32_t)(rnd() % 4096) - 512;
            continue;
        }
        mb[i].flags = (uint8_t)(rnd() % 8 == 0) | (uint8_t)((rnd() % 3 == 0) << 1);
        const int need = has_c && (res[i].chroma | res[i].chroma_dc) ? 768 : mb[i].nnz ? 256 : 0;
        res[i].coeff_offset = (int32_t)ncoeffs;
        ncoeffs += need;
    }
    if (malformed)
        ncoeffs = 16 * (int64_t)(rnd() % 160);
    uint8_t *coeffs = block((size_t)ncoeffs * cs);
    for (size_t i = 0; i < (size_t)ncoeffs * cs; i++)
        coeffs[i] = (uint8_t)rnd();                     /* every value of int16_t / int32_t */
    pic.mb = mb; pic.res = res; pic.coeffs = coeffs; pic.ncoeffs = ncoeffs;
    const int r = ffhip_h264_residual_pictures_host(bd, cfi, mb_w, mb_h, 1, &pic);
    uint32_t sum = 0;
    int bad = r != 0;
    for (int p = 0; p < 3; p++)
        for (size_t i = 0; i < bytes[p]; i += ps) {
            uint16_t v = 0;
            memcpy(&v, pic.dst[p] + i, ps);
            sum = sum * 31 + v;
            bad |= v >> bd;                             /* rule 11, and the padding was drawn below the limit too */
        }
    printf("%d bits cfi %d %d x %d pad %d malformed %d: rc %d ncoeffs %lld checksum %08x\n", bd, cfi, mb_w, mb_h, pad, (int)malformed, r,
           (long long)ncoeffs, sum);
    for (int p = 0; p < 3; p++)
        free(pic.dst[p]);
    free(mb); free(res); free(coeffs);
    return bad;
}

/* the _dev face's checks: pointers into one arena that is never dereferenced */
static int refusals(void)
{
    static uint8_t arena[1 << 20];
    FFHipH264ResPic pics[3];
    int bad = 0;
    auto fill = [&](int n, int mb_w, int ps) {
        uint8_t *at = arena;
        auto take = [&](size_t bytes) { uint8_t *p = at; at += (bytes + 63) & ~(size_t)63; return p; };
        memset(pics, 0, sizeof(pics));
        for (int i = 0; i < n; i++) {
            for (int p = 0; p < 3; p++) {
                pics[i].dst_stride[p] = (ptrdiff_t)(p ? 8 : 16) * mb_w * ps;
                pics[i].dst[p] = take((size_t)pics[i].dst_stride[p] * 64);
            }
            pics[i].mb = reinterpret_cast<const FFHipH264BsMb *>(take(4096));
            pics[i].res = reinterpret_cast<const FFHipH264ResMb *>(take(4096));
            pics[i].coeffs = take(16384);
            pics[i].ncoeffs = 16384 / (2 * ps);
        }
    };
    auto expect = [&](int want, int bd, int cfi, int w, int h, int n, const char *what) {
        const int r = ffhip_h264_residual_pictures_dev(bd, cfi, w, h, n, pics, nullptr);
        if (r != want) {
            printf("refusals: %s: rc %d, expected %d\n", what, r, want);
            bad = 1;
        }
    };
    quiet = true;
    fill(3, 2, 1); expect(FFHIP_ENOSYS, 8, 1, 2, 2, 3, "three pictures");
    fill(3, 2, 2); expect(FFHIP_ENOSYS, 14, 1, 2, 2, 3, "16-bit samples");
    fill(1, 2, 1); expect(FFHIP_ENOSYS, 8, 0, 2, 2, 1, "monochrome");
    fill(1, 2, 1); expect(FFHIP_ENOSYS, 8, 3, 2, 2, 1, "4:4:4");
    fill(1, 2, 1); expect(FFHIP_EINVAL, 11, 1, 2, 2, 1, "depth 11");
    fill(1, 2, 1); expect(FFHIP_EINVAL, 8, 1, 4097, 2, 1, "mb_w 4097");
    fill(1, 2, 1); expect(FFHIP_EINVAL, 8, 1, 2, 2, 0, "npics 0");
    fill(1, 2, 1); pics[0].dst[2] = nullptr; expect(FFHIP_EINVAL, 8, 1, 2, 2, 1, "Cr alone missing");
    fill(1, 2, 1); pics[0].res = reinterpret_cast<const FFHipH264ResMb *>(reinterpret_cast<const uint8_t *>(pics[0].res) + 2);
    expect(FFHIP_EINVAL, 8, 1, 2, 2, 1, "a misaligned res");
    fill(1, 2, 1); pics[0].coeffs = static_cast<const uint8_t *>(pics[0].coeffs) + 8; expect(FFHIP_EINVAL, 8, 1, 2, 2, 1, "a misaligned coeffs");
    fill(1, 2, 1); pics[0].ncoeffs = -1; expect(FFHIP_EINVAL, 8, 1, 2, 2, 1, "a negative ncoeffs");
    fill(1, 2, 1); pics[0].ncoeffs = INT64_MAX; expect(FFHIP_ENOSYS, 8, 1, 2, 2, 1, "the largest ncoeffs");
    fill(2, 2, 1); pics[1].coeffs = pics[0].dst[1] + 16; expect(FFHIP_EINVAL, 8, 1, 2, 2, 2, "coeffs inside another picture's destination");
    fill(2, 2, 1); pics[1].mb = reinterpret_cast<const FFHipH264BsMb *>(pics[0].dst[0] + 2); expect(FFHIP_EINVAL, 8, 1, 2, 2, 2, "mb inside a destination");
    fill(2, 2, 1); /* the two fields of one frame as two pictures of the call */
    for (int p = 0; p < 3; p++) {
        pics[1].dst[p] = pics[0].dst[p] + pics[0].dst_stride[p];
        pics[0].dst_stride[p] *= 2;
        pics[1].dst_stride[p] = pics[0].dst_stride[p];
    }
    expect(FFHIP_ENOSYS, 8, 1, 2, 1, 2, "both fields of one frame");
    pics[1].dst[0] -= 4; expect(FFHIP_EINVAL, 8, 1, 2, 1, 2, "... four bytes into the other field's rows");
    fill(1, 2, 1); pics[0].dst[0] += 31 * 32; pics[0].dst_stride[0] = -pics[0].dst_stride[0];
    expect(FFHIP_EINVAL, 8, 1, 2, 2, 1, "a destination with a negative stride");
    quiet = false;
    return bad;
}

int main(void)
{
    static const int depths[5] = { 8, 9, 10, 12, 14 };
    int bad = 0;
    for (int k = 0; k < 40; k++) {
        const int mb_w = 1 + (int)(rnd() % 11), mb_h = 1 + (int)(rnd() % 9);
        bad |= run(depths[k % 5], k % 7 != 0, mb_w, mb_h, (int)(rnd() % 3), k >= 15, k % 11 == 3);
    }
    bad |= run(8, 1, 120, 68, 0, false, false);
    bad |= run(10, 1, 120, 68, 1, true, false);
    bad |= refusals();
    puts(bad ? "FAILED" : "ok");
    return bad;
}
