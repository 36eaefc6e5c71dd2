/*
 * tools/me_interp_host_san.cpp — a stand-alone host program over ffhip_me_interp_sequence_host() and the argument checks it shares with
 * ffhip_me_interp_sequence_dev(), for AddressSanitizer and UBSan: the shapes of tests/test_me_interp_cpu.py at both block sizes, the
 * three chroma layouts and luma alone, fields of small vectors, of vectors at +-mv_range (every displacement clip at every border) and of
 * any int16, windows of any byte, every alpha of the tests, MCI and BLEND jobs over 2 sequences of 3 pictures — in heap blocks exactly as
 * large as the geometry says: a plane ends at its last sample ((rows - 1) * stride + width, not rows * stride), a field at its last
 * block, the window at (2 * mb_size)^2, the outputs at the last sample of the last job.  A read or write outside them is an error the
 * sanitizer reports, and a signed overflow in the window arithmetic one UBSan reports.  Then the refusals of both faces on plane,
 * window and field pointers they never follow.  CPU only: nothing here touches a device.
 *
 * Build and run from the repository root (the faces' file and this one, nothing else of the library):
 *   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
 *         --offload-arch=gfx950 -Iinclude -Iffmpeg_amd/csrc -Iffmpeg_amd/csrc/host ffmpeg_amd/csrc/me_api.hip \
 *         tools/me_interp_host_san.cpp -o me_interp_host_san && ./me_interp_host_san
 * Prints a checksum of the outputs per case and "ok"; the sanitizer aborts on the first finding.
 */
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ffhip.h"

/* what me_api.hip takes from the rest of the library */
static char last_error[512];
extern "C" void ffhip_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_error, sizeof(last_error), fmt, ap);
    va_end(ap);
}
int ffhip_have_device(void) { return 0; }
struct ihipStream_t;
int ffhip_launch_me_cmp(int, int, int, const uint8_t *, const int32_t *, const uint8_t *, const int32_t *, ptrdiff_t, int32_t *, int, ihipStream_t *)
{
    return FFHIP_ENOSYS;
}
int ffhip_launch_me_esa(const uint8_t *, const uint8_t *, int, int, ptrdiff_t, size_t, int, int, int, int, int16_t *, uint32_t *, ihipStream_t *)
{
    return FFHIP_ENOSYS;
}
int ffhip_launch_me_search(int, const uint8_t *, const uint8_t *, int, int, ptrdiff_t, size_t, int, int, int, int, int16_t *, uint32_t *, ihipStream_t *)
{
    return FFHIP_ENOSYS;
}
int ffhip_launch_me_search_pred(int, const uint8_t *, const uint8_t *, int, int, ptrdiff_t, size_t, int, int, int, int, const int16_t *, const int16_t *,
                                int16_t *, uint32_t *, ihipStream_t *)
{
    return FFHIP_ENOSYS;
}
int ffhip_launch_me_search_seq(int, const uint8_t *, int, int, ptrdiff_t, size_t, int, size_t, int, int, int, int, int, const int16_t *, const int16_t *,
                               int16_t *, uint32_t *, ihipStream_t *)
{
    return FFHIP_ENOSYS;
}
int ffhip_launch_me_interp(const FFHipMePlanes *, const FFHipMePlanes *, int, int, int, int, int, int, int, int, const uint8_t *, const int16_t *,
                           const int16_t *, const FFHipMeInterpJob *, int, ihipStream_t *)
{
    return FFHIP_ENOSYS;
}
int ffhip_launch_me_interp_scd(const FFHipMePlanes *, const FFHipMePlanes *, int, int, int, int, int, int, int, int, const uint8_t *, const int16_t *,
                               const int16_t *, const FFHipMeInterpJob *, int, const uint8_t *, int, ihipStream_t *)
{
    return FFHIP_ENOSYS;
}
int ffhip_launch_me_interp_bilat(const FFHipMePlanes *, const FFHipMePlanes *, int, int, int, int, int, int, int, int, const uint8_t *, const int16_t *,
                                 const FFHipMeInterpJob *, int, const uint8_t *, int, ihipStream_t *)
{
    return FFHIP_ENOSYS;
}
int ffhip_launch_me_scene(const uint8_t *, int, int, int, ptrdiff_t, size_t, int, size_t, int, double, const double *, double *, uint64_t *, float *,
                          uint8_t *, ihipStream_t *)
{
    return FFHIP_ENOSYS;
}

static uint32_t rnd_state = 13579;
static uint32_t rnd(void)
{
    rnd_state = rnd_state * 1664525u + 1013904223u;
    return rnd_state >> 8;
}

/* n bytes exactly: the byte after them is the sanitizer's */
static uint8_t *block(size_t n)
{
    uint8_t *p = static_cast<uint8_t *>(malloc(n ? n : 1));
    if (!p)
        abort();
    for (size_t i = 0; i < n; i++)
        p[i] = (uint8_t)rnd();
    return p;
}

static const int ALPHAS[6] = { 0, 1, 341, 512, 1023, 1024 };
enum { F_SMALL, F_PLUS, F_MINUS, F_ANY, F_KINDS };
enum { NSEQ = 2, NFRAMES = 3 };

static int run(int w, int h, int mb, int nplanes, int sw, int sh, int R, int fkind)
{
    const int lg = mb == 16 ? 4 : 3, bw = w >> lg, bh = h >> lg, pad[3] = { 5, 0, 3 };
    const size_t per = (size_t)bw * bh, nfield = 2 * per * NSEQ * (NFRAMES - 1);
    FFHipMeInterpJob jobs[9];
    const int njobs = 9;
    for (int j = 0; j < njobs; j++)
        jobs[j] = { j % NSEQ, (j / 2) % (NFRAMES - 1), ALPHAS[(j + fkind + mb) % 6], j % 4 == 3 ? FFHIP_ME_INTERP_BLEND : FFHIP_ME_INTERP_MCI };
    FFHipMePlanes src = {}, dst = {};
    for (int i = 0; i < nplanes; i++) {
        const int pw = i ? (w + (1 << sw) - 1) >> sw : w, ph = i ? (h + (1 << sh) - 1) >> sh : h;
        const size_t last = (size_t)(ph - 1) * (pw + pad[i]) + pw;           /* a picture ends at its last sample */
        src.stride[i] = dst.stride[i] = pw + pad[i];
        src.frame_pitch[i] = (size_t)ph * (pw + pad[i]) + 7;
        src.seq_pitch[i] = NFRAMES * src.frame_pitch[i] + 1;
        dst.frame_pitch[i] = (size_t)ph * (pw + pad[i]);
        src.base[i] = block((NSEQ - 1) * src.seq_pitch[i] + (NFRAMES - 1) * src.frame_pitch[i] + last);
        dst.base[i] = block((njobs - 1) * dst.frame_pitch[i] + last);
    }
    int16_t *f[2];
    for (int d = 0; d < 2; d++) {
        f[d] = reinterpret_cast<int16_t *>(block(nfield * 2));
        for (size_t e = 0; e < nfield / 2; e++) {
            const int bx = (int)(e % per) % (bw ? bw : 1), by = (int)(e % per) / (bw ? bw : 1);
            const int vx = fkind == F_SMALL ? (int)(rnd() % (2 * R + 1)) - R : fkind == F_PLUS ? R : -R;
            const int vy = fkind == F_SMALL ? (int)(rnd() % (2 * R + 1)) - R : fkind == F_PLUS ? R : -R;
            if (fkind == F_ANY && rnd() % 4)
                continue;                                                   /* block() filled it with any int16 */
            f[d][2 * e] = (int16_t)((bx << lg) + vx);
            f[d][2 * e + 1] = (int16_t)((by << lg) + vy);
        }
    }
    uint8_t *window = block((size_t)4 * mb * mb);
    const int r = ffhip_me_interp_sequence_host(&src, &dst, nplanes, sw, sh, w, h, NFRAMES, NSEQ, mb, R, window, f[0], f[1], jobs, njobs);
    if (r) {
        printf("%dx%d mb %d planes %d shifts %d,%d range %d field %d: %d (%s)\n", w, h, mb, nplanes, sw, sh, R, fkind, r, last_error);
        return 1;
    }
    uint64_t counts[8];
    ffhip_me_interp_host_counts(counts);
    uint32_t sum = 0;
    for (int i = 0; i < nplanes; i++) {
        const int pw = i ? (w + (1 << sw) - 1) >> sw : w, ph = i ? (h + (1 << sh) - 1) >> sh : h;
        for (int j = 0; j < njobs; j++)
            for (int y = 0; y < ph; y++)
                for (int x = 0; x < pw; x++)
                    sum = sum * 31 + dst.base[i][j * dst.frame_pitch[i] + (size_t)y * dst.stride[i] + x];
        free(src.base[i]);
        free(dst.base[i]);
    }
    printf("%dx%d mb %2d planes %d shifts %d,%d range %3d field %d: %08x taken %llu capped %llu malformed %llu clipped %llu\n", w, h, mb, nplanes, sw, sh,
           R, fkind, sum, (unsigned long long)counts[0], (unsigned long long)counts[2], (unsigned long long)counts[3], (unsigned long long)counts[5]);
    free(f[0]);
    free(f[1]);
    free(window);
    return 0;
}

/* both faces refuse, with a text, before they follow a plane, window or field pointer */
static int refusals(void)
{
    uint8_t *const wild = reinterpret_cast<uint8_t *>(16);
    int16_t *const wildf = reinterpret_cast<int16_t *>(32);
    int bad = 0;
    auto planes = [&](uint8_t *b, ptrdiff_t stride) {
        FFHipMePlanes p = {};
        for (int i = 0; i < 3; i++) {
            p.base[i] = b + (b ? i * (1 << 20) : 0);
            p.stride[i] = stride;
            p.frame_pitch[i] = 1 << 12;
            p.seq_pitch[i] = 1 << 16;
        }
        return p;
    };
    const FFHipMePlanes src = planes(wild, 64), dst = planes(wild + (1 << 24), 64);
    const FFHipMeInterpJob good[2] = { { 0, 0, 7, FFHIP_ME_INTERP_MCI }, { 1, 1, 1024, FFHIP_ME_INTERP_BLEND } };
    auto both = [&](const char *what, const FFHipMePlanes *s, const FFHipMePlanes *d, int nplanes, int sw, int sh, int w, int h, int nframes, int nseq, int mb,
                    int R, const uint8_t *win, const int16_t *fw, const int16_t *bw, const FFHipMeInterpJob *jobs, int njobs) {
        for (int face = 0; face < 2; face++) {
            last_error[0] = 0;
            const int r = face ? ffhip_me_interp_sequence_dev(s, d, nplanes, sw, sh, w, h, nframes, nseq, mb, R, win, fw, bw, jobs, njobs, nullptr)
                               : ffhip_me_interp_sequence_host(s, d, nplanes, sw, sh, w, h, nframes, nseq, mb, R, win, fw, bw, jobs, njobs);
            if (r != FFHIP_EINVAL || !last_error[0]) {
                printf("refusal `%s`, face %d: %d (%s)\n", what, face, r, last_error);
                bad++;
            }
        }
    };
    both("null src", nullptr, &dst, 3, 1, 1, 64, 32, 3, 2, 16, 8, wild, wildf, wildf, good, 2);
    both("null dst", &src, nullptr, 3, 1, 1, 64, 32, 3, 2, 16, 8, wild, wildf, wildf, good, 2);
    both("null window", &src, &dst, 3, 1, 1, 64, 32, 3, 2, 16, 8, nullptr, wildf, wildf, good, 2);
    both("null jobs", &src, &dst, 3, 1, 1, 64, 32, 3, 2, 16, 8, wild, wildf, wildf, nullptr, 2);
    both("null field", &src, &dst, 3, 1, 1, 64, 32, 3, 2, 16, 8, wild, nullptr, wildf, good, 2);
    FFHipMePlanes hole = src;
    hole.base[1] = nullptr;
    both("null plane", &hole, &dst, 3, 1, 1, 64, 32, 3, 2, 16, 8, wild, wildf, wildf, good, 2);
    both("nplanes", &src, &dst, 2, 1, 1, 64, 32, 3, 2, 16, 8, wild, wildf, wildf, good, 2);
    both("shift", &src, &dst, 3, 2, 1, 64, 32, 3, 2, 16, 8, wild, wildf, wildf, good, 2);
    both("mb_size", &src, &dst, 3, 1, 1, 64, 32, 3, 2, 4, 8, wild, wildf, wildf, good, 2);
    both("mv_range", &src, &dst, 3, 1, 1, 64, 32, 3, 2, 16, 257, wild, wildf, wildf, good, 2);
    both("negative", &src, &dst, 3, 1, 1, -64, 32, 3, 2, 16, 8, wild, wildf, wildf, good, 2);
    both("njobs", &src, &dst, 3, 1, 1, 64, 32, 3, 2, 16, 8, wild, wildf, wildf, good, -2);
    both("large", &src, &dst, 3, 1, 1, 64, 32769, 3, 2, 16, 8, wild, wildf, wildf, good, 2);
    both("stride", &src, &dst, 3, 1, 1, 65, 32, 3, 2, 16, 8, wild, wildf, wildf, good, 2);
    both("frame_pitch", &src, &dst, 3, 0, 0, 64, 65, 3, 2, 16, 8, wild, wildf, wildf, good, 2);
    both("seq_pitch", &src, &dst, 3, 1, 1, 64, 32, 17, 2, 16, 8, wild, wildf, wildf, good, 2);
    const FFHipMeInterpJob off[2] = { { 0, 0, 7, FFHIP_ME_INTERP_MCI }, { 1, 2, 5, FFHIP_ME_INTERP_BLEND } };
    both("job", &src, &dst, 3, 1, 1, 64, 32, 3, 2, 16, 8, wild, wildf, wildf, off, 2);
    const FFHipMePlanes on = planes(wild + 100, 64);
    both("overlap", &src, &on, 3, 1, 1, 64, 32, 3, 2, 16, 8, wild, wildf, wildf, good, 2);
    /* and the legal call is refused by neither check: the device face gets as far as the missing device, without a text of the checks */
    last_error[0] = 0;
    const int r = ffhip_me_interp_sequence_dev(&src, &dst, 3, 1, 1, 64, 32, 3, 2, 16, 8, wild, wildf, wildf, good, 2, nullptr);
    if (r != FFHIP_ENOSYS || last_error[0]) {
        printf("the legal call: %d (%s)\n", r, last_error);
        bad++;
    }
    return bad;
}

int main(void)
{
    static const int shapes[5][2] = { { 48, 32 }, { 52, 38 }, { 53, 37 }, { 12, 12 }, { 96, 80 } };
    static const int layouts[4][3] = { { 3, 0, 0 }, { 3, 1, 0 }, { 3, 1, 1 }, { 1, 0, 0 } };
    int bad = 0, k = 0;
    for (const auto &s : shapes)
        for (int mb = 8; mb <= 16; mb += 8)
            for (int fkind = 0; fkind < F_KINDS; fkind++, k++) {
                const int *l = layouts[k % 4];
                bad += run(s[0], s[1], mb, l[0], l[1], l[2], k % 3 == 0 ? 256 : k % 3 == 1 ? 32 : 5, fkind);
            }
    bad += run(16, 8, 16, 3, 1, 1, 0, F_SMALL);          /* no block row at all; mv_range 0 */
    bad += refusals();
    if (bad) {
        printf("%d FAILED\n", bad);
        return 1;
    }
    printf("ok\n");
    return 0;
}
