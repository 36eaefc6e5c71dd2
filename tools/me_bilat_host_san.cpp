/*
 * tools/me_bilat_host_san.cpp — a stand-alone host program over the host faces of the bilateral mode: the search,
 * ffhip_me_search_bilat_frames_host(), ffhip_me_search_bilat_sequence_host() and the test hook ffhip_me_search_bilat_cost_host(), the
 * compensation, ffhip_me_interp_bilat_sequence_host() (run_interp() below), and the argument checks they share with the device faces, for AddressSanitizer and UBSan: both methods at both block sizes, the smallest legal picture
 * (2 x 2 blocks), 6 x 5 blocks and sizes of b * mb + 3 with a padded stride, search_param = mb_size (the smallest legal), 21 and 32,
 * starting fields absent, of small vectors and of any int16, 1 and 3 sequences of 4 pictures — in heap blocks exactly as large as the
 * geometry says: a plane ends at its last sample ((rows - 1) * stride + width, not rows * stride), a field at its last block.  The
 * bilateral cost reads two windows of twice the block size that the rule clamps into the plane: a read outside it is an error the
 * sanitizer reports, and a signed overflow in the placement one UBSan reports.  Then the refusals on pointers the faces never follow.
 * CPU only: nothing here touches a device.
 *
 * Build and run from the repository root (the faces' file and this one, nothing else of the library):
 *   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
 *         --offload-arch=gfx950 -Iinclude -Iffmpeg_amd/csrc -Iffmpeg_amd/csrc/host ffmpeg_amd/csrc/me_api.hip \
 *         tools/me_bilat_host_san.cpp -o me_bilat_host_san && ./me_bilat_host_san
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

static uint32_t rnd_state = 24680;
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

enum { F_NONE, F_SMALL, F_ANY, F_KINDS };
enum { NFRAMES = 4 };

/* nseq fields of per blocks */
static int16_t *field(int fkind, int nseq, int bw, int bh, int lg)
{
    if (fkind == F_NONE)
        return nullptr;
    int16_t *f = reinterpret_cast<int16_t *>(block((size_t)nseq * bw * bh * 4));
    if (fkind == F_SMALL)
        for (int s = 0; s < nseq; s++)
            for (int by = 0; by < bh; by++)
                for (int bx = 0; bx < bw; bx++) {
                    int16_t *v = f + 2 * (((size_t)s * bh + by) * bw + bx);
                    v[0] = (int16_t)((bx << lg) + (int)(rnd() % 9) - 4);
                    v[1] = (int16_t)((by << lg) + (int)(rnd() % 9) - 4);
                }
    return f;
}

static int run(int method, int mb, int bw, int bh, int extra, int pad, int R, int fkind, int nseq)
{
    const int lg = mb == 16 ? 4 : 3, w = (bw << lg) + extra, h = (bh << lg) + extra;
    const ptrdiff_t stride = w + pad;
    const size_t pic = (size_t)stride * h, per = (size_t)bw * bh;
    /* the last picture of the last sequence ends at its last sample */
    const size_t nbytes = ((size_t)nseq * NFRAMES - 1) * pic + (size_t)(h - 1) * stride + w;
    uint8_t *frames = block(nbytes);
    int16_t *i1 = field(fkind, nseq, bw, bh, lg), *i2 = field(fkind, nseq, bw, bh, lg);
    int16_t *mv = reinterpret_cast<int16_t *>(block(per * nseq * (NFRAMES - 1) * 4));
    uint32_t *cost = reinterpret_cast<uint32_t *>(block(per * nseq * (NFRAMES - 1) * 4));
    int r = ffhip_me_search_bilat_sequence_host(method, frames, w, h, stride, pic, NFRAMES, NFRAMES * pic, nseq, mb, R, i1, i2, mv, cost);
    if (r) {
        printf("sequence face: %d %s\n", r, last_error);
        return 1;
    }
    uint32_t sum = 0;
    for (size_t i = 0; i < per * nseq * (NFRAMES - 1); i++)
        sum = sum * 31u + cost[i] + (uint16_t)mv[2 * i] + 7u * (uint16_t)mv[2 * i + 1];
    /* the pair face over the last pair of every sequence, the pairs a sequence apart, its fields the sequence's steps 1 and 0 */
    int16_t *pmv = reinterpret_cast<int16_t *>(block(per * nseq * 4));
    uint32_t *pcost = reinterpret_cast<uint32_t *>(block(per * nseq * 4));
    const uint8_t *a = frames + (NFRAMES - 2) * pic;
    /* nframes = nseq pairs seq_pitch apart: the last one ends where `frames` ends */
    r = ffhip_me_search_bilat_frames_host(method, a, a + pic, w, h, stride, NFRAMES * pic, nseq, mb, R, mv + 2 * per * nseq, mv, pmv, pcost);
    if (r) {
        printf("pair face: %d %s\n", r, last_error);
        return 1;
    }
    if (memcmp(pmv, mv + 2 * per * nseq * 2, per * nseq * 4) || memcmp(pcost, cost + per * nseq * 2, per * nseq * 4)) {
        printf("the pair face over step 2 differs from the sequence face\n");
        return 1;
    }
    /* the cost alone over the whole window of every block of the first pair */
    for (int by = 0; by < bh; by++)
        for (int bx = 0; bx < bw; bx++) {
            const int x_mb = bx << lg, y_mb = by << lg, lx = (bw - 1) << lg, ly = (bh - 1) << lg;
            const int x0 = x_mb - R < 0 ? 0 : x_mb - R, x1 = x_mb + R > lx ? lx : x_mb + R;
            const int y0 = y_mb - R < 0 ? 0 : y_mb - R, y1 = y_mb + R > ly ? ly : y_mb + R;
            for (int y = y0; y <= y1; y += 3)
                for (int x = x0; x <= x1; x++) {
                    uint32_t c;
                    r = ffhip_me_search_bilat_cost_host(frames, frames + pic, w, h, stride, mb, R, bx, by, x, y, (int)(rnd() % 65) - 32,
                                                        (int)(rnd() % 65) - 32, &c);
                    if (r) {
                        printf("cost face: %d %s\n", r, last_error);
                        return 1;
                    }
                    sum = sum * 31u + c;
                }
        }
    printf("method %d mb %2d %d x %d blocks +%d pad %d R %2d fields %d nseq %d: %08x\n", method, mb, bw, bh, extra, pad, R, fkind, nseq, sum);
    free(frames);
    free(i1);
    free(i2);
    free(mv);
    free(cost);
    free(pmv);
    free(pcost);
    return 0;
}

/* the bilateral compensation's host face: 2 sequences of 3 pictures, 9 jobs of both modes and every alpha of the tests, scene flags
 * with both actions, a field within mv_range (fkind F_SMALL) or of any int16 (most of it malformed); planes, field, window, flags and
 * outputs in heap blocks that end at their last byte */
static int run_interp(int w, int h, int mb, int nplanes, int sw, int sh, int R, int fkind, int action)
{
    enum { NS = 2, NF = 3 };
    static const int alphas[6] = { 0, 1, 341, 512, 1023, 1024 };
    const int lg = mb == 16 ? 4 : 3, bw = w >> lg, bh = h >> lg, pad[3] = { 5, 0, 3 };
    const size_t per = (size_t)bw * bh, nfield = 2 * per * NS * (NF - 1);
    FFHipMeInterpJob jobs[9];
    const int njobs = 9;
    for (int j = 0; j < njobs; j++)
        jobs[j] = { j % NS, (j / 2) % (NF - 1), alphas[(j + fkind + mb) % 6], j % 4 == 3 ? FFHIP_ME_INTERP_BLEND : FFHIP_ME_INTERP_MCI };
    FFHipMePlanes src = {}, dst = {};
    for (int i = 0; i < nplanes; i++) {
        const int pw = i ? (w + (1 << sw) - 1) >> sw : w, ph = i ? (h + (1 << sh) - 1) >> sh : h;
        const size_t last = (size_t)(ph - 1) * (pw + pad[i]) + pw;           /* a picture ends at its last sample */
        src.stride[i] = dst.stride[i] = pw + pad[i];
        src.frame_pitch[i] = (size_t)ph * (pw + pad[i]) + 7;
        src.seq_pitch[i] = NF * src.frame_pitch[i] + 1;
        dst.frame_pitch[i] = (size_t)ph * (pw + pad[i]);
        src.base[i] = block((NS - 1) * src.seq_pitch[i] + (NF - 1) * src.frame_pitch[i] + last);
        dst.base[i] = block((njobs - 1) * dst.frame_pitch[i] + last);
    }
    int16_t *f = reinterpret_cast<int16_t *>(block(nfield * 2));
    for (size_t e = 0; e < nfield / 2; e++) {
        const int bx = (int)(e % per) % (bw ? bw : 1), by = (int)(e % per) / (bw ? bw : 1);
        if (fkind == F_ANY && rnd() % 4)
            continue;                                                       /* block() filled it with any int16 */
        f[2 * e] = (int16_t)((bx << lg) + (int)(rnd() % (2 * R + 1)) - R);
        f[2 * e + 1] = (int16_t)((by << lg) + (int)(rnd() % (2 * R + 1)) - R);
    }
    uint8_t *window = block((size_t)4 * mb * mb), *scene = block((size_t)(NF - 1) * NS);
    for (int i = 0; i < (NF - 1) * NS; i++)
        scene[i] &= 1;
    const int r = ffhip_me_interp_bilat_sequence_host(&src, &dst, nplanes, sw, sh, w, h, NF, NS, mb, R, window, f, jobs, njobs, action ? scene : nullptr,
                                                      action ? action : FFHIP_ME_SCENE_BLEND);
    if (r) {
        printf("interp %dx%d mb %d planes %d shifts %d,%d range %d field %d: %d (%s)\n", w, h, mb, nplanes, sw, sh, R, fkind, r, last_error);
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
    printf("interp %dx%d mb %2d planes %d shifts %d,%d range %3d field %d action %d: %08x taken %llu capped %llu malformed %llu clipped %llu\n", w, h, mb,
           nplanes, sw, sh, R, fkind, action, sum, (unsigned long long)counts[0], (unsigned long long)counts[2], (unsigned long long)counts[3],
           (unsigned long long)counts[5]);
    free(f);
    free(window);
    free(scene);
    return counts[2] != 0;      /* the cap never binds */
}

static int refused(const char *what, int r, int want)
{
    if (r != want) {
        printf("%s: %d, not %d (%s)\n", what, r, want, last_error);
        return 1;
    }
    return 0;
}

int main(void)
{
    int bad = 0;
    for (int method = FFHIP_ME_METHOD_EPZS; method <= FFHIP_ME_METHOD_UMH; method++)
        for (int mb = 8; mb <= 16; mb += 8) {
            const int Rs[3] = { mb, 21, 32 };
            for (int ri = 0; ri < 3; ri++)
                for (int fkind = 0; fkind < F_KINDS; fkind++) {
                    bad |= run(method, mb, 2, 2, 0, 0, Rs[ri], fkind, 1);
                    bad |= run(method, mb, 6, 5, 0, 1, Rs[ri], fkind, 3);
                    bad |= run(method, mb, 4, 3, 3, 2, Rs[ri], fkind, 1);
                    bad |= run(method, mb, 2, 3, 7, 0, Rs[ri], fkind, 3);
                }
        }
    /* the compensation: sizes with and without whole blocks at the edges, a picture smaller than a block, every chroma layout */
    const int sizes[5][2] = { { 48, 32 }, { 52, 38 }, { 53, 37 }, { 63, 47 }, { 12, 12 } };
    int nth = 0;
    for (int si = 0; si < 5; si++)
        for (int mb = 8; mb <= 16; mb += 8)
            for (int fkind = F_SMALL; fkind <= F_ANY; fkind++, nth++) {
                const int nplanes = nth % 4 == 3 ? 1 : 3;
                bad |= run_interp(sizes[si][0], sizes[si][1], mb, nplanes, nth % 2, (nth / 2) % 2, nth % 3 ? 32 : 7, fkind, nth % 3);
            }
    /* the refusals, on pointers nobody follows */
    const uint8_t *p = reinterpret_cast<const uint8_t *>(0x1000000);
    int16_t *mv = reinterpret_cast<int16_t *>(0x2000000);
    uint32_t *k = reinterpret_cast<uint32_t *>(0x3000000);
    bad |= refused("search_param below mb_size", ffhip_me_search_bilat_frames_host(8, p, p, 64, 64, 64, 4096, 1, 16, 15, nullptr, nullptr, mv, k), FFHIP_EINVAL);
    bad |= refused("one block column", ffhip_me_search_bilat_frames_host(8, p, p, 31, 64, 64, 4096, 1, 16, 16, nullptr, nullptr, mv, k), FFHIP_EINVAL);
    bad |= refused("one block row", ffhip_me_search_bilat_sequence_host(9, p, 64, 31, 64, 4096, 3, 3 * 4096, 2, 16, 16, nullptr, nullptr, mv, k), FFHIP_EINVAL);
    for (int method = 1; method <= 7; method++) {
        bad |= refused("a per-block method", ffhip_me_search_bilat_frames_host(method, p, p, 64, 64, 64, 4096, 1, 16, 16, nullptr, nullptr, mv, k), FFHIP_ENOSYS);
        bad |= refused("a per-block method", ffhip_me_search_bilat_sequence_dev(method, p, 64, 64, 64, 4096, 3, 3 * 4096, 2, 16, 16, nullptr, nullptr, mv, k, nullptr),
                       FFHIP_ENOSYS);
    }
    bad |= refused("method 10", ffhip_me_search_bilat_batch_dev(10, p, p, 64, 64, 64, 4096, 1, 16, 16, nullptr, nullptr, mv, k, nullptr), FFHIP_EINVAL);
    bad |= refused("no device", ffhip_me_search_bilat_batch_dev(8, p, p, 64, 64, 64, 4096, 1, 16, 16, nullptr, nullptr, mv, k, nullptr), FFHIP_ENOSYS);
    bad |= refused("nothing to search", ffhip_me_search_bilat_sequence_host(8, p, 64, 64, 64, 4096, 1, 4096, 2, 16, 16, nullptr, nullptr, mv, k), 0);
    bad |= refused("a position outside the window", ffhip_me_search_bilat_cost_host(p, p, 64, 64, 64, 16, 16, 0, 0, 17, 0, 0, 0, k), FFHIP_EINVAL);
    if (bad)
        return 1;
    printf("ok\n");
    return 0;
}
