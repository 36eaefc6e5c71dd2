/*
 * tools/me_search_host_san.cpp — a stand-alone host program over ffhip_me_search_frames_host(), ffhip_me_search_pred_frames_host() and the
 * argument checks of ffhip_me_search_batch_dev() and ffhip_me_search_pred_batch_dev() for AddressSanitizer and UBSan: the shapes of
 * tests/test_me_search_cpu.py and tests/test_me_pred_search_cpu.py at both block sizes, every method (1 to 9) and both metrics, three frame
 * pairs each (noise, a shifted copy with exactly matching blocks, a flat one with sparse marks), the predictive methods with prev fields of
 * small vectors, of any int16 and NULL, in heap blocks exactly as large as the geometry says — the planes end at height * stride, the
 * fields and outputs at the last block — so a read or write outside them is an error the sanitizer reports, and a signed overflow in the
 * window, the step arithmetic, the relative vectors or the d loops (search_param up to INT_MAX, vectors of any int16) one UBSan reports;
 * then ffhip_me_search_pred_sequence_host() on sequences in blocks of exactly their size, every byte against the chained calls that define
 * it; then the refusals of all six faces on pointers they never follow.  CPU only: nothing here touches a device.
 *
 * Build and run from the repository root (the faces' file and this one, nothing else of the library):
 *   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
 *         --offload-arch=gfx950 -Iinclude -Iffmpeg_amd/csrc -Iffmpeg_amd/csrc/host ffmpeg_amd/csrc/me_api.hip \
 *         tools/me_search_host_san.cpp -o me_search_host_san && ./me_search_host_san
 * Prints a checksum of the outputs per case and "ok"; the sanitizer aborts on the first finding.
 */
#include <limits.h>
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
int ffhip_launch_me_interp_bilat(const FFHipMePlanes *, const FFHipMePlanes *, int, int, int, int, int, int, int, int, const uint8_t *, const int16_t *,
                                 const FFHipMeInterpJob *, int, const uint8_t *, int, ihipStream_t *)
{
    return FFHIP_ENOSYS;
}
int ffhip_launch_me_interp_scd(const FFHipMePlanes *, const FFHipMePlanes *, int, int, int, int, int, int, int, int, const uint8_t *, const int16_t *,
                               const int16_t *, const FFHipMeInterpJob *, int, const uint8_t *, int, ihipStream_t *)
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
    return p;
}

static bool predictive(int method) { return method >= FFHIP_ME_METHOD_EPZS; }

static int run(int w, int h, int pad, int mb, int R)
{
    const int nf = 3, stride = w + pad, bw = w / mb, bh = h / mb;
    const size_t plane = (size_t)h * stride, nb = (size_t)nf * bw * bh;
    uint8_t *cur = block(nf * plane), *ref = block(nf * plane);
    int16_t *mv = reinterpret_cast<int16_t *>(block(nb * 4)), *small1 = reinterpret_cast<int16_t *>(block(nb * 4));
    int16_t *small2 = reinterpret_cast<int16_t *>(block(nb * 4)), *any1 = reinterpret_cast<int16_t *>(block(nb * 4));
    int16_t *any2 = reinterpret_cast<int16_t *>(block(nb * 4));
    uint32_t *cost = reinterpret_cast<uint32_t *>(block(nb * 4));
    for (size_t i = 0; i < plane; i++) {
        ref[i] = (uint8_t)rnd();
        cur[i] = (uint8_t)rnd();                                            /* frame 0: noise against noise */
        ref[plane + i] = (uint8_t)(rnd() % 7 ? 100 + i % 23 : rnd());
        ref[2 * plane + i] = (uint8_t)(i % 37 ? 128 : 130);                /* frame 2: flat with sparse marks */
    }
    const int rs = R < 8 ? R : 8, dx = (int)(rnd() % (2 * rs + 1)) - rs;
    for (size_t i = 0; i < plane; i++) {                                    /* frame 1: a shifted copy, and blocks that match exactly */
        const ptrdiff_t j = (ptrdiff_t)i + dx;
        cur[plane + i] = i < (size_t)(2 * mb) * stride || j < 0 || j >= (ptrdiff_t)plane ? ref[plane + i] : ref[plane + j];
        cur[2 * plane + i] = (uint8_t)((i + 3) % 37 ? 128 : 130);
    }
    for (size_t b = 0; b < nb; b++)
        for (int k = 0; k < 2; k++) {
            const int o = k ? (int)(b / bw % bh) * mb : (int)(b % bw) * mb;
            small1[2 * b + k] = (int16_t)(o + (int)(rnd() % 13) - 6);
            small2[2 * b + k] = (int16_t)(o + (int)(rnd() % 13) - 6);
            any1[2 * b + k] = (int16_t)rnd();
            any2[2 * b + k] = (int16_t)rnd();
        }
    int bad = 0;
    for (int method = FFHIP_ME_METHOD_ESA; method <= FFHIP_ME_METHOD_UMH; method++)
        for (int kind = FFHIP_ME_SAD; kind <= FFHIP_ME_SATD; kind++)
            for (int prev = 0; prev < (predictive(method) ? 3 : 1); prev++) {
                const int16_t *p1 = prev == 0 ? small1 : prev == 1 ? any1 : nullptr, *p2 = prev == 0 ? small2 : prev == 1 ? any2 : nullptr;
                memset(mv, 0x5A, nb * 4);
                memset(cost, 0x5A, nb * 4);
                const int r = predictive(method) ? ffhip_me_search_pred_frames_host(method, cur, ref, w, h, stride, plane, nf, mb, R, kind, p1, p2, mv, cost)
                                                 : ffhip_me_search_frames_host(method, cur, ref, w, h, stride, plane, nf, mb, R, kind, mv, cost);
                uint64_t blocks = 0, costs = 0;
                ffhip_me_search_host_counts(&blocks, &costs);
                uint32_t sum = 0;
                for (size_t b = 0; b < nb; b++) {
                    sum = sum * 31 + (uint32_t)mv[2 * b] * 65537u + (uint32_t)mv[2 * b + 1] + cost[b];
                    const int bx = (int)(b % bw) * mb, by = (int)(b / bw % bh) * mb;
                    bad |= mv[2 * b] < 0 || mv[2 * b] > (bw - 1) * mb || mv[2 * b + 1] < 0 || mv[2 * b + 1] > (bh - 1) * mb;
                    bad |= abs(mv[2 * b] - bx) > R || abs(mv[2 * b + 1] - by) > R;          /* the window */
                    bad |= cost[b] == 0x5A5A5A5Au;                                          /* every block ends with a real cost */
                }
                bad |= r != 0 || blocks != nb || costs < (predictive(method) ? 2 : 1) * nb;
                printf("%3d x %3d pad %d mb %2d R %10d method %d kind %d prev %d: rc %d, %llu costs, checksum %08x\n", w, h, pad, mb, R, method, kind,
                       predictive(method) ? prev : -1, r, (unsigned long long)costs, sum);
            }
    free(cur); free(ref); free(mv); free(cost); free(small1); free(small2); free(any1); free(any2);
    return bad;
}

/* ffhip_me_search_pred_sequence_host(): two sequences of four pictures in one heap block that ends at the last picture's last row, the
 * starting fields and the outputs at their last block; both methods, metrics and directions, starting fields of small vectors, of any
 * int16 and NULL; every byte against the chained calls of ffhip_me_search_pred_frames_host() that define it */
static int run_seq(int w, int h, int pad, int mb, int R)
{
    const int nseq = 2, nframes = 4, np = nframes - 1, stride = w + pad, bw = w / mb, bh = h / mb;
    const size_t plane = (size_t)h * stride, seq = nframes * plane, step = (size_t)nseq * bw * bh, nb = step * np;
    uint8_t *frames = block(nseq * seq);
    int16_t *mv = reinterpret_cast<int16_t *>(block(nb * 4)), *want_mv = reinterpret_cast<int16_t *>(block(nb * 4));
    uint32_t *cost = reinterpret_cast<uint32_t *>(block(nb * 4)), *want_cost = reinterpret_cast<uint32_t *>(block(nb * 4));
    int16_t *init[2][2];    /* [small, any][init1, init2] */
    for (int k = 0; k < 4; k++)
        init[k >> 1][k & 1] = reinterpret_cast<int16_t *>(block(step * 4));
    for (size_t i = 0; i < plane; i++) {
        frames[i] = (uint8_t)(rnd() % 5 ? 90 + i % 29 : rnd());             /* sequence 0: a pattern that shifts, sequence 1: noise */
        frames[seq + i] = (uint8_t)rnd();
    }
    for (int p = 1; p < nframes; p++)
        for (size_t i = 0; i < plane; i++) {
            const size_t j = (i + (size_t)(p * (R < 3 ? R : 3))) % plane;
            frames[p * plane + i] = frames[(p - 1) * plane + j];
            frames[seq + p * plane + i] = (uint8_t)(rnd() % 4 ? frames[seq + (p - 1) * plane + i] : rnd());
        }
    for (size_t b = 0; b < step; b++)
        for (int k = 0; k < 2; k++) {
            const int o = k ? (int)(b / bw % bh) * mb : (int)(b % bw) * mb;
            init[0][0][2 * b + k] = (int16_t)(o + (int)(rnd() % 13) - 6);
            init[0][1][2 * b + k] = (int16_t)(o + (int)(rnd() % 13) - 6);
            init[1][0][2 * b + k] = (int16_t)rnd();
            init[1][1][2 * b + k] = (int16_t)rnd();
        }
    int bad = 0;
    for (int method = FFHIP_ME_METHOD_EPZS; method <= FFHIP_ME_METHOD_UMH; method++)
        for (int kind = FFHIP_ME_SAD; kind <= FFHIP_ME_SATD; kind++)
            for (int dir = 0; dir < 2; dir++)
                for (int prev = 0; prev < 3; prev++) {
                    const int16_t *i1 = prev < 2 ? init[prev][0] : nullptr, *i2 = prev < 2 ? init[prev][1] : nullptr;
                    memset(mv, 0x5A, nb * 4);
                    memset(cost, 0x5A, nb * 4);
                    const int r = ffhip_me_search_pred_sequence_host(method, frames, w, h, stride, plane, nframes, seq, nseq, dir, mb, R, kind, i1, i2, mv, cost);
                    uint64_t blocks = 0, costs = 0, want_blocks = 0, want_costs = 0;
                    ffhip_me_search_host_counts(&blocks, &costs);
                    int rc = 0;
                    for (int k = 0; k < np; k++) {
                        const uint8_t *lo = frames + k * plane, *hi = lo + plane;
                        const int16_t *p1 = k >= 1 ? want_mv + 2 * step * (k - 1) : i1, *p2 = k >= 2 ? want_mv + 2 * step * (k - 2) : k == 1 ? i1 : i2;
                        rc |= ffhip_me_search_pred_frames_host(method, dir ? lo : hi, dir ? hi : lo, w, h, stride, seq, nseq, mb, R, kind, p1, p2,
                                                               want_mv + 2 * step * k, want_cost + step * k);
                        uint64_t b1 = 0, c1 = 0;
                        ffhip_me_search_host_counts(&b1, &c1);
                        want_blocks += b1;
                        want_costs += c1;
                    }
                    uint32_t sum = 0;
                    for (size_t b = 0; b < nb; b++)
                        sum = sum * 31 + (uint32_t)mv[2 * b] * 65537u + (uint32_t)mv[2 * b + 1] + cost[b];
                    bad |= r != 0 || rc != 0 || blocks != nb || blocks != want_blocks || costs != want_costs;
                    bad |= memcmp(mv, want_mv, nb * 4) != 0 || memcmp(cost, want_cost, nb * 4) != 0;
                    printf("seq %3d x %3d pad %d mb %2d R %10d method %d kind %d dir %d init %d: rc %d, %llu costs, checksum %08x\n", w, h, pad, mb, R,
                           method, kind, dir, prev, r, (unsigned long long)costs, sum);
                }
    free(frames); free(mv); free(want_mv); free(cost); free(want_cost);
    for (int k = 0; k < 4; k++)
        free(init[k >> 1][k & 1]);
    return bad;
}

/* the refusals of the sequence faces, each with its text, on pointers they never follow; and the calls that do nothing */
static int seq_refusals(void)
{
    const size_t P = 64 * 48;
    static uint8_t arena[6 * 64 * 48];
    alignas(4) static int16_t fields[3][2 * 2 * 12 * 2 + 2];      /* mv_out: 2 pairs of 2 sequences; init1, init2: 2 fields each */
    static uint32_t cost[2 * 2 * 12];
    struct Args { int method; const uint8_t *frames; int w, h; ptrdiff_t stride; size_t pitch; int nf; size_t spitch; int nseq, dir, mb, R, kind; const int16_t *i1, *i2; int16_t *mv; uint32_t *cost; };
    const Args good = { FFHIP_ME_METHOD_EPZS, arena, 64, 48, 64, P, 3, 3 * P, 2, 0, 16, 7, FFHIP_ME_SAD, fields[1], fields[2], fields[0], cost };
    int bad = 0;
    auto expect = [&](int want_host, int want_dev, Args a, const char *what, const char *word) {
        for (int dev = 0; dev < 2; dev++) {
            last_error[0] = 0;
            memset(fields[0], 0x11, sizeof(fields[0]));
            const int r = dev ? ffhip_me_search_pred_sequence_dev(a.method, a.frames, a.w, a.h, a.stride, a.pitch, a.nf, a.spitch, a.nseq, a.dir, a.mb, a.R, a.kind, a.i1, a.i2, a.mv, a.cost, nullptr)
                              : ffhip_me_search_pred_sequence_host(a.method, a.frames, a.w, a.h, a.stride, a.pitch, a.nf, a.spitch, a.nseq, a.dir, a.mb, a.R, a.kind, a.i1, a.i2, a.mv, a.cost);
            bool untouched = true;
            for (size_t i = 0; i < sizeof(fields[0]); i++)
                untouched &= reinterpret_cast<const uint8_t *>(fields[0])[i] == 0x11;
            const bool refused = (dev ? want_dev : want_host) == FFHIP_EINVAL;
            if (r != (dev ? want_dev : want_host) || (word && !strstr(last_error, word)) || (refused && !untouched)) {
                printf("refusals: sequence face (%s), %s: rc %d (expected %d), text \"%s\"%s\n", dev ? "dev" : "host", what, r, dev ? want_dev : want_host,
                       last_error, untouched ? "" : ", mv_out written");
                bad = 1;
            }
        }
    };
    Args a = good;
#define BAD(field, value, what, word) a = good; a.field = value; expect(FFHIP_EINVAL, FFHIP_EINVAL, a, what, word)
    expect(0, FFHIP_ENOSYS, a, "a well-formed call", nullptr);
    BAD(frames, nullptr, "a NULL frames", "NULL");
    BAD(mv, nullptr, "a NULL mv_out", "NULL");
    BAD(cost, nullptr, "a NULL cost_out", "NULL");
    for (int m = 0; m <= 10; m++)
        if (!predictive(m) || m > FFHIP_ME_METHOD_UMH) {
            BAD(method, m, "a method other than 8 or 9", "neither EPZS");
        }
    BAD(mb, 4, "mb_size 4", "mb_size");
    BAD(kind, 2, "cost_kind 2", "cost_kind");
    BAD(w, -1, "a negative width", "negative");
    BAD(h, -1, "a negative height", "negative");
    BAD(nf, -1, "a negative nframes", "negative");
    BAD(R, -1, "a negative search_param", "negative");
    BAD(stride, 63, "stride < width", "stride");
    BAD(pitch, P - 1, "frame_pitch < stride * height", "frame_pitch");
    BAD(dir, 2, "direction 2", "direction 2");
    BAD(dir, -1, "direction -1", "direction -1");
    BAD(nseq, -1, "a negative nseq", "negative nseq");
    BAD(spitch, 3 * P - 1, "seq_pitch one byte short", "seq_pitch");
    BAD(spitch, 0, "seq_pitch 0", "seq_pitch");
    BAD(pitch, SIZE_MAX / 2 + 1, "a frame_pitch whose multiple overflows", "seq_pitch");
    BAD(mv, fields[0] + 1, "mv_out not 4-byte aligned", "4-byte aligned");
    BAD(i1, fields[0], "mv_out == init1", "overlaps");
    BAD(i2, fields[0] + 94, "mv_out overlapping init2", "overlaps");
    BAD(cost, reinterpret_cast<uint32_t *>(fields[0] + 2), "mv_out overlapping cost_out", "overlaps");
    BAD(mv, reinterpret_cast<int16_t *>(arena + 64), "mv_out inside frames", "overlaps");
    BAD(mv, reinterpret_cast<int16_t *>(arena + 6 * P - 4), "mv_out at the last samples of frames", "overlaps");
    a = good; a.nf = INT_MAX; a.nseq = 1; expect(FFHIP_EINVAL, FFHIP_EINVAL, a, "more blocks than an int counts", "blocks");
    a = good; a.nseq = INT_MAX; expect(FFHIP_EINVAL, FFHIP_EINVAL, a, "more blocks than an int counts, by sequences", "blocks");
    a = good; a.w = 32784; a.stride = 32784; a.h = 16; a.nseq = 1; a.pitch = 16 * 32784; expect(FFHIP_EINVAL, FFHIP_EINVAL, a, "a width above 32768", "32784");
#undef BAD
    a = good; a.nf = 0; expect(0, FFHIP_ENOSYS, a, "no pictures", nullptr);
    a = good; a.nf = 1; a.pitch = 0; a.spitch = P; expect(0, FFHIP_ENOSYS, a, "one picture, no pitch", nullptr);
    a = good; a.nseq = 0; expect(0, FFHIP_ENOSYS, a, "no sequences", nullptr);
    a = good; a.w = 15; expect(0, FFHIP_ENOSYS, a, "no whole block", nullptr);
    a = good; a.nseq = 1; a.spitch = 0; expect(0, FFHIP_ENOSYS, a, "one sequence, no seq_pitch", nullptr);
    a = good; a.i1 = nullptr; a.i2 = nullptr; a.dir = 1; expect(0, FFHIP_ENOSYS, a, "NULL starting fields, direction 1", nullptr);
    a = good; a.i2 = a.i1; expect(0, FFHIP_ENOSYS, a, "init1 == init2", nullptr);
    return bad;
}

/* the checks of the faces: pointers into arenas that are never dereferenced when the call is refused.  One table per pair of faces;
 * `word`: what the text of the refusal holds, "" for no text at all, NULL for whatever it is. */
static int refusals(void)
{
    static uint8_t arena[4 * 64 * 48];
    uint8_t *cur = arena, *ref = arena + 2 * 64 * 48;
    alignas(4) static int16_t fields[4][2 * 12 * 2 + 2];
    static uint32_t cost[2 * 12];
    int bad = 0;
    struct Args { int method; const uint8_t *cur, *ref; int w, h; ptrdiff_t stride; size_t pitch; int nf, mb, R, kind; const int16_t *p1, *p2; int16_t *mv; uint32_t *cost; };
    Args good = { FFHIP_ME_METHOD_DS, cur, ref, 64, 48, 64, 64 * 48, 2, 16, 7, FFHIP_ME_SAD, fields[1], fields[2], fields[0], cost };
    bool pred = false;      /* which pair of faces expect() calls */
    auto expect = [&](int want_host, int want_dev, Args a, const char *what, const char *word) {
        auto text_ok = [&] { return !word || (word[0] ? strstr(last_error, word) != nullptr : !last_error[0]); };
        last_error[0] = 0;
        const int rh = pred ? ffhip_me_search_pred_frames_host(a.method, a.cur, a.ref, a.w, a.h, a.stride, a.pitch, a.nf, a.mb, a.R, a.kind, a.p1, a.p2, a.mv, a.cost)
                            : ffhip_me_search_frames_host(a.method, a.cur, a.ref, a.w, a.h, a.stride, a.pitch, a.nf, a.mb, a.R, a.kind, a.mv, a.cost);
        const bool th = text_ok();
        last_error[0] = 0;
        const int rd = pred ? ffhip_me_search_pred_batch_dev(a.method, a.cur, a.ref, a.w, a.h, a.stride, a.pitch, a.nf, a.mb, a.R, a.kind, a.p1, a.p2, a.mv, a.cost, nullptr)
                            : ffhip_me_search_batch_dev(a.method, a.cur, a.ref, a.w, a.h, a.stride, a.pitch, a.nf, a.mb, a.R, a.kind, a.mv, a.cost, nullptr);
        const bool td = text_ok();
        if (rh != want_host || rd != want_dev || !th || !td) {
            printf("refusals: %s face, %s: host rc %d (expected %d), dev rc %d (expected %d), text \"%s\"\n", pred ? "predictive" : "per-block", what, rh,
                   want_host, rd, want_dev, last_error);
            bad = 1;
        }
    };
    Args a = good;
#define BAD(field, value, what, word) a = good; a.field = value; expect(FFHIP_EINVAL, FFHIP_EINVAL, a, what, word)
    /* ---- the per-block faces: FFHIP_EINVAL carries no text ---- */
    expect(0, FFHIP_ENOSYS, a, "a well-formed call", nullptr);
    BAD(cur, nullptr, "a NULL cur", "");
    BAD(ref, nullptr, "a NULL ref", "");
    BAD(mv, nullptr, "a NULL mv_out", "");
    BAD(cost, nullptr, "a NULL cost_out", "");
    BAD(method, 0, "method 0", "");
    BAD(method, 10, "method 10", "");
    BAD(mb, 4, "mb_size 4", "");
    BAD(mb, 32, "mb_size 32", "");
    BAD(kind, 2, "cost_kind 2", "");
    BAD(kind, -1, "cost_kind -1", "");
    BAD(w, -1, "a negative width", "");
    BAD(h, -1, "a negative height", "");
    BAD(nf, -1, "a negative nframes", "");
    BAD(R, -1, "a negative search_param", "");
    BAD(stride, 63, "stride < width", "");
    BAD(stride, -64, "a negative stride", "");
    BAD(pitch, 64 * 48 - 1, "frame_pitch < stride * height", "");
    BAD(nf, INT_MAX, "more blocks than an int counts", "");
    for (int method = FFHIP_ME_METHOD_EPZS; method <= FFHIP_ME_METHOD_UMH; method++) {
        a = good; a.method = method;
        expect(FFHIP_ENOSYS, FFHIP_ENOSYS, a, "EPZS / UMH", method == FFHIP_ME_METHOD_EPZS ? "EPZS" : "UMH");
        expect(FFHIP_ENOSYS, FFHIP_ENOSYS, a, "EPZS / UMH", "neighbouring blocks' vectors");
    }
    a = good; a.nf = 0; expect(0, FFHIP_ENOSYS, a, "no frames", nullptr);
    a = good; a.w = 15; expect(0, FFHIP_ENOSYS, a, "no whole block", nullptr);
    a = good; a.nf = 1; a.pitch = 0; expect(0, FFHIP_ENOSYS, a, "one frame, no pitch", nullptr);
    /* ---- the predictive faces: every refusal says why ---- */
    pred = true;
    good.method = FFHIP_ME_METHOD_EPZS;
    a = good;
    expect(0, FFHIP_ENOSYS, a, "a well-formed call", nullptr);
    BAD(cur, nullptr, "a NULL cur", "NULL");
    BAD(ref, nullptr, "a NULL ref", "NULL");
    BAD(mv, nullptr, "a NULL mv_out", "NULL");
    BAD(cost, nullptr, "a NULL cost_out", "NULL");
    for (int m = 0; m <= 10; m++)
        if (!predictive(m) || m > FFHIP_ME_METHOD_UMH) {
            BAD(method, m, "a method other than 8 or 9", "neither EPZS");
        }
    BAD(mb, 4, "mb_size 4", "mb_size");
    BAD(mb, 32, "mb_size 32", "mb_size");
    BAD(kind, 2, "cost_kind 2", "cost_kind");
    BAD(kind, -1, "cost_kind -1", "cost_kind");
    BAD(w, -1, "a negative width", "negative");
    BAD(h, -1, "a negative height", "negative");
    BAD(nf, -1, "a negative nframes", "negative");
    BAD(R, -1, "a negative search_param", "negative");
    BAD(stride, 63, "stride < width", "stride");
    BAD(stride, -64, "a negative stride", "stride");
    BAD(pitch, 64 * 48 - 1, "frame_pitch < stride * height", "frame_pitch");
    BAD(nf, INT_MAX, "more blocks than an int counts", "blocks");
    BAD(mv, fields[0] + 1, "mv_out not 4-byte aligned", "4-byte aligned");
    BAD(p1, fields[0], "mv_out == prev1", "overlaps");
    BAD(p2, fields[0] + 46, "mv_out overlapping prev2", "overlaps");
    BAD(cost, reinterpret_cast<uint32_t *>(fields[0] + 2), "mv_out overlapping cost_out", "overlaps");
    BAD(mv, reinterpret_cast<int16_t *>(arena + 64), "mv_out inside cur", "overlaps");
    BAD(mv, reinterpret_cast<int16_t *>(arena + 4 * 64 * 48 - 4), "mv_out at the last samples of ref", "overlaps");
    a = good; a.w = 32784; a.stride = 32784; a.h = 16; a.nf = 1; expect(FFHIP_EINVAL, FFHIP_EINVAL, a, "a width above 32768", "32784");
    a = good; a.h = 32776; a.w = 16; a.stride = 16; a.nf = 1; expect(FFHIP_EINVAL, FFHIP_EINVAL, a, "a height above 32768", "32776");
#undef BAD
    a = good; a.nf = 0; expect(0, FFHIP_ENOSYS, a, "no frames", nullptr);
    a = good; a.w = 15; expect(0, FFHIP_ENOSYS, a, "no whole block", nullptr);
    a = good; a.nf = 1; a.pitch = 0; expect(0, FFHIP_ENOSYS, a, "one frame, no pitch", nullptr);
    a = good; a.p1 = nullptr; a.p2 = nullptr; expect(0, FFHIP_ENOSYS, a, "NULL prev fields", nullptr);
    a = good; a.p2 = a.p1; expect(0, FFHIP_ENOSYS, a, "prev1 == prev2", nullptr);
    return bad;
}

int main(void)
{
    static const int shapes[10][5] = { { 64, 48, 0, 16, 7 }, { 52, 36, 1, 16, 5 }, { 40, 40, 0, 8, 3 }, { 16, 64, 0, 16, 7 }, { 40, 8, 0, 8, 3 },
                                       { 32, 48, 0, 16, 4 }, { 72, 56, 0, 16, 0 }, { 64, 64, 0, 8, 1 }, { 96, 80, 3, 16, 32 }, { 64, 48, 0, 8, 9 } };
    int bad = 0;
    for (int i = 0; i < 10; i++)
        for (int k = 0; k < 2; k++) {
            const int mb = k ? 24 - shapes[i][3] : shapes[i][3];
            if (shapes[i][0] >= mb && shapes[i][1] >= mb)
                bad |= run(shapes[i][0], shapes[i][1], shapes[i][2], mb, shapes[i][4]);
        }
    bad |= run(64, 48, 0, 16, INT_MAX);         /* the window, the steps, the cross and the rings without overflow or an endless loop */
    bad |= run(40, 24, 5, 8, 1 << 30);
    /* whole sequences: one block row, two rows, one column, two columns, a padded stride, R = 0, a window larger than the picture */
    static const int seq_shapes[7][5] = { { 40, 8, 0, 8, 3 }, { 64, 32, 0, 16, 7 }, { 16, 64, 0, 16, 7 }, { 32, 48, 0, 16, 4 }, { 52, 36, 1, 16, 5 },
                                          { 72, 56, 0, 16, 0 }, { 96, 80, 3, 16, 32 } };
    for (int i = 0; i < 7; i++)
        bad |= run_seq(seq_shapes[i][0], seq_shapes[i][1], seq_shapes[i][2], seq_shapes[i][3], seq_shapes[i][4]);
    bad |= run_seq(64, 48, 0, 8, INT_MAX);
    bad |= refusals();
    bad |= seq_refusals();
    puts(bad ? "FAILED" : "ok");
    return bad;
}
