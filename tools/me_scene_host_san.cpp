/*
 * tools/me_scene_host_san.cpp — a stand-alone host program over ffhip_me_scene_sequence_host() and ffhip_me_interp_sequence_scd_host()
 * and the argument checks they share with their device faces, for AddressSanitizer and UBSan: odd widths, heights, strides and pitches
 * at depths 8, 10 and 16, a frames address misaligned by 1..15 bytes (2..14 above 8 bits), 1 and 3 sequences of 1..5 pictures — in heap
 * blocks exactly as large as the geometry says: the pictures end at the last sample of the last row of the last picture
 * ((rows - 1) * stride + width samples, not rows * stride), every output at its last element, mafd_in and mafd_out at nseq doubles, the
 * scene flags at (nframes - 1) * nseq bytes.  A read or write outside them is an error the sanitizer reports.  The sums are checked
 * against a loop of this file, the carry against a second call that continues the first.  Then the refusals of all four faces on
 * pointers they never follow.  CPU only: nothing here touches a device.
 *
 * Build and run from the repository root (the faces' file and this one, nothing else of the library):
 *   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
 *         --offload-arch=gfx950 -Iinclude -Iffmpeg_amd/csrc -Iffmpeg_amd/csrc/host ffmpeg_amd/csrc/me_api.hip \
 *         tools/me_scene_host_san.cpp -o me_scene_host_san && ./me_scene_host_san
 * Prints a checksum per case and "ok"; the sanitizer aborts on the first finding.
 */
#include <math.h>
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

static uint32_t rnd_state = 97531;
static uint32_t rnd(void)
{
    rnd_state = rnd_state * 1664525u + 1013904223u;
    return rnd_state >> 8;
}

/* n bytes exactly, `mis` bytes behind a 16-byte boundary: the byte after them is the sanitizer's.  *raw is what free() takes */
static uint8_t *block(size_t n, int mis, void **raw)
{
    /* slack in FRONT only: the end of the n bytes is the end of the allocation */
    if (posix_memalign(raw, 16, mis + n ? mis + n : 1))
        abort();
    uint8_t *q = static_cast<uint8_t *>(*raw) + mis;
    for (size_t i = 0; i < n; i++)
        q[i] = (uint8_t)rnd();
    return q;
}

static int run_scene(int depth, int w, int h, int pad, int nframes, int nseq, int mis, double threshold)
{
    const int px = depth > 8 ? 2 : 1;
    const ptrdiff_t stride = (ptrdiff_t)(w + pad) * px;
    const size_t pic = (size_t)stride * h, frame_pitch = pic + 6 * px, seq_pitch = (size_t)(nframes > 0 ? nframes - 1 : 0) * frame_pitch + pic + 2 * px;
    const size_t last = (size_t)(h - 1) * stride + (size_t)w * px;
    const int steps = nframes > 1 ? nframes - 1 : 0, npairs = steps * nseq;
    void *raw[8];
    uint8_t *frames = block(nframes > 0 ? (nseq - 1) * seq_pitch + (size_t)(nframes - 1) * frame_pitch + last : 0, mis, &raw[0]);
    double *mafd_in = reinterpret_cast<double *>(block(nseq * 8, 0, &raw[1])), *mafd_out = reinterpret_cast<double *>(block(nseq * 8, 0, &raw[2]));
    double *mafd_mid = reinterpret_cast<double *>(block(nseq * 8, 0, &raw[3]));
    uint64_t *sad = reinterpret_cast<uint64_t *>(block((size_t)npairs * 8, 0, &raw[4])), *sad2 = reinterpret_cast<uint64_t *>(block((size_t)npairs * 8, 0, &raw[5]));
    float *score = reinterpret_cast<float *>(block((size_t)npairs * 4, 0, &raw[6]));
    uint8_t *flags = block((size_t)npairs, 0, &raw[7]);
    for (int s = 0; s < nseq; s++)
        mafd_in[s] = (double)(rnd() % 6000) / 100.0;
    int bad = 0;
    int r = ffhip_me_scene_sequence_host(frames, depth, w, h, stride, frame_pitch, nframes, seq_pitch, nseq, threshold, mafd_in, mafd_out, sad, score, flags);
    if (r) {
        printf("depth %d %dx%d+%d frames %d seqs %d: %d (%s)\n", depth, w, h, pad, nframes, nseq, r, last_error);
        bad++;
    }
    /* the sums, by a loop of this file */
    for (int s = 0; s < nseq && !bad; s++)
        for (int k = 0; k < steps; k++) {
            const uint8_t *A = frames + s * seq_pitch + k * frame_pitch, *B = A + frame_pitch;
            uint64_t want = 0;
            for (int y = 0; y < h; y++)
                for (int x = 0; x < w; x++) {
                    int a, b;
                    if (px == 2) {
                        uint16_t a16, b16;
                        memcpy(&a16, A + y * stride + 2 * x, 2);
                        memcpy(&b16, B + y * stride + 2 * x, 2);
                        a = a16;
                        b = b16;
                    } else {
                        a = A[y * stride + x];
                        b = B[y * stride + x];
                    }
                    want += (uint64_t)abs(a - b);
                }
            if (sad[(size_t)k * nseq + s] != want || flags[(size_t)k * nseq + s] > 1) {
                printf("depth %d %dx%d+%d: pair %d of sequence %d: sad %llu, expected %llu, flag %d\n", depth, w, h, pad, k, s,
                       (unsigned long long)sad[(size_t)k * nseq + s], (unsigned long long)want, flags[(size_t)k * nseq + s]);
                bad++;
            }
        }
    /* one call equals two joined through mafd_out and mafd_in; the second takes the sums alone */
    if (!bad && nframes >= 3) {
        const int cut = nframes / 2;
        r = ffhip_me_scene_sequence_host(frames, depth, w, h, stride, frame_pitch, cut + 1, seq_pitch, nseq, threshold, mafd_in, mafd_mid, sad2, nullptr, nullptr);
        r |= ffhip_me_scene_sequence_host(frames + cut * frame_pitch, depth, w, h, stride, frame_pitch, nframes - cut, seq_pitch, nseq, threshold, mafd_mid,
                                          mafd_in, sad2 + (size_t)cut * nseq, nullptr, nullptr);
        if (r || memcmp(sad, sad2, (size_t)npairs * 8) || memcmp(mafd_in, mafd_out, nseq * 8)) {
            printf("depth %d %dx%d+%d frames %d seqs %d: two calls differ from one (%d, %s)\n", depth, w, h, pad, nframes, nseq, r, last_error);
            bad++;
        }
    }
    uint32_t sum = 0;
    for (int i = 0; i < npairs; i++) {
        uint32_t bits;
        memcpy(&bits, &score[i], 4);
        sum = (sum * 31 + (uint32_t)sad[i]) * 31 + bits + flags[i];
    }
    printf("depth %2d %4dx%-2d +%-2d frames %d seqs %d mis %2d: %08x\n", depth, w, h, pad, nframes, nseq, mis, sum);
    for (void *p : raw)
        free(p);
    return bad;
}

/* the scd host face over flags in a block of exactly (nframes - 1) * nseq bytes, both actions; luma and 4:2:0 */
static int run_scd(int w, int h, int nplanes, int action)
{
    enum { NSEQ = 2, NFRAMES = 3, NJOBS = 6 };
    const int mb = 16, lg = 4, bw = w >> lg, bh = h >> lg, pad[3] = { 3, 0, 5 };
    const size_t per = (size_t)bw * bh, nfield = 2 * per * NSEQ * (NFRAMES - 1);
    static const int alphas[NJOBS] = { 512, 513, 0, 1024, 341, 512 };
    FFHipMeInterpJob jobs[NJOBS];
    for (int j = 0; j < NJOBS; j++)
        jobs[j] = { j % NSEQ, (j / 2) % (NFRAMES - 1), alphas[j], j == 4 ? FFHIP_ME_INTERP_BLEND : FFHIP_ME_INTERP_MCI };
    void *raw[16];
    int nraw = 0;
    FFHipMePlanes src = {}, dst = {};
    for (int i = 0; i < nplanes; i++) {
        const int pw = i ? (w + 1) >> 1 : w, ph = i ? (h + 1) >> 1 : h;
        const size_t last = (size_t)(ph - 1) * (pw + pad[i]) + pw;
        src.stride[i] = dst.stride[i] = pw + pad[i];
        src.frame_pitch[i] = (size_t)ph * (pw + pad[i]) + 7;
        src.seq_pitch[i] = NFRAMES * src.frame_pitch[i] + 1;
        dst.frame_pitch[i] = (size_t)ph * (pw + pad[i]);
        src.base[i] = block((NSEQ - 1) * src.seq_pitch[i] + (NFRAMES - 1) * src.frame_pitch[i] + last, 0, &raw[nraw++]);
        dst.base[i] = block((NJOBS - 1) * dst.frame_pitch[i] + last, 0, &raw[nraw++]);
    }
    int16_t *f[2];
    for (int d = 0; d < 2; d++) {
        f[d] = reinterpret_cast<int16_t *>(block(nfield * 2, 0, &raw[nraw++]));
        for (size_t e = 0; e < nfield / 2; e++) {
            const int bx = (int)(e % per) % (bw ? bw : 1), by = (int)(e % per) / (bw ? bw : 1);
            f[d][2 * e] = (int16_t)((bx << lg) + (int)(rnd() % 17) - 8);
            f[d][2 * e + 1] = (int16_t)((by << lg) + (int)(rnd() % 17) - 8);
        }
    }
    uint8_t *window = block((size_t)4 * mb * mb, 0, &raw[nraw++]);
    uint8_t *scene = block((NFRAMES - 1) * NSEQ, 0, &raw[nraw++]);
    for (int i = 0; i < (NFRAMES - 1) * NSEQ; i++)
        scene[i] = (uint8_t)(i % 2 ? 0 : 1 + rnd() % 255);
    int bad = 0;
    const int r = ffhip_me_interp_sequence_scd_host(&src, &dst, nplanes, 1, 1, w, h, NFRAMES, NSEQ, mb, 8, window, f[0], f[1], jobs, NJOBS, scene, action);
    if (r) {
        printf("scd %dx%d planes %d action %d: %d (%s)\n", w, h, nplanes, action, r, last_error);
        bad++;
    }
    /* a flagged MCI job under DUP is picture A or B, sample for sample */
    for (int j = 0; j < NJOBS && !bad && action == FFHIP_ME_SCENE_DUP; j++) {
        if (jobs[j].mode != FFHIP_ME_INTERP_MCI || !scene[jobs[j].pair * NSEQ + jobs[j].seq])
            continue;
        for (int i = 0; i < nplanes; i++) {
            const int pw = i ? (w + 1) >> 1 : w, ph = i ? (h + 1) >> 1 : h;
            const uint8_t *P = src.base[i] + jobs[j].seq * src.seq_pitch[i] + (jobs[j].pair + (jobs[j].alpha > 512)) * src.frame_pitch[i];
            for (int y = 0; y < ph; y++)
                if (memcmp(dst.base[i] + j * dst.frame_pitch[i] + (size_t)y * dst.stride[i], P + (size_t)y * src.stride[i], pw)) {
                    printf("scd %dx%d planes %d: job %d plane %d row %d is not the duplicated picture\n", w, h, nplanes, j, i, y);
                    bad++;
                }
        }
    }
    uint64_t counts[8];
    ffhip_me_interp_host_counts(counts);
    printf("scd %dx%d planes %d action %d: samples %llu of them by a blend or an action %llu\n", w, h, nplanes, action, (unsigned long long)counts[6],
           (unsigned long long)counts[7]);
    for (int i = 0; i < nraw; i++)
        free(raw[i]);
    return bad;
}

/* all four faces refuse, with a text, before they follow a pointer */
static int refusals(void)
{
    uint8_t *const wild = reinterpret_cast<uint8_t *>(64);
    double *const wd = reinterpret_cast<double *>(1 << 20), *const wd2 = reinterpret_cast<double *>(2 << 20);
    uint64_t *const ws = reinterpret_cast<uint64_t *>(3 << 20);
    float *const wf = reinterpret_cast<float *>(4 << 20);
    uint8_t *const wfl = reinterpret_cast<uint8_t *>(5 << 20);
    int bad = 0;
    auto both = [&](const char *what, int want, const uint8_t *frames, int depth, int w, int h, ptrdiff_t stride, size_t fp, int nframes, size_t sp, int nseq,
                    double thr, const double *in, double *out, uint64_t *sad, float *score, uint8_t *flags) {
        for (int face = 0; face < 2; face++) {
            last_error[0] = 0;
            const int r = face ? ffhip_me_scene_sequence_dev(frames, depth, w, h, stride, fp, nframes, sp, nseq, thr, in, out, sad, score, flags, nullptr)
                               : ffhip_me_scene_sequence_host(frames, depth, w, h, stride, fp, nframes, sp, nseq, thr, in, out, sad, score, flags);
            if (r != want || (want == FFHIP_EINVAL) != (last_error[0] != 0)) {
                printf("refusal `%s`, face %d: %d (%s)\n", what, face, r, last_error);
                bad++;
            }
        }
    };
    const int E = FFHIP_EINVAL;
    both("null frames", E, nullptr, 8, 64, 32, 64, 2048, 3, 8192, 2, 10.0, wd, wd2, ws, wf, wfl);
    both("no output", E, wild, 8, 64, 32, 64, 2048, 3, 8192, 2, 10.0, wd, wd2, nullptr, nullptr, nullptr);
    both("depth", E, wild, 17, 64, 32, 128, 4096, 3, 16384, 2, 10.0, wd, wd2, ws, wf, wfl);
    both("width", E, wild, 8, 0, 32, 64, 2048, 3, 8192, 2, 10.0, wd, wd2, ws, wf, wfl);
    both("height", E, wild, 8, 64, 32769, 64, 2048, 3, 8192, 2, 10.0, wd, wd2, ws, wf, wfl);
    both("negative", E, wild, 8, 64, 32, 64, 2048, -3, 8192, 2, 10.0, wd, wd2, ws, wf, wfl);
    both("stride", E, wild, 10, 64, 32, 127, 4096, 3, 16384, 2, 10.0, wd, wd2, ws, wf, wfl);
    both("odd", E, wild + 1, 10, 64, 32, 128, 4096, 3, 16384, 2, 10.0, wd, wd2, ws, wf, wfl);
    both("frame_pitch", E, wild, 8, 64, 32, 64, 2047, 3, 8192, 2, 10.0, wd, wd2, ws, wf, wfl);
    both("seq_pitch", E, wild, 8, 64, 32, 64, 2048, 3, 6143, 2, 10.0, wd, wd2, ws, wf, wfl);
    both("threshold", E, wild, 8, 64, 32, 64, 2048, 3, 8192, 2, NAN, wd, wd2, ws, wf, wfl);
    both("overlap", E, wild, 8, 64, 32, 64, 2048, 3, 8192, 2, 10.0, wd, wd2, ws, reinterpret_cast<float *>(ws + 3), wfl);
    both("pairs", E, wild, 8, 8, 2, 8, 16, 65537, 65537 * 16, 32768, 10.0, nullptr, nullptr, nullptr, nullptr, wfl);
    /* no sequence: nothing to do, in both faces; the legal call gets as far as the missing device in the device face */
    both("no sequence", 0, wild, 8, 64, 32, 64, 2048, 3, 8192, 0, 10.0, nullptr, nullptr, ws, wf, wfl);
    last_error[0] = 0;
    const int r = ffhip_me_scene_sequence_dev(wild, 8, 64, 32, 64, 2048, 3, 8192, 2, 10.0, wd, wd2, ws, wf, wfl, nullptr);
    if (r != FFHIP_ENOSYS || last_error[0]) {
        printf("the legal call: %d (%s)\n", r, last_error);
        bad++;
    }
    /* the scd faces: an unknown action, dst on the flags */
    FFHipMePlanes src = {}, dst = {};
    for (int i = 0; i < 3; i++) {
        src.base[i] = wild + i * (1 << 20);
        dst.base[i] = wild + (1 << 24) + i * (1 << 20);
        src.stride[i] = dst.stride[i] = 64;
        src.frame_pitch[i] = dst.frame_pitch[i] = 1 << 12;
        src.seq_pitch[i] = 1 << 16;
    }
    const FFHipMeInterpJob good[2] = { { 0, 0, 7, FFHIP_ME_INTERP_MCI }, { 1, 1, 1024, FFHIP_ME_INTERP_BLEND } };
    const int16_t *const wmv = reinterpret_cast<const int16_t *>(7 << 20);
    for (int face = 0; face < 2; face++)
        for (int what = 0; what < 2; what++) {
            const uint8_t *scene = what ? dst.base[1] + 5 : wfl;
            const int action = what ? FFHIP_ME_SCENE_DUP : 3;
            last_error[0] = 0;
            const int q = face ? ffhip_me_interp_sequence_scd_dev(&src, &dst, 3, 1, 1, 64, 32, 3, 2, 16, 8, wild, wmv, wmv, good, 2, scene, action, nullptr)
                               : ffhip_me_interp_sequence_scd_host(&src, &dst, 3, 1, 1, 64, 32, 3, 2, 16, 8, wild, wmv, wmv, good, 2, scene, action);
            if (q != FFHIP_EINVAL || !last_error[0]) {
                printf("scd refusal %d, face %d: %d (%s)\n", what, face, q, last_error);
                bad++;
            }
        }
    return bad;
}

int main(void)
{
    static const int widths[] = { 1, 3, 15, 16, 17, 63, 65, 257, 1000 }, heights[] = { 1, 2, 5, 37 }, pads[] = { 0, 1, 13 }, depths[] = { 8, 10, 16 };
    int bad = 0, k = 0;
    for (int depth : depths)
        for (int w : widths)
            for (int h : heights)
                for (int pad : pads) {
                    const int mis = depth > 8 ? 2 * (1 + k % 7) : 1 + k % 15;
                    bad += run_scene(depth, w, h, pad, 1 + k % 5, k % 2 ? 3 : 1, mis, k % 3 ? 10.0 : 0.5);
                    k++;
                }
    bad += run_scene(16, 256, 257, 0, 2, 1, 0, 50.0);       /* the shape of the tests' saturation case, random samples */
    bad += run_scene(8, 7, 3, 2, 0, 2, 5, 10.0);            /* no picture at all */
    for (int action = FFHIP_ME_SCENE_BLEND; action <= FFHIP_ME_SCENE_DUP; action++) {
        bad += run_scd(52, 38, 3, action);
        bad += run_scd(53, 37, 1, action);
    }
    bad += refusals();
    if (bad) {
        printf("%d FAILED\n", bad);
        return 1;
    }
    printf("ok\n");
    return 0;
}
