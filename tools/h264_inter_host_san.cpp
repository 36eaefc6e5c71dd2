/*
 * tools/h264_inter_host_san.cpp — a stand-alone host program over ffhip_h264_inter_plan_pictures_host() and the argument checks of
 * ffhip_h264_inter_pictures_dev() for AddressSanitizer and UBSan: random and malformed pictures (slice indices, ref_idx, num_ref, slots,
 * denominators and use_weight out of range) in heap blocks exactly as large as the geometry says, so a read or write outside a map
 * is an error the sanitizer reports; then the refusals and the row-overlap rule of the _dev face on pointers it never follows.  CPU
 * only: nothing here touches a device.
 *
 * Build and run from the repository root (the face's file and this one, nothing else of the library):
 *   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
 *         --offload-arch=gfx950 -Iinclude -Iffmpeg_amd/csrc -Iffmpeg_amd/csrc/host ffmpeg_amd/csrc/shims_h264_inter.hip \
 *         tools/h264_inter_host_san.cpp -o h264_inter_host_san && ./h264_inter_host_san
 * Prints a checksum of the plans per case and "ok"; the sanitizer aborts on the first finding.
 */
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ffhip.h"

/* what shims_h264_inter.hip takes from the rest of the library */
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

static uint32_t rnd_state = 54321;
static uint32_t rnd(void)
{
    rnd_state = rnd_state * 1664525u + 1013904223u;
    return rnd_state >> 8;
}

template <class T>
static T *block(size_t n)
{
    return static_cast<T *>(malloc(n * sizeof(T) ? n * sizeof(T) : 1));
}

static int run(int mb_w, int mb_h, int nslices, int nrefs, int pad, bool malformed)
{
    const size_t nmb = (size_t)mb_w * mb_h;
    const int w4 = 4 * mb_w, h4 = 4 * mb_h, stride = w4 + pad;
    /* the last row of the motion field ends with the picture, not with the stride */
    const size_t nmvf = (size_t)(h4 - 1) * stride + w4;
    FFHipH264BsMb *mb = block<FFHipH264BsMb>(nmb);
    FFHipH264MvField *mvf = block<FFHipH264MvField>(nmvf);
    FFHipH264InterSlice *slices = block<FFHipH264InterSlice>(nslices);
    FFHipH264InterBlockPlan *plans = block<FFHipH264InterBlockPlan>(nmb * 16);
    for (size_t i = 0; i < nmb; i++) {
        memset(&mb[i], 0, sizeof(mb[i]));
        mb[i].slice = (uint16_t)(malformed && rnd() % 8 == 0 ? rnd() : (i * nslices) / nmb);
        mb[i].flags = (uint8_t)(malformed ? rnd() % 4 : rnd() % 5 == 0);
    }
    for (size_t i = 0; i < nmvf; i++) {
        memset(&mvf[i], 0, sizeof(mvf[i]));
        for (int l = 0; l < 2; l++) {
            mvf[i].mv[l][0] = (int16_t)rnd();
            mvf[i].mv[l][1] = (int16_t)rnd();
            mvf[i].ref_idx[l] = (int8_t)(!malformed ? (int)(rnd() % 4) - 1 : rnd() % 8 ? (int)(rnd() % 36) - 2 : (int)rnd());
        }
    }
    for (int s = 0; s < nslices; s++) {
        uint8_t *raw = reinterpret_cast<uint8_t *>(&slices[s]);
        for (size_t k = 0; k < sizeof(slices[s]); k++)
            raw[k] = (uint8_t)rnd();                    /* weights of every value */
        if (malformed && s % 2)
            continue;                                   /* every field random: lists, counts, denominators, use_weight */
        for (int l = 0; l < 2; l++) {
            for (int k = 0; k < 32; k++)
                slices[s].ref[l][k] = (uint8_t)(rnd() % (nrefs ? nrefs : 1));
            slices[s].num_ref[l] = (uint8_t)(malformed ? rnd() % 40 : 3);
        }
        slices[s].use_weight = (uint8_t)(rnd() % 3);
        slices[s].use_weight_chroma = (uint8_t)(rnd() & 1);
        slices[s].luma_log2_denom = (uint8_t)(rnd() % 8);
        slices[s].chroma_log2_denom = (uint8_t)(rnd() % 8);
    }
    FFHipH264InterPlanPic pic;
    memset(&pic, 0, sizeof(pic));
    pic.mb = mb; pic.mvf = mvf; pic.slices = slices; pic.plans = plans;
    pic.mvf_stride = stride; pic.nslices = nslices; pic.nrefs = nrefs;
    const int r = ffhip_h264_inter_plan_pictures_host(mb_w, mb_h, 1, &pic);
    uint32_t sum = 0, modes[5] = { 0, 0, 0, 0, 0 };
    for (size_t i = 0; i < nmb * 16 * sizeof(FFHipH264InterBlockPlan); i++)
        sum = sum * 31 + reinterpret_cast<const uint8_t *>(plans)[i];
    int bad = r != 0;
    for (size_t i = 0; i < nmb * 16; i++) {
        bad |= plans[i].mode > FFHIP_H264_INTER_BI_W || plans[i].slot[0] >= 32 || plans[i].slot[1] >= 32 ||
               (plans[i].mode && (plans[i].slot[0] >= nrefs || plans[i].slot[1] >= nrefs)) || plans[i].luma_log2_denom > 7 ||
               plans[i].chroma_log2_denom > 7;
        modes[plans[i].mode <= 4 ? plans[i].mode : 0]++;
    }
    printf("%d x %d slices %d refs %d pad %d malformed %d: rc %d modes %u %u %u %u %u checksum %08x\n", mb_w, mb_h, nslices, nrefs, pad, (int)malformed,
           r, modes[0], modes[1], modes[2], modes[3], modes[4], sum);
    free(mb); free(mvf); free(slices); free(plans);
    return bad;
}

/* the _dev face's checks: pointers into one arena that is never dereferenced */
static int refusals(void)
{
    static uint8_t arena[1 << 20];
    FFHipH264InterPic *pics = block<FFHipH264InterPic>(3);
    int bad = 0;
    auto fill = [&](int n, int mb_w, int ps) {
        uint8_t *at = arena;
        auto take = [&](size_t bytes) { uint8_t *p = at; at += (bytes + 63) & ~(size_t)63; return p; };
        memset(pics, 0, 3 * sizeof(*pics));
        for (int i = 0; i < n; i++) {
            for (int p = 0; p < 3; p++) {
                pics[i].dst_stride[p] = (ptrdiff_t)(p ? 8 : 16) * mb_w * ps;
                pics[i].dst[p] = take((size_t)pics[i].dst_stride[p] * 64);
            }
            pics[i].mb = reinterpret_cast<const FFHipH264BsMb *>(take(4096));
            pics[i].mvf = reinterpret_cast<const FFHipH264MvField *>(take(16384));
            pics[i].slices = reinterpret_cast<const FFHipH264InterSlice *>(take(2888));
            pics[i].mvf_stride = 4 * mb_w; pics[i].nslices = 1; pics[i].nrefs = 32;
            for (int k = 0; k < 32; k++)
                for (int p = 0; p < 3; p++) {
                    pics[i].ref[k].stride[p] = (ptrdiff_t)(p ? 8 : 16) * mb_w * ps;
                    pics[i].ref[k].base[p] = take((size_t)pics[i].ref[k].stride[p] * 32);
                }
        }
    };
    auto expect = [&](int want, int bd, int cfi, int w, int h, int n, const char *what) {
        const int r = ffhip_h264_inter_pictures_dev(bd, cfi, w, h, n, pics, nullptr);
        if (r != want) {
            printf("refusals: %s: rc %d, expected %d\n", what, r, want);
            bad = 1;
        }
    };
    quiet = true;
    fill(3, 2, 1); expect(FFHIP_ENOSYS, 8, 1, 2, 2, 3, "three pictures, 32 references each");
    fill(3, 2, 2); expect(FFHIP_ENOSYS, 14, 1, 2, 2, 3, "16-bit samples");
    fill(1, 2, 1); expect(FFHIP_ENOSYS, 8, 2, 2, 2, 1, "4:2:2");
    fill(1, 2, 1); expect(FFHIP_EINVAL, 11, 1, 2, 2, 1, "depth 11");
    fill(1, 2, 1); expect(FFHIP_EINVAL, 8, 1, 4097, 2, 1, "mb_w 4097");
    fill(1, 2, 1); expect(FFHIP_EINVAL, 8, 1, 2, 2, 0, "npics 0");
    fill(1, 2, 1); pics[0].nrefs = 33; expect(FFHIP_EINVAL, 8, 1, 2, 2, 1, "nrefs 33");
    fill(1, 2, 1); pics[0].dst[2] = nullptr; expect(FFHIP_EINVAL, 8, 1, 2, 2, 1, "Cr alone missing");
    fill(1, 2, 1); pics[0].ref[31].base[1] = nullptr; expect(FFHIP_EINVAL, 8, 1, 2, 2, 1, "a NULL reference plane");
    fill(2, 2, 1); pics[1].ref[7].base[0] = pics[0].dst[0] + 3; expect(FFHIP_EINVAL, 8, 1, 2, 2, 2, "a reference inside another picture's destination");
    fill(1, 2, 1); /* the two fields of one frame: destination the top field, reference 0 the bottom field */
    for (int p = 0; p < 3; p++) {
        pics[0].ref[0].base[p] = pics[0].dst[p] + pics[0].dst_stride[p];
        pics[0].dst_stride[p] *= 2;
        pics[0].ref[0].stride[p] = pics[0].dst_stride[p];
    }
    expect(FFHIP_ENOSYS, 8, 1, 2, 1, 1, "a field predicted from the other field of its frame");
    pics[0].ref[0].base[0] -= 1; expect(FFHIP_EINVAL, 8, 1, 2, 1, 1, "... one byte into the destination's rows");
    fill(1, 2, 1); pics[0].ref[3].stride[0] = -pics[0].ref[3].stride[0]; pics[0].ref[3].base[0] += 31 * 32;
    expect(FFHIP_ENOSYS, 8, 1, 2, 2, 1, "a reference with a negative stride");
    quiet = false;
    free(pics);
    return bad;
}

int main(void)
{
    int bad = 0;
    for (int k = 0; k < 24; k++) {
        const int mb_w = 1 + (int)(rnd() % 11), mb_h = 1 + (int)(rnd() % 9);
        bad |= run(mb_w, mb_h, 1 + (int)(rnd() % 4), (int)(rnd() % 33), (int)(rnd() % 4), k >= 8);
    }
    bad |= run(120, 68, 4, 16, 0, false);
    bad |= run(120, 68, 4, 3, 3, true);
    bad |= refusals();
    puts(bad ? "FAILED" : "ok");
    return bad;
}
