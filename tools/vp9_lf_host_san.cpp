/*
 * tools/vp9_lf_host_san.cpp — a stand-alone host program over ffhip_vp9_lf_tables_pictures_host() for AddressSanitizer and UBSan:
 * random partitions and malformed record sets (any byte in any field, sb_first decreasing or beyond nblocks, hundreds of records in
 * a superblock) in heap blocks exactly as large as the geometry says, so a read or write outside an array is an error the sanitizer
 * reports.  CPU only: nothing here touches a device.
 *
 * Build and run from the repository root (the face's file and this one, nothing else of the library):
 *   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
 *         --offload-arch=gfx950 -Iinclude -Iffmpeg_amd/csrc -Iffmpeg_amd/csrc/host ffmpeg_amd/csrc/shims_vp9_lf_tab.hip \
 *         tools/vp9_lf_host_san.cpp -o vp9_lf_host_san && ./vp9_lf_host_san
 * Prints a checksum of the tables per case and "ok"; the sanitizer aborts on the first finding.
 */
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ffhip.h"

/* what shims_vp9_lf_tab.hip takes from the rest of the library */
extern "C" void ffhip_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
}
int ffhip_have_device(void) { return 0; }
struct ihipStream_t;
int ffhip_launch_vp9_lf_tables_pictures(int, int, int, int, int, const FFHipVp9LfTabPic *, ihipStream_t *) { return FFHIP_ENOSYS; }

static uint32_t rnd_state = 24680;
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

/* a quad-tree partition of one superblock into valid records */
static size_t partition(FFHipVp9LfBlock *out, int r7, int c7, int n)
{
    static const int bs_of_square[9] = { 0, 9, 6, 0, 3, 0, 0, 0, 0 };
    if (n > 1 && rnd() % 100 < 55) {
        size_t k = 0;
        for (int q = 0; q < 4; q++)
            k += partition(out + k, r7 + (q >> 1) * (n / 2), c7 + (q & 1) * (n / 2), n / 2);
        return k;
    }
    const int bs = n == 1 && (rnd() & 1) ? 10 + (int)(rnd() % 3) : bs_of_square[n];
    const int max_tx = bs > 9 ? 0 : n >= 4 ? 3 : n;
    out->pos = (uint8_t)(r7 << 3 | c7);
    out->bs = (uint8_t)bs;
    out->tx_skip = (uint8_t)(rnd() % (max_tx + 1) | (rnd() % 3 == 0) << 2);
    out->lvl_idx = (uint8_t)(rnd() & 63);
    return 1;
}

static int run(int ss_h, int ss_v, int cols, int rows, int mode /* 0 valid, 1 random bytes, 2 crowded, 3 no records */)
{
    const int sbc = (cols + 7) >> 3, sbr = (rows + 7) >> 3, nsb = sbc * sbr;
    const size_t per = mode == 2 ? 200 : 64;
    FFHipVp9LfBlock *tmp = block<FFHipVp9LfBlock>((size_t)nsb * per);
    uint32_t *sb_first = block<uint32_t>((size_t)nsb + 1);
    size_t n = 0;
    for (int sb = 0; sb < nsb; sb++) {
        sb_first[sb] = (uint32_t)n;
        if (mode == 0)
            n += partition(tmp + n, 0, 0, 8);
        else if (mode == 1 || mode == 2)
            for (size_t k = 0, cnt = mode == 2 ? per : rnd() % per; k < cnt; k++, n++) {
                const uint32_t v = mode == 1 && rnd() % 4 == 0 ? rnd() << 8 ^ rnd() : (rnd() & 63) | (rnd() % 13) << 8 | (rnd() & 7) << 16 | (rnd() & 63) << 24;
                memcpy(tmp + n, &v, 4);
            }
    }
    sb_first[nsb] = (uint32_t)n;
    uint32_t nblocks = (uint32_t)n;
    if (mode == 1) { /* decreasing pairs, entries beyond nblocks, nblocks below the last entry */
        for (int sb = 0; sb <= nsb; sb++)
            if (rnd() % 5 == 0)
                sb_first[sb] = rnd() % 3 ? rnd() % (uint32_t)(n + 1) : rnd() << 8;
        nblocks = (uint32_t)(n - n / 7);
    }
    /* the records in a block of exactly nblocks */
    FFHipVp9LfBlock *blocks = block<FFHipVp9LfBlock>(nblocks);
    memcpy(blocks, tmp, (size_t)nblocks * sizeof(*blocks));
    free(tmp);
    FFHipVp9LfSb *tables = block<FFHipVp9LfSb>(nsb);
    FFHipVp9LfSbC *ctables = ss_h != ss_v ? block<FFHipVp9LfSbC>(nsb) : nullptr;
    FFHipVp9Filter *filters = rnd() & 1 ? block<FFHipVp9Filter>(nsb) : nullptr;
    FFHipVp9LfTabPic pic;
    memset(&pic, 0, sizeof(pic));
    pic.blocks = nblocks ? blocks : nullptr;
    pic.sb_first = sb_first;
    pic.nblocks = nblocks;
    for (int i = 0; i < 64; i++) {
        pic.level[i] = (uint8_t)(rnd() % 8 ? rnd() & 63 : 0);
        pic.lim_lut[i] = (uint8_t)rnd();
        pic.mblim_lut[i] = (uint8_t)rnd();
    }
    pic.tables = tables; pic.ctables = ctables; pic.filters = filters;
    const int r = ffhip_vp9_lf_tables_pictures_host(ss_h, ss_v, cols, rows, 1, &pic);
    uint32_t sum = 0;
    for (size_t i = 0; i < (size_t)nsb * sizeof(*tables); i++)
        sum = sum * 31 + ((const uint8_t *)tables)[i];
    for (size_t i = 0; ctables && i < (size_t)nsb * sizeof(*ctables); i++)
        sum = sum * 31 + ((const uint8_t *)ctables)[i];
    for (size_t i = 0; filters && i < (size_t)nsb * sizeof(*filters); i++)
        sum = sum * 31 + ((const uint8_t *)filters)[i];
    printf("ss %d %d, %d x %d blocks, mode %d, %u records: rc %d checksum %08x\n", ss_h, ss_v, cols, rows, mode, nblocks, r, sum);
    free(blocks); free(sb_first); free(tables); free(ctables); free(filters);
    return r;
}

int main(void)
{
    int bad = 0;
    for (int k = 0; k < 48; k++) {
        const int cols = 1 + (int)(rnd() % 40), rows = 1 + (int)(rnd() % 30);
        bad |= run(k & 1, (k >> 1) & 1, cols, rows, (k >> 2) % 4) != 0;
    }
    for (int ss = 0; ss < 4; ss++) {
        bad |= run(ss & 1, ss >> 1, 480, 270, 0) != 0;
        bad |= run(ss & 1, ss >> 1, 479, 269, 1) != 0;
    }
    puts(bad ? "FAILED" : "ok");
    return bad;
}
