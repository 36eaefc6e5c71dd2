/* kernels/h264_mc_rules.h on the CPU against the oracle (oracle/liboracle.so): the per-sample luma statement at all 16 positions, the
 * chroma statement at all 64 fractions, weight / biweight over the ladder of tests/test_gpu_mc_matrix.py::h264_weight_cells, the packed
 * average against the scalar one.  Prints the first disagreement and exits 1; prints the number of comparisons and exits 0.
 * Built and run by tests/test_h264_mc_rules_cpu.py. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

extern "C" {
#include "ffo.h"
}
#include "kernels/h264_mc_rules.h"

static uint32_t rng_state = 12345;
static uint32_t rnd() { return rng_state = rng_state * 1664525u + 1013904223u, rng_state >> 8; }

template <class P>
struct Win {
    const P *p;      /* the sample under the output sample */
    ptrdiff_t s;
    int at(int dx, int dy) const { return (int)p[dy * s + dx]; }
};

static long checks = 0;
#define FAIL(...) do { printf(__VA_ARGS__); printf("\n"); exit(1); } while (0)

/* kind 0: random samples; 1: only 0 and maxv */
template <class P>
static void fill(P *a, int n, int maxv, int kind)
{
    for (int i = 0; i < n; i++)
        a[i] = (P)(kind ? (rnd() & 1 ? maxv : 0) : rnd() % (unsigned)(maxv + 1));
}

template <class P>
static void luma(int bd)
{
    const int maxv = (1 << bd) - 1, W = 9;      /* a 4 x 4 block's window: 2 samples before, 3 after */
    P win[W * W], dst[4 * W], old[4 * W];
    for (int rep = 0; rep < 400; rep++) {
        fill(win, W * W, maxv, rep & 1);
        fill(old, 4 * W, maxv, (rep >> 1) & 1);
        for (int mc = 0; mc < 16; mc++)
            for (int avg = 0; avg < 2; avg++) {
                for (int i = 0; i < 4 * W; i++)
                    dst[i] = old[i];
                ffo_h264_qpel_bd(bd, avg, 2, mc, (uint8_t *)dst, (const uint8_t *)(win + 2 * W + 2), W * sizeof(P));
                for (int y = 0; y < 4; y++)
                    for (int x = 0; x < 4; x++) {
                        const Win<P> S = { win + (2 + y) * W + 2 + x, W };
                        int v = h264mc_luma(S, mc & 3, mc >> 2, maxv);
                        if (avg)
                            v = h264mc_avg((int)old[y * W + x], v);
                        checks++;
                        if (v != (int)dst[y * W + x])
                            FAIL("h264mc_luma: %d bits, mcxy %d, avg %d, window %d, sample (%d, %d): %d, the oracle %d", bd, mc, avg, rep, x, y, v,
                                 (int)dst[y * W + x]);
                    }
            }
    }
}

template <class P>
static void chroma(int bd)
{
    const int maxv = (1 << bd) - 1, W = 3;      /* a 2 x 2 block and its right / lower neighbours */
    P win[W * W], dst[2 * W], old[2 * W];
    for (int rep = 0; rep < 200; rep++) {
        fill(win, W * W, maxv, rep & 1);
        fill(old, 2 * W, maxv, (rep >> 1) & 1);
        for (int f = 0; f < 64; f++)
            for (int avg = 0; avg < 2; avg++) {
                for (int i = 0; i < 2 * W; i++)
                    dst[i] = old[i];
                ffo_h264_chroma_mc_bd(bd, avg, 2, (uint8_t *)dst, (const uint8_t *)win, W * sizeof(P), 2, f & 7, f >> 3);
                for (int y = 0; y < 2; y++)
                    for (int x = 0; x < 2; x++) {
                        const Win<P> S = { win + y * W + x, W };
                        int v = h264mc_chroma(S, f & 7, f >> 3);
                        if (avg)
                            v = h264mc_avg((int)old[y * W + x], v);
                        checks++;
                        if (v != (int)dst[y * W + x])
                            FAIL("h264mc_chroma: %d bits, fraction (%d, %d), avg %d, window %d, sample (%d, %d): %d, the oracle %d", bd, f & 7, f >> 3,
                                 avg, rep, x, y, v, (int)dst[y * W + x]);
                    }
            }
    }
}

template <class P>
static void weight(int bd)
{
    static const int ladder[5] = { -128, -1, 0, 1, 127 }, offs[3] = { -128, 0, 127 };
    const int maxv = (1 << bd) - 1;
    P blk[4], src[4], old[4];
    for (int ld = 0; ld < 8; ld++)
        for (int wi = 0; wi < 5; wi++)
            for (int oi = 0; oi < 3; oi++)
                for (int rep = 0; rep < 6; rep++) {
                    const int wd = ladder[wi], o = offs[oi];
                    fill(old, 4, maxv, rep & 1);
                    fill(src, 4, maxv, (rep >> 1) & 1);
                    for (int i = 0; i < 4; i++)
                        blk[i] = old[i];
                    ffo_h264_weight_bd(bd, 2, (uint8_t *)blk, 2 * sizeof(P), 2, ld, wd, o);
                    for (int i = 0; i < 4; i++) {
                        const int v = h264mc_weight((int)old[i], bd, ld, wd, o);
                        checks++;
                        if (v != (int)blk[i])
                            FAIL("h264mc_weight: %d bits, log2_denom %d, weight %d, offset %d, sample %d: %d, the oracle %d", bd, ld, wd, o, (int)old[i],
                                 v, (int)blk[i]);
                    }
                    for (int si = 0; si < 5; si++) {
                        const int ws = ladder[si];
                        for (int i = 0; i < 4; i++)
                            blk[i] = old[i];
                        ffo_h264_biweight_bd(bd, 2, (uint8_t *)blk, (const uint8_t *)src, 2 * sizeof(P), 2, ld, wd, ws, o);
                        for (int i = 0; i < 4; i++) {
                            const int v = h264mc_biweight((int)old[i], (int)src[i], bd, ld, wd, ws, o);
                            checks++;
                            if (v != (int)blk[i])
                                FAIL("h264mc_biweight: %d bits, log2_denom %d, weights %d (dst) %d (src), offset %d, samples %d %d: %d, the oracle %d",
                                     bd, ld, wd, ws, o, (int)old[i], (int)src[i], v, (int)blk[i]);
                        }
                    }
                }
}

int main()
{
    luma<uint8_t>(8);
    luma<uint16_t>(10);
    luma<uint16_t>(14);
    chroma<uint8_t>(8);
    chroma<uint16_t>(10);
    chroma<uint16_t>(14);
    weight<uint8_t>(8);
    weight<uint16_t>(9);
    weight<uint16_t>(10);
    weight<uint16_t>(12);
    weight<uint16_t>(14);
    for (int rep = 0; rep < 100000; rep++) {    /* the packed average is four scalar ones */
        const uint32_t a = (rnd() << 8) ^ rnd(), b = rep & 1 ? (rnd() << 8) ^ rnd() : a ^ (1u << (rep & 31));
        uint32_t want = 0;
        for (int i = 0; i < 4; i++)
            want |= (uint32_t)h264mc_avg((a >> 8 * i) & 255, (b >> 8 * i) & 255) << 8 * i;
        checks++;
        if (h264mc_avg4(a, b) != want)
            FAIL("h264mc_avg4(%08x, %08x) = %08x, four h264mc_avg %08x", a, b, h264mc_avg4(a, b), want);
    }
    printf("%ld comparisons, no disagreement\n", checks);
    return 0;
}
