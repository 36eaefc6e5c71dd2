/* kernels/vp9_mc_rules.h on the CPU against the oracle (oracle/liboracle.so): vp9mc_pass and the 2-D form through clipped temporaries
 * against ffo_vp9_mc_bd (filters 0..3, all 16 x 16 fractions, 8 / 10 / 12 bits, put and avg), the scaled walk with vp9mc_pass0 against
 * ffo_vp9_smc_bd (steps 1 .. 32 on each axis, all start fractions, the 134-row block whole and in strips), the generated operand
 * tables against the taps and against words written out by hand, and vp9mc_avg4 against vp9mc_avg.  argv[1]: the number of random
 * windows per fraction of the unscaled walk.  Prints the first disagreement and exits 1; prints the number of comparisons and exits 0.
 * Built and run by tests/test_vp9_mc_rules_cpu.py, which works the number out on its own. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

extern "C" {
#include "ffo.h"
}
#include "kernels/vp9_mc_rules.h"

static uint32_t rng_state = 12345;
static uint32_t rnd() { return rng_state = rng_state * 1664525u + 1013904223u, rng_state >> 8; }

static long checks = 0;
#define FAIL(...) do { printf(__VA_ARGS__); printf("\n"); exit(1); } while (0)

/* blocks are N wide, N or TALL high and start at (O, O) of a WW x WH window; SROWS and TROWS are vp9_inter_frame.hip's: output rows per
 * strip, rows of temporaries */
enum { N = 4, O = 3, WW = 16, WH = 140, TALL = 64, SROWS = 32, TROWS = 64 + 7 };
static const int steps[6] = { 1, 8, 11, 16, 24, 32 }; /* 16x up .. 2x down; 16 is the unscaled form */

/* the taps of a pass as the kernels' packed forms see them: the bilinear is (16 - m, m) at taps 3 and 4 */
static int tap(int filter, int m, int t) { return filter < 3 ? vp9mc_tap(filter, m, t) : t == 3 ? 16 - m : t == 4 ? m : 0; }

/* kind 0: random; 1: all 0; 2: all maxv; 3: sign-matched to the filters of (mx, my) around the block's first sample — maxv where the
 * horizontal tap over a column and the vertical tap over a row are positive together or not positive together (a missing filter counts
 * as positive), 0 elsewhere: each horizontal sum is at one end of its range, the end its vertical tap's sign asks for, so both passes
 * reach their clips; 4: its inverse */
template <class P>
static void fill(P *win, int rows, int maxv, int kind, int filter, int mx, int my)
{
    for (int r = 0; r < rows; r++)
        for (int c = 0; c < WW; c++) {
            int v;
            if (kind == 0) {
                v = (int)(rnd() % (unsigned)(maxv + 1));
            } else if (kind <= 2) {
                v = kind == 1 ? 0 : maxv;
            } else {
                const bool hp = mx ? tap(filter, mx, c) > 0 : true, vp = my ? tap(filter, my, r) > 0 : true;
                v = ((hp == vp) == (kind == 3)) ? maxv : 0;
            }
            win[r * WW + c] = (P)v;
        }
}

/* mc[][filter][][!!mx][!!my] for the sample at p: the 2-D form through the eight (bilinear: two) clipped temporaries of its column */
template <class P>
static int mc_sample(const P *p, int filter, int mx, int my, int maxv)
{
    if (mx && my) {
        P col[8];
        for (int r = -3; r <= 4; r++)
            col[r + 3] = (P)vp9mc_pass(filter, mx, maxv, [&](int k) { return (int)p[r * WW + k]; });
        return vp9mc_pass(filter, my, maxv, [&](int k) { return (int)col[k + 3]; });
    }
    if (mx)
        return vp9mc_pass(filter, mx, maxv, [&](int k) { return (int)p[k]; });
    if (my)
        return vp9mc_pass(filter, my, maxv, [&](int k) { return (int)p[k * WW]; });
    return p[0];
}

/* smc[][filter][] of an N x h block at src, in strips of `srows` output rows: the horizontal pass over the rows a strip reads, into
 * pixel temporaries, then the vertical pass.  Returns the most rows a strip's horizontal pass made */
template <class P>
static int smc_block(int *out, const P *src, int h, int filter, int mx, int my, int dx, int dy, int maxv, int srows)
{
    static P tmp[135 * N];
    const int before = vp9mc_before(filter);
    int most = 0;
    for (int y0 = 0; y0 < h; y0 += srows) {
        const int sh = h - y0 < srows ? h - y0 : srows, p0 = vp9mc_pos(my, y0, dy), m0 = vp9mc_frac(p0);
        const int rows = vp9mc_rows(filter, m0, sh, dy);
        const P *top = src + (vp9mc_whole(p0) - before) * WW;
        most = rows > most ? rows : most;
        for (int r = 0; r < rows; r++)
            for (int x = 0; x < N; x++) {
                const int pos = vp9mc_pos(mx, x, dx);
                const P *p = top + r * WW + vp9mc_whole(pos);
                tmp[r * N + x] = (P)vp9mc_pass0(filter, vp9mc_frac(pos), maxv, [&](int k) { return (int)p[k]; });
            }
        for (int y = 0; y < sh; y++)
            for (int x = 0; x < N; x++) {
                const int pos = vp9mc_pos(m0, y, dy);
                const P *t = tmp + (vp9mc_whole(pos) + before) * N + x;
                out[(y0 + y) * N + x] = vp9mc_pass0(filter, vp9mc_frac(pos), maxv, [&](int k) { return (int)t[k * N]; });
            }
    }
    return most;
}

/* an N x h block of `got` against the oracle's put, and its vp9mc_avg with dst0 against the oracle's avg */
template <class P>
static void against(const char *what, const int *got, const P *put, const P *avg, const P *dst0, int h, int bd, int filter, int mx, int my, int dx,
                    int dy, int k)
{
    for (int i = 0; i < N * h; i++) {
        checks += 2;
        if (got[i] != (int)put[i])
            FAIL("%s: %d bits, filter %d, (mx, my) (%d, %d), steps (%d, %d), window %d, sample (%d, %d): %d, the oracle %d", what, bd, filter, mx,
                 my, dx, dy, k, i % N, i / N, got[i], (int)put[i]);
        if (vp9mc_avg(dst0[i], got[i]) != (int)avg[i])
            FAIL("%s, avg: %d bits, filter %d, (mx, my) (%d, %d), steps (%d, %d), window %d, sample (%d, %d): (%d, %d) gives %d, the oracle %d",
                 what, bd, filter, mx, my, dx, dy, k, i % N, i / N, (int)dst0[i], got[i], vp9mc_avg(dst0[i], got[i]), (int)avg[i]);
    }
}

template <class P>
static void walks(int bd, int nrand)
{
    const int maxv = (1 << bd) - 1;
    static P win[WH * WW], put[N * TALL], avg[N * TALL], dst0[N * TALL];
    static int got[N * TALL], whole[N * TALL];
    const uint8_t *src = (const uint8_t *)(win + O * WW + O);
    const ptrdiff_t ss = WW * sizeof(P), ds = N * sizeof(P);
    auto fresh_dst = [&](int h) {
        for (int i = 0; i < N * h; i++)
            dst0[i] = avg[i] = (P)(rnd() % (unsigned)(maxv + 1));
    };
    for (int filter = 0; filter < 4; filter++)
        for (int f = 0; f < 256; f++) {
            const int mx = f & 15, my = f >> 4;
            /* unscaled: `nrand` random windows and the four fixed ones */
            for (int k = 0; k < nrand + 4; k++) {
                fill(win, N + 7, maxv, k < nrand ? 0 : k - nrand + 1, filter, mx, my);
                fresh_dst(N);
                ffo_vp9_mc_bd(bd, filter, 0, (uint8_t *)put, ds, src, ss, N, N, mx, my);
                ffo_vp9_mc_bd(bd, filter, 1, (uint8_t *)avg, ds, src, ss, N, N, mx, my);
                for (int y = 0; y < N; y++)
                    for (int x = 0; x < N; x++)
                        got[y * N + x] = mc_sample(win + (O + y) * WW + O + x, filter, mx, my, maxv);
                against("vp9mc_pass", got, put, avg, dst0, N, bd, filter, mx, my, 16, 16, k);
            }
            /* scaled: every pair of steps on a random window */
            for (int sx = 0; sx < 6; sx++)
                for (int sy = 0; sy < 6; sy++) {
                    const int dx = steps[sx], dy = steps[sy];
                    fill(win, N + 3 * 32 / 16 + 8, maxv, 0, filter, mx, my);
                    fresh_dst(N);
                    ffo_vp9_smc_bd(bd, filter, 0, (uint8_t *)put, ds, src, ss, N, N, mx, my, dx, dy);
                    ffo_vp9_smc_bd(bd, filter, 1, (uint8_t *)avg, ds, src, ss, N, N, mx, my, dx, dy);
                    smc_block(got, win + O * WW + O, N, filter, mx, my, dx, dy, maxv, N);
                    against("the scaled walk", got, put, avg, dst0, N, bd, filter, mx, my, dx, dy, 0);
                    if (dx == 16 && dy == 16) { /* the unscaled form */
                        ffo_vp9_mc_bd(bd, filter, 0, (uint8_t *)put, ds, src, ss, N, N, mx, my);
                        for (int i = 0; i < N * N; i++) {
                            checks++;
                            if (got[i] != (int)put[i])
                                FAIL("the scaled walk at steps of 16: %d bits, filter %d, (mx, my) (%d, %d), sample (%d, %d): %d, unscaled %d", bd,
                                     filter, mx, my, i % N, i / N, got[i], (int)put[i]);
                        }
                    }
                }
        }
    /* the tallest block at 2x down: 134 rows under the horizontal pass, whole and in vp9_inter_frame.hip's strips */
    for (int filter = 0; filter < 4; filter++) {
        const int mx = 5, my = 15, dx = 32, dy = 32, want_rows = filter == 3 ? 128 : 134;
        fill(win, WH, maxv, 0, filter, mx, my);
        fresh_dst(TALL);
        ffo_vp9_smc_bd(bd, filter, 0, (uint8_t *)put, ds, src, ss, N, TALL, mx, my, dx, dy);
        ffo_vp9_smc_bd(bd, filter, 1, (uint8_t *)avg, ds, src, ss, N, TALL, mx, my, dx, dy);
        const int rows = smc_block(whole, win + O * WW + O, TALL, filter, mx, my, dx, dy, maxv, TALL);
        checks++;
        if (rows != want_rows)
            FAIL("vp9mc_rows: filter %d, 64 rows from fraction %d at step %d: %d, by hand %d", filter, my, dy, rows, want_rows);
        against("the scaled walk, 4 x 64", whole, put, avg, dst0, TALL, bd, filter, mx, my, dx, dy, 0);
        const int most = smc_block(got, win + O * WW + O, TALL, filter, mx, my, dx, dy, maxv, SROWS);
        checks++;
        if (most > TROWS)
            FAIL("vp9mc_rows: filter %d, a strip of %d rows at step %d reads %d rows, more than %d", filter, SROWS, dy, most, TROWS);
        for (int i = 0; i < N * TALL; i++) {
            checks++;
            if (got[i] != whole[i])
                FAIL("the scaled walk in strips of %d: %d bits, filter %d, sample (%d, %d): %d, whole %d", SROWS, bd, filter, i % N, i / N, got[i],
                     whole[i]);
        }
    }
}

/* the generated tables, unpacked: the dword rows are the taps as bytes, the dot2 operands the taps shifted by zero and by one row */
static void tables()
{
    constexpr auto h8 = vp9mc_tap_dwords();
    constexpr auto v2 = vp9mc_dot2_rows();
    for (int f = 0; f < 3; f++)
        for (int m = 0; m < 16; m++) {
            const int row = f * 16 + m;
            int sum = 0;
            for (int t = 0; t < 8; t++) {
                const int got = (int8_t)(h8.v[row][t >> 2] >> (8 * (t & 3)));
                sum += vp9mc_tap(f, m, t);
                checks++;
                if (got != vp9mc_tap(f, m, t))
                    FAIL("vp9mc_tap_dwords: filter %d, fraction %d, tap %d: %d, the tap %d", f, m, t, got, vp9mc_tap(f, m, t));
            }
            checks++; /* vm_hrow4's and k_vp9_mc_m's seeds undo the -128 bias with 128 * 128 */
            if (sum != (m ? 128 : 0))
                FAIL("vp9mc_tap: filter %d, fraction %d: the taps sum to %d", f, m, sum);
            for (int odd = 0; odd < 2; odd++)
                for (int q = 0; q < 5; q++)
                    for (int half = 0; half < 2; half++) {
                        const int got = (int16_t)(v2.v[row][odd * 5 + q] >> (16 * half)), want = vp9mc_tap(f, m, 2 * q + half - odd);
                        checks++;
                        if (got != want)
                            FAIL("vp9mc_dot2_rows: filter %d, fraction %d, parity %d, pair %d, half %d: %d, the tap %d", f, m, odd, q, half, got, want);
                    }
            for (int q = 10; q < 12; q++) {
                checks++;
                if (v2.v[row][q])
                    FAIL("vp9mc_dot2_rows: filter %d, fraction %d, padding word %d is %08x", f, m, q, v2.v[row][q]);
            }
        }
}

/* the layouts themselves, pinned by words of the tables these generators replaced: smooth 1 is (-3, -1, 32, 64, 38, 1, -3, 0), regular 5
 * (-1, 5, -18, 105, 48, -14, 4, -1), sharp 15 (0, 1, -3, 8, 127, -7, 3, -1); dot2 words [0 .. 4] the first row even, [5 .. 9] odd */
static void layout()
{
    constexpr auto h8 = vp9mc_tap_dwords();
    constexpr auto v2 = vp9mc_dot2_rows();
    const struct { const char *what; uint32_t got, want; } w[12] = {
        { "dwords, smooth 1, low", h8.v[1][0], 0x4020fffdu },          { "dwords, smooth 1, high", h8.v[1][1], 0x00fd0126u },
        { "dwords, regular 5, low", h8.v[21][0], 0x69ee05ffu },        { "dwords, regular 5, high", h8.v[21][1], 0xff04f230u },
        { "dwords, sharp 15, low", h8.v[47][0], 0x08fd0100u },         { "dwords, sharp 15, high", h8.v[47][1], 0xff03f97fu },
        { "dot2, smooth 1, even, pair 1: (32, 64)", v2.v[1][1], 0x00400020u },   { "dot2, smooth 1, odd, pair 0: (0, -3)", v2.v[1][5], 0xfffd0000u },
        { "dot2, regular 5, even, pair 2: (48, -14)", v2.v[21][2], 0xfff20030u }, { "dot2, regular 5, odd, pair 3: (-14, 4)", v2.v[21][8], 0x0004fff2u },
        { "dot2, sharp 15, even, pair 3: (3, -1)", v2.v[47][3], 0xffff0003u },   { "dot2, sharp 15, odd, pair 4: (-1, 0)", v2.v[47][9], 0x0000ffffu } };
    for (int i = 0; i < 12; i++) {
        checks++;
        if (w[i].got != w[i].want)
            FAIL("%s is %08x, by hand %08x", w[i].what, w[i].got, w[i].want);
    }
}

/* the packed average against four scalar ones: every pair of bytes in one lane (a different lane from pair to pair), the other three
 * lanes filled from the generator */
static void avg4()
{
    for (int a = 0; a < 256; a++)
        for (int b = 0; b < 256; b++) {
            const int lane = (a + b) & 3;
            uint32_t A = rnd() << 8 ^ rnd(), B = rnd() << 8 ^ rnd();
            A = (A & ~(0xffu << (8 * lane))) | (uint32_t)a << (8 * lane);
            B = (B & ~(0xffu << (8 * lane))) | (uint32_t)b << (8 * lane);
            const uint32_t got = vp9mc_avg4(A, B);
            for (int l = 0; l < 4; l++) {
                const int want = vp9mc_avg((int)(A >> (8 * l) & 255), (int)(B >> (8 * l) & 255));
                checks++;
                if ((int)(got >> (8 * l) & 255) != want)
                    FAIL("vp9mc_avg4(%08x, %08x) = %08x: lane %d should be %d", A, B, got, l, want);
            }
        }
}

int main(int argc, char **argv)
{
    const int nrand = argc > 1 ? atoi(argv[1]) : 4;
    walks<uint8_t>(8, nrand);
    walks<uint16_t>(10, nrand);
    walks<uint16_t>(12, nrand);
    tables();
    layout();
    avg4();
    printf("%ld comparisons, no disagreement\n", checks);
    return 0;
}
