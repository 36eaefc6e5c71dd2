/* kernels/hevc_mc_rules.h on the CPU against the oracle (oracle/liboracle.so): the per-sample intermediate hevcmc_sample at all 16 luma
 * and 64 chroma fractions and the five output stages of hevcmc_out, at 8, 10 and 12 bits, and the generated operand tables against the
 * taps and against a few words written out by hand.  argv[1]: the number of random windows per fraction.  Prints the first
 * disagreement and exits 1; prints the number of comparisons and exits 0.  Built and run by tests/test_hevc_mc_rules_cpu.py, which
 * works the number out on its own. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

extern "C" {
#include "ffo.h"
}
#include "kernels/hevc_mc_rules.h"

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

enum { W = 9, O = 3, N = 2 };  /* a 2 x 2 block's window for either filter: 3 samples before, 4 after; the block starts at (O, O) */

static int tap(int chroma, int f, int t) { return chroma ? hevcmc_tap<4>(f, t) : hevcmc_tap<8>(f, t); }

/* kind 0: random; 1: all 0; 2: all maxv; 3: sign-matched to the filters of (mx, my) around the block's first sample — maxv where the
 * horizontal tap over a column and the vertical tap over a row are positive together or not positive together (a missing filter counts
 * as positive), 0 elsewhere: each horizontal sum is at one end of its range, the end its vertical tap's sign asks for; 4: its inverse */
template <class P>
static void fill(P *win, int maxv, int kind, int chroma, int mx, int my)
{
    const int B = chroma ? 1 : 3;
    for (int r = 0; r < W; r++)
        for (int c = 0; c < W; c++) {
            int v;
            if (kind == 0) {
                v = (int)(rnd() % (unsigned)(maxv + 1));
            } else if (kind <= 2) {
                v = kind == 1 ? 0 : maxv;
            } else {
                const bool hp = mx ? tap(chroma, mx, c - O + B) > 0 : true, vp = my ? tap(chroma, my, r - O + B) > 0 : true;
                v = ((hp == vp) == (kind == 3)) ? maxv : 0;
            }
            win[r * W + c] = (P)v;
        }
}

/* put and uni on `nrand` random windows and the four fixed ones, every fraction */
template <class P>
static void interp(int bd, int nrand)
{
    const int maxv = (1 << bd) - 1;
    P win[W * W], d8[N * N];
    int16_t d16[N * 64];
    for (int chroma = 0; chroma < 2; chroma++)
        for (int f = 0; f < (chroma ? 64 : 16); f++) {
            const int mx = chroma ? f & 7 : f & 3, my = chroma ? f >> 3 : f >> 2;
            for (int k = 0; k < nrand + 4; k++) {
                fill(win, maxv, k < nrand ? 0 : k - nrand + 1, chroma, mx, my);
                const uint8_t *src = (const uint8_t *)(win + O * W + O);
                ffo_hevc_mc_bd(bd, chroma, 0, d16, 0, src, W * sizeof(P), N, mx, my, N);
                ffo_hevc_mc_bd(bd, chroma, 1, d8, N * sizeof(P), src, W * sizeof(P), N, mx, my, N);
                for (int y = 0; y < N; y++)
                    for (int x = 0; x < N; x++) {
                        const Win<P> S = { win + (O + y) * W + O + x, W };
                        const int v = hevcmc_sample(S, chroma, mx, my, bd);
                        checks += 2;
                        if ((int16_t)v != d16[y * 64 + x])   /* the put stage stores int16 */
                            FAIL("hevcmc_sample: %d bits, chroma %d, (mx, my) (%d, %d), window %d, sample (%d, %d): %d, the oracle %d", bd, chroma,
                                 mx, my, k, x, y, v, d16[y * 64 + x]);
                        const int u = hevcmc_out(HEVCMC_UNI, v, 0, 0, 0, 0, 0, bd);
                        if (u != (int)d8[y * N + x])
                            FAIL("hevcmc_out(uni): %d bits, chroma %d, (mx, my) (%d, %d), window %d, sample (%d, %d): %d, the oracle %d", bd, chroma,
                                 mx, my, k, x, y, u, (int)d8[y * N + x]);
                    }
            }
        }
}

/* the weight sets of tests/mc_matrix.py:weights(), both kinds, as grids over the ends of their ranges */
struct Wt { int denom, wx0, wx1, ox; };
static int weight_sets(Wt *out)
{
    static const int den[3] = { 0, 7, 12 }, wl[3] = { 0, 128, 255 }, ol[2] = { 0, 255 };
    static const int d0[3] = { -128, -1, 127 }, d1[3] = { -128, 0, 127 }, o2[3] = { -256, -1, 254 };
    int n = 0;
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++)
            for (int c = 0; c < 3; c++)
                for (int d = 0; d < 2; d++)
                    out[n++] = Wt{ den[a], wl[b], wl[c], ol[d] };
    for (int d = 0; d < 8; d++)
        for (int b = 0; b < 3; b++)
            for (int c = 0; c < 3; c++)
                for (int e = 0; e < 3; e++)
                    out[n++] = Wt{ d, (1 << d) + d0[b], (1 << d) + d1[c], o2[e] };
    return n;
}

/* uni_w, bi and bi_w over the weight sets; the other list at -8192, 0, the largest intermediate and random */
template <class P>
static void weighted(int bd)
{
    const int maxv = (1 << bd) - 1;
    static Wt wts[512];
    const int nw = weight_sets(wts);
    P win[W * W], d8[N * N];
    int16_t src2[N * 64];
    /* the largest value the put stage produces: the sign-matched window under the filters with the largest positive taps, (2, 2) of
     * luma — as far as the int16 it is stored in goes */
    fill(win, maxv, 3, 0, 2, 2);
    const Win<P> top = { win + O * W + O, W };
    int vmax = hevcmc_sample(top, false, 2, 2, bd);
    vmax = vmax > INT16_MAX ? INT16_MAX : vmax;
    int turn = 0;
    for (int chroma = 0; chroma < 2; chroma++)
        for (int i = 0; i < nw; i++)
            for (int k2 = 0; k2 < 4; k2++)
                for (int mode = HEVCMC_UNI_W; mode <= HEVCMC_BI_W; mode++) {
                    const Wt &w = wts[i];
                    const int f = turn++ % (chroma ? 64 : 16), mx = chroma ? f & 7 : f & 3, my = chroma ? f >> 3 : f >> 2;
                    fill(win, maxv, 0, chroma, mx, my);
                    for (int y = 0; y < N; y++)
                        for (int x = 0; x < N; x++)
                            src2[y * 64 + x] = (int16_t)(k2 == 0 ? -8192 : k2 == 1 ? 0 : k2 == 2 ? vmax : (int)(rnd() % 24576u) - 8192);
                    ffo_hevc_mc_w_bd(bd, chroma, mode, (uint8_t *)d8, N * sizeof(P), (const uint8_t *)(win + O * W + O), W * sizeof(P), src2, N,
                                     w.denom, w.wx0, w.wx1, w.ox, mx, my, N);
                    for (int y = 0; y < N; y++)
                        for (int x = 0; x < N; x++) {
                            const Win<P> S = { win + (O + y) * W + O + x, W };
                            const int v = hevcmc_sample(S, chroma, mx, my, bd);
                            const int o = hevcmc_out(mode, v, src2[y * 64 + x], w.wx0, w.wx1, hevcmc_offset(w.ox, bd), hevcmc_wshift(w.denom, bd), bd);
                            checks++;
                            if (o != (int)d8[y * N + x])
                                FAIL("hevcmc_out: %d bits, chroma %d, mode %d, (mx, my) (%d, %d), denom %d, wx0 %d, wx1 %d, ox %d, v %d, v2 %d: %d, "
                                     "the oracle %d", bd, chroma, mode, mx, my, w.denom, w.wx0, w.wx1, w.ox, v, src2[y * 64 + x], o, (int)d8[y * N + x]);
                        }
                }
}

/* the generated tables, unpacked: the dot2 operands are the taps shifted by zero and by one row, the byte rows are the taps */
template <int TAPS>
static void tables()
{
    constexpr int NP = TAPS / 2 + 1, NF = 32 / TAPS;
    constexpr auto d2 = hevcmc_dot2_rows<TAPS>();
    constexpr auto by = hevcmc_tap_bytes<TAPS>();
    for (int f = 0; f < NF; f++) {
        for (int odd = 0; odd < 2; odd++)
            for (int q = 0; q < NP; q++)
                for (int half = 0; half < 2; half++) {
                    const int got = (int16_t)(d2.v[f][odd * NP + q] >> (16 * half)), want = hevcmc_tap<TAPS>(f, 2 * q + half - odd);
                    checks++;
                    if (got != want)
                        FAIL("hevcmc_dot2_rows<%d>: fraction %d, parity %d, pair %d, half %d: %d, the tap %d", TAPS, f, odd, q, half, got, want);
                }
        for (int q = 2 * NP; q < TAPS + 4; q++) {
            checks++;
            if (d2.v[f][q])
                FAIL("hevcmc_dot2_rows<%d>: fraction %d, padding word %d is %08x", TAPS, f, q, d2.v[f][q]);
        }
        for (int t = 0; t < TAPS; t++) {
            checks++;
            if (by.v[f][t] != hevcmc_tap<TAPS>(f, t))
                FAIL("hevcmc_tap_bytes<%d>: fraction %d, tap %d: %d, the tap %d", TAPS, f, t, by.v[f][t], hevcmc_tap<TAPS>(f, t));
        }
    }
}

/* the row-pair layout itself, pinned by words written out by hand from the taps (pk(a, b) = a | b << 16): luma fraction 1 is
 * (-1, 4, -10, 58, 17, -5, 1, 0), chroma fraction 3 is (-6, 46, 28, -4); [0 .. NP-1] the first row even, [NP .. 2NP-1] odd */
static void layout()
{
    constexpr auto l = hevcmc_dot2_rows<8>();
    constexpr auto c = hevcmc_dot2_rows<4>();
    const struct { const char *what; uint32_t got, want; } w[6] = {
        { "luma 1, even, pair 0: (-1, 4)", l.v[1][0], 0x0004ffffu },   { "luma 1, even, pair 4: (0, 0)", l.v[1][4], 0x00000000u },
        { "luma 1, odd, pair 0: (0, -1)", l.v[1][5], 0xffff0000u },    { "luma 1, odd, pair 2: (58, 17)", l.v[1][7], 0x0011003au },
        { "chroma 3, even, pair 1: (28, -4)", c.v[3][1], 0xfffc001cu }, { "chroma 3, odd, pair 2: (-4, 0)", c.v[3][5], 0x0000fffcu } };
    for (int i = 0; i < 6; i++) {
        checks++;
        if (w[i].got != w[i].want)
            FAIL("hevcmc_dot2_rows: %s is %08x, by hand %08x", w[i].what, w[i].got, w[i].want);
    }
}

int main(int argc, char **argv)
{
    const int nrand = argc > 1 ? atoi(argv[1]) : 20;
    interp<uint8_t>(8, nrand);
    interp<uint16_t>(10, nrand);
    interp<uint16_t>(12, nrand);
    weighted<uint8_t>(8);
    weighted<uint16_t>(10);
    weighted<uint16_t>(12);
    tables<8>();
    tables<4>();
    layout();
    printf("%ld comparisons, no disagreement\n", checks);
    return 0;
}
