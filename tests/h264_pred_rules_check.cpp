/* kernels/h264_pred_rules.h on the CPU against the oracle (oracle/liboracle.so, ffo_h264pred.c) at 8 bits: the rules read a small window
 * in place, through callables, as the reconstruction kernels read their tile.  Every prediction case is run twice, the second time on a
 * copy of the window in which every neighbour the mode's mask does not name has another value: the result must not move.  Windows:
 * argv[1] random ones, then all 0, all maximum, a checkerboard of both, and two ramps steep enough that the plane predictor leaves the
 * sample range at both ends.  Also: the table forms of h264_intra_mb.h decoded against the rules; the two places the depth enters (mid,
 * maxv) at 9, 10, 12 and 14 bits; the whole-block DC against pred16x16 and against the RV40 rule text of h264_pred_codec.inc.
 * Prints the first disagreement and exits 1; prints the number of comparisons and exits 0.  Built and run by
 * tests/test_h264_pred_rules_cpu.py, which works the number out on its own. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

extern "C" {
#include "ffo.h"
}
#include "kernels/h264_intra_mb.h" /* the table forms; it includes kernels/h264_pred_rules.h */

static uint32_t rng_state = 12345;
static uint32_t rnd() { return rng_state = rng_state * 1664525u + 1013904223u, rng_state >> 8; }

static long checks = 0;
#define FAIL(...) do { printf(__VA_ARGS__); printf("\n"); exit(1); } while (0)
#define SAME(got, want, ...) do { checks++; if ((got) != (want)) { printf("%d for %d: ", (int)(got), (int)(want)); FAIL(__VA_ARGS__); } } while (0)

/* a window of PW x PH samples, the block's first sample at (OX, OY): room for a 16 x 16 block, its left column, the row above and the
 * eight samples to its right */
enum { PW = 32, PH = 24, OX = 8, OY = 4, FIXED = 5 };
template <class P>
struct Win {
    P s[PH * PW];
    P *at(int x, int y) { return s + (OY + y) * PW + OX + x; }
    int operator()(int x, int y) const { return s[(OY + y) * PW + OX + x]; }
};

/* kind < nrand: random; then all 0, all maxv, checkerboard, ramp up, ramp down.  A ramp is 0 up to the fourth diagonal, maxv from the
 * seventh on: the gradient the plane predictor fits to the border carries on beyond both ends of the range */
template <class P>
static void fill(Win<P> &w, int maxv, int kind, int nrand)
{
    for (int y = -OY; y < PH - OY; y++)
        for (int x = -OX; x < PW - OX; x++) {
            const int k = kind - nrand, d = x + y + 2, ramp = d <= 3 ? 0 : d >= 7 ? maxv : maxv * (d - 3) / 4;
            *w.at(x, y) = (P)(k < 0 ? (int)(rnd() % (unsigned)(maxv + 1)) : k == 0 ? 0 : k == 1 ? maxv : k == 2 ? ((x + y) & 1 ? maxv : 0) : k == 3 ? ramp : maxv - ramp);
        }
}

/* the copy with other values where `named` is false: left rows lrows.., the row above 0..ntop - 1, the corner, the row above from ntop on */
template <class P>
static Win<P> disturb(const Win<P> &a, int h, int ntop, bool left, int lrows, bool top, bool corner, bool tr0, bool tr)
{
    Win<P> b = a;
    for (int y = 0; y < h; y++)
        if (!left || y >= lrows)
            *b.at(-1, y) ^= 0x55;
    for (int x = 0; x < 16; x++)
        if (x < ntop ? !top : x == ntop ? !tr0 : !tr)
            *b.at(x, -1) ^= 0x55;
    if (!corner)
        *b.at(-1, -1) ^= 0x55;
    return b;
}

/* the edge line of an N x N block read in place: left column bottom-up, corner, row above and on to the right */
template <int N, class P>
struct Line {
    const Win<P> &w;
    int operator()(int k) const { return k < N ? w(-1, N - 1 - k) : w(k - N - 1, -1); }
};

/* ---- pred4x4 ---- */
static void pred4(const Win<uint8_t> &w, int mode, int out[16])
{
    const Line<4, uint8_t> e{ w };
    const int dc = hp_dir_dc_e<4>(mode, e);
    for (int i = 0; i < 16; i++)
        out[i] = hp_dir_sample_e<4>(mode, e, i & 3, i >> 2, dc);
}
static void check4(const Win<uint8_t> &a, int kind)
{
    for (int mode = 0; mode < 12; mode++) {
        const unsigned need = hp_need(mode);
        Win<uint8_t> o = a;
        ffo_h264_pred4x4(mode, o.at(0, 0), a.s + (OY - 1) * PW + OX + 4, PW);
        int got[16], again[16];
        pred4(a, mode, got);
        pred4(disturb(a, 4, 4, need & 1, 4, need & 2, need & 4, need & 8, need & 8), mode, again);
        for (int i = 0; i < 16; i++) {
            SAME(got[i], o(i & 3, i >> 2), "pred4x4 mode %d window %d sample %d", mode, kind, i);
            SAME(again[i], got[i], "pred4x4 mode %d window %d sample %d moved with a neighbour hp_need() does not name", mode, kind, i);
        }
    }
}

/* ---- pred8x8l ---- */
static void pred8l(const Win<uint8_t> &w, int mode, bool tl, bool tr, int out[64])
{
    const Line<8, uint8_t> raw{ w };
    int f[25];
    for (int j = 0; j < 25; j++)
        f[j] = hp_filter8_e(raw, j, hp_need(mode), tl, tr);
    const int dc = hp_dir_dc<8>(mode, f);
    for (int i = 0; i < 64; i++)
        out[i] = hp_dir_sample<8>(mode, f, i & 7, i >> 3, dc);
}
static void check8l(const Win<uint8_t> &a, int kind)
{
    for (int mode = 0; mode < 12; mode++)
        for (int c = 0; c < 4; c++) {
            const bool tl = c & 1, tr = c & 2;
            const unsigned need = hp_need(mode);
            Win<uint8_t> o = a;
            ffo_h264_pred8x8l(mode, o.at(0, 0), tl, tr, PW);
            int got[64], again[64];
            pred8l(a, mode, tl, tr, got);
            /* the edge filter also reads the corner of a block that has one, and the first sample to the right of one that has those */
            pred8l(disturb(a, 8, 8, need & 1, 8, need & 2, (need & 4) || (tl && (need & 3)), tr && (need & 10), tr && (need & 8)), mode, tl, tr, again);
            for (int i = 0; i < 64; i++) {
                SAME(got[i], o(i & 7, i >> 3), "pred8x8l mode %d tl %d tr %d window %d sample %d", mode, tl, tr, kind, i);
                SAME(again[i], got[i], "pred8x8l mode %d tl %d tr %d window %d sample %d moved with a neighbour not named", mode, tl, tr, kind, i);
            }
        }
}

/* ---- pred8x8l_filter_add with no residual: every line of the block repeats its filtered edge sample ---- */
static void check_filter_add(const Win<uint8_t> &a, int kind)
{
    for (int mode = 0; mode < 2; mode++)
        for (int c = 0; c < 4; c++) {
            const bool tl = c & 1, tr = c & 2, vert = mode == 0;
            Win<uint8_t> o = a;
            int16_t block[64] = { 0 };
            ffo_h264_pred8x8l_filter_add(mode, o.at(0, 0), block, tl, tr, PW);
            const Line<8, uint8_t> raw{ a };
            for (int i = 0; i < 8; i++) {
                const int v = hp_filter8_e(raw, vert ? 9 + i : 7 - i, vert ? 2u : 1u, tl, tr);
                for (int j = 0; j < 8; j++)
                    SAME(v, vert ? o(i, j) : o(j, i), "pred8x8l_filter_add mode %d tl %d tr %d window %d line %d", mode, tl, tr, kind, i);
            }
        }
}

/* ---- pred8x8 / pred8x16 / pred16x16, the way the tile readers go about it ---- */
template <int W, int H, class P>
static void pred_blk(const Win<P> &w, int mode, int mid, int maxv, int *out, int *raw_min = nullptr, int *raw_max = nullptr)
{
    auto TOP = [&](int i) { return w(i, -1); };
    auto LEFT = [&](int i) { return w(-1, i); };
    const bool ut = hp_blk_top(mode), ul = hp_blk_left(mode);
    const int lrows = hp_blk_lrows(mode, H);
    const HpPlane pl = mode == 3 ? hp_plane<W, H>(TOP, LEFT) : HpPlane{ 0, 0, 0 };
    int sl = 0, st = 0, tq[2] = { 0, 0 }, lq[4] = { 0, 0, 0, 0 };
    for (int i = 0; i < W; i++)
        st += ut ? TOP(i) : 0, tq[(i >> 2) & 1] += ut ? TOP(i) : 0;
    for (int i = 0; i < H; i++)
        sl += ul && i < lrows ? LEFT(i) : 0, lq[(i >> 2) & 3] += ul && i < lrows ? LEFT(i) : 0;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            int v;
            if (mode == 1) {
                v = LEFT(y);
            } else if (mode == 2) {
                v = TOP(x);
            } else if (mode == 3) {
                v = hp_plane_sample(pl, x, y, maxv);
                const int r = hp_plane_raw(pl, x, y);
                if (raw_min && r < *raw_min)
                    *raw_min = r;
                if (raw_max && r > *raw_max)
                    *raw_max = r;
            } else {
                v = W == 16 ? hp_dc16(mode, sl, st, mid) : hp_cell_dc(mode, y >> 2, x >> 2, tq[0], tq[1], lq[0], lq[y >> 2], mid);
            }
            out[y * W + x] = v;
        }
}
template <int W, int H>
static void check_blk(const Win<uint8_t> &a, int kind, int modes, const char *name, void (*oracle)(int, uint8_t *, ptrdiff_t))
{
    for (int mode = 0; mode < modes; mode++) {
        Win<uint8_t> o = a;
        oracle(mode, o.at(0, 0), PW);
        static int got[W * H], again[W * H];
        pred_blk<W, H>(a, mode, 128, 255, got);
        const unsigned need = hp_blk_need(mode);
        pred_blk<W, H>(disturb(a, H, W, need & 1, hp_blk_lrows(mode, H), need & 2, need & 4, false, false), mode, 128, 255, again);
        for (int i = 0; i < W * H; i++) {
            SAME(got[i], o(i % W, i / W), "%s mode %d window %d sample %d", name, mode, kind, i);
            SAME(again[i], got[i], "%s mode %d window %d sample %d moved with a neighbour hp_blk_need() / hp_blk_lrows() do not name", name, mode, kind, i);
        }
    }
}

/* ---- the table forms of h264_intra_mb.h against the rules, over lines of random samples ---- */
static int weigh(int kind, int a, int b, int c) { return kind == 0 ? hp_a3(a, b, c) : kind == 1 ? hp_a2(a, b) : a; }
static void check_tables(int lines)
{
    static const int dir[8] = { 0, 1, 3, 4, 5, 6, 7, 8 }; /* the modes that are table rules: all but the DC family */
    for (int n = 0; n < lines; n++) {
        int e[25];
        for (int k = 0; k < 25; k++)
            e[k] = (int)(rnd() & 255);
        for (int m = 0; m < 8; m++) {
            const int mode = dir[m];
            for (int i = 0; i < 16; i++) {
                const uint32_t c = imb_p4_entry(mode, i & 3, i >> 2);
                SAME(weigh((int)(c >> 12), e[c & 15], e[(c >> 4) & 15], e[(c >> 8) & 15]), hp_dir_sample<4>(mode, e, i & 3, i >> 2, -1),
                     "imb_p4_entry mode %d sample %d", mode, i);
            }
            for (int i = 0; i < 64; i++) {
                const uint32_t c = imb_tab(IMB_P4_TAB + IMB_P8_EDGE_TAB + 64 * mode + i);
                SAME(weigh((int)(c >> 15), e[c & 31], e[(c >> 5) & 31], e[(c >> 10) & 31]), hp_dir_sample<8>(mode, e, i & 7, i >> 3, -1),
                     "imb_p8_tab mode %d sample %d", mode, i);
            }
        }
        /* imb_p8_edge_tab: where entry j of the filtered line finds its three raw samples in the tile, from the block's first sample */
        uint8_t tile[17 * 32];
        for (int k = 0; k < 17 * 32; k++)
            tile[k] = (uint8_t)rnd();
        const uint8_t *o = tile + imb_yi(4, 8);
        auto raw = [&](int k) { return (int)(k < 8 ? o[(7 - k) * 32 - 1] : o[-32 + k - 9]); };
        for (int c = 0; c < 4; c++)
            for (int j = 0; j < 25; j++) {
                const uint32_t ent = imb_tab(IMB_P4_TAB + (c & 1 ? 64 : 0) + (c & 2 ? 32 : 0) + j);
                SAME(hp_a3(o[(int)(ent & 511u) - 33], o[(int)((ent >> 9) & 511u) - 33], o[(int)((ent >> 18) & 511u) - 33]),
                     hp_filter8_e(raw, j, 15u, c & 1, c & 2), "imb_p8_edge_tab tl %d tr %d entry %d", c & 1, (c >> 1) & 1, j);
            }
    }
}

/* ---- the depth: mid and maxv ---- */
static long inside = 0; /* plane samples the 8-bit oracle does not clip */
template <int W, int H>
static void check_plane_depth(int bd, int nrand, void (*oracle)(int, uint8_t *, ptrdiff_t))
{
    const int maxv = (1 << bd) - 1, mid = 1 << (bd - 1);
    static int got[W * H];
    /* windows of the depth: 0, the maximum, the two ramps */
    int lo = 0, hi = 0;
    for (int kind = 0; kind < FIXED; kind++) {
        if (kind == 2)
            continue;
        Win<uint16_t> w;
        fill(w, maxv, kind, 0);
        pred_blk<W, H>(w, 3, mid, maxv, got, &lo, &hi);
        for (int i = 0; i < W * H; i++) {
            checks++;
            if (got[i] < 0 || got[i] > maxv)
                FAIL("plane %d x %d at %d bits, window %d sample %d: %d outside 0..%d", W, H, bd, kind, i, got[i], maxv);
        }
    }
    if (lo >= 0 || hi <= maxv)
        FAIL("plane %d x %d at %d bits: the ramps reach %d..%d before the clip, inside 0..%d", W, H, bd, lo, hi, maxv);
    /* 8-bit windows: below the clip the result does not depend on the depth */
    for (int kind = 0; kind < nrand + FIXED; kind++) {
        Win<uint8_t> a;
        fill(a, 255, kind, nrand);
        Win<uint8_t> o = a;
        oracle(3, o.at(0, 0), PW);
        pred_blk<W, H>(a, 3, mid, maxv, got);
        for (int i = 0; i < W * H; i++) {
            const int want = o(i % W, i / W);
            checks++;
            inside += want > 0 && want < 255;
            if (want < 255 ? got[i] != want : got[i] < 255)
                FAIL("plane %d x %d at %d bits, window %d sample %d: %d, the oracle at 8 bits has %d", W, H, bd, kind, i, got[i], want);
        }
    }
}
static void check_mid(int bd)
{
    const int mid = 1 << (bd - 1);
    int e[25] = { 0 };
    SAME(hp_dir_dc_e<4>(11, HpArr{ e }, mid), mid, "pred4x4 DC_128 at %d bits", bd);
    SAME(hp_dir_dc_e<8>(11, HpArr{ e }, mid), mid, "pred8x8l DC_128 at %d bits", bd);
    SAME(hp_dc16(6, 0, 0, mid), mid, "pred16x16 DC_128 at %d bits", bd);
    SAME(hp_sides_dc<8>(false, false, 0, 0, mid), mid, "whole-block DC of no side, 8 x 8, at %d bits", bd);
    SAME(hp_sides_dc<16>(false, false, 0, 0, mid), mid, "whole-block DC of no side, 16 x 16, at %d bits", bd);
    for (int cell = 0; cell < 8; cell++) {
        SAME(hp_cell_dc(6, cell >> 1, cell & 1, 0, 0, 0, 0, mid), mid, "DC_128 cell %d at %d bits", cell, bd);
        if ((cell >> 1) == 1) /* L00 leaves the cells of rows 4..7 at mid, 0L0 those of rows 0..3 */
            SAME(hp_cell_dc(9, cell >> 1, cell & 1, 0, 0, 0, 0, mid), mid, "L00 cell %d at %d bits", cell, bd);
        if ((cell >> 1) == 0)
            SAME(hp_cell_dc(10, cell >> 1, cell & 1, 0, 0, 0, 0, mid), mid, "0L0 cell %d at %d bits", cell, bd);
    }
}

/* ---- the whole-block DC ---- */
static void check_sides_dc(const Win<uint8_t> &a, int kind)
{
    static const int m16[4] = { 0, 4, 5, 6 };
    for (int k = 0; k < 4; k++) {
        const int mode = m16[k];
        const bool left = mode == 0 || mode == 4, top = mode == 0 || mode == 5;
        int sl = 0, st = 0;
        for (int i = 0; i < 16; i++)
            sl += a(-1, i), st += a(i, -1);
        Win<uint8_t> o = a;
        ffo_h264_pred16x16(mode, o.at(0, 0), PW);
        SAME(hp_sides_dc<16>(left, top, sl, st, 128), o(0, 0), "whole-block DC against pred16x16 mode %d, window %d", mode, kind);
    }
    /* RV40's pred8x8 DCs as h264_pred_codec.inc states them */
    for (int mode = FFHIP_H264_PREDV8_DC_RV40; mode <= FFHIP_H264_PREDV8_TOP_DC_RV40; mode++) {
        const int x = 0, y = 0;
        auto t = [&](int i) -> int { return a(i, -1); };
        auto lraw = [&](int i) -> int { return a(-1, i); };
        auto l = [&](int i) -> int { return lraw(i); };
        auto clip = [](int v) -> int { return v < 0 ? 0 : v > 255 ? 255 : v; };
        auto min = [](int p, int q) -> int { return p < q ? p : q; }; /* the device's, in the text's other rules */
        int v = 0;
#define HP_CODEC_LT a(-1, -1)
#include "kernels/h264_pred_codec.inc"
#undef HP_CODEC_LT
        (void)l; (void)clip; (void)min; (void)x; (void)y;
        int sl = 0, st = 0;
        for (int i = 0; i < 8; i++)
            sl += a(-1, i), st += a(i, -1);
        SAME(hp_sides_dc<8>(mode != FFHIP_H264_PREDV8_TOP_DC_RV40, mode != FFHIP_H264_PREDV8_LEFT_DC_RV40, sl, st, 128), v,
             "whole-block DC against the RV40 rule %d, window %d", mode, kind);
    }
}

int main(int argc, char **argv)
{
    const int nrand = argc > 1 ? atoi(argv[1]) : 4;
    for (int kind = 0; kind < nrand + FIXED; kind++) {
        Win<uint8_t> a;
        fill(a, 255, kind, nrand);
        check4(a, kind);
        check8l(a, kind);
        check_filter_add(a, kind);
        check_blk<8, 8>(a, kind, 11, "pred8x8", ffo_h264_pred8x8);
        check_blk<8, 16>(a, kind, 11, "pred8x16", ffo_h264_pred8x16);
        check_blk<16, 16>(a, kind, 7, "pred16x16", ffo_h264_pred16x16);
        check_sides_dc(a, kind);
    }
    check_tables(nrand);
    static const int depths[4] = { 9, 10, 12, 14 };
    for (int d = 0; d < 4; d++) {
        check_mid(depths[d]);
        check_plane_depth<8, 8>(depths[d], nrand, ffo_h264_pred8x8);
        check_plane_depth<8, 16>(depths[d], nrand, ffo_h264_pred8x16);
        check_plane_depth<16, 16>(depths[d], nrand, ffo_h264_pred16x16);
    }
    if (!inside)
        FAIL("no plane sample of any window lies inside 1..254: the depth comparison compared nothing");
    printf("%ld comparisons, no disagreement\n", checks);
    return 0;
}
