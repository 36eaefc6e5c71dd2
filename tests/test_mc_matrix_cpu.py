"""CPU tier of the motion-compensation matrix (tests/mc_matrix.py): the slots are private, the lists cover what they claim, the
footprint definition is the oracle's own, and the oracle equals the reference at the heights the matrix adds."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import ffi
import mc_matrix as M
from ffi import ptr, u8p, i16p

STRIDES = [(1024, 1200), (1021, 1203)]


def _disjoint(rects, rows, cols):
    """no two rectangles (y0, y1, x0, x1) overlap, all inside rows x cols"""
    count = np.zeros((rows, cols), np.uint8)
    for y0, y1, x0, x1 in rects:
        assert 0 <= y0 < y1 <= rows and 0 <= x0 < x1 <= cols, (y0, y1, x0, x1)
        count[y0:y1, x0:x1] += 1
    return int(count.max()) == 1


def _batches():
    for ss, sd in STRIDES:
        for chroma in (0, 1):
            for mode in (0, 1, 4):
                yield M.lay_out_hevc(chroma, mode, ss, sd)
        for filt in (0, 3):
            yield M.lay_out_vp9(filt, ss, sd)


def test_slots_are_private():
    for b in _batches():
        assert _disjoint(b.sslot, b.srows, b.sstride)
        # a guard row above and below the slots: a chunk load that starts left of the first slot stays in the plane
        assert min(s[0] for s in b.sslot) >= 1 and max(s[1] for s in b.sslot) <= b.srows - 1
        for c, (py, px), f, s in zip(b.cells, b.spos, b.foot, b.sslot):
            assert f[0] - M.SLACK_Y >= s[0] and f[1] + M.SLACK_Y <= s[1] and f[2] - M.SLACK_X >= s[2] and f[3] + M.SLACK_X <= s[3], (c, f, s)
            assert M.SLACK_Y >= 8 and M.SLACK_X >= 8
            assert (py * b.sstride + px) % 4 == c.smod
            bef, aft = b.margin
            assert f == (py - bef * bool(c.my), py + c.h + aft * bool(c.my), px - bef * bool(c.mx), px + c.w + aft * bool(c.mx))
        if b.flat:
            assert all(a[1] <= n[0] for a, n in zip(b.dslot, b.dslot[1:])) and b.dslot[0][0] == 0 and b.dslot[-1][1] == b.dlen
            for c, o, s in zip(b.cells, b.dpos, b.dslot):
                assert o - M.DSLACK >= s[0] and o + 64 * 64 + M.DSLACK <= s[1] and o % 4 == c.dmod
        else:
            assert _disjoint(b.dslot, b.drows, b.dstride)
            for c, (py, px), s in zip(b.cells, b.dpos, b.dslot):
                assert py - M.DSLACK >= s[0] and py + 64 + M.DSLACK <= s[1] and px - M.DSLACK >= s[2] and px + 64 + M.DSLACK <= s[3]
                assert (py * b.dstride + px) % 4 == c.dmod
        # the other list's block: 64 rows of pitch 64, and the three int16 k_hevc_mc may read beyond a row's width, inside its slot
        assert all(i * b.s2size <= o and o + 64 * 64 + 3 <= (i + 1) * b.s2size for i, o in enumerate(b.s2pos))
        assert all(o % 4 == c.s2mod for c, o in zip(b.cells, b.s2pos))


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("chroma", [0, 1])
def test_hevc_coverage(chroma, mode):
    cells = M.hevc_cells(chroma, mode)
    nf = 8 if chroma else 4
    assert cells == M.hevc_cells(chroma, mode), "deterministic"
    assert len(cells) == 1600 + 10 * nf * nf
    W, H = M.HEVC_WIDTHS, M.HEVC_HEIGHTS
    assert W == [2, 4, 6, 8, 12, 16, 24, 32, 48, 64] and H == W
    want = list(itertools.product(W, H, M.CLASSES, range(4)))
    assert not M.missing(cells, lambda c: (c.w, c.h, M.klass(c), c.smod), want)
    assert len([c for c in cells[:1600]]) == len(want)
    assert M.covers(cells, lambda c: (c.w, c.mx), itertools.product(W, range(nf)))
    assert M.covers(cells, lambda c: (c.w, c.my), itertools.product(W, range(nf)))
    assert M.covers(cells[:1600], lambda c: (c.w, c.mx), itertools.product(W, range(1, nf))), "already in the class blocks"
    assert M.covers(cells[:1600], lambda c: (c.w, c.my), itertools.product(W, range(1, nf)))
    assert M.covers(cells, lambda c: (c.w, c.mx, c.my), itertools.product(W, range(nf), range(nf)))
    assert M.covers(cells[1600:], lambda c: c.h, H), "heights in turn"
    assert M.covers(cells, lambda c: (c.w, M.klass(c), c.dmod), itertools.product(W, M.CLASSES, range(4)))
    assert M.covers(cells, lambda c: (c.w, c.smod, c.dmod), itertools.product(W, range(4), range(4)))
    assert M.covers(cells, lambda c: (c.w, c.s2mod), itertools.product(W, range(4)))
    if not chroma:
        # the launcher's split: 16 x 16 records scattered among the others, and a last group of 64 records that is not full
        at = [i for i, c in enumerate(cells) if c.w == 16 and c.h == 16]
        assert len(cells) % 64 and len(at) >= 16 and len({i // 64 for i in at}) >= 2 and len({i % 4 for i in at}) == 4
    # the weights are tests/test_gpu_hevc.py's: the same draws from the same generator
    rng = np.random.default_rng(5)
    ref = []
    for rep in range(6):
        if rep % 3 == 0:
            ref.append((int(rng.choice([0, 7, 12])), int(rng.choice([0, 128, 255])), int(rng.choice([0, 128, 255])), int(rng.choice([0, 255]))))
        else:
            d = int(rng.integers(0, 8))
            ref.append((d, (1 << d) + int(rng.integers(-128, 128)), (1 << d) + int(rng.integers(-128, 128)), int(rng.integers(-256, 255))))
    rng = np.random.default_rng(5)
    assert [M.weights(rng, rep) for rep in range(6)] == ref


@pytest.mark.parametrize("filt", [0, 1, 2, 3])
def test_vp9_coverage(filt):
    cells = M.vp9_cells(filt)
    assert cells == M.vp9_cells(filt)
    W, H = M.VP9_WIDTHS, M.VP9_HEIGHTS
    assert W == [4, 8, 16, 32, 64] and H == [1, 2, 3, 4, 8, 16, 32, 33, 64]
    assert len(cells) == 360 + 5 * 256 and all(c.filt == filt for c in cells)
    assert not M.missing(cells[:360], lambda c: (c.w, c.h, M.klass(c), c.avg), itertools.product(W, H, M.CLASSES, (0, 1)))
    assert not M.missing(cells[:360], lambda c: (c.w, M.klass(c), c.avg, c.smod), itertools.product(W, M.CLASSES, (0, 1), range(4)))
    assert not M.missing(cells[360:], lambda c: (c.w, c.mx, c.my), itertools.product(W, range(16), range(16)))
    assert M.covers(cells[360:], lambda c: (c.w, c.h), itertools.product(W, H))
    assert M.covers(cells[360:], lambda c: (c.w, c.avg), itertools.product(W, (0, 1)))
    assert M.covers(cells, lambda c: (c.w, M.klass(c), c.avg, c.dmod), itertools.product(W, M.CLASSES, (0, 1), range(4)))
    at = [i for i, c in enumerate(cells) if c.w == 16 and c.h == 16]
    assert len(cells) % 64 and len(at) >= 16 and len({i // 64 for i in at}) >= 2


def _hevc_pair(chroma, mode, bd, strides):
    b = M.lay_out_hevc(chroma, mode, *strides)
    src, dst0, s2 = b.source(bd, 1), b.destination(bd, 2), b.src2(3)
    return b, dst0, M.hevc_want(b, chroma, mode, bd, src, dst0, s2), M.hevc_want(b, chroma, mode, bd, b.poisoned(src, bd), dst0, s2), src


def _footprint_checks(b, dst0, want, again, src, bd):
    assert b.first_bad(again, want) is None, b.first_bad(again, want)
    ins = b.inside()
    assert np.array_equal(want[~ins], dst0[~ins]), "the oracle stays inside the blocks"
    assert (want[ins] != dst0[ins]).mean() > .5
    fp = b.footprints()
    poisoned = b.poisoned(src, bd)
    assert np.array_equal(poisoned[fp], src[fp]) and (poisoned[~fp] != src[~fp]).all()
    assert (~fp).mean() > .3


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("chroma", [0, 1])
def test_hevc_footprint_is_the_oracles(chroma, mode):
    """the bytes outside the union of the footprints do not reach the oracle's output"""
    b, dst0, want, again, src = _hevc_pair(chroma, mode, 8, STRIDES[(chroma + mode) & 1])
    _footprint_checks(b, dst0, want, again, src, 8)
    if mode == 0:
        assert want.max() > 255 << 6 and want.min() < 0, "the intermediates leave the range of a copy on both sides"
    else:
        ins = b.inside()
        assert (want[ins] == 0).any() and (want[ins] == 255).any(), "both clips"


@pytest.mark.parametrize("chroma,mode", [(0, 1), (1, 4)])
def test_hevc_footprint_is_the_oracles_10bit(chroma, mode):
    b, dst0, want, again, src = _hevc_pair(chroma, mode, 10, STRIDES[1])
    _footprint_checks(b, dst0, want, again, src, 10)


@pytest.mark.parametrize("filt,bd", [(0, 8), (1, 8), (2, 8), (3, 8), (1, 10), (3, 10)])
def test_vp9_footprint_is_the_oracles(filt, bd):
    b = M.lay_out_vp9(filt, *STRIDES[filt & 1])
    src, dst0 = b.source(bd, 4), b.destination(bd, 5)
    want, again = M.vp9_want(b, bd, src, dst0), M.vp9_want(b, bd, b.poisoned(src, bd), dst0)
    _footprint_checks(b, dst0, want, again, src, bd)
    ins = b.inside()
    assert (want[ins] == 0).any() and (want[ins] == (1 << bd) - 1).any(), "both clips"


def test_footprint_is_tight_where_a_tap_is_not_zero():
    """complementing a footprint's own outermost row changes the oracle's block: the definition is not merely large enough"""
    O = ffi.oracle()
    rng = np.random.default_rng(9)
    src = rng.integers(0, 256, (40, 48), dtype=np.uint8)
    for chroma, my, first, last in [(0, 2, -3, 4), (1, 4, -1, 2)]:         # (-1, 4, .., -1) and (-4, 36, 36, -4): no zero tap
        for edge in (first, last):
            a, b = np.zeros((64, 64), np.int16), np.zeros((64, 64), np.int16)
            O.ffo_hevc_mc(chroma, 0, a.ctypes.data, 0, C.cast(src.ctypes.data + 12 * 48 + 12, u8p), 48, 8, my, my, 8)
            p = src.copy()
            p[12 + edge if edge < 0 else 12 + 7 + edge] ^= 255
            O.ffo_hevc_mc(chroma, 0, b.ctypes.data, 0, C.cast(p.ctypes.data + 12 * 48 + 12, u8p), 48, 8, my, my, 8)
            assert not np.array_equal(a, b)
            p = src.copy()
            p[:, 12 + edge if edge < 0 else 12 + 7 + edge] ^= 255
            O.ffo_hevc_mc(chroma, 0, b.ctypes.data, 0, C.cast(p.ctypes.data + 12 * 48 + 12, u8p), 48, 8, my, my, 8)
            assert not np.array_equal(a, b)
    for filt, m, first, last in [(2, 8, -3, 4), (3, 8, 0, 1)]:              # sharp's (-4, 11, .., -4); bilinear's two taps
        for edge in (first, last):
            a = np.zeros((16, 16), np.uint8)
            O.ffo_vp9_mc(filt, 0, ptr(a), 16, C.cast(src.ctypes.data + 12 * 48 + 12, u8p), 48, 8, 8, m, m)
            for axis in (0, 1):
                p, b = src.copy(), np.zeros((16, 16), np.uint8)
                at = 12 + edge if edge <= 0 else 12 + 7 + edge
                if axis:
                    p[:, at] ^= 255
                else:
                    p[at] ^= 255
                O.ffo_vp9_mc(filt, 0, ptr(b), 16, C.cast(p.ctypes.data + 12 * 48 + 12, u8p), 48, 8, 8, m, m)
                assert not np.array_equal(a, b) or edge == 0, (filt, edge, axis)


# ---------------------------------------------------------------------------------------------------------------------------
# oracle == reference at the heights the matrix adds (tests/test_oracle_vs_ref.py draws h from {2, 4, 8, 16, 64}; VP9 never 3)
# ---------------------------------------------------------------------------------------------------------------------------
needs_ref = pytest.mark.skipif(not os.path.exists(ffi.REF_SO), reason="oracle/_ref/libffref.so not built")
NEW_HEIGHTS = [6, 12, 24, 48]


@needs_ref
def test_hevc_mc_new_heights():
    """put_hevc_{qpel,epel}{,_uni,_uni_w,_bi,_bi_w} at the AMP and chroma heights: every width x class, 8 bits"""
    from test_oracle_vs_ref import hevc_weight_case
    R, O = ffi.ref(), ffi.oracle()
    rng = np.random.default_rng(781)
    src = rng.integers(0, 256, (80, 96), dtype=np.uint8)
    src[:40] = rng.choice(np.array([0, 255], np.uint8), (40, 96))
    rep = 0
    for chroma in (0, 1):
        nfrac = 8 if chroma else 4
        for w in M.HEVC_WIDTHS:
            for h in NEW_HEIGHTS:
                for cls in range(4):
                    mx = int(rng.integers(1, nfrac)) if cls & 1 else 0
                    my = int(rng.integers(1, nfrac)) if cls & 2 else 0
                    y0 = int(rng.integers(4, 80 - h - 5)); x0 = int(rng.integers(4, 96 - w - 5))
                    sp = C.cast(src.ctypes.data + y0 * 96 + x0, u8p)
                    a16, b16 = np.zeros((64, 64), np.int16), np.zeros((64, 64), np.int16)
                    R.ffref_hevc_mc(chroma, 0, a16.ctypes.data, 0, sp, 96, h, mx, my, w)
                    O.ffo_hevc_mc(chroma, 0, b16.ctypes.data, 0, sp, 96, h, mx, my, w)
                    assert np.array_equal(a16, b16), (chroma, w, h, mx, my)
                    a8, b8 = np.full((64, 80), 7, np.uint8), np.full((64, 80), 7, np.uint8)
                    R.ffref_hevc_mc(chroma, 1, a8.ctypes.data, 80, sp, 96, h, mx, my, w)
                    O.ffo_hevc_mc(chroma, 1, b8.ctypes.data, 80, sp, 96, h, mx, my, w)
                    assert np.array_equal(a8, b8), (chroma, w, h, mx, my, "uni")
                    src2 = rng.integers(-8192, 16384, (64, 64)).astype(np.int16) if rep % 4 else np.full((64, 64), 16383 if rep % 8 else -8192, np.int16)
                    for mode in (2, 3, 4):
                        rep += 1
                        d, wx0, wx1, ox = hevc_weight_case(rng, rep)
                        a8, b8 = np.full((64, 80), 7, np.uint8), np.full((64, 80), 7, np.uint8)
                        R.ffref_hevc_mc_w(chroma, mode, ptr(a8), 80, sp, 96, ptr(src2, i16p), h, d, wx0, wx1, ox, mx, my, w)
                        O.ffo_hevc_mc_w(chroma, mode, ptr(b8), 80, sp, 96, ptr(src2, i16p), h, d, wx0, wx1, ox, mx, my, w)
                        assert np.array_equal(a8, b8), (chroma, mode, w, h, mx, my, d, wx0, wx1, ox)


@pytest.fixture
def depth(request):
    R = ffi.ref()
    R.ffref_hevc_set_bit_depth(request.param)
    yield request.param
    R.ffref_hevc_set_bit_depth(8)


@needs_ref
@pytest.mark.parametrize("depth", [10], indirect=True)
def test_hevc_mc_new_heights_10bit(depth):
    from test_oracle_vs_ref import hevc_weight_case
    from test_oracle_vs_ref_hbd import at, pix
    R, O = ffi.ref(), ffi.oracle()
    rng = np.random.default_rng(782)
    src = pix(rng, (80, 96), depth, extremes=True)
    rep = 0
    for chroma in (0, 1):
        nfrac = 8 if chroma else 4
        for w in M.HEVC_WIDTHS:
            for h in NEW_HEIGHTS:
                for cls in range(4):
                    mx = int(rng.integers(1, nfrac)) if cls & 1 else 0
                    my = int(rng.integers(1, nfrac)) if cls & 2 else 0
                    y0, x0 = int(rng.integers(4, 80 - h - 5)), int(rng.integers(4, 96 - w - 5))
                    sp = at(src, y0, x0)
                    a16, b16 = np.zeros((64, 64), np.int16), np.zeros((64, 64), np.int16)
                    R.ffref_hevc_mc(chroma, 0, a16.ctypes.data, 0, sp, 192, h, mx, my, w)
                    O.ffo_hevc_mc_bd(depth, chroma, 0, b16.ctypes.data, 0, sp, 192, h, mx, my, w)
                    assert np.array_equal(a16, b16), (chroma, w, h, mx, my)
                    a, b = np.full((64, 80), 7, np.uint16), np.full((64, 80), 7, np.uint16)
                    R.ffref_hevc_mc(chroma, 1, a.ctypes.data, 160, sp, 192, h, mx, my, w)
                    O.ffo_hevc_mc_bd(depth, chroma, 1, b.ctypes.data, 160, sp, 192, h, mx, my, w)
                    assert np.array_equal(a, b), (chroma, w, h, mx, my, "uni")
                    src2 = rng.integers(-8192, 16384, (64, 64)).astype(np.int16) if rep % 4 else np.full((64, 64), 16383 if rep % 8 else -8192, np.int16)
                    for mode in (2, 3, 4):
                        rep += 1
                        d, wx0, wx1, ox = hevc_weight_case(rng, rep)
                        a, b = np.full((64, 80), 7, np.uint16), np.full((64, 80), 7, np.uint16)
                        R.ffref_hevc_mc_w(chroma, mode, ptr(a), 160, sp, 192, ptr(src2, i16p), h, d, wx0, wx1, ox, mx, my, w)
                        O.ffo_hevc_mc_w_bd(depth, chroma, mode, ptr(b), 160, sp, 192, ptr(src2, i16p), h, d, wx0, wx1, ox, mx, my, w)
                        assert np.array_equal(a, b), (chroma, mode, w, h, mx, my, d, wx0, wx1, ox)


@needs_ref
def test_vp9_mc_new_heights():
    """VP9DSPContext.mc at 3 and 33 rows: every filter x put / avg x width x class"""
    R, O = ffi.ref(), ffi.oracle()
    rng = np.random.default_rng(961)
    src = rng.integers(0, 256, (90, 100), dtype=np.uint8)
    src[:30] = rng.choice(np.array([0, 255], np.uint8), (30, 100))
    for f in range(4):
        for avg in (0, 1):
            for w in M.VP9_WIDTHS:
                for h in (3, 33):
                    for cls in range(4):
                        for rep in range(3):
                            mx = int(rng.integers(1, 16)) if cls & 1 else 0
                            my = int(rng.integers(1, 16)) if cls & 2 else 0
                            y0, x0 = int(rng.integers(4, 90 - h - 5)), int(rng.integers(4, 100 - w - 5))
                            sp = C.cast(src.ctypes.data + y0 * 100 + x0, u8p)
                            d0 = rng.integers(0, 256, (64, 72), dtype=np.uint8)
                            a, b = d0.copy(), d0.copy()
                            R.ffref_vp9_mc(f, avg, ptr(a), 72, sp, 100, w, h, mx, my)
                            O.ffo_vp9_mc(f, avg, ptr(b), 72, sp, 100, w, h, mx, my)
                            assert np.array_equal(a, b), (f, avg, w, h, mx, my)
