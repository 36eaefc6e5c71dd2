"""CPU tier of H.264's motion-compensation matrix (tests/h264_mc_matrix.py): the lists cover what they claim (predicates over the
cells, nothing counted by hand), the slots are private, the footprints are the oracle's own (probed), the content reaches both
clips of every position, and the numpy clamp model of FFHIP_MC_EMU is the reference's emulated_edge_mc()."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import ffi
import h264_mc_matrix as H
import mc_matrix as M
from test_mc_matrix_cpu import _disjoint

LUMA_STRIDES = [2048, 2052, 2051]      # tests/test_gpu_h264_mc_matrix.py's: whole 16 bytes, whole dwords only, odd
CHROMA_STRIDES = [1024, 1021]
TAILS = [1, 2, 3, 5, 63, 65, 1025]


# ---------------------------------------------------------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------------------------------------------------------
def test_luma_coverage():
    cells = H.luma_cells()
    assert cells == H.luma_cells(), "deterministic"
    assert len(cells) >= 16384 and len(cells) % 4 and len(cells) % 16, "k_h264_qpel_l<4>'s threshold; a cut group; a cut workgroup"
    cross = cells[:H.N_CROSS]
    want = list(itertools.product(H.SIZES, range(16), (0, 1), range(16), range(4)))
    assert len(want) == 6144 == len(cross)
    assert not M.missing(cross, lambda c: (c.w, c.mcxy, c.avg, c.smod, c.dmod % 4), want)
    assert all(c.w == c.h and c.mcxy == c.mx + 4 * c.my and not c.flag for c in cells)
    # neighbours differ in size and alignment; no four in a row pass the tile test
    assert all(a.w != b.w and a.smod != b.smod and a.dmod % 4 != b.dmod % 4 for a, b in zip(cross, cross[1:]))
    assert not any(H.tile_candidate(four) for i, four in H.groups(cells) if i < H.N_CROSS)
    # the binary class reaches every (size, mcxy), put and avg
    binary = [c for i, c in enumerate(cells) if H.content_class(i) == "binary"]
    assert M.covers(binary, lambda c: (c.w, c.mcxy, c.avg), itertools.product(H.SIZES, range(16), (0, 1)))
    for k in H.CONTENT:
        assert M.covers([c for i, c in enumerate(cells) if H.content_class(i) == k], lambda c: (c.w, c.mcxy), itertools.product(H.SIZES, range(16)))
    # the group family
    assert H.N_CROSS % 16 == 0
    fam = [(i, four) for i, four in H.groups(cells) if i >= H.N_CROSS]
    assert all(len({c.fam for c in four}) == 1 for i, four in fam)
    by = {v: [four for i, four in fam if four[0].fam == v] for v in ("tiled", "offdword", "small")}
    assert all(H.tile_candidate(four) for four in by["tiled"])
    assert all(len({c.dmod for c in four}) == 1 and four[0].dmod in (0, 4, 8, 12) for four in by["tiled"])
    tiled = [(four[0].dmod, k, c) for four in by["tiled"] for k, c in enumerate(four)]
    assert {(d, c.mcxy) for d, k, c in tiled} == set(itertools.product((0, 4, 8, 12), range(16))), "every mcxy in a tiled group at each dst % 16"
    assert {(k, c.mcxy) for d, k, c in tiled} == set(itertools.product(range(4), range(16))), "and at each position of the group"
    assert {(d, k, c.avg) for d, k, c in tiled} == set(itertools.product((0, 4, 8, 12), range(4), (0, 1)))
    assert all(0 < sum(c.avg for c in four) < 4 for four in by["tiled"]), "put and avg mixed inside every tiled group"
    assert {(k, H.content_class(i + k)) for i, four in fam if four[0].fam == "tiled" for k in range(4)} == set(itertools.product(range(4), H.CONTENT))
    # one member off the dword grid: sizes pass the tile test, one address fails it
    for four in by["offdword"]:
        off = [k for k, c in enumerate(four) if c.dmod % 4]
        assert len(off) == 1 and all(c.w == 16 for c in four) and len({c.dmod - c.dmod % 4 for c in four}) == 1
    assert {(four[0].dmod - four[0].dmod % 4, k, c.dmod % 4) for four in by["offdword"] for k, c in enumerate(four) if c.dmod % 4} == \
        set(itertools.product((0, 4, 8, 12), range(4), (1, 2, 3)))
    for four in by["small"]:
        assert sorted(c.w for c in four) == [8, 16, 16, 16] and all(c.dmod % 4 == 0 for c in four) and len({c.dmod for c in four}) == 1
    assert {(four[0].dmod, k) for four in by["small"] for k, c in enumerate(four) if c.w == 8} == set(itertools.product((0, 4, 8, 12), range(4)))
    # the tails of tests/test_gpu_h264_mc_matrix.py: a prefix of the group family cuts a group that was a tile candidate
    for n in TAILS:
        assert n % 4 and H.tile_candidate(cells[H.N_CROSS + n - n % 4:H.N_CROSS + n - n % 4 + 4]), n
    assert 1025 % 4 == 1 and 65 % 16 and 8193 % 8 == 1 and 1023 % 4 == 3


def test_the_predicates_notice_a_missing_family():
    """what test_luma_coverage asserts does fail on a list with a family taken away"""
    cells = H.luma_cells()
    key, want = (lambda c: (c.w, c.mcxy, c.avg, c.smod, c.dmod % 4)), list(itertools.product(H.SIZES, range(16), (0, 1), range(16), range(4)))
    assert len(M.missing([c for c in cells if c.fam == "cross" and c.smod != 15], key, want)) == 384
    assert len(M.missing([c for c in cells if c.fam != "cross"], key, want)) > 4000
    without = [c for c in cells if c.fam != "tiled"]
    assert (len(cells) - len(without)) % 4 == 0 and not any(H.tile_candidate(four) for i, four in H.groups(without))
    assert len(without) < 16384


def test_chroma_coverage():
    cells = H.chroma_cells()
    assert cells == H.chroma_cells() and len(cells) % 16
    W, Hs = H.CHROMA_WIDTHS, H.CHROMA_HEIGHTS
    assert W == [8, 4, 2] and Hs == [2, 4, 8, 16]
    want = list(itertools.product(W, Hs, M.CLASSES, range(4), range(4), (0, 1)))
    assert not M.missing(cells, lambda c: (c.w, c.h, M.klass(c), c.smod, c.dmod, c.avg), want)
    assert M.covers(cells, lambda c: (c.w, c.mx, c.my), itertools.product(W, range(8), range(8)))
    assert all(0 <= c.mx < 8 and 0 <= c.my < 8 for c in cells)
    # the halves layout (8 wide, h <= 8) and the row-per-lane one (h == 16), each with the byte-store and the dword-store branch
    assert M.covers(cells, lambda c: (c.w == 8 and c.h <= 8, c.dmod == 0, c.avg), itertools.product((False, True), (False, True), (0, 1)))
    for k in H.CONTENT:
        assert M.covers([c for i, c in enumerate(cells) if H.content_class(i) == k], lambda c: (c.w, M.klass(c)), itertools.product(W, M.CLASSES))
    assert sum(a.w != b.w or a.h != b.h for a, b in zip(cells, cells[1:])) > .9 * len(cells)


def _rung_facts(o, length, lo, hi):
    first, last = o - lo, o + hi
    return first, last, max(0, min(last, length - 1) - max(first, 0) + 1) if last >= 0 and first <= length - 1 else 0


def test_ladder():
    """a rung is what its name says, for every footprint the edge lists use"""
    for length, lo, hi in [(48, 2, 18), (32, 2, 18), (48, 2, 10), (32, 2, 6), (24, 0, 8), (24, 0, 7), (24, 0, 1), (16, 0, 2), (16, 0, 4), (16, 0, 8)]:
        f = lo + hi + 1
        rungs = dict(H.ladder(length, lo, hi))
        assert list(rungs) == H.LADDER_NAMES and len(rungs) == 15
        inside = lambda name: _rung_facts(rungs[name], length, lo, hi)[2]
        first = lambda name: rungs[name] - lo
        last = lambda name: rungs[name] + hi
        assert last("far before") < -f and first("far after") > length - 1 + f
        assert inside("touches before") == 1 and last("touches before") == 0
        assert inside("touches after") == 1 and first("touches after") == length - 1
        for k in (1, 2, 3):
            assert first("straddles before by %d" % k) == -k and last("straddles after by %d" % k) == length - 1 + k
        assert first("starts at 0") == 0 and last("ends at the last") == length - 1
        assert inside("interior") == f and first("interior") > 0 and last("interior") < length - 1
        assert rungs["-3000"] == -3000 and rungs["+3000"] == 3000


def test_edge_coverage():
    names = H.LADDER_NAMES
    pairs = set(itertools.product(names, names))
    cells = H.luma_edge_cells()
    flagged = [c for c in cells if c.flag]
    assert all(c.fam == "edge" and c.flag == H.MC_EMU for c in flagged) and all(c.fam == "interior" for c in cells if not c.flag)
    assert not M.missing(flagged, lambda c: (c.w, c.mcxy) + c.rung, [(s, mc) + p for s in H.SIZES for mc in range(16) for p in pairs])
    assert M.covers(flagged, lambda c: (c.w, c.mcxy, c.avg), itertools.product(H.SIZES, range(16), (0, 1)))
    assert M.covers(flagged, lambda c: (c.w, c.dmod % 4), itertools.product(H.SIZES, range(4)))
    for c in flagged:                                  # the origins are the ladders' (and fit the record's int16)
        assert c.sx == dict(H.ladder(48, 2, c.w + 2))[c.rung[0]] and c.sy == dict(H.ladder(32, 2, c.w + 2))[c.rung[1]]
        assert -32768 <= c.sx < 32768 and -32768 <= c.sy < 32768
    plain = [c for c in cells if not c.flag]
    assert len(plain) >= len(cells) // 6 and M.covers(plain, lambda c: (c.w, c.mcxy), itertools.product(H.SIZES, range(16)))
    assert all(c.sx - 2 >= 0 and c.sy - 2 >= 0 and c.sx + c.w + 2 <= 47 and c.sy + c.w + 2 <= 31 for c in plain), "the window inside the picture"
    assert len(cells) >= 8192, "the dword stride takes the list to k_h264_qpel_l<2>, a stride of whole 16 bytes past k_h264_qpel_t's 1024"

    cells = H.chroma_edge_cells()
    flagged = [c for c in cells if c.flag]
    assert not M.missing(flagged, lambda c: (c.w, M.klass(c)) + c.rung, [(w, k) + p for w in H.CHROMA_WIDTHS for k in M.CLASSES for p in pairs])
    assert M.covers(flagged, lambda c: c.h, H.CHROMA_HEIGHTS) and M.covers(flagged, lambda c: (c.w, c.avg), itertools.product(H.CHROMA_WIDTHS, (0, 1)))
    for c in flagged:
        assert c.sx == dict(H.ladder(24, 0, c.w - 1 + bool(c.mx)))[c.rung[0]] and c.sy == dict(H.ladder(16, 0, c.h - 1 + bool(c.my)))[c.rung[1]]
    plain = [c for c in cells if not c.flag]
    assert len(plain) >= len(cells) // 6
    assert all(c.sx >= 0 and c.sy >= 0 and c.sx + c.w <= 23 and c.sy + c.h <= 15 for c in plain)


# ---------------------------------------------------------------------------------------------------------------------------
# layout
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,stride", [("luma", s) for s in LUMA_STRIDES] + [("chroma", s) for s in CHROMA_STRIDES])
def test_slots_are_private(kind, stride):
    b = H.lay_out(kind, stride)
    mod = 4 if b.chroma else 16
    bef, aft = b.margin
    assert b.sstride == b.dstride == stride
    assert _disjoint(b.sslot, b.srows, stride) and _disjoint(b.dslot, b.drows, stride)
    # the planes begin and end with slack: a guard row, then the first slot's own SLACK_Y rows
    assert min(s[0] for s in b.sslot) >= 1 and max(s[1] for s in b.sslot) <= b.srows - 1
    assert M.SLACK_Y >= 8 and M.SLACK_X >= 16 and M.DSLACK >= 8
    for i, (c, (py, px), f, s) in enumerate(zip(b.cells, b.spos, b.foot, b.sslot)):
        assert (py * stride + px) % mod == c.smod and b.src_offset(i, 1) == py * stride + px
        # the whole window a kernel may load (luma: 21 x 21 whatever the position; the chunk loaders up to 15 bytes either side;
        # the matrix-core kernels one row below the block at the positions without a vertical plane) lies inside the slot
        assert py - bef - M.SLACK_Y >= s[0] and py + c.h + aft + M.SLACK_Y <= s[1], (c, s)
        assert px - bef - M.SLACK_X >= s[2] and px + c.w + aft + M.SLACK_X <= s[3], (c, s)
        assert f == (py - bef * bool(c.my), py + c.h + aft * bool(c.my), px - bef * bool(c.mx), px + c.w + aft * bool(c.mx))
    for i, (c, (py, px), s) in enumerate(zip(b.cells, b.dpos, b.dslot)):
        assert (py * stride + px) % mod == c.dmod and b.dst_offset(i, 1) == py * stride + px
        assert py - M.DSLACK >= s[0] and py + 16 + M.DSLACK <= s[1] and px - M.DSLACK >= s[2] and px + 16 + M.DSLACK <= s[3]
    # the records say the same
    rec = b.records(1)
    assert rec.itemsize == (20 if b.chroma else 16)
    i = len(rec) // 2
    c = b.cells[i]
    assert (rec[i]["dst_offset"], rec[i]["src_offset"], rec[i]["avg"], rec[i]["flags"]) == (b.dst_offset(i, 1), b.src_offset(i, 1), c.avg, 0)
    if b.chroma:
        assert (8 >> rec[i]["w_idx"], rec[i]["h"], rec[i]["x"], rec[i]["y"]) == (c.w, c.h, c.mx, c.my)
    else:
        assert (16 >> rec[i]["size_idx"], rec[i]["mcxy"]) == (c.w, c.mcxy)


@pytest.mark.parametrize("kind,stride", [("luma_edge", 2048), ("luma_edge", 2051), ("chroma_edge", 1021)])
def test_edge_layout(kind, stride):
    b = H.lay_out(kind, stride)
    pw, ph = b.pic
    assert (pw, ph) == ((24, 16) if b.chroma else (48, 32))
    assert _disjoint(b.dslot, b.drows, stride)
    pic = b.picture()
    assert pic.shape == (b.srows, stride) and pic.sum() == pw * ph
    ys, xs = np.nonzero(pic)
    # slack round the picture for the unflagged records' chunk loads: 8 rows, 16 samples and more
    assert ys.min() >= 8 and ys.max() < b.srows - 8 and xs.min() >= 16 and xs.max() < stride - 32
    assert (ys.min() * stride + xs.min()) % 4, "the picture's origin is on no dword"
    src = b.source(8, 1)
    poisoned = b.poisoned(src, 8)
    assert np.array_equal(poisoned[pic], src[pic]) and (poisoned[~pic] != src[~pic]).all()
    for i, c in enumerate(b.cells):
        y, x = divmod(b.src_offset(i, 1), stride)
        assert (y, x) == ((ys.min(), xs.min()) if c.flag else (ys.min() + c.sy, xs.min() + c.sx))
    rec = b.records(1)
    assert all((r["flags"], r["src_x"], r["src_y"]) == ((1, c.sx, c.sy) if c.flag else (0, 0, 0)) for r, c in zip(rec, b.cells))
    # the clamp model: sample (x, y) at row clamp(y, 0, h - 1), column clamp(x, 0, w - 1), written out the slow way for a few cells
    bef = b.margin[0]
    for c in [k for k in b.cells if k.flag][::97]:
        win = b.gather(src, c)
        for r, q in [(0, 0), (20, 20), (3, 17), (11, 2)]:
            yy, xx = min(max(c.sy - bef + r, 0), ph - 1), min(max(c.sx - bef + q, 0), pw - 1)
            assert win[r, q] == src[ys.min() + yy, xs.min() + xx]


# ---------------------------------------------------------------------------------------------------------------------------
# footprints: probed, not stated
# ---------------------------------------------------------------------------------------------------------------------------
def _band(size, first, count):
    m = np.zeros(H.PROBE, bool)
    m[first:first + count] = True
    return m


def test_luma_footprints_are_the_oracles():
    """one sample at a time of the 21 x 21 window complemented: which ones change the oracle's output.  The expectation below is
    written from the planes a position combines — block (F), rows of the block x all size + 5 columns (H), the transpose (V), the
    whole window (J) — so H + V gives a cross, not a rectangle"""
    for size in H.SIZES:
        for mc in range(16):
            got = H.luma_mask(size, mc)
            f, h, v, j = H.luma_planes(mc)
            mx, my = mc & 3, mc >> 2
            own, all_ = _band(size, 2, size), _band(size, 0, size + 5)
            want = np.zeros((H.PROBE, H.PROBE), bool)
            if f:
                want |= np.outer(_band(size, 2 + (mc == 12), size), _band(size, 2 + (mc == 3), size))
            if h:
                want |= np.outer(_band(size, 2 + (my == 3), size), all_)
            if v:
                want |= np.outer(all_, _band(size, 2 + (mx == 3), size))
            if j:
                want |= np.outer(all_, all_)
            assert np.array_equal(got, want), (size, mc, got.astype(int))
            if h and v and not j:
                assert got.sum() == 2 * size * (size + 5) - size * size and not got[0, 0] and not got[size + 4, size + 4], "a cross"
            # the 8-bit functions read nothing more (what they may not show at 8 bits, a weight of 1 / 1024, the check of the whole
            # list below settles)
            at8 = H.probe(0, H._luma(size, mc, 0, 0, 0, "probe"), 2, bd=8)
            assert not (at8 & ~got).any() and at8.sum() >= .7 * got.sum(), (size, mc)


def test_chroma_footprints_are_the_oracles():
    for w in H.CHROMA_WIDTHS:
        for h in H.CHROMA_HEIGHTS:
            for x, y in [(0, 0), (3, 0), (0, 5), (1, 1), (7, 7)]:
                got = H.chroma_mask(w, h, bool(x), bool(y))
                want = np.outer(_band(h, 0, h + bool(y)), _band(w, 0, w + bool(x)))
                assert np.array_equal(got, want), (w, h, x, y)
                c = H._chroma(w, h, x, y, 0, 0, 0, "probe")
                assert np.array_equal(H.probe(1, c, 0, bd=8), want), "every (x, y) of a class reads what its class reads"


@functools.lru_cache(maxsize=None)
def _list(kind, stride, bd):
    b = H.lay_out(kind, stride)
    src, dst0 = b.source(bd, 11 + bd), b.destination(bd, 12 + bd)
    return b, src, dst0, b.want(bd, src, dst0)


@pytest.mark.parametrize("kind,stride,bd", [("luma", 2048, 8), ("luma", 2051, 10), ("chroma", 1024, 8), ("chroma", 1021, 14)])
def test_nothing_outside_the_footprints_reaches_the_oracle(kind, stride, bd):
    b, src, dst0, want = _list(kind, stride, bd)
    fp = b.footprints()
    poisoned = b.poisoned(src, bd)
    assert np.array_equal(poisoned[fp], src[fp]) and (poisoned[~fp] != src[~fp]).all() and (~fp).mean() > .3
    again = b.want(bd, poisoned, dst0)
    assert b.first_bad(again, want) is None, b.first_bad(again, want)
    # the footprint is inside its bounding box, the box inside its slot
    box = np.zeros_like(fp)
    for y0, y1, x0, x1 in b.foot:
        box[y0:y1, x0:x1] = True
    assert not (fp & ~box).any()


@pytest.mark.parametrize("kind,stride,bd", [("luma", 2048, 8), ("luma", 2051, 10), ("chroma", 1024, 8), ("chroma", 1021, 14),
                                            ("luma_edge", 2048, 8), ("chroma_edge", 1021, 8), ("luma_edge", 2051, 14)])
def test_the_oracle_changes_the_blocks_and_nothing_else(kind, stride, bd):
    b, src, dst0, want = _list(kind, stride, bd)
    ins = b.inside()
    assert (want[ins] != dst0[ins]).mean() > .5
    assert np.array_equal(want[~ins], dst0[~ins])
    # a prefix: the records after it stay as they were
    n = len(b.cells) // 3
    part = b.want(bd, src, dst0, 0, n)
    head = b.inside(0, n)
    assert np.array_equal(part[head], want[head]) and np.array_equal(part[~head], dst0[~head])
    if kind.endswith("edge"):
        again = b.want(bd, b.poisoned(src, bd), dst0)
        assert b.first_bad(again, want) is None, "the surroundings of the picture reach no record: " + str(b.first_bad(again, want))


@pytest.mark.parametrize("bd", [8, 10])
def test_content_reaches_the_clips(bd):
    """over the blocks of every mcxy but 0 (a copy), the oracle's output holds both 0 and the maximum in a block whose source is not
    flat: binary noise puts c = d = max, b = e = 0 (a sum of 40 x max and more) and c = d = 0, b = max (negative) under the taps"""
    b, src, dst0, want = _list("luma", 2048 if bd == 8 else 2051, bd)
    maxv = (1 << bd) - 1
    low, high = set(), set()
    for i, (c, (y, x)) in enumerate(zip(b.cells, b.dpos)):
        if H.content_class(i) in ("noise", "binary") and not c.avg:
            out = want[y:y + c.h, x:x + c.w]
            if (out == 0).any():
                low.add((c.w, c.mcxy))
            if (out == maxv).any():
                high.add((c.w, c.mcxy))
    wanted = set(itertools.product(H.SIZES, range(1, 16)))
    assert wanted <= low and wanted <= high, (sorted(wanted - low), sorted(wanted - high))
    # chroma is a convex mix: the extremes come from the flat and binary slots
    b, src, dst0, want = _list("chroma", 1024 if bd == 8 else 1021, 8 if bd == 8 else 14)
    ins = b.inside()
    assert (want[ins] == 0).any() and (want[ins] == (255 if bd == 8 else 16383)).any()


def test_first_bad_names_the_cell():
    b, src, dst0, want = _list("luma", 2048, 8)
    assert b.first_bad(want, want) is None
    i = H.N_CROSS + 4 * 33 + 2
    got = want.copy()
    y, x = b.dpos[i]
    got[y + 3, x + 5] ^= 1
    c = b.cells[i]
    text = b.first_bad(got, want)
    for part in ("1 mismatches", "block %d " % i, c.fam, "size 16", "mcxy %d" % c.mcxy, "avg" if c.avg else "put", "src mod 16 %d" % c.smod,
                 "dst mod 4 %d" % (c.dmod % 4), "position 2 in its group of four", "row 3 column 5"):
        assert part in text, (part, text)
    got = want.copy()
    got[b.dslot[i][0], b.dslot[i][2]] ^= 1                          # a store that left its block: in the slot's slack
    assert "row -8 column" in b.first_bad(got, want)
    e, esrc, edst0, ewant = _list("luma_edge", 2048, 8)
    i = next(k for k, c in enumerate(e.cells) if c.flag and c.rung == ("touches before", "+3000"))
    got = ewant.copy()
    got[e.dpos[i]] ^= 1
    assert "FFHIP_MC_EMU" in e.first_bad(got, ewant) and "x touches before, y +3000" in e.first_bad(got, ewant)
    ch, csrc, cdst0, cwant = _list("chroma", 1024, 8)
    got = cwant.copy()
    got[ch.dpos[7]] ^= 1
    c = ch.cells[7]
    assert "w %d, h %d, x %d, y %d" % (c.w, c.h, c.mx, c.my) in ch.first_bad(got, cwant) and "src mod 4 %d" % c.smod in ch.first_bad(got, cwant)


# ---------------------------------------------------------------------------------------------------------------------------
# the clamp model == the reference's emulated_edge_mc() (the only test here that may skip)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not ffi.have_ref(), reason="oracle/_ref/libffref.so not built")
@pytest.mark.parametrize("kind", ["luma_edge", "chroma_edge"])
def test_clamp_model_is_emulated_edge_mc(kind):
    """videodsp_template.c:24-100 into a 21 x 21 buffer, for every flagged record of the ladders"""
    R = ffi.ref()
    R.ffref_emulated_edge_mc.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_ssize_t, C.c_ssize_t] + [C.c_int] * 6
    R.ffref_emulated_edge_mc.restype = None
    stride = 2048 if kind == "luma_edge" else 1021
    b = H.lay_out(kind, stride)
    src = b.source(8, 5)
    pw, ph = b.pic
    bef = b.margin[0]
    org = src.ctypes.data + H.PIC_AT[0] * stride + H.PIC_AT[1]
    buf = np.zeros((H.PROBE, stride), np.uint8)
    n = 0
    for c in b.cells:
        if not c.flag:
            continue
        x, y = c.sx - bef, c.sy - bef
        buf[:] = 0x5a
        R.ffref_emulated_edge_mc(8, buf.ctypes.data, org + y * stride + x, stride, stride, H.PROBE, H.PROBE, x, y, pw, ph)
        assert np.array_equal(buf[:, :H.PROBE], b.gather(src, c)), (c, buf[:, :H.PROBE], b.gather(src, c))
        n += 1
    assert n == 225 * (48 if kind == "luma_edge" else 12)
