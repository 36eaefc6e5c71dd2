"""The generator of tests/hevc_lf_matrix.py, pinned without a GPU: its numpy models equal the oracle byte for byte on every generated
case (so the cell labels can be trusted), every required (route, cell) pair occurs (the cap on omitted cells is zero), and the
layouts hold what the GPU test relies on: private tiles and slots, records inside their buffers, and route labels that equal what
the kernel's own conditions give for the addresses."""
import ctypes as C
import functools

import numpy as np
import pytest

import ffi
import hevc_lf_matrix as M


@functools.lru_cache(maxsize=None)
def _lf(bd, group):
    return M.lf_launches(bd, group)


@functools.lru_cache(maxsize=None)
def _sao(bd, edge, bytewise):
    return M.sao_launches(bd, edge, bytewise)


def _disjoint(shape, rects):
    """the rectangles (y0, y1, x0, x1) lie inside `shape` and do not overlap"""
    seen = np.zeros(shape, np.int32)
    for y0, y1, x0, x1 in rects:
        assert 0 <= y0 < y1 <= shape[0] and 0 <= x0 < x1 <= shape[1], (y0, y1, x0, x1, shape)
        seen[y0:y1, x0:x1] += 1
    return seen.max() <= 1


@pytest.mark.parametrize("group", M.LF_GROUPS)
@pytest.mark.parametrize("bd", M.DEPTHS)
def test_lf_model_is_the_oracle(bd, group):
    changed = 0
    for L in _lf(bd, group):
        want = L.want_oracle()
        bad = L.first_bad(L.want_model(), want)
        assert bad is None, bad
        p0, p1 = L.plane(L.buf), L.plane(want)
        for i, s in enumerate(L.segs):
            for j, lab in enumerate(s.labels):
                r = L.group_region(i, j)
                moved = bool((p0[r] != p1[r]).any())
                assert moved == lab.changed, (L.name, i, j, lab)
                if M.should_change(lab) is not None:
                    assert moved == M.should_change(lab), (L.name, i, j, lab)
                changed += moved
    assert changed


@pytest.mark.parametrize("bd", M.DEPTHS)
def test_lf_coverage(bd):
    """every luma cell on each of R1 .. R6 (and on R56, the alternating lines), every chroma cell on R1 and on every R7 route"""
    launches = [L for g in M.LF_GROUPS if g != "counts" for L in _lf(bd, g)]
    for route in M.LUMA_ROUTES:
        assert M.lf_missing(launches, route, 0) == [], route
    for route in M.CHROMA_ROUTES:
        assert M.lf_missing(launches, route, 1) == [], route
    # R3 through an odd record offset and through an unaligned base; R2's vertical record as the first, a middle and the last of a wave
    r3 = [(L.k != 0, (s.offset // L.ps) % 4 != 0) for L in _lf(bd, "R3") for s in L.segs]
    assert (True, False) in r3 and (False, True) in r3
    assert {L.k % 4 for L in _lf(bd, "R3")} == {0, 1, 2, 3}
    assert {(s.offset // L.ps) % 4 for L in _lf(bd, "R3") if not L.k for s in L.segs} == {1, 2, 3}
    assert {L.ss % 4 for L in _lf(bd, "R4")} == {1, 2, 3}
    mixed = _lf(bd, "R2")[0]
    at = {i % 32 if i + 1 < len(mixed.segs) else "last" for i, s in enumerate(mixed.segs) if s.vertical}
    assert at == {0, 15, 31, "last"} or at == {0, 15, "last"}
    assert {(L.k + s.offset // L.ps - 4) % 4 for L in _lf(bd, "R6")[:1] for s in L.segs} == {1, 2, 3}      # p3's address
    # the ragged launches: every count with record 0 luma and chroma, through hgroup and through hevc_lf_lines
    counts = {(len(L.segs), L.segs[0].spec.chroma, M.kernel_route(L, 0) == "R1") for L in _lf(bd, "counts")}
    assert counts == {(n, c, h) for n in M.COUNTS for c in (0, 1) for h in (False, True)}


@pytest.mark.parametrize("group", M.LF_GROUPS)
@pytest.mark.parametrize("bd", M.DEPTHS)
def test_lf_layout(bd, group):
    for L in _lf(bd, group):
        n = len(L.segs)
        assert L.stride % L.ps == 0 and (L.k * L.ps) % L.ps == 0
        assert _disjoint((L.rows, L.ss), [L.tile(i) for i in range(n)]), L.name
        for i, s in enumerate(L.segs):
            (y0, y1, x0, x1), (ty0, ty1, tx0, tx1) = L.foot(i), L.tile(i)
            assert y0 - ty0 >= 8 and ty1 - y1 >= 8 and x0 - tx0 >= 8 and tx1 - x1 >= 8, (L.name, i)       # the guard
            # the whole dwords (8-byte words) that the wide and hgroup accesses touch lie in the footprint
            if M.kernel_route(L, i) in ("R1", "R5"):
                assert ((L.k + y0 * L.ss + x0) * L.ps) % (4 * L.ps) == 0, (L.name, i)
            assert 0 <= s.offset and s.offset == (s.y * L.ss + s.x) * L.ps
            assert L.k * L.ps + (y1 - 1) * L.stride + x1 * L.ps <= L.buf.size
            assert M.kernel_route(L, i) == s.route, (L.name, i, s.route, M.kernel_route(L, i))


CASES = [(bd, e, b) for bd in M.DEPTHS for e in (0, 1) for b in (0, 1)]


@pytest.mark.parametrize("bd,edge,bytewise", CASES)
def test_sao_model_is_the_oracle(bd, edge, bytewise):
    for L in _sao(bd, edge, bytewise):
        want = L.want_oracle()
        bad = L.first_bad(L.want_model(), want)
        assert bad is None, bad
        ins = L.inside()
        assert (want[ins] != L.dst0[ins]).mean() > .5 and np.array_equal(want[~ins], L.dst0[~ins])


@pytest.mark.parametrize("bd,edge,bytewise", CASES)
def test_sao_coverage_and_layout(bd, edge, bytewise):
    launches = _sao(bd, edge, bytewise)
    assert M.sao_missing(launches[:2], bd, edge, bytewise) == []
    assert [len(L.blocks) for L in launches[2:]] == M.SAO_COUNTS
    lo, hi = (-128, 127) if bd == 8 else (-128 << (bd - 8), 127 << (bd - 8))
    for L in launches:
        assert _disjoint(L.dst0.shape, L.dslot) and _disjoint(L.src.shape, L.sslot), L.name
        for i, b in enumerate(L.blocks):
            assert any(not lo <= v <= hi for v in b.off) == bool(bytewise), b
            (y, x), (y0, y1, x0, x1) = L.dpos[i], L.dslot[i]
            assert y - y0 >= 8 and x - x0 >= 8 and y1 - (y + b.h) >= 8 and x1 - (x + b.w) >= 8
            (y, x), (y0, y1, x0, x1) = L.spos[i], L.sslot[i]
            assert y - y0 >= 9 and x - x0 >= 9 and y1 - (y + b.h) >= 9 and x1 - (x + b.w) >= 9
            assert L.dst_offset(i) % 4 == b.dmod and L.src_offset(i) % 4 == b.smod and (bd == 8 or b.dmod != b.smod)
            assert 1 <= b.w <= 64 and 1 <= b.h <= 64


@pytest.mark.parametrize("bd", M.DEPTHS)
def test_restore_model_is_the_oracle(bd):
    O = ffi.oracle()
    rng = np.random.default_rng(bd)
    dt = np.uint8 if bd == 8 else np.uint16
    cases = M.restore_cases(bd)
    assert {(c[4], c[5]) for c in cases} == set(M.RESTORE_SIZES)
    changed = 0
    for case in cases:
        var, eo, off0, borders, w, h, ve, he, de = case
        src = rng.integers(0, 1 << bd, (h, w)).astype(dt)
        dst = rng.integers(0, 1 << bd, (h, w)).astype(dt)
        want = dst.copy()
        O.ffo_hevc_sao_edge_restore_bd(bd, var, ffi.ptr(want), ffi.ptr(src), w * dst.itemsize, w * dst.itemsize, eo, off0, ffi.ptr(borders, ffi.i32p),
                                       w, h, ffi.ptr(ve), ffi.ptr(he), ffi.ptr(de))
        assert np.array_equal(M.restore_model(dst, src, bd, case), want), case
        changed += int((want != dst).any())
    assert changed > 10
