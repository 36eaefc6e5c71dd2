"""The generator of tests/vp9_lf_matrix.py, pinned without a GPU: its model equals the oracle byte for byte on every cell at every
depth and in both directions and gives every cell the label and the changed samples it was built for; every (route, cell) pair and
every wave composition occurs; the route labels equal what the kernel's own condition gives for the addresses; every mutation of the
model changes some cell's output on every route; and in the frame cell pictures every line comes out as the model's output of its
cell, so the lines are independent."""
import numpy as np
import pytest

import vp9_lf_matrix as M


def _disjoint(shape, rects):
    seen = np.zeros(shape, np.int32)
    for y0, y1, x0, x1 in rects:
        assert 0 <= y0 < y1 <= shape[0] and 0 <= x0 < x1 <= shape[1], (y0, y1, x0, x1, shape)
        seen[y0:y1, x0:x1] += 1
    return seen.max() <= 1


@pytest.mark.parametrize("bd", M.DEPTHS)
def test_cells_are_what_they_are_built_for(bd):
    """the model's label and changed samples per cell; the cells the issue names are present"""
    maxv = (1 << bd) - 1
    names = set()
    for c in M.cells(bd):
        out, label = M.lf_model(c.px, c.wd, c.E, c.I, c.H, bd)
        assert label == c.label, (c.name, label)
        assert all(0 <= v <= maxv for v in out), c.name
        assert {k for k in range(16) if out[k] != c.px[k]} == set(c.changed), (c.name, out, c.px)
        names.add(c.name)
    assert {c.label for c in M.cells(bd)} == set(M.LABELS)
    spans = {(min(c.changed), max(c.changed)) for c in M.cells(bd) if c.changed}
    assert spans >= {(7, 8), (6, 9), (5, 10), (1, 14)}
    for t in M.I_TESTS:
        assert {"fm_%s_eq" % t, "fm_%s_plus1" % t} <= names
    for t in M.F8_TESTS:
        assert {"f8_w%d_%s_%s" % (w, t, e) for w in (8, 16) for e in ("eq", "plus1")} <= names
    for t in M.F16_TESTS:
        assert {"f16_%s_eq" % t, "f16_%s_plus1" % t} <= names
    # the window sums the rounding cells were built for
    for c in M.cells(bd):
        if c.name.startswith("round_"):
            wide = c.wd == 16
            s = sum(a * b for a, b in zip(M._weights(wide)[7], c.px))
            assert s % (16 if wide else 8) == int(c.name.rsplit("_", 1)[1]), c.name
            assert (0 in c.px[:8]) == ("_zero_" in c.name) and (maxv in c.px[8:]) == ("_max_" in c.name), c.name


@pytest.mark.parametrize("group", M.BATCH_GROUPS)
@pytest.mark.parametrize("bd", M.DEPTHS)
def test_model_is_the_oracle(bd, group):
    """over the whole buffer of every batch launch: both directions, every residue; and per line the designed changes"""
    for L in M.batch_launches(bd, group):
        want = L.want_oracle()
        bad = L.first_bad(L.want_model(), want)
        assert bad is None, bad
        for i, s in enumerate(L.segs):
            a, b = L.lines(L.buf, i), L.lines(want, i)
            for line, c in enumerate(s.rec.cells):
                assert set(np.flatnonzero(a[line] != b[line]).tolist()) == set(c.changed), (L.name, i, line, c.name)


@pytest.mark.parametrize("bd", M.DEPTHS)
def test_batch_coverage_and_routes(bd):
    launches = [L for g in M.BATCH_GROUPS for L in M.batch_launches(bd, g)]
    for route in M.BATCH_ROUTES:
        pool = [L for L in launches if L.name.startswith("Rmix")] if route == "Rmix" else [L for L in launches if not L.name.startswith("counts")]
        assert M.missing(pool, route) == [], route
    ps = 1 if bd == 8 else 2
    for L in launches:
        n = len(L.segs)
        assert _disjoint((L.rows, L.ss), [L.tile(i) for i in range(n)]), L.name
        for i, s in enumerate(L.segs):
            (y0, y1, x0, x1), (ty0, ty1, tx0, tx1) = L.foot(i), L.tile(i)
            assert y0 - ty0 >= 8 and ty1 - y1 >= 8 and x0 - tx0 >= 8 and tx1 - x1 >= 8, (L.name, i)       # the guard
            assert s.offset == (s.y * L.ss + s.x) * ps and L.k * ps + (y1 - 1) * L.stride + x1 * ps <= L.buf.size
            assert M.kernel_route(L, i) == s.route, (L.name, i, s.route, M.kernel_route(L, i))
    # R2 through every residue, by the record's offset and by the base; R4: stride odd (8 bits), 4 n + 2 bytes (16 bits)
    r2 = M.batch_launches(bd, "R2")
    assert {(L.k * ps + s.offset) % 4 for L in r2 for s in L.segs} == ({1, 2, 3} if ps == 1 else {2})
    assert any(L.k and not s.offset % 4 for L in r2 for s in L.segs) and any(not L.k and s.offset % 4 for L in r2 for s in L.segs)
    assert all(L.stride % 4 == (1 if ps == 1 else 2) for L in M.batch_launches(bd, "R4"))
    # every wave of Rmix: both directions, the three widths, both column paths
    for L in M.batch_launches(bd, "Rmix"):
        for w0 in range(0, len(L.segs) - 7, 8):
            wave = L.segs[w0:w0 + 8]
            assert {s.dir for s in wave} == {0, 1} and {s.rec.wd for s in wave} == {4, 8, 16}, (L.name, w0)
            assert {s.route for s in wave} == {"R1", "R2", "R3"}, (L.name, w0)
    assert [len(L.segs) for L in M.batch_launches(bd, "counts")] == M.COUNTS


@pytest.mark.parametrize("fmt", list(M.FORMATS))
@pytest.mark.parametrize("bd", M.DEPTHS)
def test_frame_cell_pictures(bd, fmt):
    """run_tables / run_ctables on the hand-written tables leave every line equal to the model's output of its cell; nothing else
    moves; no entry reaches out of the picture; every frame route holds every cell and the waves every composition"""
    pics = M.frame_pics(bd, fmt)
    dt = np.uint8 if bd == 8 else np.uint16
    for P in pics:
        want = P.want_oracle()
        model = [b.copy() for b in P.before]
        for pl in P.places:
            a = P.before[pl.plane]
            y0, y1, x0, x1 = (pl.y - 8, pl.y + 8, pl.x, pl.x + 8) if pl.d else (pl.y, pl.y + 8, pl.x - 8, pl.x + 8)
            assert 0 <= y0 and 0 <= x0 and y1 <= a.shape[0] and x1 <= 8 * P.cols >> (P.ss[0] if pl.plane else 0), (P.name, pl)
            lines = P.lines(P.before, pl)
            assert np.array_equal(lines, M.rec_lines(pl.rec)), (P.name, pl.plane, pl.y, pl.x)
            if pl.valid:
                M.BatchLaunch._put(model[pl.plane], pl.d, pl.y, pl.x, M.rec_model(pl.rec, bd).astype(dt))
        for k in range(3):
            assert np.array_equal(want[k], model[k]), (P.name, k, np.argwhere(want[k] != model[k])[:4])
    for route in M.FRAME_ROUTES:
        if route.startswith(fmt):
            assert M.missing(pics, route) == [], route
    for d in (0, 1):
        assert M.compositions_missing(pics, d) == [], d
    assert any(P.sbc == 3 for P in pics)
    # the mixed picture: both directions, entries 8 apart, entries on position 0 of an inner superblock; it moves samples
    X = M.mixed_pic(bd, fmt)
    assert {pl.d for pl in X.places} == {0, 1}
    along = sorted({(pl.plane, pl.d, pl.y, pl.x) for pl in X.places})
    assert any(b[:2] == a[:2] and (b[2] - a[2], b[3] - a[3]) in ((0, 8), (8, 0)) for a in along for b in along)
    assert any(pl.d == 0 and pl.x % 64 == 0 for pl in X.places if pl.plane == 0) and any(pl.d == 1 and pl.y % 64 == 0 for pl in X.places if pl.plane == 0)
    assert sum(int((a != b).sum()) for a, b in zip(X.want_oracle(), X.before)) > 1000


@pytest.mark.parametrize("bd", M.DEPTHS)
def test_mutations_change_a_cell_on_every_route(bd):
    """every one-decision change of the model shows on every batch route and every frame route: a kernel wrong there would fail"""
    launches = [L for g in M.BATCH_GROUPS if g != "counts" for L in M.batch_launches(bd, g)]
    routes = {}
    for route in M.BATCH_ROUTES:
        pool = [L for L in launches if L.name.startswith("Rmix")] if route == "Rmix" else launches
        routes[route] = {c.name for L in pool for i, s in enumerate(L.segs) for line, c in enumerate(s.rec.cells)
                         if route == "Rmix" or M.line_route(L, i, line) == route}
    for fmt in M.FORMATS:
        for P in M.frame_pics(bd, fmt):
            for pl in P.places:
                if pl.valid:
                    routes.setdefault(P.route(pl), set()).update(c.name for c in pl.rec.cells)
    assert set(routes) == set(M.BATCH_ROUTES) | set(M.FRAME_ROUTES)
    assert len(set(M.MUTATIONS)) == len(M.MUTATIONS) >= 60
    for mut in M.MUTATIONS:
        assert M.mutation_caught(bd, {c.name for c in M.cells(bd)}, mut), mut
        for route, names in routes.items():
            assert M.mutation_caught(bd, names, mut), (mut, route)
