"""The generator of tests/h264_lf_matrix.py, pinned without a GPU: its model gives every cell the label and the changed samples it was
built for and equals the oracle byte for byte over the whole buffer of every batch launch and every frame picture; every route holds
every cell of its classes, every hand-off class and every lane composition occurs; the route labels equal what the kernels' own
conditions and launch arithmetic give; every observable mutation of the model changes some cell on every route that runs the mutated
class; and the changes listed as unobservable change nothing."""
import numpy as np
import pytest

import h264_lf_matrix as M


def _disjoint(shape, rects):
    seen = np.zeros(shape, np.int32)
    for y0, y1, x0, x1 in rects:
        assert 0 <= y0 < y1 <= shape[0] and 0 <= x0 < x1 <= shape[1], (y0, y1, x0, x1, shape)
        seen[y0:y1, x0:x1] += 1
    return seen.max() <= 1


@pytest.mark.parametrize("bd", M.MEMBER_DEPTHS)
def test_cells_are_what_they_are_built_for(bd):
    """the model's label and changed samples per cell; the cells the matrix is made of are present"""
    maxv, F = (1 << bd) - 1, 1 << (bd - 8)
    names = set()
    for c in M.cells(bd):
        out, label, changed = M.lf_model(c.px, c.cls, c.alpha, c.beta, c.tc0, bd)
        assert label == c.label, (c.name, label)
        assert all(0 <= v <= maxv for v in out), c.name
        assert changed == c.changed == {k for k in range(8) if out[k] != c.px[k]}, (c.name, out, c.px)
        if c.cls & 1:
            assert not changed & {0, 1, 2, 5, 6, 7}, c.name                  # chroma: p0 and q0 alone
        assert not changed & {0, 7}, c.name
        if c.cls >= 2:                                                      # the tc0 bytes of a bS = 4 record must not matter
            assert all(M.lf_model(c.px, c.cls, c.alpha, c.beta, t, bd)[0] == out for t in M.INTRA_TC0), c.name
        names.add(c.name)
    assert {c.label for c in M.cells(bd)} == set(M.LABELS)
    for cls, labels in enumerate([{l for l in M.LABELS if l[0] == "n"}, {"none", "c"}, {"none", "weak", "s00", "s10", "s01", "s11"}, {"none", "ci"}]):
        assert {c.label for c in M.cells(bd) if c.cls == cls} == labels, cls
    for c in ("l", "c", "li", "ci"):
        for g in ("a", "bp", "bq"):
            assert {"%s_gate_%s_%s_%s" % (c, g, r, s) for r in ("pass", "fail") for s in ("pgt", "plt")} <= names
        assert {"%s_alpha255_inside" % c, "%s_beta0" % c, "%s_alpha0" % c} <= names
    assert {"l_tc0_%d" % t for t in (-128, -1, 0, 1, 25, 127)} | {"c_tc0_%d" % t for t in (-128, 0, 1, 2, 127)} <= names
    assert {"%s_sum_%d" % (c, s) for c in "lc" for s in (-12, -9, -8, -5, -4, -1, 0, 3, 4, 7, 8)} <= names
    assert {"%s_clip_%s" % (c, s) for c in "lc" for s in ("p0_hi", "p0_lo", "q0_hi", "q0_lo")} | {"l_only_p0", "l_only_q0", "c_only_p0", "c_only_q0"} <= names
    assert {"l_%s_%s_%s_%s%d" % (a, t, s, b, o) for a, b in (("ap", "aq"), ("aq", "ap")) for t in ("m1", "eq") for s in ("pgt", "plt") for o in (0, 1)} <= names
    assert {"l_delta_k%d_%s" % (k, t) for k in range(3) for t in ("below", "lo", "hi", "above")} <= names
    assert {"l_%scorr_%s" % (s, t) for s in ("p1", "q1") for t in ("below", "lo", "hi", "above")} <= names
    assert {"li_alpha%d_limit%s_%s" % (a, m, s) for a in (4, 5, 6, 7, 255) for m in ("", "_m1") for s in ("pgt", "plt")} <= names
    by = M.cell_by_name(bd)
    # what the named cells are built on, from their samples alone
    for k in range(3):
        tc = 3 * F + k
        assert [by["l_delta_k%d_%s" % (k, t)].px[4] - by["l_delta_k%d_%s" % (k, t)].px[3] for t in ("below", "lo", "hi", "above")] == \
               [2 * r for r in (-tc - 1, -tc, tc, tc + 1)]
    for c in "lc":
        for s in (-12, -9, -8, -5, -4, -1, 0, 3, 4, 7, 8):
            p3, p2, p1, p0, q0, q1, q2, q3 = by["%s_sum_%d" % (c, s)].px
            assert 4 * (q0 - p0) + (p1 - q1) + 4 == s
    for a in (4, 5, 6, 7, 255):
        limit = ((a << (bd - 8)) >> 2) + 2
        for s in ("pgt", "plt"):
            x, y = by["li_alpha%d_limit_m1_%s" % (a, s)], by["li_alpha%d_limit_%s" % (a, s)]
            assert abs(x.px[3] - x.px[4]) == limit - 1 and abs(y.px[3] - y.px[4]) == limit and (x.px[3] > x.px[4]) == (s == "pgt")
    for form, div in (("sp0", 8), ("sp1", 4), ("sp2", 8), ("sq0", 8), ("sq1", 4), ("sq2", 8), ("wp0", 4), ("wq0", 4)):
        for c in (("li", "ci") if form[0] == "w" else ("li",)):
            for side in ("zero", "max"):
                res = set()
                for r in range(div):
                    x = by["%s_%s_%s_r%d" % (c, form, side, r)]
                    s, sh, k = M._formulas(x.px)[form]
                    res.add(s % div)
                    assert (0 if side == "zero" else maxv) in x.px, x.name
                assert res == set(range(div)), (form, side)
    p = by["li_p3_q3_far"].px
    assert abs(p[0] - p[1]) >= 50 * F and abs(p[7] - p[6]) >= 50 * F
    # every record: one class, alpha and beta; the tc0 of a bS < 4 line is its cell's; bS = 4 records carry INTRA_TC0
    for cls in range(4):
        for inner in {2 if cls & 1 else 4} | {i for k, i in M.MEMBERS if (k >> 1 & 1) | (k >> 2 & 1) << 1 == cls}:
            recs = M.records(bd, cls, inner)
            assert {c.name for r in recs for c in r.cells} - {"fill"} == {c.name for c in M.cells(bd) if c.cls == cls}
            for r in recs:
                for n in range(4):
                    x = M.rot(r, n)
                    assert len(x.cells) == 4 * inner and sorted(c.name for c in x.cells) == sorted(c.name for c in r.cells)
                    for k, c in enumerate(x.cells):
                        assert c.name == "fill" or (c.cls, c.alpha, c.beta) == (cls, r.alpha, r.beta)
                        assert cls >= 2 or c.name == "fill" or x.tc0[k // inner] == c.tc0
                    assert cls < 2 or x.tc0 == M.INTRA_TC0
                assert {M.rot(r, n).cells.index(c) // inner for n in range(4) for c in r.cells[:1]} == {0, 1, 2, 3}      # every tc0 slot


@pytest.mark.parametrize("bd,group", [(bd, g) for bd in M.DEPTHS for g in M.BATCH_GROUPS] + [(bd, "members") for bd in M.MEMBER_DEPTHS])
def test_model_is_the_oracle_batch(bd, group):
    """over the whole buffer of every batch launch: ffo_h264_loop_filter at 8 bits, ffo_h264_loop_filter_bd at every depth; and per
    line the designed changes"""
    for L in (M.member_launches(bd) if group == "members" else M.batch_launches(bd, group)):
        want = L.want_oracle(plain=False)
        bad = L.first_bad(L.want_model(), want)
        assert bad is None, bad
        if bd == 8 and all(s.rec.inner == (2 if s.rec.cls & 1 else 4) for s in L.segs):
            assert np.array_equal(L.want_oracle(plain=True), want), L.name
        assert (want != L.buf).any()
        for i, s in enumerate(L.segs):
            a, b = L.lines(L.buf, i), L.lines(want, i)
            for line, c in enumerate(s.rec.cells):
                assert np.array_equal(a[line], c.px)
                if s.rec.cls >= 2 or c.name == "fill":
                    ch = M.lf_model(c.px, s.rec.cls, s.rec.alpha, s.rec.beta, 0, bd)[2]
                else:
                    ch = c.changed
                assert set(np.flatnonzero(a[line] != b[line]).tolist()) == set(ch), (L.name, i, line, c.name)


@pytest.mark.parametrize("bd", M.DEPTHS)
def test_batch_coverage_and_routes(bd):
    launches = [L for g in M.BATCH_GROUPS for L in M.batch_launches(bd, g)]
    for route in M.BATCH_ROUTES:
        pool = [L for L in launches if L.name.startswith("Bmix")] if route == "Bmix" else [L for L in launches if not L.name.startswith("counts")]
        assert M.batch_missing(pool, route) == [], route
    ps = 1 if bd == 8 else 2
    for L in launches + M.member_launches(bd):
        n = len(L.segs)
        assert n <= 400 and _disjoint((L.rows, L.ss), [L.tile(i) for i in range(n)]), L.name
        for i, s in enumerate(L.segs):
            (y0, y1, x0, x1), (ty0, ty1, tx0, tx1) = L.foot(i), L.tile(i)
            assert y0 - ty0 >= 8 and ty1 - y1 >= 8 and x0 - tx0 >= 8 and tx1 - x1 >= 8, (L.name, i)       # the guard
            assert s.offset == (s.y * L.ss + s.x) * ps and L.k * ps + (y1 - 1) * L.stride + x1 * ps <= L.buf.size
            assert M.kernel_route(L, i) == s.route, (L.name, i, s.route, M.kernel_route(L, i))
    # B2 through every residue, by the record's offset and by the base; B4: stride odd (8 bits), 4 n + 2 bytes (16 bits)
    b2 = M.batch_launches(bd, "B2")
    assert {(L.k * ps + s.offset) % 4 for L in b2 for s in L.segs} == ({1, 2, 3} if ps == 1 else {2})
    assert any(L.k and not s.offset % 4 for L in b2 for s in L.segs) and any(not L.k and s.offset % 4 for L in b2 for s in L.segs)
    assert all(L.stride % 4 == (1 if ps == 1 else 2) for L in M.batch_launches(bd, "B4"))
    # B1: lines that change p samples only, q samples only, p0 q0 only, all six (a dword path writes back whole dwords)
    b1 = {frozenset(c.changed) for L in M.batch_launches(bd, "B1") for s in L.segs for c in s.rec.cells}
    assert {frozenset({3}), frozenset({4}), frozenset({1, 2, 3}), frozenset({4, 5, 6}), frozenset({3, 4}), frozenset({1, 2, 3, 4, 5, 6})} <= b1
    # every workgroup of Bmix: all eight kinds
    for L in M.batch_launches(bd, "Bmix"):
        for w0 in range(0, len(L.segs) - 15, 16):
            assert {L.kind(i) for i in range(w0, w0 + 16)} == set(range(8)), (L.name, w0)
    assert [len(L.segs) for L in M.batch_launches(bd, "counts")] == M.COUNTS
    # the members: each of the 14, every cell of its class, both directions over the family
    mem = M.member_launches(bd)
    assert [(L.kind(0), L.segs[0].rec.inner) for L in mem] == M.MEMBERS
    for L in mem:
        cls = L.segs[0].rec.cls
        assert M.batch_missing([L], "any", [cls]) == [], L.name


def _frame_sets(bd, chroma):
    return list(M.frame_pics(bd, chroma)) + list(M.waves_pics(bd, chroma))


@pytest.mark.parametrize("chroma", [0, 1])
@pytest.mark.parametrize("bd", M.DEPTHS)
def test_frame_cell_pictures(bd, chroma):
    """the oracle's frame functions on the hand-written tables leave every line equal to the model's output of its cell and nothing
    else moves, at every stride padding the GPU tier uses; every (direction, k class) holds every cell of the plane's classes; the
    k == 0 horizontal route holds every hand-off class of every kernel; the waves pictures hold every composition"""
    pics = M.frame_pics(bd, chroma)
    assert len({(P.mb_w, P.mb_h) for P in pics}) == 1
    for P in _frame_sets(bd, chroma):
        assert P.before.shape[0] <= 544 and P.before.shape[1] <= 128
        live = {}
        for p in P.places:
            assert (p.mx, p.my) not in live and not (p.k == 0 and (p.my if p.dir else p.mx) == 0), (P.name, p)
            live[(p.mx, p.my)] = p
            assert (p.rec.cls >= 2) == (p.kind >= 4) and np.array_equal(P.lines(P.before, p), M.rec_lines(p.rec)), (P.name, p.mx, p.my)
            if not P.kind.startswith("waves"):
                assert (p.mx + p.my) % 2 == 0 and P.dk(p) == P.kind
        e = P.edges.reshape(P.mb_h, P.mb_w, 2, P.ne)
        for my in range(P.mb_h):                                             # every other record is dead
            for mx in range(P.mb_w):
                for d in range(2):
                    for k in range(P.ne):
                        p = live.get((mx, my))
                        if p is None or (p.dir, p.k) != (d, k):
                            assert e[my, mx, d, k]["alpha"] == 0 or e[my, mx, d, k]["beta"] == 0
        for pad in ((0, 3, 4, 16) if bd == 8 else (0, 8)):
            want = P.want_oracle(pad)
            bad = P.first_bad(P.want_model(pad), want, "the model")
            assert bad is None, bad
            assert (want != P.embed(pad)).sum() > 300, P.name
        if bd == 8:
            assert np.array_equal(P.want_oracle(0, plain=True), P.want_oracle(0, plain=False)), P.name
    for dk in M.FRAME_DK:
        assert M.frame_missing(pics, dk, pics[0].classes) == [], dk
        kinds = {p.kind for P in pics for p in P.places if P.dk(p) == dk}
        assert kinds == set(range(8)), (dk, kinds)                          # bits 0 / 1 of the kind byte in every state
    for kernel in M.KERNELS:
        if not (chroma and kernel == "row"):
            for nf in (1, 3):
                assert M.handoff_missing(pics, kernel, nf) == [], (kernel, nf)
    for P in M.waves_pics(bd, chroma):
        have = M.compositions(P)
        assert [c for c in M.COMPOSITIONS if c not in have] == [], P.name
        Q = 64 // P.MB
        for (band, s) in P.diags:                                            # whole diagonals inside the picture
            assert 0 <= s - (Q - 1) * M.DB_SKEW and s < P.mb_w and (band + 1) * Q <= P.mb_h
    X = M.mixed_pic(bd, chroma)
    e = X.edges
    assert {int(k) for k in e["kind"]} == set(range(8)) and (e["alpha"] == 0).any() and (e["beta"] == 0).any()
    want = X.want_oracle(0)
    assert (want != X.before).sum() > 1000
    first = X.edges.reshape(X.mb_h, X.mb_w, 2, X.ne)
    assert (first[:, 0, 0, 0]["alpha"] != 0).any() and (first[0, :, 1, 0]["alpha"] != 0).any()          # live records on the picture edges


@pytest.mark.parametrize("bd", [8, 10])
def test_c422_cell_pictures(bd):
    """the object route of 4:2:2 chroma: ffo_h264_deblock_frame_c422_bd leaves every line equal to the model's output of its cell; every
    chroma cell on each (direction, k class) of each plane; vertical edges of 16 lines with tc0 per 4, horizontal ones at y = 4, 8, 12
    as well; every row of the k == 0 horizontal picture is handed off (a workgroup per macroblock row)"""
    for plane in (1, 2):
        pics = M.c422_pics(bd, plane)
        for P in pics[:-1]:
            for pad in (0, 8):
                want = P.want_oracle(pad)
                bad = P.first_bad(P.want_model(pad), want, "the model")
                assert bad is None, bad
                assert (want != P.embed(pad)).sum() > 100
            assert all((len(p.rec.cells), p.rec.inner) == ((8, 2) if p.dir else (16, 4)) and (p.mx + p.my) % 2 == 0 for p in P.places)
        for dk in M.FRAME_DK:
            assert M.frame_missing(pics[:-1], dk, (1, 3)) == [], dk
        assert {p.k for P in pics for p in P.places if p.dir == 1} == {0, 1, 2, 3} and {p.k for P in pics for p in P.places if p.dir == 0} == {0, 1}
        assert {p.my for P in pics for p in P.places if p.dir == 1 and p.k == 0} == set(range(1, pics[0].mb_h))
        X = pics[-1]
        assert (X.want_oracle(0) != X.before).sum() > 300 and {int(k) for k in X.edges["kind"]} == set(range(8))
    assert [P.name for P in M.c422_pics(bd, 1)] == [P.name for P in M.c422_pics(bd, 2)]
    assert not np.array_equal(M.c422_pics(bd, 1)[0].before, M.c422_pics(bd, 2)[0].before)


@pytest.mark.parametrize("bd", [8, 10])
def test_mbaff_calls(bd):
    """the MBAFF object route: one call per live pair and plane, inside its pair's tile as mbaff_place_call() demands, footprints
    disjoint; the oracle call by call leaves every line equal to the model's output of its cell; every cell of the plane's classes on
    the ordinary members and on the _mbaff members; both at the frame's and at twice the line size; row and column edges"""
    P = M.mbaff_pic(bd)
    assert all(P.in_tile(c) for c in P.calls)
    for plane in range(3):
        cs = [c for c in P.calls if c.plane == plane]
        seen = np.zeros(P.before[plane].shape, np.int32)
        for c in cs:
            assert (c.mb_x + c.mb_y // 2) % 2 == 0 and np.array_equal(P._rect(P.before[plane], c), M.rec_lines(c.rec))
            P._rect(seen, c)[:] += 1
        assert seen.max() == 1 and len({(c.mb_x, c.mb_y // 2) for c in cs}) == len(cs)
        classes = (1, 3) if plane else (0, 2)
        want = {x.name for x in M.cells(bd) if x.cls in classes}
        for half in (0, M.CALL_MBAFF):
            assert {x.name for c in cs if c.flags & M.CALL_MBAFF == half for x in c.rec.cells} - {"fill"} == want, (plane, half)
            assert {len(c.rec.cells) for c in cs if c.flags & M.CALL_MBAFF == half} == {(8 if plane else 16) >> (half > 0)}
        assert {(c.col, c.flags) for c in cs} == {(1, 0), (1, 1), (1, 2), (1, 3), (0, 0), (0, 1)}, plane
        assert any(c.col and c.x == (8 if plane else 16) * c.mb_x for c in cs)                        # k = 0: into the pair on the left
    for pad in (0, 8):
        want, model = P.want_oracle(pad), P.want_model(pad)
        bad = P.first_bad(model, want)
        assert bad is None, bad
        assert all((w != a).sum() > 100 for w, a in zip(want, P.embed(pad)))


def test_frame_kernel_choice():
    """frame_kernel() and handoff_class() restate deblock_frames(): the strides the GPU tier uses reach the kernels they are meant for"""
    K = M.frame_kernel
    for chroma, w in ((0, 128), (1, 64)):
        assert K(8, chroma, 0, w, w * 8) == K(8, chroma, 0, w + 16, (w + 16) * 8) == "skew"
        assert K(8, chroma, 0, w + 4, (w + 4) * 8) == "band"
        assert K(8, chroma, 0, w, w * 8, old=2) == "band"
        assert K(10, chroma, 0, 2 * w, 2 * w * 8) == K(14, chroma, 0, 2 * w + 16, 16 * w) == "skew"
        assert K(10, chroma, 0, 2 * w + 8, 16 * w) is None
    assert K(8, 0, 0, 131, 131 * 8) == K(8, 0, 0, 128, 1024, old=1) == "row"
    assert K(8, 1, 0, 67, 67 * 8) is None and K(8, 1, 0, 64, 512, old=1) == "band"
    assert K(8, 0, 0, 128, 1024, edges_addr=4) == "band"
    H = M.handoff_class
    assert [H("skew", 8, 0, y) for y in (1, 3, 4, 12, 16, 32)] == ["same wave"] * 2 + ["other wave"] * 2 + ["other workgroup"] * 2
    assert [H("skew", 10, 0, y) for y in (3, 4, 8, 12, 24)] == ["same wave", "other wave", "other wave", "other workgroup", "other workgroup"]
    assert [H("skew", 14, 1, y) for y in (7, 8, 24, 32, 64)] == ["same wave", "other wave", "other wave", "other workgroup", "other workgroup"]
    assert [H("band", 8, 0, y, 3, 34) for y in (1, 4, 5, 8)] == ["inside the band", "across bands"] * 2
    assert H("band", 8, 0, 4, 64, 34) == "inside the band" and H("row", 8, 0, 9) == "every row"


def _routes(bd):
    """route -> the (cell, tc0, kind) triples its lines hold"""
    launches = [L for g in M.BATCH_GROUPS if g != "counts" for L in M.batch_launches(bd, g)]
    routes = {}
    for route in M.BATCH_ROUTES:
        routes[route] = M.batch_triples([L for L in launches if L.name.startswith("Bmix")] if route == "Bmix" else launches, route)
    for L in M.member_launches(bd):
        routes[L.name] = M.batch_triples([L], "any")
    for chroma in (0, 1):
        for dk in M.FRAME_DK:
            routes["frame/%s/%s" % ("chroma" if chroma else "luma", dk)] = {t for P in M.frame_pics(bd, chroma) for t in P.triples(dk)}
    return routes


@pytest.mark.parametrize("bd", M.MEMBER_DEPTHS)
def test_mutations_change_a_cell_on_every_route(bd):
    """every one-decision change of the model shows on every route that runs the class it changes: a kernel wrong there would fail.
    The depth mistakes are the rule itself at 8 bits and are required above.  `kind4only` needs a record of kind 5, 6 or 7: the
    batch row routes of luma (kind 4 alone) cannot show it."""
    if bd in M.DEPTHS:
        routes = _routes(bd)
        assert set(routes) == set(M.BATCH_ROUTES) | {L.name for L in M.member_launches(bd)} | \
            {"frame/%s/%s" % (c, dk) for c in ("luma", "chroma") for dk in M.FRAME_DK}
    else:
        routes = {L.name: M.batch_triples([L], "any") for L in M.member_launches(bd)}
    by = M.cell_by_name(bd)
    assert len(set(M.MUTATIONS)) == len(M.MUTATIONS) >= 70 and not set(M.MUTATIONS) & set(M.UNOBSERVABLE)
    checked = 0
    for mut in M.MUTATIONS:
        if bd == 8 and mut in M.DEPTH_MUTATIONS:
            for route, triples in routes.items():
                assert not any(M.mutation_caught(bd, triples, mut, cls) for cls in range(4)), (mut, route)
            continue
        for route, triples in routes.items():
            for cls in M.MUT_CLASSES[mut]:
                mine = [t for t in triples if by[t[0]].cls == cls]
                if not mine or (mut == "kind4only" and not any(t[2] in (5, 6, 7) for t in mine)):
                    continue
                assert M.mutation_caught(bd, triples, mut, cls), (mut, route, M.CLASSES[cls])
                checked += 1
    assert checked > 400


@pytest.mark.parametrize("bd", M.MEMBER_DEPTHS)
def test_unobservable_changes(bd):
    """the `if (tc_orig)` guard of the p1 / q1 corrections and chroma's `tc <= 0` against `tc < 0` cannot show in any output: over every
    cell in every tc0 slot, and by the arithmetic itself - which is why db_edge may drop the guard"""
    sh = bd - 8
    for mut in M.UNOBSERVABLE:
        for c in M.cells(bd):
            for t in {c.tc0, 0, 1, -1, 127, -128}:
                assert M.lf_model(c.px, c.cls, c.alpha, c.beta, t, bd)[0] == M.lf_model(c.px, c.cls, c.alpha, c.beta, t, bd, mut)[0], (mut, c.name, t)
    clip3 = lambda v, lo, hi: lo if v < lo else hi if v > hi else v
    assert all(clip3(x, -0, 0) == 0 for x in range(-300, 300))                                   # the guarded store adds 0
    assert [t for t in range(-128, 128) if ((t - 1) << sh) + 1 == 0] == ([0] if sh == 0 else [])   # chroma tc == 0: 8 bits, tc0 == 0 alone
