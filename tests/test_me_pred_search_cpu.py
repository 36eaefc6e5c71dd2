"""CPU tier of the filter's predictive motion searches, EPZS and UMH (ffhip_me_search_pred_frames_host / ffhip_me_search_pred_batch_dev):
the host face runs kernels/me_search_pred_rules.h — the code the kernel runs — on the CPU in raster order, and must equal
tests/me_pred_search_model.py, the model written from the rules text of include/ffhip.h, in vectors, costs and cost counts, for both
methods, both metrics and both block sizes; the model's counters show that the inputs reach every branch of the rules.  No device is
needed.  tests/test_gpu_me_pred_search.py takes its inputs and references from here."""
import ctypes as C
import collections
import functools

import numpy as np
import pytest

import ffi
import me_pred_search_model as M
from test_me_search_cpu import GUARD, NG, Guarded  # noqa: F401

EINVAL, ENOSYS = -22, -38

#: (w, h, pad, mb, R) of the issue: one column, one row, two columns, R = 0, R = 1, a window larger than the picture, R = 9 (two rings)
SHAPES = [(64, 48, 0, 16, 7), (52, 36, 1, 16, 5), (16, 64, 0, 16, 7), (40, 8, 0, 8, 3), (32, 48, 0, 16, 4), (72, 56, 0, 16, 0),
          (64, 64, 0, 8, 1), (96, 80, 3, 16, 32), (64, 48, 0, 8, 9)]
#: every shape at both block sizes where the other size leaves a block (its own first)
CASES = [(w, h, pad, m, R) for (w, h, pad, mb, R) in SHAPES for m in (mb, 24 - mb) if w >= m and h >= m]
METHODS = [M.EPZS, M.UMH]
KINDS = [M.SAD, M.SATD]
NF = 3              # independent pairs per call


def _lib():
    from ffmpeg_amd import _lib
    return _lib.lib()


def texture(rng, h, w):
    """noise smoothed by two 5 x 5 box filters, stretched to 0..255: a slope for a pattern search to follow"""
    a = rng.random((h + 8, w + 8))
    for _ in range(2):
        a = sum(a[dy:dy + a.shape[0] - 4, dx:dx + a.shape[1] - 4] for dy in range(5) for dx in range(5))
    a = (a - a.min()) / (a.max() - a.min()) * 255.0
    return a[:h, :w]


def _window(bx, by, w, h, mb, R):
    bw, bh = w // mb, h // mb
    return max(0, bx * mb - R), min(bx * mb + R, (bw - 1) * mb), max(0, by * mb - R), min(by * mb + R, (bh - 1) * mb)


@functools.lru_cache(maxsize=None)
def pairs(w, h, pad, mb, R):
    """three independent frame pairs.  0: every block of the current frame is a block of the (rough) reference at a position of its
    own inside its window — now and then its left, top, top-right or top-left neighbour's vector, or none — so that no neighbour
    helps unless made to; 1: a smooth texture moved by one vector, plus noise of +-2, and blocks that match exactly where they are;
    2: flat with sparse marks (ties everywhere).  -> cur, ref (3, h, stride) uint8 and pair 0's vectors (b_h, b_w, 2), read-only"""
    rng = np.random.default_rng(ffi.stable_seed("me_pred_search", w, h, pad, mb, R))
    stride, m = w + pad, 40
    bw, bh = w // mb, h // mb
    cur, ref = np.zeros((NF, h, stride), np.uint8), np.zeros((NF, h, stride), np.uint8)
    ref[0, :, :w] = np.round(0.5 * texture(rng, h, w) + 0.5 * rng.integers(0, 256, (h, w)))
    cur[0, :, :w] = rng.integers(0, 256, (h, w))
    vecs = np.zeros((bh, bw, 2), np.int64)
    for by in range(bh):
        for bx in range(bw):
            x0, x1, y0, y1 = _window(bx, by, w, h, mb, min(R, 6))
            v = (int(rng.integers(x0, x1 + 1)) - bx * mb, int(rng.integers(y0, y1 + 1)) - by * mb)
            copy = int(rng.integers(0, 8))      # 0..3: the vector of the left, top, top-right, top-left neighbour; 4: none; else its own
            nx, ny = [(bx - 1, by), (bx, by - 1), (bx + 1, by - 1), (bx - 1, by - 1)][copy] if copy < 4 else (bx, by)
            if copy < 4 and 0 <= nx < bw and 0 <= ny < bh:
                v = tuple(vecs[ny, nx])
            if copy == 4:
                v = (0, 0)
            x, y = bx * mb + v[0], by * mb + v[1]
            if not (x0 <= x <= x1 and y0 <= y <= y1):
                x, y, v = bx * mb, by * mb, (0, 0)
            vecs[by, bx] = v
            cur[0, by * mb:(by + 1) * mb, bx * mb:(bx + 1) * mb] = ref[0, y:y + mb, x:x + mb]
    big = texture(rng, h + 2 * m, w + 2 * m)
    s = max(1, min(R, 6))
    dx, dy = (int(v) for v in rng.integers(-s, s + 1, 2))
    ref[1, :, :w] = np.round(big[m:m + h, m:m + w])
    cur[1, :, :w] = np.clip(np.round(big[m + dy:m + dy + h, m + dx:m + dx + w] + rng.integers(-2, 3, (h, w))), 0, 255)
    cur[1, :min(h, 2 * mb), :min(w, 2 * mb)] = ref[1, :min(h, 2 * mb), :min(w, 2 * mb)]
    ref[2, :, :w] = 128
    ref[2, ::5, :w:7] = 130
    cur[2, :, :w] = 128
    cur[2, 1::5, 2:w:7] = 130
    for a in (cur, ref, vecs):
        a.setflags(write=False)
    return cur, ref, vecs


@functools.lru_cache(maxsize=None)
def prev_fields(w, h, pad, mb, R, what):
    """fields of the two previous pairs.  "made", by hand: pair 0's fields hand each block its real vector through one list entry chosen
    per block — the collocated block of prev1, the accelerator (rel1 = v + e, rel2 = v + 2e), prev1's left, top, right or bottom
    neighbour — or through none; what no block claimed holds small, window-sized or far-away vectors.  The other pairs' hold small
    vectors.  "noise": any int16; "none": NULL, NULL.  -> prev1, prev2 (3, b_h * b_w * 2) int16, or None"""
    if what == "none":
        return None, None
    rng = np.random.default_rng(ffi.stable_seed("me_pred_prev", w, h, pad, mb, R, what))
    bw, bh = w // mb, h // mb
    if what == "noise":
        out = [rng.integers(-32768, 32768, (NF, bh * bw * 2)).astype(np.int16) for _ in range(2)]
    else:
        vecs = pairs(w, h, pad, mb, R)[2]
        rel = np.zeros((2, NF, bh, bw, 2), np.int64)
        for k in range(2):
            for n in range(NF):
                for by in range(bh):
                    for bx in range(bw):
                        mode = int(rng.integers(0, 4))
                        lim = [3, R + 1, 3000, 0][mode]
                        rel[k, n, by, bx] = rng.integers(-lim, lim + 1, 2)
        claimed = np.zeros((bh, bw), bool)
        for by in range(bh):
            for bx in range(bw):
                slot = int(rng.integers(0, 8))
                v = vecs[by, bx]
                if slot == 0 and not claimed[by, bx]:
                    rel[0, 0, by, bx] = v
                    claimed[by, bx] = True
                elif slot == 1 and not claimed[by, bx]:
                    e = rng.integers(-3, 4, 2)
                    rel[0, 0, by, bx], rel[1, 0, by, bx] = v + e, v + 2 * e
                    claimed[by, bx] = True
                elif 2 <= slot < 6:
                    nx, ny = [(bx - 1, by), (bx, by - 1), (bx + 1, by), (bx, by + 1)][slot - 2]
                    if 0 <= nx < bw and 0 <= ny < bh and not claimed[ny, nx]:
                        rel[0, 0, ny, nx] = v
                        claimed[ny, nx] = True
        origin = np.array([[(bx * mb, by * mb) for bx in range(bw)] for by in range(bh)], np.int64)
        out = [np.clip(rel[k] + origin, -32768, 32767).astype(np.int16).reshape(NF, bh * bw * 2) for k in range(2)]
    for a in out:
        a.setflags(write=False)
    return out[0], out[1]


@functools.lru_cache(maxsize=None)
def reference(method, kind, w, h, pad, mb, R, what="made"):
    """the model's vectors and costs of pairs(...) with prev_fields(..., what), computed once, with the branch counters that run added:
    (mv, cost, ncosts, Counter)"""
    cur, ref, _ = pairs(w, h, pad, mb, R)
    p1, p2 = prev_fields(w, h, pad, mb, R, what)
    before = collections.Counter(M.COUNTS)
    mv, cost, n = M.frames(method, cur, ref, w, h, mb, R, kind, p1, p2)
    took = collections.Counter(M.COUNTS)
    took.subtract(before)
    mv.setflags(write=False)
    cost.setflags(write=False)
    return mv, cost, n, took


def host_face(method, kind, cur, ref, w, h, mb, R, prev1, prev2):
    """ffhip_me_search_pred_frames_host on guarded copies -> mv, cost, (blocks, costs); asserts that nothing outside the outputs changed"""
    nf, _, stride = cur.shape
    bw, bh = w // mb, h // mb
    gc, gr = Guarded(cur), Guarded(ref)
    g1, g2 = (None if p is None else Guarded(p) for p in (prev1, prev2))
    gm, gk = Guarded(np.full((nf, bh * bw * 2), 0x5A5A, np.int16)), Guarded(np.full((nf, bh * bw), 0x5A5A5A5A, np.uint32))
    L = _lib()
    rc = L.ffhip_me_search_pred_frames_host(method, gc.addr, gr.addr, w, h, stride, h * stride, nf, mb, R, kind, g1 and g1.addr, g2 and g2.addr,
                                            gm.addr, gk.addr)
    assert rc == 0, (rc, L.ffhip_last_error())
    assert gc.unchanged() and gr.unchanged() and gm.guards_intact() and gk.guards_intact()
    assert (g1 is None or g1.unchanged()) and (g2 is None or g2.unchanged())
    blocks, costs = C.c_uint64(), C.c_uint64()
    L.ffhip_me_search_host_counts(C.byref(blocks), C.byref(costs))
    return gm.body().copy(), gk.body().copy(), (blocks.value, costs.value)


def _check(method, kind, case, what):
    w, h, pad, mb, R = case
    cur, ref, _ = pairs(*case)
    p1, p2 = prev_fields(*case, what)
    wmv, wcost, wn, _ = reference(method, kind, *case, what)
    mv, cost, (blocks, costs) = host_face(method, kind, cur, ref, w, h, mb, R, p1, p2)
    assert np.array_equal(cost, wcost)
    assert np.array_equal(mv, wmv)
    assert blocks == NF * (w // mb) * (h // mb) and costs == wn     # the rules header evaluates what the text says, no more


@pytest.mark.parametrize("kind", KINDS, ids=["sad", "satd"])
@pytest.mark.parametrize("method", METHODS, ids=[M.NAMES[m] for m in METHODS])
@pytest.mark.parametrize("w,h,pad,mb,R", CASES)
def test_host_face_equals_the_model(w, h, pad, mb, R, method, kind):
    _check(method, kind, (w, h, pad, mb, R), "made")


#: the shapes the other prev fields run on: several rows and columns, one column, the large window
PREV_CASES = [CASES[0], (16, 64, 0, 16, 7), (96, 80, 3, 16, 32)]


@pytest.mark.parametrize("what", ["none", "noise"])
@pytest.mark.parametrize("method", METHODS, ids=[M.NAMES[m] for m in METHODS])
@pytest.mark.parametrize("w,h,pad,mb,R", PREV_CASES)
def test_null_and_arbitrary_prev_fields(w, h, pad, mb, R, method, what):
    """NULL is a field of zero vectors; any int16 content is legal (relative vectors in 32 bits, refused outside the window)"""
    _check(method, M.SAD, (w, h, pad, mb, R), what)


def test_one_null_field_is_a_zero_field():
    """each of prev1, prev2 alone NULL == that field holding every block's origin"""
    case = CASES[0]
    w, h, pad, mb, R = case
    cur, ref, _ = pairs(*case)
    p1, p2 = prev_fields(*case, "made")
    bw, bh = w // mb, h // mb
    origins = np.tile(np.array([[(bx * mb, by * mb) for bx in range(bw)] for by in range(bh)], np.int16).reshape(-1), (NF, 1))
    for a, b, za, zb in ((None, p2, origins, p2), (p1, None, p1, origins)):
        got = host_face(M.EPZS, M.SAD, cur, ref, w, h, mb, R, a, b)
        want = host_face(M.EPZS, M.SAD, cur, ref, w, h, mb, R, za, zb)
        assert all(np.array_equal(x, y) for x, y in zip(got[:2], want[:2])) and got[2] == want[2]


@functools.lru_cache(maxsize=None)
def chain():
    """five pictures of one sequence (a texture that drifts by a changing vector), 64 x 48, and the model's run over its four pairs:
    prev NULL at first, then the run's own earlier outputs.  -> pictures (5, 48, 64), [(mv, cost, ncosts)] per pair and method"""
    rng = np.random.default_rng(ffi.stable_seed("me_pred_chain"))
    big = texture(rng, 48 + 80, 64 + 80)
    pos, pics = (40, 40), []
    for k, (dx, dy) in enumerate([(0, 0), (2, 1), (3, 1), (3, -2), (-1, -3)]):
        pos = (pos[0] + dx, pos[1] + dy)
        pics.append(np.clip(np.round(big[pos[1]:pos[1] + 48, pos[0]:pos[0] + 64] + rng.integers(-1, 2, (48, 64))), 0, 255).astype(np.uint8))
    pics = np.stack(pics)
    pics.setflags(write=False)
    want = {}
    for method in METHODS:
        outs = []
        for k in range(4):
            p1 = outs[k - 1][0] if k >= 1 else None
            p2 = outs[k - 2][0] if k >= 2 else None
            outs.append(M.frames(method, pics[k + 1:k + 2], pics[k:k + 1], 64, 48, 16, 7, M.SAD, p1, p2))
        want[method] = outs
    return pics, want


@pytest.mark.parametrize("method", METHODS, ids=[M.NAMES[m] for m in METHODS])
def test_chained_run_of_four_frames(method):
    pics, want = chain()
    outs = []
    for k in range(4):
        p1 = outs[k - 1][0] if k >= 1 else None
        p2 = outs[k - 2][0] if k >= 2 else None
        outs.append(host_face(method, M.SAD, pics[k + 1:k + 2], pics[k:k + 1], 64, 48, 16, 7, p1, p2))
        wmv, wcost, wn = want[method][k]
        assert np.array_equal(outs[k][0], wmv) and np.array_equal(outs[k][1], wcost) and outs[k][2] == (12, wn), k


def test_the_inputs_reach_every_branch():
    """every counter of the model is non-zero over the inputs of the tests above"""
    total = collections.Counter()
    for case in CASES:
        for method in METHODS:
            for kind in KINDS:
                total.update(reference(method, kind, *case)[3])
    for case in PREV_CASES:
        for method in METHODS:
            for what in ("none", "noise"):
                total.update(reference(method, M.SAD, *case, what)[3])
    assert not [b for b in M.BRANCHES if total[b] <= 0], total


# ---- hand-made cases ------------------------------------------------------------------------------------------------------------------
def _bowl(target, method, prev1=None, prev2=None, R=7, size=64, at=(2, 2), mb=16):
    """size x size; the block `at` holds what the reference holds at its origin + target, every other block what the reference holds
    where it is (cost 0 at the origin).  -> (mv - origin, cost) of that block by host face and model (equal), the counters of the
    model's run of that block, the costs the host face evaluated over the picture"""
    yy, xx = np.mgrid[0:size, 0:size]
    ref = ((xx * xx + yy * yy) // (2 * size * size // 250 + 1)).astype(np.uint8)[None]
    cur = ref.copy()
    ox, oy = at[0] * mb, at[1] * mb
    cur[0, oy:oy + mb, ox:ox + mb] = ref[0, oy + target[1]:oy + target[1] + mb, ox + target[0]:ox + target[0] + mb]
    bw = size // mb
    f = lambda p: None if p is None else np.ascontiguousarray(p, np.int16).reshape(1, -1)
    mv, cost, (blocks, costs) = host_face(method, M.SAD, cur, ref, size, size, mb, R, f(prev1), f(prev2))
    field = mv[0].reshape(bw, bw, 2)
    g = lambda p: None if p is None else np.asarray(p).reshape(bw, bw, 2)
    before = collections.Counter(M.COUNTS)
    x, y, c, n = M.search(method, cur[0], ref[0], size, size, mb, R, M.SAD, at[0], at[1], field, g(prev1), g(prev2))
    took = collections.Counter(M.COUNTS)
    took.subtract(before)
    b = at[1] * bw + at[0]
    assert (int(mv[0, 2 * b]), int(mv[0, 2 * b + 1]), int(cost[0, b])) == (x, y, c)
    return (x - ox, y - oy), c, took, n


def _origins(size=64, mb=16):
    bw = size // mb
    return np.array([[(bx * mb, by * mb) for bx in range(bw)] for by in range(bw)], np.int64)


def test_a_single_block_evaluates_exactly_its_lists():
    """a picture of one block: the window is the origin alone.  EPZS: median, (0,0), collocated, accelerator — four times the same
    position, duplicates evaluated again — and dia1 refused; UMH: median, (0,0), and the origin once more in the raster.  No early
    return at cost 0."""
    a = np.full((1, 16, 16), 9, np.uint8)
    for method, n in ((M.EPZS, 4), (M.UMH, 3)):
        mv, cost, counts = host_face(method, M.SAD, a, a, 16, 16, 16, 7, None, None)
        assert mv.tolist() == [[0, 0]] and cost.tolist() == [[0]] and counts == (1, n)
        assert M.search(method, a[0], a[0], 16, 16, 16, 7, M.SAD, 0, 0, np.zeros((1, 1, 2), np.int16), None, None) == (0, 0, 0, n)


def test_umh_counts_in_a_flat_picture():
    """80 x 80, flat: nothing ever moves.  The block at (32, 32) with R = 4 has every candidate in its window: 5 predictors (median,
    (0,0), left, top, top-right), the cross 4 + 2 (d = 1 with, d = 3 without the vertical arm), the raster 25, one ring of 15 (entry 0
    of hex4 is not evaluated), hex2 6, dia1 4"""
    a = np.full((1, 80, 80), 77, np.uint8)
    field = _origins(80).astype(np.int16)
    assert M.search(M.UMH, a[0], a[0], 80, 80, 16, 4, M.SAD, 2, 2, field, None, None) == (32, 32, 0, 5 + 6 + 25 + 15 + 6 + 4)
    mv, cost, (blocks, costs) = host_face(M.UMH, M.SAD, a, a, 80, 80, 16, 4, None, None)
    assert np.array_equal(mv.reshape(5, 5, 2), field) and costs == M.frames(M.UMH, a, a, 80, 80, 16, 4, M.SAD)[2]


def test_epzs_collocated_and_accelerator():
    """the match lies at (6, -5): with prev1 pointing there the collocated predictor takes it, and with rel1 = (3, -2), rel2 = (0, 1)
    the accelerator 2 * rel1 - rel2 does; without either the median, (0, 0), is the first and best of the list"""
    o = _origins()
    mv, cost, took, _ = _bowl((6, -5), M.EPZS)
    assert took["wins_median"] == 1                     # every neighbour stands still: the median is (0, 0) and (0, 0) only ties
    p1 = o.copy()
    p1[2, 2] += (6, -5)
    mv, cost, took, _ = _bowl((6, -5), M.EPZS, p1)
    assert (mv, cost) == ((6, -5), 0) and took["wins_collocated"] == 1
    p1, p2 = o.copy(), o.copy()
    p1[2, 2] += (3, -2)
    p2[2, 2] += (0, 1)
    mv, cost, took, _ = _bowl((6, -5), M.EPZS, p1, p2)
    assert (mv, cost) == ((6, -5), 0) and took["wins_accelerator"] == 1


@pytest.mark.parametrize("where,label", [((-1, 0), "prev_left"), ((0, -1), "prev_top"), ((1, 0), "prev_right"), ((0, 1), "prev_bottom")])
def test_epzs_takes_prev1_of_the_four_neighbours(where, label):
    p1 = _origins()
    p1[2 + where[1], 2 + where[0]] += (-5, 6)
    mv, cost, took, _ = _bowl((-5, 6), M.EPZS, p1)
    assert (mv, cost) == ((-5, 6), 0) and took["wins_" + label] == 1
    assert _bowl((-5, 6), M.UMH, p1)[2]["wins_" + label] == 0       # UMH reads neither field


def test_umh_takes_the_top_left_block_in_the_last_column_and_epzs_does_not():
    """the block at (3, 2) of 4 x 4: UMH has the top-left block as its fourth predictor (n = 4), EPZS has three (n = 3); and the other
    counts of the median rule"""
    assert _bowl((0, 0), M.UMH, at=(3, 2))[2]["median_n4"] == 1
    assert _bowl((0, 0), M.EPZS, at=(3, 2))[2]["median_n3"] == 1
    assert _bowl((0, 0), M.UMH, at=(0, 2))[2]["median_n3"] == 1
    assert _bowl((0, 0), M.UMH, at=(2, 0))[2]["median_n2"] == 1
    assert _bowl((0, 0), M.UMH, at=(0, 0))[2]["median_n1"] == 1


# ---- arguments ------------------------------------------------------------------------------------------------------------------
def _args(**over):
    """a well-formed call on 64 x 48, two pairs; buffers are kept alive by the returned dict"""
    a = dict(method=M.EPZS, width=64, height=48, stride=64, frame_pitch=64 * 48, nframes=2, mb_size=16, search_param=7, cost_kind=M.SAD)
    a["cur"], a["ref"] = np.zeros(2 * 64 * 48, np.uint8), np.zeros(2 * 64 * 48, np.uint8)
    a["prev1"], a["prev2"] = np.zeros(2 * 12 * 2, np.int16), np.zeros(2 * 12 * 2, np.int16)
    a["mv"], a["cost"] = np.full(2 * 12 * 2, 7, np.int16), np.zeros(2 * 12, np.uint32)
    a.update(over)
    return a


def _addr(v):
    return None if v is None else v if isinstance(v, int) else v.ctypes.data


def _call(face, a):
    args = [a["method"], _addr(a["cur"]), _addr(a["ref"]), a["width"], a["height"], a["stride"], a["frame_pitch"], a["nframes"], a["mb_size"],
            a["search_param"], a["cost_kind"], _addr(a["prev1"]), _addr(a["prev2"]), _addr(a["mv"]), _addr(a["cost"])]
    L = _lib()
    return L.ffhip_me_search_pred_frames_host(*args) if face == "host" else L.ffhip_me_search_pred_batch_dev(*(args + [None]))


def _bad():
    """name -> (overrides, a word of the text).  The overlapping ones carve both arrays out of one buffer."""
    pool = np.zeros(4096, np.int16)
    mv = pool[:48]
    bad = {"a NULL cur": (dict(cur=None), "NULL"), "a NULL ref": (dict(ref=None), "NULL"), "a NULL mv_out": (dict(mv=None), "NULL"),
           "a NULL cost_out": (dict(cost=None), "NULL"), "mb_size 4": (dict(mb_size=4), "mb_size 4"), "mb_size 32": (dict(mb_size=32), "mb_size 32"),
           "cost_kind 2": (dict(cost_kind=2), "cost_kind 2"), "cost_kind -1": (dict(cost_kind=-1), "cost_kind -1"),
           "a negative width": (dict(width=-16), "negative"), "a negative height": (dict(height=-16), "negative"),
           "a negative nframes": (dict(nframes=-1), "negative"), "a negative search_param": (dict(search_param=-1), "negative"),
           "stride < width": (dict(stride=63), "stride < width"), "a negative stride": (dict(stride=-64), "stride < width"),
           "frame_pitch < stride * height": (dict(frame_pitch=64 * 48 - 1), "frame_pitch"),
           "method 0": (dict(method=0), "method 0 is neither EPZS"), "method 10": (dict(method=10), "method 10 is neither EPZS"),
           "a width above 32768": (dict(width=32784, stride=32784, height=16, nframes=1, cur=np.zeros(16 * 32784, np.uint8),
                                        ref=np.zeros(16 * 32784, np.uint8), mv=np.zeros(2 * 2049, np.int16), cost=np.zeros(2049, np.uint32),
                                        prev1=None, prev2=None), "32784 x 16"),
           "a height above 32768": (dict(height=32776, width=16, stride=16, nframes=1, cur=np.zeros(16 * 32776, np.uint8),
                                         ref=np.zeros(16 * 32776, np.uint8), mv=np.zeros(2 * 2048, np.int16), cost=np.zeros(2048, np.uint32),
                                         prev1=None, prev2=None), "16 x 32776"),
           "mv_out at an odd dword": (dict(mv=pool[1:49]), "4-byte aligned"),
           "mv_out overlapping prev1": (dict(mv=mv, prev1=pool[46:94]), "overlaps"),
           "mv_out overlapping prev2": (dict(mv=mv, prev2=pool[2:50]), "overlaps"),
           "mv_out equal to prev1": (dict(mv=mv, prev1=mv), "overlaps"),
           "mv_out overlapping cost_out": (dict(mv=mv, cost=pool[40:88].view(np.uint32)), "overlaps"),
           "mv_out inside cur": (dict(mv=mv, cur=pool.view(np.uint8)[:2 * 64 * 48]), "overlaps"),
           "mv_out at the last sample of ref": (dict(mv=pool[3070:3118], ref=pool.view(np.uint8)[:2 * 64 * 48]), "overlaps")}
    for m in range(1, 8):
        bad["method %d" % m] = (dict(method=m), "method %d is neither EPZS" % m)
    return bad


BAD = _bad()


@pytest.mark.parametrize("face", ["host", "dev"])
@pytest.mark.parametrize("what", sorted(BAD))
def test_einval(what, face):
    """each refusal alone, on both faces, before any device check, with its text; nothing is written.  The well-formed call goes to
    the device face only where there is no device: these are host arrays, and a launch would follow their pointers"""
    if face == "host":
        assert _call(face, _args()) == 0
    elif _lib().ffhip_device_count() == 0:
        assert _call(face, _args()) == ENOSYS
    over, word = BAD[what]
    a = _args(**over)
    if a["mv"] is not None:
        a["mv"][:] = 7
    assert _call(face, a) == EINVAL
    text = _lib().ffhip_last_error().decode()
    assert "ffhip_me_search_pred" in text and word in text and "FFHIP_" not in text, text
    assert a["mv"] is None or (a["mv"] == 7).all()


def test_what_is_legal_at_the_edges():
    pool = np.zeros(4096, np.int16)
    assert _call("host", _args(frame_pitch=1, nframes=1)) == 0                    # one frame: the pitch is not used
    a = _args(nframes=0)
    assert _call("host", a) == 0 and (a["mv"] == 7).all()                         # nothing is done
    a = _args(width=15)
    assert _call("host", a) == 0 and (a["mv"] == 7).all()                         # no whole block
    assert _call("host", _args(nframes=0, mv=pool[:48], prev1=pool[:48])) == 0    # no blocks: nothing overlaps
    assert _call("host", _args(search_param=0)) == 0
    assert _call("host", _args(search_param=2 ** 31 - 1)) == 0                    # the window and the d loops do not overflow
    assert _call("host", _args(method=M.UMH, search_param=2 ** 31 - 1)) == 0
    assert _call("host", _args(width=0, height=0, stride=0)) == 0
    assert _call("host", _args(prev1=None)) == 0 and _call("host", _args(prev2=None)) == 0
    assert _call("host", _args(mv=pool[:48], prev1=pool[48:96], prev2=pool[96:144])) == 0     # touching is not overlapping
    assert _call("host", _args(prev1=pool[:48], prev2=pool[:48])) == 0            # the two inputs may be one field
    assert _call("host", _args(width=32768, stride=32768, height=16, nframes=1, cur=np.zeros(16 * 32768, np.uint8), ref=np.zeros(16 * 32768, np.uint8),
                               mv=np.zeros(2 * 2048, np.int16), cost=np.zeros(2048, np.uint32), prev1=None, prev2=None, search_param=1)) == 0


@pytest.mark.parametrize("face", ["host", "dev"])
@pytest.mark.parametrize("method,name", [(8, "EPZS"), (9, "UMH")])
def test_the_per_block_face_still_refuses_epzs_and_umh(method, name, face):
    import test_me_search_cpu as T
    a = T._args(method=method, mv=np.full(48, 7, np.int16))
    assert T._call(face, a) == ENOSYS and (a["mv"] == 7).all()
    text = _lib().ffhip_last_error().decode()
    assert name in text and "neighbouring blocks' vectors" in text


def test_device_face_without_a_device():
    L = _lib()
    if L.ffhip_device_count() > 0:
        pytest.skip("a HIP device is present: the refusal is not reachable")
    for method in METHODS:
        a = _args(method=method)
        assert _call("dev", a) == ENOSYS and (a["mv"] == 7).all()


def test_python_face_on_the_host():
    from ffmpeg_amd import me
    assert (me.EPZS, me.UMH) == (M.EPZS, M.UMH)
    case = CASES[0]
    w, h, pad, mb, R = case
    cur, ref, _ = pairs(*case)
    p1, p2 = prev_fields(*case, "made")
    for method in METHODS:
        wmv, wcost, wn, _ = reference(method, M.SATD, *case)
        mv, cost = np.zeros_like(wmv), np.zeros_like(wcost)
        got = me.search_pred_frames_host(method, np.ascontiguousarray(cur), np.ascontiguousarray(ref), w, h, w + pad, h * (w + pad), NF, mb, R,
                                         me.SATD, np.array(p1), np.array(p2), mv, cost)
        assert np.array_equal(mv, wmv) and np.array_equal(cost, wcost) and got == (NF * 12, wn)
    wmv, wcost, wn, _ = reference(M.UMH, M.SAD, *case, "none")
    got = me.search_pred_frames_host(me.UMH, np.ascontiguousarray(cur), np.ascontiguousarray(ref), w, h, w + pad, h * (w + pad), NF, mb, R, me.SAD,
                                     None, None, mv, cost)
    assert np.array_equal(mv, wmv) and np.array_equal(cost, wcost) and got == (NF * 12, wn)
    with pytest.raises(RuntimeError, match="neither EPZS"):
        me.search_pred_frames_host(me.DS, np.ascontiguousarray(cur), np.ascontiguousarray(ref), w, h, w + pad, h * (w + pad), NF, mb, R, me.SAD,
                                   None, None, mv, cost)
