"""CPU tier of the bilateral motion search (ffhip_me_search_bilat_frames_host / _sequence_host and the refusals of the device faces):
the host faces against the model of tests/me_bilat_model.py, which is written from the rule text of include/ffhip.h, in vectors, costs
and cost counts; the cost alone, block by block at every corner and edge, for every position of the window; pictures whose motion the
search has to find; the sequence face against its definition, the loop of pair calls; every refusal with its text.  No device is
needed.  tests/test_gpu_me_bilat.py takes its inputs and references from here."""
import ctypes as C
import functools

import numpy as np
import pytest

import ffi
import me_bilat_model as M
from test_me_search_cpu import Guarded

EINVAL, ENOSYS = -22, -38
METHODS = (M.EPZS, M.UMH)
IDS = [M.NAMES[m] for m in METHODS]

#: (blocks across, blocks down, extra samples, stride padding): the smallest legal picture, 6 x 5 blocks, a width and height of b * mb + 3
SHAPES = [(2, 2, 0, 0), (6, 5, 0, 1), (4, 3, 3, 2)]
PREVS = ("none", "made", "any")
NSEQ, NFRAMES = 3, 4


def _lib():
    from ffmpeg_amd import _lib
    return _lib.lib()


def me():
    from ffmpeg_amd import me
    return me


def blur9(a):
    """a 9-tap box blur along both axes"""
    k = np.ones(9) / 9.0
    a = np.apply_along_axis(lambda r: np.convolve(r, k, mode="same"), 0, a)
    return np.apply_along_axis(lambda r: np.convolve(r, k, mode="same"), 1, a)


def texture(rng, h, w):
    """the 9-tap box blur of uniform noise, rescaled to 0..255"""
    t = blur9(rng.random((h + 16, w + 16)))[8:-8, 8:-8]
    return np.round((t - t.min()) * (255.0 / (t.max() - t.min())))


def moved(big, m, w, h, stride, v):
    """A(p) = T(p - v), B(p) = T(p + v) as (h, stride) uint8; `big` has a margin of m samples round the picture"""
    A, B = np.zeros((h, stride), np.uint8), np.zeros((h, stride), np.uint8)
    A[:, :w] = big[m - v[1]:m - v[1] + h, m - v[0]:m - v[0] + w]
    B[:, :w] = big[m + v[1]:m + v[1] + h, m + v[0]:m + v[0] + w]
    return A, B


@functools.lru_cache(maxsize=None)
def sequences(bw, bh, extra, pad, mb):
    """NSEQ sequences of NFRAMES pictures: a texture that drifts by a few samples a picture, noise of +-1 on top (0), the same with a
    frozen corner block (1), flat with sparse marks (2: ties everywhere); and per kind of prev field two fields.
    -> pics (NSEQ, NFRAMES, h, stride) uint8, {kind: (f1, f2)} with (NSEQ, b * 2) int16 fields or None; read-only"""
    w, h = bw * mb + extra, bh * mb + extra
    stride, m = w + pad, 24
    rng = np.random.default_rng(ffi.stable_seed("me_bilat", bw, bh, extra, pad, mb))
    pics = np.zeros((NSEQ, NFRAMES, h, stride), np.uint8)
    for s in range(2):
        big = texture(rng, h + 2 * m, w + 2 * m)
        x, y = m, m
        for p in range(NFRAMES):
            x, y = x + int(rng.integers(-3, 4)), y + int(rng.integers(-3, 4))
            pics[s, p, :, :w] = np.clip(big[y:y + h, x:x + w] + rng.integers(-1, 2, (h, w)), 0, 255)
            if s == 1 and p:
                pics[s, p, :mb, :mb] = pics[s, p - 1, :mb, :mb]
    for p in range(NFRAMES):
        pics[2, p, :, :w] = 128
        pics[2, p, p % 5::5, (2 * p) % 7:w:7] = 131
    o = np.array([[(x * mb, y * mb) for x in range(bw)] for y in range(bh)], np.int64).reshape(-1)
    lim = np.tile([(bw - 1) * mb, (bh - 1) * mb], bw * bh)
    made = [np.clip(o + rng.integers(-4, 5, (NSEQ, o.size)), 0, lim).astype(np.int16) for _ in range(2)]
    anyf = [rng.integers(-32768, 32768, (NSEQ, o.size)).astype(np.int16) for _ in range(2)]
    fields = {"none": (None, None), "made": tuple(made), "any": tuple(anyf)}
    for a in [pics] + made + anyf:
        a.setflags(write=False)
    return pics, fields


def geometry(bw, bh, extra, pad, mb):
    w, h = bw * mb + extra, bh * mb + extra
    return w, h, w + pad


def host_pairs(method, A, B, w, h, mb, R, p1, p2, face=None):
    """ffhip_me_search_bilat_frames_host on guarded copies -> mv, cost, (blocks, costs); nothing outside the outputs may change"""
    nf, _, stride = A.shape
    per = (w // mb) * (h // mb)
    ga, gb = Guarded(A), Guarded(B)
    g1, g2 = (None if p is None else Guarded(p) for p in (p1, p2))
    gm, gk = Guarded(np.full((nf, per * 2), 0x5A5A, np.int16)), Guarded(np.full((nf, per), 0x5A5A5A5A, np.uint32))
    L = _lib()
    rc = L.ffhip_me_search_bilat_frames_host(method, ga.addr, gb.addr, w, h, stride, h * stride, nf, mb, R, g1 and g1.addr, g2 and g2.addr,
                                             gm.addr, gk.addr)
    assert rc == 0, (rc, L.ffhip_last_error())
    assert ga.unchanged() and gb.unchanged() and gm.guards_intact() and gk.guards_intact()
    assert all(g is None or g.unchanged() for g in (g1, g2))
    blocks, costs = C.c_uint64(), C.c_uint64()
    L.ffhip_me_search_host_counts(C.byref(blocks), C.byref(costs))
    return gm.body().copy(), gk.body().copy(), (blocks.value, costs.value)


def host_sequence(method, pics, w, h, mb, R, i1, i2):
    """ffhip_me_search_bilat_sequence_host on guarded copies -> mv (np, nseq, b * 2), cost (np, nseq, b), (blocks, costs)"""
    nseq, nfr, _, stride = pics.shape
    per = (w // mb) * (h // mb)
    gp = Guarded(pics)
    g1, g2 = (None if p is None else Guarded(p) for p in (i1, i2))
    gm, gk = Guarded(np.full((nfr - 1, nseq, per * 2), 0x5A5A, np.int16)), Guarded(np.full((nfr - 1, nseq, per), 0x5A5A5A5A, np.uint32))
    L = _lib()
    rc = L.ffhip_me_search_bilat_sequence_host(method, gp.addr, w, h, stride, h * stride, nfr, nfr * h * stride, nseq, mb, R, g1 and g1.addr,
                                               g2 and g2.addr, gm.addr, gk.addr)
    assert rc == 0, (rc, L.ffhip_last_error())
    assert gp.unchanged() and gm.guards_intact() and gk.guards_intact() and all(g is None or g.unchanged() for g in (g1, g2))
    blocks, costs = C.c_uint64(), C.c_uint64()
    L.ffhip_me_search_host_counts(C.byref(blocks), C.byref(costs))
    return gm.body().copy(), gk.body().copy(), (blocks.value, costs.value)


@functools.lru_cache(maxsize=None)
def pair_reference(method, shape, mb, R, prev):
    """the model over pictures 0 and 1 of every sequence, once"""
    pics, fields = sequences(*shape, mb)
    w, h, _ = geometry(*shape, mb)
    mv, cost, n = M.frames(method, np.ascontiguousarray(pics[:, 0]), np.ascontiguousarray(pics[:, 1]), w, h, mb, R, *fields[prev])
    mv.setflags(write=False)
    cost.setflags(write=False)
    return mv, cost, n


@functools.lru_cache(maxsize=None)
def sequence_reference(method, shape, mb, R, prev):
    """the model's loop of pair calls over all of sequences(...), sequence by sequence; a call over the first nseq is a prefix"""
    pics, fields = sequences(*shape, mb)
    w, h, _ = geometry(*shape, mb)
    i1, i2 = fields[prev]
    outs = [M.sequence(method, pics[s:s + 1], w, h, mb, R, None if i1 is None else i1[s:s + 1], None if i2 is None else i2[s:s + 1])
            for s in range(NSEQ)]
    mv, cost = np.concatenate([o[0] for o in outs], 1), np.concatenate([o[1] for o in outs], 1)
    mv.setflags(write=False)
    cost.setflags(write=False)
    return mv, cost, [o[2] for o in outs]


def search_params(mb):
    return (mb, 32)         # the smallest legal, and 32


@pytest.mark.parametrize("prev", PREVS)
@pytest.mark.parametrize("big_r", (False, True), ids=["R=mb", "R=32"])
@pytest.mark.parametrize("shape", SHAPES, ids=["2x2", "6x5", "4x3+3"])
@pytest.mark.parametrize("mb", (8, 16))
@pytest.mark.parametrize("method", METHODS, ids=IDS)
def test_host_face_equals_the_model(method, mb, shape, big_r, prev):
    R = search_params(mb)[big_r]
    pics, fields = sequences(*shape, mb)
    w, h, _ = geometry(*shape, mb)
    wmv, wcost, wn = pair_reference(method, shape, mb, R, prev)
    mv, cost, (blocks, costs) = host_pairs(method, np.ascontiguousarray(pics[:, 0]), np.ascontiguousarray(pics[:, 1]), w, h, mb, R, *fields[prev])
    assert np.array_equal(mv, wmv)
    assert np.array_equal(cost, wcost)
    assert blocks == NSEQ * shape[0] * shape[1] and costs == wn


@pytest.mark.parametrize("nseq", (1, 3))
@pytest.mark.parametrize("prev", ("none", "any"))
@pytest.mark.parametrize("mb,shape", [(8, SHAPES[2]), (16, SHAPES[1]), (16, SHAPES[0])], ids=["mb8-4x3+3", "mb16-6x5", "mb16-2x2"])
@pytest.mark.parametrize("method", METHODS, ids=IDS)
def test_a_chained_run_of_four_pictures_is_the_loop_of_pair_calls(method, mb, shape, prev, nseq):
    R = 32
    pics, fields = sequences(*shape, mb)
    w, h, _ = geometry(*shape, mb)
    i1, i2 = (None if f is None else f[:nseq] for f in fields[prev])
    wmv, wcost, wn = sequence_reference(method, shape, mb, R, prev)
    # the sequences of a call are seq_pitch apart: a contiguous copy of the first nseq
    mv, cost, (blocks, costs) = host_sequence(method, np.ascontiguousarray(pics[:nseq]), w, h, mb, R, i1, i2)
    assert np.array_equal(mv, wmv[:, :nseq]) and np.array_equal(cost, wcost[:, :nseq])
    assert blocks == (NFRAMES - 1) * nseq * shape[0] * shape[1] and costs == sum(wn[:nseq])
    # and the loop over the host pair face itself
    outs = []
    for k in range(NFRAMES - 1):
        p1 = outs[k - 1][0] if k >= 1 else i1
        p2 = outs[k - 2][0] if k >= 2 else (i1 if k == 1 else i2)
        outs.append(host_pairs(method, np.ascontiguousarray(pics[:nseq, k]), np.ascontiguousarray(pics[:nseq, k + 1]), w, h, mb, R, p1, p2))
    assert np.array_equal(mv, np.stack([o[0] for o in outs])) and np.array_equal(cost, np.stack([o[1] for o in outs]))


@pytest.mark.parametrize("R", (16, 21, 32))
@pytest.mark.parametrize("mb,bw,bh,extra", [(16, 3, 3, 3), (8, 3, 3, 0), (8, 2, 2, 5)])
def test_the_cost_alone_at_every_corner_and_edge(mb, bw, bh, extra, R):
    """cost(X, Y) of single blocks — all four corners, all four edges, the middle — for every (X, Y) of the block's window: this is
    the clamp of the two overlapped windows and nothing else"""
    w, h = bw * mb + extra, bh * mb + extra
    rng = np.random.default_rng(ffi.stable_seed("me_bilat_cost", mb, bw, bh, extra, R))
    A, B = (rng.integers(0, 256, (h, w + 3)).astype(np.uint8) for _ in range(2))
    ga, gb = Guarded(A), Guarded(B)
    for by in range(bh):
        for bx in range(bw):
            pred = (int(rng.integers(-9, 10)), int(rng.integers(-9, 10)))
            x_min, x_max, y_min, y_max = M.window(w, h, mb, R, bx * mb, by * mb)
            for Y in range(y_min, y_max + 1):
                for X in range(x_min, x_max + 1):
                    got = me().search_bilat_cost_host(ga.addr, gb.addr, w, h, w + 3, mb, R, bx, by, X, Y, pred)
                    assert got == M.cost(A, B, w, h, mb, R, bx * mb, by * mb, X, Y, pred), (bx, by, X, Y)
    assert ga.unchanged() and gb.unchanged()


MB, BW, BH, RR = 16, 6, 5, 32


@functools.lru_cache(maxsize=None)
def found_pictures(v):
    """A(p) = T(p - v), B(p) = T(p + v), mb 16, 6 x 5 blocks"""
    w, h, m = BW * MB, BH * MB, 8
    big = texture(np.random.default_rng(ffi.stable_seed("me_bilat_found")), h + 2 * m, w + 2 * m)
    A, B = moved(big, m, w, h, w, v)
    for a in (A, B, big):
        a.setflags(write=False)
    return A, B, big[m:m + h, m:m + w].astype(np.uint8)


@pytest.mark.parametrize("v", [(1, 0), (2, 1), (-3, 2)])
@pytest.mark.parametrize("method", METHODS, ids=IDS)
def test_found_motion(method, v):
    """every interior block's half-vector is v, with a sum of 0"""
    A, B, _ = found_pictures(v)
    w, h = BW * MB, BH * MB
    mv, cost, _ = host_pairs(method, A[None], B[None], w, h, MB, RR, None, None)
    wmv, wcost, _ = M.frames(method, A[None], B[None], w, h, MB, RR)
    assert np.array_equal(mv, wmv) and np.array_equal(cost, wcost)
    field = mv.reshape(BH, BW, 2)
    for by in range(1, BH - 1):
        for bx in range(1, BW - 1):
            X, Y = (int(c) for c in field[by, bx])
            assert (X - bx * MB, Y - by * MB) == v, (bx, by)
            assert M.sbad(A, B, w, h, MB, RR, bx * MB, by * MB, X, Y) == 0


# ---- refusals: identically in the host and the device faces, before any device check ---------------------------------------------------
def _pair_args(**over):
    w, h, mb = 48, 40, 16
    a = dict(method=M.EPZS, cur=np.zeros((h, w), np.uint8), ref=np.zeros((h, w), np.uint8), width=w, height=h, stride=w, frame_pitch=w * h, nframes=1,
             mb_size=mb, search_param=16, prev1=None, prev2=None, mv_out=np.zeros(2 * 6, np.int16), cost_out=np.zeros(6, np.uint32))
    a.update(over)
    return a


def _seq_args(**over):
    w, h, mb = 48, 40, 16
    a = dict(method=M.EPZS, frames=np.zeros((2, 3, h, w), np.uint8), width=w, height=h, stride=w, frame_pitch=w * h, nframes=3, seq_pitch=3 * w * h,
             nseq=2, mb_size=mb, search_param=16, init1=None, init2=None, mv_out=np.zeros(2 * 2 * 2 * 6, np.int16), cost_out=np.zeros(2 * 2 * 6, np.uint32))
    a.update(over)
    return a


def _addr(v):
    return v.ctypes.data if isinstance(v, np.ndarray) else v


def _call(name, a):
    L = _lib()
    args = [_addr(v) for v in a.values()]
    if name.endswith("_dev"):
        args.append(None)
    rc = getattr(L, name)(*args)
    return rc, L.ffhip_last_error().decode()


_odd = np.zeros(64, np.int16)
PAIR_REFUSALS = {
    "a NULL cur": (dict(cur=None), EINVAL, "a NULL cur, ref, mv_out or cost_out"),
    "a NULL cost_out": (dict(cost_out=None), EINVAL, "a NULL cur, ref, mv_out or cost_out"),
    "mb_size 4": (dict(mb_size=4), EINVAL, "mb_size 4 (16 or 8)"),
    "stride < width": (dict(stride=40), EINVAL, "stride < width"),
    "a negative nframes": (dict(nframes=-1), EINVAL, "a negative width, height"),
    "method 0": (dict(method=0), EINVAL, "method 0 is neither EPZS (8) nor UMH (9)"),
    "method 10": (dict(method=10), EINVAL, "method 10 is neither EPZS (8) nor UMH (9)"),
    "a width above 32768": (dict(width=32784, stride=32784, cur=0x1000, ref=0x1000, frame_pitch=32784 * 40), EINVAL, "do not fit the int16 vector fields"),
    "mv_out not 4-byte aligned": (dict(mv_out=_odd.ctypes.data + 2), EINVAL, "mv_out is not 4-byte aligned"),
    "search_param below mb_size": (dict(search_param=15), EINVAL, "search_param 15 below mb_size 16"),
    "one block column": (dict(width=31, stride=48), EINVAL, "31 x 40 is 1 x 2 blocks: the bilateral cost needs two block columns and two block rows"),
    "one block row": (dict(height=31), EINVAL, "48 x 31 is 3 x 1 blocks"),
}


@pytest.mark.parametrize("face", ("ffhip_me_search_bilat_batch_dev", "ffhip_me_search_bilat_frames_host"))
@pytest.mark.parametrize("what", sorted(PAIR_REFUSALS))
def test_pair_faces_refuse(what, face):
    over, want, text = PAIR_REFUSALS[what]
    rc, err = _call(face, _pair_args(**over))
    assert rc == want and text in err and err.startswith("ffhip_me_search_bilat_batch_dev / _frames_host: "), (rc, err)


def test_pair_faces_refuse_an_overlapping_mv_out():
    for face in ("ffhip_me_search_bilat_batch_dev", "ffhip_me_search_bilat_frames_host"):
        a = _pair_args()
        a["prev1"] = a["mv_out"]
        rc, err = _call(face, a)
        assert rc == EINVAL and "mv_out overlaps prev1, prev2, cur, ref or cost_out" in err


SEQ_REFUSALS = {
    "a NULL frames": (dict(frames=None), EINVAL, "a NULL frames, mv_out or cost_out"),
    "a negative nseq": (dict(nseq=-1), EINVAL, "a negative nseq (-1)"),
    "seq_pitch too small": (dict(seq_pitch=3 * 48 * 40 - 1), EINVAL, "the pictures of two sequences would share bytes"),
    "method 10": (dict(method=10), EINVAL, "method 10 is neither EPZS (8) nor UMH (9)"),
    "search_param below mb_size": (dict(search_param=0), EINVAL, "search_param 0 below mb_size 16"),
    "one block row": (dict(height=16), EINVAL, "48 x 16 is 3 x 1 blocks"),
}


@pytest.mark.parametrize("face", ("ffhip_me_search_bilat_sequence_dev", "ffhip_me_search_bilat_sequence_host"))
@pytest.mark.parametrize("what", sorted(SEQ_REFUSALS))
def test_sequence_faces_refuse(what, face):
    over, want, text = SEQ_REFUSALS[what]
    rc, err = _call(face, _seq_args(**over))
    assert rc == want and text in err and err.startswith("ffhip_me_search_bilat_sequence_dev / _host: "), (rc, err)


@pytest.mark.parametrize("method,name", list(zip(range(1, 8), ("ESA", "TSS", "TDLS", "NTSS", "FSS", "DS", "HEXBS"))))
def test_the_per_block_methods_are_refused_by_name(method, name):
    for face, args in (("ffhip_me_search_bilat_batch_dev", _pair_args), ("ffhip_me_search_bilat_frames_host", _pair_args),
                       ("ffhip_me_search_bilat_sequence_dev", _seq_args), ("ffhip_me_search_bilat_sequence_host", _seq_args)):
        rc, err = _call(face, args(method=method))
        assert rc == ENOSYS and "method %d (%s)" % (method, name) in err, (face, rc, err)


def test_the_order_of_the_refusals():
    """a per-block method goes through the shared checks and the field checks first (EINVAL), then is refused by name (ENOSYS), before
    search_param and the block counts are looked at"""
    odd = np.zeros(64, np.int16)
    for face, args in (("ffhip_me_search_bilat_batch_dev", _pair_args), ("ffhip_me_search_bilat_frames_host", _pair_args),
                       ("ffhip_me_search_bilat_sequence_dev", _seq_args), ("ffhip_me_search_bilat_sequence_host", _seq_args)):
        rc, err = _call(face, args(method=3, mb_size=4))
        assert rc == EINVAL and "mb_size 4 (16 or 8)" in err and "cost_kind" not in err, (face, rc, err)
        rc, err = _call(face, args(method=3, mv_out=odd.ctypes.data + 2))
        assert rc == EINVAL and "mv_out is not 4-byte aligned" in err, (face, rc, err)
        rc, err = _call(face, args(method=3, search_param=1, height=16))
        assert rc == ENOSYS and "method 3 (TDLS)" in err, (face, rc, err)
        rc, err = _call(face, args(method=10, search_param=1))
        assert rc == EINVAL and "method 10 is neither" in err, (face, rc, err)


def test_what_is_legal_at_the_edges():
    """nothing to search is no refusal: no pair, a picture smaller than a block, a sequence of one picture — and nothing is written"""
    for over in (dict(nframes=0), dict(width=15, height=40), dict(width=48, height=7)):
        a = _pair_args(**over)
        a["mv_out"][:] = 0x5A5A
        rc, err = _call("ffhip_me_search_bilat_frames_host", a)
        assert rc == 0 and (a["mv_out"] == 0x5A5A).all(), (over, rc, err)
    for over in (dict(nframes=1), dict(nframes=0), dict(nseq=0), dict(height=16, nframes=1)):
        a = _seq_args(**over)
        a["mv_out"][:] = 0x5A5A
        rc, err = _call("ffhip_me_search_bilat_sequence_host", a)
        assert rc == 0 and (a["mv_out"] == 0x5A5A).all(), (over, rc, err)


def test_device_faces_without_a_device():
    if _lib().ffhip_device_count() > 0:
        pytest.skip("a HIP device is present: the refusal is not reachable")
    for face, args in (("ffhip_me_search_bilat_batch_dev", _pair_args), ("ffhip_me_search_bilat_sequence_dev", _seq_args)):
        rc, _ = _call(face, args())
        assert rc == ENOSYS


def test_python_faces_on_the_host():
    shape, mb, R = SHAPES[0], 16, 16
    pics, _ = sequences(*shape, mb)
    w, h, stride = geometry(*shape, mb)
    per = shape[0] * shape[1]
    mv, cost = np.zeros((NSEQ, per * 2), np.int16), np.zeros((NSEQ, per), np.uint32)
    A, B = np.ascontiguousarray(pics[:, 0]), np.ascontiguousarray(pics[:, 1])
    blocks, costs = me().search_bilat_frames_host(M.EPZS, A, B, w, h, stride, h * stride, NSEQ, mb, R, None, None, mv, cost)
    wmv, wcost, wn = pair_reference(M.EPZS, shape, mb, R, "none")
    assert np.array_equal(mv, wmv) and np.array_equal(cost, wcost) and (blocks, costs) == (NSEQ * per, wn)
    smv, scost = np.zeros((NFRAMES - 1, NSEQ, per * 2), np.int16), np.zeros((NFRAMES - 1, NSEQ, per), np.uint32)
    me().search_bilat_sequence_host(M.EPZS, pics, w, h, stride, h * stride, NFRAMES, NFRAMES * h * stride, NSEQ, mb, R, None, None, smv, scost)
    assert np.array_equal(smv[0], wmv) and np.array_equal(scost[0], wcost)
    with pytest.raises(RuntimeError, match="method 6 .DS. is not offered under the bilateral cost"):
        me().search_bilat_frames_host(6, A, B, w, h, stride, h * stride, NSEQ, mb, R, None, None, mv, cost)
