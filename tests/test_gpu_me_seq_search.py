"""GPU tier of the predictive motion searches of whole sequences: ffhip_me_search_pred_sequence_dev == ffhip_me_search_pred_sequence_host ==
the chained calls of ffhip_me_search_pred_batch_dev it is defined by, byte for byte, on the inputs of tests/test_me_seq_search_cpu.py
(the three made sequences, which only a kernel that reads the published fields of the pairs before solves, included).  The kernel runs a
sequence as a wavefront over (pair, row), one wave per block row of a pair; so beside the shapes there are runs with the number of
workgroups fixed (one wave doing every unit in ticket order, three leaving awaited units to each other), calls split into launches at a
pair boundary, a call continued by another on the same stream, and a 1920 x 1080 sequence."""
import functools

import numpy as np
import pytest

import me_pred_search_model as M
import test_me_pred_search_cpu as T
import test_me_seq_search_cpu as S
from test_gpu_me_search import Guarded

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def seq_dev(torch, method, kind, frames, w, h, mb, R, direction, init1, init2):
    """the device face on guarded buffers -> mv (np, nseq, b * 2), cost (np, nseq, b); asserts that nothing outside the outputs changed
    and no hand-off was lost"""
    from ffmpeg_amd import _lib, me
    nseq, nframes, _, stride = frames.shape
    per, np_ = (w // mb) * (h // mb), max(nframes - 1, 0)
    gf = Guarded(torch, frames)
    g1, g2 = (None if p is None else Guarded(torch, p) for p in (init1, init2))
    gm, gk = Guarded(torch, np.full((np_, nseq, per * 2), 0x5A5A, np.int16)), Guarded(torch, np.full((np_, nseq, per), 0x5A5A5A5A, np.uint32))
    me.search_pred_sequence(method, gf.t, w, h, stride, h * stride, nframes, nframes * h * stride, nseq, direction, mb, R, kind, g1 and g1.t,
                            g2 and g2.t, gm.t, gk.t)
    assert _lib.lib().ffhip_stream_synchronize(None) == 0, _lib.lib().ffhip_last_error()
    torch.cuda.synchronize()
    assert gf.unchanged() and gm.guards_intact() and gk.guards_intact()
    assert (g1 is None or g1.unchanged()) and (g2 is None or g2.unchanged())
    return gm.host(), gk.host()


def chained_dev(torch, method, kind, frames, w, h, mb, R, direction, init1, init2):
    """the definition on the device: one call of the pair face per step, queued on one stream, each step's prev fields the two steps
    before it in the same output buffers; guarded alike"""
    from ffmpeg_amd import _lib, me
    nseq, nframes, _, stride = frames.shape
    per, plane = (w // mb) * (h // mb), h * stride
    gf = Guarded(torch, frames)
    g1, g2 = (None if p is None else Guarded(torch, p) for p in (init1, init2))
    gm, gk = Guarded(torch, np.full((nframes - 1, nseq, per * 2), 0x5A5A, np.int16)), Guarded(torch, np.full((nframes - 1, nseq, per), 0x5A5A5A5A, np.uint32))
    step = lambda g, k, unit: g.t[k * nseq * per * unit:(k + 1) * nseq * per * unit]
    for k in range(nframes - 1):
        lo, hi = gf.t[k * plane:], gf.t[(k + 1) * plane:]
        p1 = step(gm, k - 1, 4) if k >= 1 else g1 and g1.t
        p2 = step(gm, k - 2, 4) if k >= 2 else (g1 and g1.t) if k == 1 else g2 and g2.t
        me.search_pred_batch(method, lo if direction else hi, hi if direction else lo, w, h, stride, nframes * plane, nseq, mb, R, kind, p1, p2,
                             step(gm, k, 4), step(gk, k, 4))
    assert _lib.lib().ffhip_stream_synchronize(None) == 0, _lib.lib().ffhip_last_error()
    torch.cuda.synchronize()
    assert gf.unchanged() and gm.guards_intact() and gk.guards_intact()
    return gm.host(), gk.host()


def _check(torch, method, kind, frames, case, direction, i1, i2, chain=True):
    """device == host face (== the chained host face and the model: tests/test_me_seq_search_cpu.py) == chained device calls"""
    w, h, _, mb, R = case
    hmv, hcost, _ = S.seq_host(method, kind, frames, w, h, mb, R, direction, i1, i2)
    mv, cost = seq_dev(torch, method, kind, frames, w, h, mb, R, direction, i1, i2)
    what = (M.NAMES[method], kind, direction, frames.shape[:2])
    assert np.array_equal(cost, hcost), what
    assert np.array_equal(mv, hmv), what
    if chain:
        cmv, ccost = chained_dev(torch, method, kind, frames, w, h, mb, R, direction, i1, i2)
        assert np.array_equal(ccost, cost) and np.array_equal(cmv, mv), what
    return mv, cost


@pytest.mark.parametrize("direction", S.DIRECTIONS)
@pytest.mark.parametrize("kind", T.KINDS, ids=["sad", "satd"])
@pytest.mark.parametrize("w,h,pad,mb,R", S.CASES)
def test_device_equals_host_equals_chained_device_calls(w, h, pad, mb, R, kind, direction):
    torch = _torch()
    case = (w, h, pad, mb, R)
    for method in T.METHODS:
        wmv, wcost, _ = S.reference(method, kind, direction, *case)
        for nseq, nframes, frames, i1, i2 in S.calls(case):
            mv, cost = _check(torch, method, kind, frames, case, direction, i1, i2)
            assert np.array_equal(mv, wmv[:nframes - 1, :nseq]) and np.array_equal(cost, wcost[:nframes - 1, :nseq])


@pytest.mark.parametrize("method", T.METHODS, ids=[M.NAMES[m] for m in T.METHODS])
def test_the_chained_run_of_five_pictures(method):
    torch = _torch()
    pics, want = T.chain()
    mv, cost = _check(torch, method, M.SAD, np.ascontiguousarray(pics[None]), (64, 48, 0, 16, 7), 0, None, None)
    for k in range(4):
        assert np.array_equal(mv[k], want[method][k][0]) and np.array_equal(cost[k], want[method][k][1]), k


@pytest.mark.parametrize("kind", T.KINDS, ids=["sad", "satd"])
def test_the_made_sequences(kind):
    """white noise, every block's only match where the accelerator, the collocated vector or one of prev1's four neighbours points: a
    stale or unpublished field of the pair before cannot give these bytes (SAD: cost 0 in every block)"""
    torch = _torch()
    frames, i1, i2, _ = S.made()
    for method in T.METHODS:
        for nseq in (3, 1):
            mv, cost = _check(torch, method, kind, np.ascontiguousarray(frames[:nseq]), S.MADE, 0, i1[:nseq], i2[:nseq])
            if method == M.EPZS and kind == M.SAD and nseq == 3:
                wmv, wcost, _ = S.made_reference()
                assert np.array_equal(mv, wmv) and np.array_equal(cost, wcost) and not cost.any()


#: one block row, two rows, 6 rows of 8 blocks
ROUNDS = [S.CASES[0], S.CASES[1], (64, 48, 0, 8, 9)]


@pytest.mark.parametrize("wgs", ["1", "3"])
@pytest.mark.parametrize("w,h,pad,mb,R", ROUNDS)
def test_ticket_rounds(w, h, pad, mb, R, wgs, monkeypatch):
    """5 pairs of 2 sequences, 10 to 60 units, on one wave and on three: with one wave every awaited unit is finished before the next
    begins; three waves leave the units they await to each other"""
    torch = _torch()
    monkeypatch.setenv("FFHIP_ME_PRED_WGS", wgs)
    case = (w, h, pad, mb, R)
    frames, i1, i2 = S.pictures(*case)
    for kind in T.KINDS:
        for method in T.METHODS:
            _check(torch, method, kind, np.ascontiguousarray(frames[:2]), case, 0, i1[:2], i2[:2], chain=False)
    if case == S.CASES[1]:
        mframes, m1, m2, _ = S.made()
        _check(torch, M.EPZS, M.SAD, np.ascontiguousarray(mframes[:2]), S.MADE, 0, m1[:2], m2[:2], chain=False)


@functools.lru_cache(maxsize=None)
def _long(nseq):
    """1032 pictures of 16 x 64 per sequence, each with content of its own: a noise strip that shifts by a vector that changes from
    picture to picture, one pixel in 16 drawn again"""
    rng = np.random.default_rng(1032 + nseq)
    base = rng.integers(0, 256, (nseq, 64 + 16, 16 + 16), dtype=np.uint8)
    frames = np.zeros((nseq, 1032, 64, 16), np.uint8)
    for s in range(nseq):
        x = y = 8
        for p in range(1032):
            x, y = min(max(x + int(rng.integers(-2, 3)), 0), 16), min(max(y + int(rng.integers(-2, 3)), 0), 16)
            frames[s, p] = base[s, y:y + 64, x:x + 16]
    fresh = rng.random(frames.shape) < 1 / 16
    frames[fresh] = rng.integers(0, 256, int(fresh.sum()), dtype=np.uint8)
    frames.setflags(write=False)
    return frames


@pytest.mark.parametrize("nseq", [1, 3])
def test_a_call_split_into_launches_at_a_pair_boundary(nseq):
    """16 x 64 at 8 x 8 has 8 block rows: 1023 units of one sequence fill a progress-pool slot, so 1031 pairs are two launches (1023 + 8)
    and the second reads the first's fields plainly; three sequences take 341 pairs per launch (8184 units), where a launch does not
    end at a slot's last counter"""
    torch = _torch()
    frames = _long(nseq)
    for method in T.METHODS:
        _check(torch, method, M.SAD, frames, (16, 64, 0, 8, 5), 0, None, None, chain=False)


@pytest.mark.parametrize("method", T.METHODS, ids=[M.NAMES[m] for m in T.METHODS])
def test_a_call_continues_the_one_before_on_one_stream(method):
    """4 + 3 pictures queued on one stream without a synchronisation in between, the second call's starting fields the first call's
    last two steps where it wrote them, == one call of 6"""
    from ffmpeg_amd import _lib, me
    torch = _torch()
    frames, i1, i2, _ = S.made()
    w, h, _, mb, R = S.MADE
    per, plane = (w // mb) * (h // mb), w * h
    want = S.seq_host(method, M.SAD, frames, w, h, mb, R, 0, i1, i2)
    # the two calls see sequences of 4 and of 3 pictures, seq_pitch apart as in the one array
    gf, g1, g2 = Guarded(torch, frames), Guarded(torch, i1), Guarded(torch, i2)
    gm, gk = Guarded(torch, np.full((5, 3, per * 2), 0x5A5A, np.int16)), Guarded(torch, np.full((5, 3, per), 0x5A5A5A5A, np.uint32))
    step = lambda g, k: g.t[k * 3 * per * 4:]
    me.search_pred_sequence(method, gf.t, w, h, w, plane, 4, 6 * plane, 3, 0, mb, R, M.SAD, g1.t, g2.t, gm.t, gk.t)
    me.search_pred_sequence(method, gf.t[3 * plane:], w, h, w, plane, 3, 6 * plane, 3, 0, mb, R, M.SAD, step(gm, 2), step(gm, 1), step(gm, 3), step(gk, 3))
    assert _lib.lib().ffhip_stream_synchronize(None) == 0, _lib.lib().ffhip_last_error()
    torch.cuda.synchronize()
    assert gf.unchanged() and g1.unchanged() and g2.unchanged() and gm.guards_intact() and gk.guards_intact()
    assert np.array_equal(gk.host(), want[1]) and np.array_equal(gm.host(), want[0])


@functools.lru_cache(maxsize=None)
def _hd_sequence():
    rng = np.random.default_rng(1080)
    big = T.texture(rng, 1080 + 64, 1920 + 64)
    frames = np.zeros((1, 5, 1080, 1920), np.uint8)
    x, y = 32, 32
    for p in range(5):
        x, y = x + int(rng.integers(-6, 7)), y + int(rng.integers(-6, 7))
        frames[0, p] = np.clip(np.round(big[y:y + 1080, x:x + 1920] + rng.integers(-2, 3, (1080, 1920))), 0, 255)
    frames.setflags(write=False)
    return frames


@pytest.mark.parametrize("method", T.METHODS, ids=[M.NAMES[m] for m in T.METHODS])
def test_1080p_against_the_host_face(method):
    """120 x 67 blocks and 4 pairs: 268 units in flight, each pair three blocks behind the one before"""
    torch = _torch()
    _check(torch, method, M.SAD, _hd_sequence(), (1920, 1080, 0, 16, 16), 0, None, None, chain=False)


def test_no_pairs_and_no_sequences_launch_nothing():
    from ffmpeg_amd import me
    torch = _torch()
    frames = torch.zeros(3 * 64 * 48, dtype=torch.uint8, device="cuda:0")
    mv = torch.full((128,), 7, dtype=torch.int16, device="cuda:0")
    cost = torch.full((64,), 7, dtype=torch.int32, device="cuda:0")
    for nframes, nseq, width in ((1, 1, 64), (0, 1, 64), (3, 0, 64), (3, 1, 15)):
        me.search_pred_sequence(me.EPZS, frames, width, 48, 64, 64 * 48, nframes, 3 * 64 * 48, nseq, 0, 16, 7, me.SAD, None, None, mv, cost)
    with pytest.raises(RuntimeError, match="direction 2"):
        me.search_pred_sequence(me.EPZS, frames, 64, 48, 64, 64 * 48, 3, 3 * 64 * 48, 1, 2, 16, 7, me.SAD, None, None, mv, cost)
    with pytest.raises(RuntimeError, match="overlaps"):
        me.search_pred_sequence(me.EPZS, frames, 64, 48, 64, 64 * 48, 3, 3 * 64 * 48, 1, 0, 16, 7, me.SAD, mv, None, mv, cost)
    torch.cuda.synchronize()
    assert bool((mv == 7).all()) and bool((cost == 7).all())


def test_umh_pairs_are_independent():
    """UMH reads no prev field: the sequence face gives the bytes of np * nseq independent pairs through the pair face, whatever the
    starting fields hold"""
    from test_gpu_me_pred_search import device_face
    torch = _torch()
    case = S.CASES[4]
    w, h, pad, mb, R = case
    frames, i1, i2 = S.pictures(*case)
    mv, cost = seq_dev(torch, M.UMH, M.SAD, frames, w, h, mb, R, 0, i1, i2)
    for s in range(S.NSEQ):
        pmv, pcost = device_face(torch, M.UMH, M.SAD, frames[s, 1:], frames[s, :-1], w, h, mb, R, None, None)
        assert np.array_equal(mv[:, s], pmv) and np.array_equal(cost[:, s], pcost), s
