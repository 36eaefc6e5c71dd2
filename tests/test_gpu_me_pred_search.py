"""GPU tier of the filter's predictive motion searches: ffhip_me_search_pred_batch_dev == ffhip_me_search_pred_frames_host == the model of
tests/me_pred_search_model.py, on the inputs and references of tests/test_me_pred_search_cpu.py (computed once, shared).  The kernel
searches the blocks of a pair in wavefront order, one wave per block row, the rows handing their vectors on through mv_out; so beside
the shapes there are runs with the number of workgroups fixed (several ticket rounds, one wave doing every row in turn), a call split
into several launches by pairs, a chained run on one stream and a 1920 x 1080 pair."""
import functools

import numpy as np
import pytest

import me_pred_search_model as M
import test_me_pred_search_cpu as T
from test_gpu_me_search import Guarded

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def device_face(torch, method, kind, cur, ref, w, h, mb, R, prev1, prev2):
    """the device face on guarded buffers -> mv, cost; asserts that nothing outside the outputs changed and no hand-off was lost"""
    from ffmpeg_amd import _lib, me
    nf, _, stride = cur.shape
    bw, bh = w // mb, h // mb
    gc, gr = Guarded(torch, cur), Guarded(torch, ref)
    g1, g2 = (None if p is None else Guarded(torch, p) for p in (prev1, prev2))
    gm, gk = Guarded(torch, np.full((nf, bh * bw * 2), 0x5A5A, np.int16)), Guarded(torch, np.full((nf, bh * bw), 0x5A5A5A5A, np.uint32))
    me.search_pred_batch(method, gc.t, gr.t, w, h, stride, h * stride, nf, mb, R, kind, g1 and g1.t, g2 and g2.t, gm.t, gk.t)
    assert _lib.lib().ffhip_stream_synchronize(None) == 0, _lib.lib().ffhip_last_error()
    torch.cuda.synchronize()
    assert gc.unchanged() and gr.unchanged() and gm.guards_intact() and gk.guards_intact()
    assert (g1 is None or g1.unchanged()) and (g2 is None or g2.unchanged())
    return gm.host(), gk.host()


def _check(torch, method, kind, case, what="made"):
    w, h, pad, mb, R = case
    cur, ref, _ = T.pairs(*case)
    p1, p2 = T.prev_fields(*case, what)
    wmv, wcost, _, _ = T.reference(method, kind, *case, what)
    hmv, hcost, _ = T.host_face(method, kind, cur, ref, w, h, mb, R, p1, p2)
    assert np.array_equal(hcost, wcost) and np.array_equal(hmv, wmv), M.NAMES[method]
    mv, cost = device_face(torch, method, kind, cur, ref, w, h, mb, R, p1, p2)
    assert np.array_equal(cost, wcost), M.NAMES[method]
    assert np.array_equal(mv, wmv), M.NAMES[method]


@pytest.mark.parametrize("kind", T.KINDS, ids=["sad", "satd"])
@pytest.mark.parametrize("w,h,pad,mb,R", T.CASES)
def test_device_equals_host_equals_model(w, h, pad, mb, R, kind):
    torch = _torch()
    for method in T.METHODS:
        _check(torch, method, kind, (w, h, pad, mb, R))


@pytest.mark.parametrize("what", ["none", "noise"])
@pytest.mark.parametrize("w,h,pad,mb,R", T.PREV_CASES)
def test_null_and_arbitrary_prev_fields(w, h, pad, mb, R, what):
    torch = _torch()
    for method in T.METHODS:
        _check(torch, method, M.SAD, (w, h, pad, mb, R), what)


@pytest.mark.parametrize("wgs", ["1", "3"])
@pytest.mark.parametrize("w,h,pad,mb,R", [T.CASES[0], T.CASES[1], (64, 48, 0, 8, 9)])
def test_ticket_rounds(w, h, pad, mb, R, wgs, monkeypatch):
    """9 to 18 block rows (3 pairs of 3 to 6) on one wave and on three: a wave takes row after row in ticket order, and with one wave
    every awaited row is finished before the next begins"""
    torch = _torch()
    monkeypatch.setenv("FFHIP_ME_PRED_WGS", wgs)
    for kind in T.KINDS:
        for method in T.METHODS:
            _check(torch, method, kind, (w, h, pad, mb, R))


def test_a_call_split_into_several_launches():
    """16 x 64 at 8 x 8 has 8 block rows: 1023 pairs fill a progress-pool slot, so 1030 pairs are two launches (1023 + 7); each pair
    has its own content and its own prev fields"""
    torch = _torch()
    nf, w, h, mb, R = 1030, 16, 64, 8, 5
    rng = np.random.default_rng(1030)
    ref = rng.integers(0, 256, (nf, h, w), dtype=np.uint8)
    cur = np.roll(ref, (1, -1), (1, 2))
    cur[::2] = np.roll(ref[::2], (-2, 1), (1, 2))
    origin = np.array([[(bx * mb, by * mb) for bx in range(w // mb)] for by in range(h // mb)], np.int64).reshape(-1)
    p1 = (origin + rng.integers(-4, 5, (nf, origin.size))).astype(np.int16)
    p2 = (origin + rng.integers(-4, 5, (nf, origin.size))).astype(np.int16)
    for method in T.METHODS:
        hmv, hcost, (blocks, _) = T.host_face(method, M.SAD, cur, ref, w, h, mb, R, p1, p2)
        assert blocks == nf * 16
        mv, cost = device_face(torch, method, M.SAD, cur, ref, w, h, mb, R, p1, p2)
        assert np.array_equal(cost, hcost) and np.array_equal(mv, hmv)


@pytest.mark.parametrize("method", T.METHODS, ids=[M.NAMES[m] for m in T.METHODS])
def test_chained_run_of_four_frames_on_one_stream(method):
    """three vector buffers rotated, four calls queued on one stream without a synchronisation in between: prev NULL at first, then
    the run's own earlier outputs"""
    from ffmpeg_amd import me
    torch = _torch()
    pics, want = T.chain()
    d = torch.from_numpy(np.array(pics)).cuda()
    bufs = [torch.full((24,), 0x5A5A, dtype=torch.int16, device="cuda:0") for _ in range(3)]
    costs = [torch.zeros((12,), dtype=torch.int32, device="cuda:0") for _ in range(4)]
    got = []
    for k in range(4):
        p1 = bufs[(k - 1) % 3] if k >= 1 else None
        p2 = bufs[(k - 2) % 3] if k >= 2 else None
        me.search_pred_batch(method, d[k + 1], d[k], 64, 48, 64, 64 * 48, 1, 16, 7, M.SAD, p1, p2, bufs[k % 3], costs[k])
        got.append(bufs[k % 3].clone())         # in stream order, behind the call
    torch.cuda.synchronize()
    for k in range(4):
        wmv, wcost, _ = want[method][k]
        assert np.array_equal(got[k].cpu().numpy(), wmv[0]) and np.array_equal(costs[k].cpu().numpy().view(np.uint32), wcost[0]), k


@functools.lru_cache(maxsize=None)
def _hd_pair():
    rng = np.random.default_rng(1080)
    big = T.texture(rng, 1080 + 32, 1920 + 32)
    ref = np.round(big[16:16 + 1080, 16:16 + 1920]).astype(np.uint8)[None]
    cur = np.clip(np.round(big[16 - 5:16 - 5 + 1080, 16 + 9:16 + 9 + 1920] + rng.integers(-2, 3, (1080, 1920))), 0, 255).astype(np.uint8)[None]
    p1 = rng.integers(-12, 13, (1, 120 * 67 * 2)).astype(np.int16)
    p1 += np.array([[(bx * 16, by * 16) for bx in range(120)] for by in range(67)], np.int16).reshape(1, -1)
    for a in (cur, ref, p1):
        a.setflags(write=False)
    return cur, ref, p1


@pytest.mark.parametrize("method", T.METHODS, ids=[M.NAMES[m] for m in T.METHODS])
def test_1080p_against_the_host_face(method):
    """120 x 67 blocks, the last 8 rows of the picture in no block: 67 rows in flight, each two blocks behind the one above"""
    torch = _torch()
    cur, ref, p1 = _hd_pair()
    hmv, hcost, (blocks, _) = T.host_face(method, M.SAD, cur, ref, 1920, 1080, 16, 16, p1, None)
    assert blocks == 120 * 67
    mv, cost = device_face(torch, method, M.SAD, cur, ref, 1920, 1080, 16, 16, p1, None)
    assert np.array_equal(cost, hcost) and np.array_equal(mv, hmv)


def test_no_frames_and_no_blocks_launch_nothing():
    from ffmpeg_amd import me
    torch = _torch()
    cur = torch.zeros(64 * 48, dtype=torch.uint8, device="cuda:0")
    mv = torch.full((64,), 7, dtype=torch.int16, device="cuda:0")
    cost = torch.full((32,), 7, dtype=torch.int32, device="cuda:0")
    me.search_pred_batch(me.EPZS, cur, cur, 64, 48, 64, 64 * 48, 0, 16, 7, me.SAD, None, None, mv, cost)
    me.search_pred_batch(me.UMH, cur, cur, 15, 48, 64, 64 * 48, 1, 16, 7, me.SAD, None, None, mv, cost)
    with pytest.raises(RuntimeError, match="neither EPZS"):
        me.search_pred_batch(me.DS, cur, cur, 64, 48, 64, 64 * 48, 1, 16, 7, me.SAD, None, None, mv, cost)
    with pytest.raises(RuntimeError, match="overlaps"):
        me.search_pred_batch(me.EPZS, cur, cur, 64, 48, 64, 64 * 48, 1, 16, 7, me.SAD, mv, None, mv, cost)
    torch.cuda.synchronize()
    assert bool((mv == 7).all()) and bool((cost == 7).all())
