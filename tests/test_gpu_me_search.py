"""GPU tier of the filter's per-block motion searches: ffhip_me_search_batch_dev == ffhip_me_search_frames_host == the model of
tests/me_search_model.py, on the inputs and references of tests/test_me_search_cpu.py (computed once, shared); method 1 == the
exhaustive face byte for byte; one 1920 x 1080 pair per method against the host face (more blocks than waves stay resident, and
b_h * mb < height); and the grid-stride loop on a small picture, with the number of workgroups fixed by the measurement build's knob."""
import functools

import numpy as np
import pytest

import me_search_model as M
import test_me_search_cpu as T
from test_gpu_me import _shifted_pair

pytestmark = pytest.mark.gpu

NG = 4096           # guard bytes on each side of every device buffer
GUARD = 0xA5


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


class Guarded:
    """a device copy of `a` between two runs of guard bytes; .t is the tensor to pass"""

    def __init__(self, torch, a):
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        self.buf = torch.full((raw.size + 2 * NG,), GUARD, dtype=torch.uint8, device="cuda:0")
        self.t = self.buf[NG:NG + raw.size]
        self.t.copy_(torch.from_numpy(raw.copy()))
        self.before, self.dtype, self.shape = raw.copy(), a.dtype, a.shape

    def host(self):
        return self.t.cpu().numpy().view(self.dtype).reshape(self.shape)

    def guards_intact(self):
        return bool((self.buf[:NG] == GUARD).all()) and bool((self.buf[-NG:] == GUARD).all())

    def unchanged(self):
        return self.guards_intact() and np.array_equal(self.t.cpu().numpy(), self.before)


def device_face(torch, method, kind, cur, ref, w, h, mb, R, face=None):
    """the device face on guarded buffers -> mv, cost; asserts that nothing outside the outputs changed"""
    from ffmpeg_amd import me
    nf, _, stride = cur.shape
    bw, bh = w // mb, h // mb
    gc, gr = Guarded(torch, cur), Guarded(torch, ref)
    gm, gk = Guarded(torch, np.full((nf, bh * bw * 2), 0x5A5A, np.int16)), Guarded(torch, np.full((nf, bh * bw), 0x5A5A5A5A, np.uint32))
    if face is None:
        me.search_batch(method, gc.t, gr.t, w, h, stride, h * stride, nf, mb, R, kind, gm.t, gk.t)
    else:
        face(gc.t, gr.t, w, h, stride, h * stride, nf, mb, R, kind, gm.t, gk.t)
    torch.cuda.synchronize()
    assert gc.unchanged() and gr.unchanged() and gm.guards_intact() and gk.guards_intact()
    return gm.host(), gk.host()


@pytest.mark.parametrize("kind", T.KINDS, ids=["sad", "satd"])
@pytest.mark.parametrize("w,h,pad,mb,R", T.CASES)
def test_device_equals_host_equals_model(w, h, pad, mb, R, kind):
    torch = _torch()
    cur, ref = T.pairs(w, h, pad, mb, R)
    for method in T.METHODS:
        wmv, wcost, _, _ = T.reference(method, kind, w, h, pad, mb, R)
        hmv, hcost, _ = T.host_face(method, kind, cur, ref, w, h, mb, R)
        assert np.array_equal(hcost, wcost) and np.array_equal(hmv, wmv), M.NAMES[method]
        mv, cost = device_face(torch, method, kind, cur, ref, w, h, mb, R)
        assert np.array_equal(cost, wcost), M.NAMES[method]
        assert np.array_equal(mv, wmv), M.NAMES[method]


@pytest.mark.parametrize("kind", T.KINDS, ids=["sad", "satd"])
@pytest.mark.parametrize("w,h,pad,mb,R", T.CASES)
def test_method_1_is_the_exhaustive_face(w, h, pad, mb, R, kind):
    from ffmpeg_amd import me
    torch = _torch()
    cur, ref = T.pairs(w, h, pad, mb, R)
    mv, cost = device_face(torch, M.ESA, kind, cur, ref, w, h, mb, R)
    emv, ecost = device_face(torch, M.ESA, kind, cur, ref, w, h, mb, R, face=me.esa_batch)
    assert mv.tobytes() == emv.tobytes() and cost.tobytes() == ecost.tobytes()


@functools.lru_cache(maxsize=None)
def _hd_pair():
    cur, ref, _, _ = _shifted_pair(np.random.default_rng(1080), 1920, 1080, 1920, 16)
    cur, ref = cur[None], ref[None]
    cur.setflags(write=False)
    ref.setflags(write=False)
    return cur, ref


@pytest.mark.parametrize("method", T.METHODS, ids=[M.NAMES[m] for m in T.METHODS])
def test_1080p_against_the_host_face(method):
    """120 x 67 blocks, the last 8 rows of the picture in no block"""
    torch = _torch()
    cur, ref = _hd_pair()
    hmv, hcost, (blocks, _) = T.host_face(method, M.SAD, cur, ref, 1920, 1080, 16, 16)
    assert blocks == 120 * 67
    mv, cost = device_face(torch, method, M.SAD, cur, ref, 1920, 1080, 16, 16)
    assert np.array_equal(cost, hcost) and np.array_equal(mv, hmv)


@pytest.mark.parametrize("wgs", ["1", "3"])
@pytest.mark.parametrize("w,h,pad,mb,R", [T.CASES[0], T.CASES[1]])
def test_grid_stride_rounds(w, h, pad, mb, R, wgs, monkeypatch):
    """36 blocks (16x16) and 144 blocks (8x8) on 4 and on 12 waves: every wave takes several blocks, the last round is ragged"""
    torch = _torch()
    monkeypatch.setenv("FFHIP_ME_SEARCH_WGS", wgs)
    cur, ref = T.pairs(w, h, pad, mb, R)
    for kind in T.KINDS:
        for method in T.METHODS[1:]:
            wmv, wcost, _, _ = T.reference(method, kind, w, h, pad, mb, R)
            mv, cost = device_face(torch, method, kind, cur, ref, w, h, mb, R)
            assert np.array_equal(cost, wcost) and np.array_equal(mv, wmv), (M.NAMES[method], kind)


def test_no_frames_and_no_blocks_launch_nothing():
    from ffmpeg_amd import me
    torch = _torch()
    cur = torch.zeros(64 * 48, dtype=torch.uint8, device="cuda:0")
    mv = torch.full((64,), 7, dtype=torch.int16, device="cuda:0")
    cost = torch.full((32,), 7, dtype=torch.int32, device="cuda:0")
    me.search_batch(me.DS, cur, cur, 64, 48, 64, 64 * 48, 0, 16, 7, me.SAD, mv, cost)
    me.search_batch(me.DS, cur, cur, 15, 48, 64, 64 * 48, 1, 16, 7, me.SAD, mv, cost)
    with pytest.raises(RuntimeError, match="EPZS"):
        me.search_batch(me.EPZS, cur, cur, 64, 48, 64, 64 * 48, 1, 16, 7, me.SAD, mv, cost)
    torch.cuda.synchronize()
    assert bool((mv == 7).all()) and bool((cost == 7).all())
