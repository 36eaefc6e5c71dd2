"""The predictive motion searches on a caller's stream, with the staged runs of tests/picture_faces.py (imported, not edited): on a
created (non-blocking) stream behind a delay with every tensor poisoned until the stream itself puts the real bytes in place, and behind
a busy NULL stream.  The search takes a progress-pool slot per launch, zeroed in stream order, and reads mv_out back while it writes it;
these runs show that nothing of that leaves the caller's stream."""
import ctypes as C

import numpy as np
import pytest

import me_pred_search_model as M
import picture_faces as PF
import test_me_pred_search_cpu as T

pytestmark = pytest.mark.gpu

WHAT = ["epzs-sad-16", "umh-sad-16", "epzs-satd-8", "umh-satd-8"]


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _lib():
    from ffmpeg_amd import _lib
    return _lib.lib()


class MePredSearch(PF.Face):
    """tests/picture_faces.py's adapter interface: three frame pairs of 64 x 48 in one call, with both prev fields"""
    name = "me_pred_search"

    def __init__(self, what):
        method, kind, mb = what.split("-")
        self.method = {v: k for k, v in M.NAMES.items()}[method]
        self.kind, self.mb = {"sad": M.SAD, "satd": M.SATD}[kind], int(mb)

    def build(self, seed=None):
        self.case = (64, 48, 0, self.mb, 7 if self.mb == 16 else 9)
        self.cur, self.ref, _ = T.pairs(*self.case)
        self.prev = T.prev_fields(*self.case, "made")
        self.want = T.reference(self.method, self.kind, *self.case)[:2]
        return self

    def upload(self, torch):
        self.d_cur, self.d_ref = torch.from_numpy(np.array(self.cur)).cuda(), torch.from_numpy(np.array(self.ref)).cuda()
        self.d_prev = [torch.from_numpy(np.array(p)).cuda() for p in self.prev]
        self.d_mv = torch.full(self.want[0].shape, 0x5A5A, dtype=torch.int16, device="cuda:0")
        self.d_cost = torch.full(self.want[1].shape, 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")

    def call(self, stream):
        from ffmpeg_amd import me
        w, h, pad, mb, R = self.case
        me.search_pred_batch(self.method, self.d_cur, self.d_ref, w, h, w + pad, h * (w + pad), T.NF, mb, R, self.kind, self.d_prev[0],
                             self.d_prev[1], self.d_mv, self.d_cost, stream=stream)

    def inputs(self):
        return [self.d_cur, self.d_ref] + self.d_prev

    def outputs(self):
        return [self.d_mv, self.d_cost]

    def compare(self, view=lambda t: t):
        assert np.array_equal(view(self.d_cost).cpu().numpy().view(np.uint32), self.want[1]), self.name
        assert np.array_equal(view(self.d_mv).cpu().numpy(), self.want[0]), self.name


@pytest.fixture(scope="module")
def delay():
    return PF.Delay(_torch())


@pytest.fixture
def stream():
    L = _lib()
    assert L.ffhip_set_device(0) == 0
    st = C.c_void_p()
    assert L.ffhip_stream_create(C.byref(st)) == 0, L.ffhip_last_error()
    yield st
    assert L.ffhip_stream_destroy(st) == 0


@pytest.mark.parametrize("what", WHAT)
def test_on_a_created_stream(what, stream, delay):
    torch = _torch()
    f = MePredSearch(what).build()
    view, ins, keep = PF.run_staged(torch, _lib(), stream, [f], delay)
    PF.check_staged(torch, [f], view, ins)


@pytest.mark.parametrize("what", WHAT)
def test_behind_a_busy_null_stream(what, stream, delay):
    torch = _torch()
    f = MePredSearch(what).build()
    view, ins, keep = PF.run_staged(torch, _lib(), stream, [f], delay, late=True)
    PF.check_staged(torch, [f], view, ins)
