"""The per-block and the predictive motion searches on a caller's stream, with the staged runs of tests/picture_faces.py (imported, not
edited): on a created (non-blocking) stream behind a delay with every tensor poisoned until the stream itself puts the real bytes in
place, and behind a busy NULL stream.  The per-block search uses no progress pool and leaves nothing on another stream; the predictive
one takes a progress-pool slot per launch, zeroed in stream order, and reads mv_out back while it writes it.  These runs show that
nothing of either leaves the caller's stream."""
import ctypes as C

import numpy as np
import pytest

import me_pred_search_model as MP
import me_search_model as M
import picture_faces as PF
import test_me_pred_search_cpu as TP
import test_me_search_cpu as T

pytestmark = pytest.mark.gpu

WHAT = (["%s-sad-16" % M.NAMES[m] for m in T.METHODS] + ["hexbs-satd-8", "ntss-satd-16"] +
        ["epzs-sad-16", "umh-sad-16", "epzs-satd-8", "umh-satd-8"])


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _lib():
    from ffmpeg_amd import _lib
    return _lib.lib()


class MeSearch(PF.Face):
    """tests/picture_faces.py's adapter interface: three frame pairs of 64 x 48 in one call; EPZS and UMH with both prev fields"""
    name = "me_search"

    def __init__(self, what):
        method, kind, mb = what.split("-")
        self.method = {v: k for k, v in list(M.NAMES.items()) + list(MP.NAMES.items())}[method]
        self.pred = self.method in TP.METHODS
        self.kind, self.mb = {"sad": M.SAD, "satd": M.SATD}[kind], int(mb)

    def build(self, seed=None):
        self.case = (64, 48, 0, self.mb, 9 if self.pred and self.mb == 8 else 7)
        self.cur, self.ref = (TP if self.pred else T).pairs(*self.case)[:2]
        self.prev = TP.prev_fields(*self.case, "made") if self.pred else []
        self.want = (TP if self.pred else T).reference(self.method, self.kind, *self.case)[:2]
        return self

    def upload(self, torch):
        self.d_cur, self.d_ref = torch.from_numpy(np.array(self.cur)).cuda(), torch.from_numpy(np.array(self.ref)).cuda()
        self.d_prev = [torch.from_numpy(np.array(p)).cuda() for p in self.prev]
        self.d_mv = torch.full(self.want[0].shape, 0x5A5A, dtype=torch.int16, device="cuda:0")
        self.d_cost = torch.full(self.want[1].shape, 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")

    def call(self, stream):
        from ffmpeg_amd import me
        w, h, pad, mb, R = self.case
        face = me.search_pred_batch if self.pred else me.search_batch
        face(self.method, self.d_cur, self.d_ref, w, h, w + pad, h * (w + pad), 3, mb, R, self.kind, *self.d_prev, self.d_mv, self.d_cost,
             stream=stream)

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
    f = MeSearch(what).build()
    view, ins, keep = PF.run_staged(torch, _lib(), stream, [f], delay)
    PF.check_staged(torch, [f], view, ins)


@pytest.mark.parametrize("what", WHAT)
def test_behind_a_busy_null_stream(what, stream, delay):
    torch = _torch()
    f = MeSearch(what).build()
    view, ins, keep = PF.run_staged(torch, _lib(), stream, [f], delay, late=True)
    PF.check_staged(torch, [f], view, ins)
