"""The predictive motion searches of whole sequences on a caller's stream, with the staged runs of tests/picture_faces.py (imported, not
edited), in the manner of tests/test_gpu_me_search_streams.py: on a created (non-blocking) stream behind a delay with every tensor
poisoned until the stream itself puts the real bytes in place, and behind a busy NULL stream.  The face takes a progress-pool slot per
launch, zeroed in stream order, and reads the fields of earlier pairs back from mv_out while it writes it.  These runs show that nothing
of it leaves the caller's stream."""
import ctypes as C

import numpy as np
import pytest

import me_pred_search_model as M
import picture_faces as PF
import test_me_seq_search_cpu as S

pytestmark = pytest.mark.gpu

WHAT = ["epzs-sad-16", "umh-sad-16", "epzs-satd-8", "umh-satd-8", "epzs-sad-made"]


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _lib():
    from ffmpeg_amd import _lib
    return _lib.lib()


class MeSeqSearch(PF.Face):
    """tests/picture_faces.py's adapter interface: three sequences of six pictures in one call, both starting fields; "made": the
    white-noise sequences that only the chaining solves.  The reference is the chained loop of the existing host face."""
    name = "me_seq_search"

    def __init__(self, what):
        method, kind, mb = what.split("-")
        self.method = {v: k for k, v in M.NAMES.items()}[method]
        self.kind, self.mb = {"sad": M.SAD, "satd": M.SATD}[kind], mb

    def build(self, seed=None):
        if self.mb == "made":
            self.case = S.MADE
            self.frames, self.i1, self.i2, _ = S.made()
        else:
            self.case = (64, 32, 0, 16, 7) if self.mb == "16" else (64, 48, 0, 8, 9)
            self.frames, self.i1, self.i2 = S.pictures(*self.case)
        w, h, _, mb, R = self.case
        self.want = S.chained_host(self.method, self.kind, self.frames, w, h, mb, R, 0, self.i1, self.i2)[:2]
        return self

    def upload(self, torch):
        self.d_frames = torch.from_numpy(np.array(self.frames)).cuda()
        self.d_init = [torch.from_numpy(np.array(p)).cuda() for p in (self.i1, self.i2)]
        self.d_mv = torch.full(self.want[0].shape, 0x5A5A, dtype=torch.int16, device="cuda:0")
        self.d_cost = torch.full(self.want[1].shape, 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")

    def call(self, stream):
        from ffmpeg_amd import me
        w, h, pad, mb, R = self.case
        plane = h * (w + pad)
        me.search_pred_sequence(self.method, self.d_frames, w, h, w + pad, plane, S.NFRAMES, S.NFRAMES * plane, S.NSEQ, 0, mb, R, self.kind,
                                *self.d_init, self.d_mv, self.d_cost, stream=stream)

    def inputs(self):
        return [self.d_frames] + self.d_init

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
    f = MeSeqSearch(what).build()
    view, ins, keep = PF.run_staged(torch, _lib(), stream, [f], delay)
    PF.check_staged(torch, [f], view, ins)


@pytest.mark.parametrize("what", WHAT)
def test_behind_a_busy_null_stream(what, stream, delay):
    torch = _torch()
    f = MeSeqSearch(what).build()
    view, ins, keep = PF.run_staged(torch, _lib(), stream, [f], delay, late=True)
    PF.check_staged(torch, [f], view, ins)
