"""The H.264 whole-picture residual face, and the chain from the inter prediction through it into the edge parameters and the in-loop
filter, on a caller's stream, with the staged runs of tests/picture_faces.py (imported, not edited): on a created (non-blocking)
stream behind a delay with every tensor poisoned until the stream itself puts the real bytes in place, and behind a busy NULL stream
with every progress-pool slot dirtied by a decoy."""
import ctypes as C

import pytest

import picture_faces as PF
import test_gpu_h264_res_picture as T

pytestmark = pytest.mark.gpu

SEED = 9820


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _lib():
    from ffmpeg_amd import _lib
    return _lib.lib()


class H264ResidualPictures(T.Face, PF.Face):
    """tests/picture_faces.py's adapter interface on the face's own adapter: two pictures of 5 x 4 macroblocks in one call"""


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


def _make(what):
    return T.Chain(int(what[5:])).build() if what.startswith("chain") else H264ResidualPictures(int(what)).build(SEED)


@pytest.mark.parametrize("what", ["8", "10", "chain8", "chain10"])
def test_on_a_created_stream(what, stream, delay):
    torch = _torch()
    f = _make(what)
    view, ins, keep = PF.run_staged(torch, _lib(), stream, [f], delay)
    PF.check_staged(torch, [f], view, ins)


@pytest.mark.parametrize("what", ["8", "10", "chain8", "chain10"])
def test_behind_a_busy_null_stream(what, stream, delay):
    torch = _torch()
    f = _make(what)
    view, ins, keep = PF.run_staged(torch, _lib(), stream, [f], delay, late=True)
    PF.check_staged(torch, [f], view, ins)
