"""The VP9 loop-filter table face and its chain into the loop-filter faces on a caller's stream, with the staged runs of
tests/picture_faces.py (imported, not edited): on a created (non-blocking) stream behind a delay with every tensor poisoned until the
stream itself puts the real bytes in place, and behind a busy NULL stream with every progress-pool slot dirtied by a decoy."""
import ctypes as C

import pytest

import picture_faces as PF
import test_gpu_vp9_lf_tables as T

pytestmark = pytest.mark.gpu

SEED = 9840
WHAT = ["face", "chain420_8", "chain420_10", "chain422_8"]


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _lib():
    from ffmpeg_amd import _lib
    return _lib.lib()


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
    if what == "face":
        return T.Face().build(SEED)
    return T.Chain(10 if what.endswith("_10") else 8, (1, 0) if "422" in what else (1, 1)).build()


@pytest.mark.parametrize("what", WHAT)
def test_on_a_created_stream(what, stream, delay):
    torch = _torch()
    f = _make(what)
    view, ins, keep = PF.run_staged(torch, _lib(), stream, [f], delay)
    PF.check_staged(torch, [f], view, ins)


@pytest.mark.parametrize("what", WHAT)
def test_behind_a_busy_null_stream(what, stream, delay):
    torch = _torch()
    f = _make(what)
    view, ins, keep = PF.run_staged(torch, _lib(), stream, [f], delay, late=True)
    PF.check_staged(torch, [f], view, ins)
