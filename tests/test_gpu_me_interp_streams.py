"""vf_minterpolate's compensation on a caller's stream, with the staged runs of tests/picture_faces.py (imported, not edited), in the
manner of tests/test_gpu_me_seq_search_streams.py: on a created (non-blocking) stream behind a delay with every tensor poisoned until
the stream itself puts the real bytes in place, behind a busy NULL stream with every pool slot dirtied, and as the first call a fresh
process makes into the library.  The face sends its window table and its jobs in a progress-pool slot, in stream order: these runs show
that neither that copy nor the kernel leaves the caller's stream."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import me_interp_cases as K
import me_interp_model as M
import picture_faces as PF

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WHAT = ["mb16-420", "mb8-444", "mb16-luma"]
#: seconds; tests/test_gpu_picture_streams.py's bound for a child of the same kind (nearly all of it is the start of a process with torch)
CHILD_TIMEOUT = 9


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _lib():
    from ffmpeg_amd import _lib
    return _lib.lib()


class MeInterp(PF.Face):
    """tests/picture_faces.py's adapter interface: jobs of both modes over 2 sequences of 3 pictures in one call.  The reference is the
    host face, which tests/test_me_interp_cpu.py pins to the model."""
    name = "me_interp"

    def __init__(self, what):
        self.what = what

    def build(self, seed=None):
        mb, fmt = self.what.split("-")
        chroma = {"420": (1, 1), "444": (0, 0), "luma": None}[fmt]
        jobs = [(j % 2, (j // 2) % 2, (j * 211) % 1025, M.BLEND if j % 5 == 2 else M.MCI) for j in range(10)]
        self.c = K.Call("streams-" + self.what, 72, 40, int(mb[2:]), chroma, "random", "ramp", jobs, R=16, nseq=2, nframes=3, seed=21)
        self.want = self.c.host()[0]
        return self

    def upload(self, torch):
        c = self.c
        self.d_src = [torch.from_numpy(b.a).cuda() for b in c.src]
        self.d_fields = [torch.from_numpy(b.a).cuda() for b in c.fields]
        self.d_dst = [torch.from_numpy(b.a).cuda() for b in c.dst]

    def call(self, stream):
        from ffmpeg_amd import me
        me.interp_sequence(*self.c.args(me, [t.data_ptr() for t in self.d_src], [t.data_ptr() for t in self.d_dst],
                                        [t.data_ptr() for t in self.d_fields]), stream=stream)

    def inputs(self):
        return self.d_src + self.d_fields

    def outputs(self):
        return self.d_dst

    def compare(self, view=lambda t: t):
        for i, t in enumerate(self.d_dst):
            assert np.array_equal(view(t).cpu().numpy(), self.want[i]), "%s plane %d" % (self.name, i)


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
    f = MeInterp(what).build()
    view, ins, keep = PF.run_staged(torch, _lib(), stream, [f], delay)
    PF.check_staged(torch, [f], view, ins)


@pytest.mark.parametrize("what", WHAT)
def test_behind_a_busy_null_stream(what, stream, delay):
    torch = _torch()
    f = MeInterp(what).build()
    view, ins, keep = PF.run_staged(torch, _lib(), stream, [f], delay, late=True)
    PF.check_staged(torch, [f], view, ins)


def test_first_use_on_a_created_stream():
    """the creation of the progress pool and the first launch under a non-blocking stream: a fresh child process (never an exec of this
    one, which holds the GPU)"""
    r = subprocess.run([sys.executable, os.path.join(HERE, "me_interp_stream_child.py")] + WHAT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=CHILD_TIMEOUT)
    assert r.returncode == 0, "me_interp_stream_child.py exited with %d:\n%s" % (r.returncode, r.stdout)
    assert "%d faces ok" % len(WHAT) in r.stdout, r.stdout
