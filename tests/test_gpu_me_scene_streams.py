"""Frame-rate conversion as four calls on a caller's stream with nothing read back — search forward, search backward, scene detection,
interpolation with the flags — with the staged runs of tests/picture_faces.py (imported, not edited), in the manner of
tests/test_gpu_me_interp_streams.py: on a created (non-blocking) stream behind a delay with every tensor poisoned until the stream itself
puts the real bytes in place, behind a busy NULL stream with every pool slot dirtied, and as the first calls a fresh process makes into
the library.  The detection zeroes its sums in a progress-pool slot in stream order and the interpolation reads the flags the detection
wrote: these runs show that nothing of that leaves the caller's stream.

The sequence has one hard cut: a moving texture of small amplitude plus a flat level that jumps once, so that at threshold 10 the cut
pair alone is flagged.  The reference is the same pipeline on the host faces."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import me_interp_cases as K
import picture_faces as PF

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WHAT = ["blend", "dup"]
#: seconds; tests/test_gpu_picture_streams.py's bound for a child of the same kind (nearly all of it is the start of a process with torch)
CHILD_TIMEOUT = 9
W, H, MB, R, N, CUT = 64, 48, 16, 8, 6, 3       # pictures 0..2 at one level, 3..5 at the other
THRESHOLD = 10.0


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _lib():
    from ffmpeg_amd import _lib
    return _lib.lib()


class MeScenePipeline(PF.Face):
    """tests/picture_faces.py's adapter interface over the four calls"""
    name = "me_scene_pipeline"

    def __init__(self, what):
        self.what = what

    def build(self, seed=None):
        from ffmpeg_amd import me
        self.action = {"blend": me.SCENE_BLEND, "dup": me.SCENE_DUP}[self.what]
        rng = np.random.default_rng(31)
        base = rng.integers(0, 32, (H + 16, W + 16), dtype=np.uint8)
        self.frames = np.stack([base[8 + p:8 + p + H, 8 - p:8 - p + W] + (20 if p < CUT else 140) for p in range(N)]).astype(np.uint8).copy()
        self.per = (W // MB) * (H // MB)
        self.jobs = [(0, k, a, me.MCI) for k in range(N - 1) for a in (341, 683)]
        self.window = K.window("ramp", MB)
        mv = [np.zeros((N - 1) * self.per * 2, np.int16) for _ in range(2)]
        cost = [np.zeros((N - 1) * self.per, np.uint32) for _ in range(2)]
        for d in range(2):
            me.search_pred_sequence_host(me.EPZS, self.frames, W, H, W, W * H, N, N * W * H, 1, d, MB, R, me.SAD, None, None, mv[d], cost[d])
        flags = np.full(N - 1, 9, np.uint8)
        me.scene_sequence_host(self.frames, 8, W, H, W, W * H, N, N * W * H, 1, THRESHOLD, flags_out=flags)
        assert list(flags) == [int(k == CUT - 1) for k in range(N - 1)], flags
        out = np.zeros((len(self.jobs), H, W), np.uint8)
        counts = me.interp_sequence_scd_host(me.planes([self.frames], [W], [W * H], [N * W * H]), me.planes([out], [W], [W * H]), 1, 0, 0, W, H, N, 1,
                                             MB, R, self.window, mv[0], mv[1], self.jobs, flags, self.action)
        assert counts["taken"] > 0 and counts["blend"] == 2 * W * H
        self.want = mv + cost + [flags, out]
        return self

    def upload(self, torch):
        self.d_frames = torch.from_numpy(self.frames).cuda()
        self.d_out = [torch.zeros(w.shape, dtype={"int16": torch.int16, "uint32": torch.int32, "uint8": torch.uint8}[w.dtype.name], device="cuda:0")
                      for w in self.want]

    def call(self, stream):
        from ffmpeg_amd import me
        mv0, mv1, cost0, cost1, flags, out = self.d_out
        for d, (mv, cost) in enumerate(((mv0, cost0), (mv1, cost1))):
            me.search_pred_sequence(me.EPZS, self.d_frames, W, H, W, W * H, N, N * W * H, 1, d, MB, R, me.SAD, None, None, mv, cost, stream=stream)
        me.scene_sequence(self.d_frames, 8, W, H, W, W * H, N, N * W * H, 1, THRESHOLD, flags_out=flags, stream=stream)
        me.interp_sequence_scd(me.planes([self.d_frames], [W], [W * H], [N * W * H]), me.planes([out], [W], [W * H]), 1, 0, 0, W, H, N, 1, MB, R,
                               self.window, mv0, mv1, self.jobs, flags, self.action, stream=stream)

    def inputs(self):
        return [self.d_frames]

    def outputs(self):
        return list(self.d_out)

    def compare(self, view=lambda t: t):
        for i, (t, w) in enumerate(zip(self.d_out, self.want)):
            got = view(t).cpu().numpy().view(w.dtype).reshape(w.shape)
            assert np.array_equal(got, w), "%s %s: output %d differs" % (self.name, self.what, i)


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
    f = MeScenePipeline(what).build()
    view, ins, keep = PF.run_staged(torch, _lib(), stream, [f], delay)
    PF.check_staged(torch, [f], view, ins)


@pytest.mark.parametrize("what", WHAT)
def test_behind_a_busy_null_stream(what, stream, delay):
    torch = _torch()
    f = MeScenePipeline(what).build()
    view, ins, keep = PF.run_staged(torch, _lib(), stream, [f], delay, late=True)
    PF.check_staged(torch, [f], view, ins)


def test_first_use_on_a_created_stream():
    """the creation of the progress pool and the first launches under a non-blocking stream: a fresh child process (never an exec of this
    one, which holds the GPU)"""
    r = subprocess.run([sys.executable, os.path.join(HERE, "me_scene_stream_child.py")] + WHAT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=CHILD_TIMEOUT)
    assert r.returncode == 0, "me_scene_stream_child.py exited with %d:\n%s" % (r.returncode, r.stdout)
    assert "%d faces ok" % len(WHAT) in r.stdout, r.stdout
