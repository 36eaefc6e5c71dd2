"""The bilateral motion search on a caller's stream, with the staged runs of tests/picture_faces.py (imported, not edited), in the manner
of tests/test_gpu_me_seq_search_streams.py: on a created (non-blocking) stream behind a delay with every tensor poisoned until the
stream itself puts the real bytes in place, behind a busy NULL stream, and as the first use of the library in a fresh child process.
The faces take a progress-pool slot per launch, zeroed in stream order, and read the fields of earlier rows and pairs back from mv_out
while they write it.  These runs show that nothing of it leaves the caller's stream."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import me_bilat_model as M
import picture_faces as PF
import test_me_bilat_search_cpu as B

pytestmark = pytest.mark.gpu

WHAT = ["epzs-seq-16", "umh-seq-8", "epzs-pairs-8", "umh-pairs-16"]


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _lib():
    from ffmpeg_amd import _lib
    return _lib.lib()


class MeBilatSearch(PF.Face):
    """tests/picture_faces.py's adapter interface: three sequences of four pictures in one call of the sequence face, or their first
    pairs in one call of the pair face, both starting fields given.  The reference is the model's (== the host face's: CPU tier)."""
    name = "me_bilat_search"

    def __init__(self, what):
        method, self.face, mb = what.split("-")
        self.what = what
        self.method = {v: k for k, v in M.NAMES.items()}[method]
        self.mb = int(mb)
        self.shape = B.SHAPES[1] if self.mb == 16 else B.SHAPES[2]

    def build(self, seed=None):
        self.pics, fields = B.sequences(*self.shape, self.mb)
        self.i1, self.i2 = fields["made"]
        ref = B.sequence_reference if self.face == "seq" else B.pair_reference
        self.want = ref(self.method, self.shape, self.mb, 32, "made")[:2]
        return self

    def upload(self, torch):
        self.d_pics = torch.from_numpy(np.array(self.pics)).cuda()
        self.d_init = [torch.from_numpy(np.array(p)).cuda() for p in (self.i1, self.i2)]
        self.d_mv = torch.full(self.want[0].shape, 0x5A5A, dtype=torch.int16, device="cuda:0")
        self.d_cost = torch.full(self.want[1].shape, 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")

    def call(self, stream):
        from ffmpeg_amd import me
        w, h, stride = B.geometry(*self.shape, self.mb)
        plane = h * stride
        if self.face == "seq":
            me.search_bilat_sequence(self.method, self.d_pics, w, h, stride, plane, B.NFRAMES, B.NFRAMES * plane, B.NSEQ, self.mb, 32, *self.d_init,
                                     self.d_mv, self.d_cost, stream=stream)
        else:       # pictures 0 and 1 of every sequence: the pairs are a sequence's pictures apart
            me.search_bilat_batch(self.method, self.d_pics.data_ptr(), self.d_pics.data_ptr() + plane, w, h, stride, B.NFRAMES * plane, B.NSEQ, self.mb,
                                  32, *self.d_init, self.d_mv, self.d_cost, stream=stream)

    def inputs(self):
        return [self.d_pics] + self.d_init

    def outputs(self):
        return [self.d_mv, self.d_cost]

    def compare(self, view=lambda t: t):
        assert np.array_equal(view(self.d_cost).cpu().numpy().view(np.uint32), self.want[1]), self.what
        assert np.array_equal(view(self.d_mv).cpu().numpy(), self.want[0]), self.what


class BilatPipeline(PF.Face):
    """a whole conversion under me_mode=bilat as one face: search, scene detection, bilateral interpolation with the flags, three calls
    queued on the caller's stream with nothing in between.  5 pictures of 64 x 48 with a cut before the fourth, two instants per pair;
    the reference is the same three calls of the host faces."""
    name = "me_bilat_pipeline"
    W, H, MB, R, N = 64, 48, 16, 16, 5

    def build(self, seed=None):
        from ffmpeg_amd import me
        import me_interp_cases as K
        W, H, mb, R, n = self.W, self.H, self.MB, self.R, self.N
        self.per = (W // mb) * (H // mb)
        rng = np.random.default_rng(23)
        base = [B.texture(rng, H + 16, W + 16).astype(np.uint8) for _ in range(2)]
        self.frames = np.stack([base[p >= 3][8 + p:8 + p + H, 8 - p:8 - p + W] for p in range(n)]).copy()      # a pan, a cut, a pan
        self.jobs = [(0, k, a, me.MCI) for k in range(n - 1) for a in (341, 683)]
        self.window = K.window("ramp", mb)
        self.mv, self.cost = np.zeros((n - 1) * self.per * 2, np.int16), np.zeros((n - 1) * self.per, np.uint32)
        me.search_bilat_sequence_host(me.EPZS, self.frames, W, H, W, W * H, n, n * W * H, 1, mb, R, None, None, self.mv, self.cost)
        self.flags = np.zeros(n - 1, np.uint8)
        me.scene_sequence_host(self.frames, 8, W, H, W, W * H, n, n * W * H, 1, 8.0, flags_out=self.flags)
        assert self.flags.tolist() == [0, 0, 1, 0]
        self.want = np.zeros((len(self.jobs), H, W), np.uint8)
        me.interp_bilat_sequence_host(me.planes([self.frames], [W], [W * H], [n * W * H]), me.planes([self.want], [W], [W * H]), 1, 0, 0, W, H, n, 1, mb, R,
                                      self.window, self.mv, self.jobs, self.flags, me.SCENE_DUP)
        assert me.interp_host_counts()["taken"] > 0 and me.interp_host_counts()["blend"] > 0
        return self

    def upload(self, torch):
        n = self.N
        self.d_frames = torch.from_numpy(self.frames).cuda()
        self.d_mv = torch.full(((n - 1) * self.per * 2,), 0x5A5A, dtype=torch.int16, device="cuda:0")
        self.d_cost = torch.full(((n - 1) * self.per,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
        self.d_flags = torch.full((n - 1,), 0x5A, dtype=torch.uint8, device="cuda:0")
        self.d_out = torch.full(self.want.shape, 0x5A, dtype=torch.uint8, device="cuda:0")

    def call(self, stream):
        from ffmpeg_amd import me
        W, H, mb, R, n = self.W, self.H, self.MB, self.R, self.N
        me.search_bilat_sequence(me.EPZS, self.d_frames, W, H, W, W * H, n, n * W * H, 1, mb, R, None, None, self.d_mv, self.d_cost, stream=stream)
        me.scene_sequence(self.d_frames, 8, W, H, W, W * H, n, n * W * H, 1, 8.0, flags_out=self.d_flags, stream=stream)
        me.interp_bilat_sequence(me.planes([self.d_frames], [W], [W * H], [n * W * H]), me.planes([self.d_out], [W], [W * H]), 1, 0, 0, W, H, n, 1, mb, R,
                                 self.window, self.d_mv, self.jobs, self.d_flags, me.SCENE_DUP, stream=stream)

    def inputs(self):
        return [self.d_frames]

    def outputs(self):
        return [self.d_mv, self.d_cost, self.d_flags, self.d_out]

    def compare(self, view=lambda t: t):
        assert np.array_equal(view(self.d_mv).cpu().numpy(), self.mv), self.name
        assert np.array_equal(view(self.d_cost).cpu().numpy().view(np.uint32), self.cost), self.name
        assert np.array_equal(view(self.d_flags).cpu().numpy(), self.flags), self.name
        assert np.array_equal(view(self.d_out).cpu().numpy(), self.want), self.name


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
    f = MeBilatSearch(what).build()
    view, ins, keep = PF.run_staged(torch, _lib(), stream, [f], delay)
    PF.check_staged(torch, [f], view, ins)


@pytest.mark.parametrize("what", WHAT)
def test_behind_a_busy_null_stream(what, stream, delay):
    torch = _torch()
    f = MeBilatSearch(what).build()
    view, ins, keep = PF.run_staged(torch, _lib(), stream, [f], delay, late=True)
    PF.check_staged(torch, [f], view, ins)


@pytest.mark.parametrize("late", (False, True), ids=["on-a-created-stream", "behind-a-busy-null-stream"])
def test_search_detection_interpolation_on_one_stream(late, stream, delay):
    torch = _torch()
    f = BilatPipeline().build()
    view, ins, keep = PF.run_staged(torch, _lib(), stream, [f], delay, late=late)
    PF.check_staged(torch, [f], view, ins)


def test_first_use_in_a_fresh_process():
    """the library's first calls in a new process create a stream and run the bilateral faces on it"""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "me_bilat_stream_child.py")
    r = subprocess.run([sys.executable, child] + WHAT[:2], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "2 faces ok" in r.stdout, r.stdout
