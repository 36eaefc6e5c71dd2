"""vf_minterpolate's compensation on the device: ffhip_me_interp_sequence_dev() (k_me_interp, kernels/me_interp.hip) against the host
face and the model, byte for byte, guards included, over the calls of tests/me_interp_cases.py; many jobs in one launch, the same jobs
in two calls, a job count beyond one launch's table, 1080p against the host face (which the small shapes pin to the model), and the
all-device pipeline search forward, search backward, interpolation on one created stream against the same pipeline on the host."""
import ctypes as C

import numpy as np
import pytest

import me_interp_cases as K
import me_interp_model as M

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _lib():
    from ffmpeg_amd import _lib
    return _lib.lib()


def run_dev(c, parts=None, stream=None):
    """the call on the device, its jobs in the given slices (one call each, in order); returns the output buffers"""
    torch = _torch()
    from ffmpeg_amd import me
    src = [torch.from_numpy(b.a).cuda() for b in c.src]
    fields = [torch.from_numpy(b.a).cuda() for b in c.fields]
    dst = [torch.from_numpy(b.a).cuda() for b in c.dst]
    torch.cuda.synchronize()
    for lo, hi in parts or [(0, len(c.jobs))]:
        a = list(c.args(me, [t.data_ptr() for t in src], [t.data_ptr() + lo * c.dpitch[i] for i, t in enumerate(dst)],
                        [t.data_ptr() for t in fields]))
        a[-1] = c.jobs[lo:hi]
        me.interp_sequence(*a, stream=stream)
    torch.cuda.synchronize()
    for t, b in zip(src + fields, c.src + c.fields):
        assert np.array_equal(t.cpu().numpy(), b.a), "%s: the device changed an input" % c.name
    return [t.cpu().numpy() for t in dst]


def same(c, got, want):
    c.check_guards(got)
    for i in range(c.nplanes):
        bad = np.flatnonzero(got[i] != want[i])
        assert bad.size == 0, "%s: plane %d: %d bytes differ, first at buffer offset %d" % (c.name, i, bad.size, bad[0])


@pytest.mark.parametrize("name", K.NAMES)
def test_device_equals_host_equals_model(name):
    c = K.calls()[name]
    bufs, _ = c.host()
    want, _ = c.model()
    for j in range(len(c.jobs)):
        for got, ref in zip(c.output(j, bufs), want[j]):
            assert np.array_equal(got, ref)
    same(c, run_dev(c), bufs)


@pytest.fixture(scope="module")
def many():
    """64 jobs over 3 sequences of 4 pictures: every pair several times, both modes"""
    jobs = [(j % 3, (j // 3) % 3, (j * 37) % 1025, M.BLEND if j % 7 == 3 else M.MCI) for j in range(64)]
    return K.Call("64-jobs", 52, 38, 8, (1, 1), "random", "ramp", jobs, R=12, nseq=3, nframes=4, seed=7)


def test_64_jobs_over_3_sequences_in_one_launch(many):
    same(many, run_dev(many), many.host()[0])


def test_the_same_jobs_in_two_calls_on_one_stream(many):
    same(many, run_dev(many, parts=[(0, 23), (23, 64)]), many.host()[0])


def test_more_jobs_than_one_launch_holds():
    """a launch's table holds 1024 jobs: 1030 make the launcher split"""
    jobs = [(0, 0, j % 1025, M.BLEND if j % 5 == 4 else M.MCI) for j in range(1030)]
    c = K.Call("1030-jobs", 24, 16, 8, None, "random", "holes", jobs, R=8, seed=8)
    same(c, run_dev(c), c.host()[0])


@pytest.mark.parametrize("mb", [16, 8])
def test_1080p(mb):
    c = K.Call("1080p-mb%d" % mb, 1920, 1080, mb, (1, 1), "random", "ramp", [(0, 0, 341, M.MCI)], R=32, seed=mb)
    same(c, run_dev(c), c.host()[0])


def test_the_pipeline_on_one_created_stream():
    """search forward, search backward, interpolation with two alphas per pair: EPZS, 5 pictures of 64 x 48, nothing but the created
    stream orders the three calls"""
    torch = _torch()
    from ffmpeg_amd import me
    L = _lib()
    W, H, mb, R, n = 64, 48, 16, 8, 5
    per = (W // mb) * (H // mb)
    rng = np.random.default_rng(11)
    base = rng.integers(0, 256, (H + 16, W + 16), dtype=np.uint8)
    frames = np.stack([base[8 + p:8 + p + H, 8 - p:8 - p + W] for p in range(n)]).copy()        # a pan
    frames[:, 10:20, 30:40] = rng.integers(0, 256, (n, 10, 10), dtype=np.uint8)               # and something the search cannot follow
    jobs = [(0, k, a, me.MCI) for k in range(n - 1) for a in (341, 683)]
    window = K.window("ramp", mb)
    # the host pipeline
    mv = [np.zeros((n - 1) * per * 2, np.int16) for _ in range(2)]
    for d in range(2):
        me.search_pred_sequence_host(me.EPZS, frames, W, H, W, W * H, n, n * W * H, 1, d, mb, R, me.SAD, None, None, mv[d],
                                     np.zeros((n - 1) * per, np.uint32))
    want = np.zeros((len(jobs), H, W), np.uint8)
    me.interp_sequence_host(me.planes([frames], [W], [W * H], [n * W * H]), me.planes([want], [W], [W * H]), 1, 0, 0, W, H, n, 1, mb, R,
                            window, mv[0], mv[1], jobs)
    assert me.interp_host_counts()["taken"] > 0
    # the device pipeline
    assert L.ffhip_set_device(0) == 0
    st = C.c_void_p()
    assert L.ffhip_stream_create(C.byref(st)) == 0, L.ffhip_last_error()
    try:
        d_frames = torch.from_numpy(frames).cuda()
        d_mv = [torch.full(((n - 1) * per * 2,), 0x5A5A, dtype=torch.int16, device="cuda:0") for _ in range(2)]
        d_cost = torch.zeros((n - 1) * per, dtype=torch.int32, device="cuda:0")
        d_out = torch.full((len(jobs), H, W), 0x5A, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        for d in range(2):
            me.search_pred_sequence(me.EPZS, d_frames, W, H, W, W * H, n, n * W * H, 1, d, mb, R, me.SAD, None, None, d_mv[d], d_cost,
                                    stream=st.value)
        me.interp_sequence(me.planes([d_frames], [W], [W * H], [n * W * H]), me.planes([d_out], [W], [W * H]), 1, 0, 0, W, H, n, 1, mb, R,
                           window, d_mv[0], d_mv[1], jobs, stream=st.value)
        assert L.ffhip_stream_synchronize(st) == 0, L.ffhip_last_error()
        for d in range(2):
            assert np.array_equal(d_mv[d].cpu().numpy(), mv[d])
        assert np.array_equal(d_out.cpu().numpy(), want)
    finally:
        assert L.ffhip_stream_destroy(st) == 0
