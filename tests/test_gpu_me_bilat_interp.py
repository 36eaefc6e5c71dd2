"""The bilateral compensation on the device: ffhip_me_interp_bilat_sequence_dev() (k_me_interp_bilat, kernels/me_interp.hip) against the
host face and the model, byte for byte, guards included, over the calls of tests/test_me_bilat_interp_cpu.py (scene flags and both
actions among them); 64 jobs in one launch, the same jobs in two calls, a job count beyond one launch's table, and 1080p against the
host face, which the small shapes pin to the model."""
import numpy as np
import pytest

import me_interp_cases as K
import me_interp_model as I
import test_me_bilat_interp_cpu as T
from test_gpu_me_interp import same

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def run_dev(c, scene=None, action=1, parts=None):
    """the call on the device, its jobs in the given slices (one call each, in order); returns the output buffers"""
    torch = _torch()
    from ffmpeg_amd import me
    src = [torch.from_numpy(b.a).cuda() for b in c.src]
    field = torch.from_numpy(c.fields[0].a).cuda()
    dst = [torch.from_numpy(b.a).cuda() for b in c.dst]
    d_scene = None if scene is None else torch.from_numpy(np.ascontiguousarray(scene)).cuda()
    torch.cuda.synchronize()
    for lo, hi in parts or [(0, len(c.jobs))]:
        a = c.args(me, [t.data_ptr() for t in src], [t.data_ptr() + lo * c.dpitch[i] for i, t in enumerate(dst)], [field.data_ptr()] * 2)
        me.interp_bilat_sequence(*a[:12], a[12], c.jobs[lo:hi], d_scene, action)
    torch.cuda.synchronize()
    for t, b in zip(src + [field], c.src + [c.fields[0]]):
        assert np.array_equal(t.cpu().numpy(), b.a), "%s: the device changed an input" % c.name
    return [t.cpu().numpy() for t in dst]


def host_of(c, scene=None, action=1):
    from ffmpeg_amd import me
    me.interp_bilat_sequence_host(*T.bilat_args(c, me, [b.a.ctypes.data for b in c.src], [b.a.ctypes.data for b in c.dst], c.fields[0].a.ctypes.data,
                                                scene, action))
    bufs = [b.a.copy() for b in c.dst]
    for b in c.dst:
        b.a[:] = K.FILL
    return bufs


@pytest.mark.parametrize("name", T.NAMES)
def test_device_equals_host_equals_model(name):
    c, scene, action = T.calls()[name]
    bufs, _ = T.host(name)
    want, _ = T.model(name)
    for j in range(len(c.jobs)):
        for got, ref in zip(c.output(j, bufs), want[j]):
            assert np.array_equal(got, ref)
    same(c, run_dev(c, scene, action), bufs)


@pytest.fixture(scope="module")
def many():
    """64 jobs over 3 sequences of 4 pictures: every pair several times, both modes"""
    jobs = [(j % 3, (j // 3) % 3, (j * 37) % 1025, I.BLEND if j % 7 == 3 else I.MCI) for j in range(64)]
    return K.Call("64-jobs", 52, 38, 8, (1, 1), "random", "ramp", jobs, R=12, nseq=3, nframes=4, seed=7)


def test_64_jobs_over_3_sequences_in_one_launch(many):
    same(many, run_dev(many), host_of(many))


def test_the_same_jobs_in_two_calls_on_one_stream(many):
    same(many, run_dev(many, parts=[(0, 23), (23, 64)]), host_of(many))


def test_more_jobs_than_one_launch_holds():
    """a launch's table holds 1024 jobs: 1030 make the launcher split"""
    jobs = [(0, 0, j % 1025, I.BLEND if j % 5 == 4 else I.MCI) for j in range(1030)]
    c = K.Call("1030-jobs", 24, 16, 8, None, "random", "holes", jobs, R=8, seed=8)
    same(c, run_dev(c), host_of(c))


@pytest.mark.parametrize("mb", [16, 8])
def test_1080p(mb):
    c = K.Call("1080p-mb%d" % mb, 1920, 1080, mb, (1, 1), "random", "ramp", [(0, 0, 341, I.MCI)], R=32, seed=mb)
    same(c, run_dev(c), host_of(c))
