"""The scene-change detection on the device: ffhip_me_scene_sequence_dev() (k_me_scene_sad and k_me_scene_flags, kernels/me_scene.hip)
against the host face and the model — sums exactly, floats and doubles as bit patterns, guard elements included — over the calls of
tests/me_scene_cases.py; more pairs than a launch's sums hold, split over sequences and over steps; a sum past 2^32; 1080p; two calls
chained on the device through mafd_out; and ffhip_me_interp_sequence_scd_dev() with the flags the detection left on the device."""
import numpy as np
import pytest

import me_interp_cases as K
import me_scene_cases as S
import me_scene_model as M

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def run_dev(args, npairs, nseq, buf, mafd_in=None, outputs=("sad", "score", "flags", "mafd"), d_buf=None):
    """the call on the device over the uploaded buffer `buf` (args: the face's arguments behind `frames`, with the offset of frames in
    buf first); returns Outputs.results() of the downloaded arrays"""
    torch = _torch()
    from ffmpeg_amd import me
    d_buf = torch.from_numpy(buf).cuda() if d_buf is None else d_buf
    o = S.Outputs(npairs, nseq)
    d_out = [torch.from_numpy(a.view(np.uint8)).cuda() for a in o.arrays()]
    d_in = None if mafd_in is None else torch.from_numpy(np.asarray(mafd_in, np.float64)).cuda()
    sad, score, flags, mafd = o.addresses([t.data_ptr() for t in d_out])
    torch.cuda.synchronize()
    me.scene_sequence(d_buf.data_ptr() + args[0], *args[1:], mafd_in=d_in, mafd_out=mafd if "mafd" in outputs else None,
                      sad_out=sad if "sad" in outputs else None, score_out=score if "score" in outputs else None,
                      flags_out=flags if "flags" in outputs else None)
    torch.cuda.synchronize()
    assert np.array_equal(d_buf.cpu().numpy(), buf), "the device changed an input"
    if mafd_in is not None:
        assert np.array_equal(d_in.cpu().numpy(), np.asarray(mafd_in, np.float64))
    return o.results([t.cpu().numpy().view(a.dtype) for t, a in zip(d_out, o.arrays())])


@pytest.mark.parametrize("depth", S.DEPTHS)
def test_device_equals_host_equals_model(depth):
    for c in S.cases(depth):
        want = c.host()
        assert want == c.model(), c.name
        got = run_dev(c.args(0), c.npairs, c.nseq, c.buf, c.mafd_in)
        for what, g, w in zip(("sad", "score", "flags", "mafd_out"), got, want):
            assert g == w, "%s: %s differs: %r, the host face has %r" % (c.name, what, g, w)


def _host(buf, args, npairs, nseq, mafd_in=None):
    from ffmpeg_amd import me
    o = S.Outputs(npairs, nseq)
    sad, score, flags, mafd = o.addresses()
    me.scene_sequence_host(buf.ctypes.data + args[0], *args[1:], mafd_in=mafd_in, mafd_out=mafd, sad_out=sad, score_out=score, flags_out=flags)
    return o.results()


@pytest.mark.parametrize("nseq, nframes", [(70000, 2), (7, 10001)])
def test_70000_pairs_of_8x2_pictures(nseq, nframes):
    """past a grid dimension and past the 4096 sums of a launch: 70,000 sequences split into groups, and 10,000 steps of 7 sequences
    split into runs of whole steps with the carried doubles waiting in the group's slot"""
    npairs = (nframes - 1) * nseq
    assert npairs == 70000
    rng = np.random.default_rng(nseq)
    buf = rng.integers(0, 256, nseq * nframes * 16, dtype=np.uint8)
    buf[::3] >>= 3                                   # sums that move
    args = (0, 8, 8, 2, 8, 16, nframes, nframes * 16, nseq, 10.0)
    mafd_in = rng.random(nseq) * 40.0
    want = _host(buf, args, npairs, nseq, mafd_in)
    pics = buf.reshape(nseq, nframes, 2, 8).astype(np.int64)
    assert want[0] == [int(v) for v in np.abs(pics[:, 1:] - pics[:, :-1]).sum(axis=(2, 3)).T.reshape(-1)]
    for s in range(0, nseq, max(nseq // 5, 1)):     # the model, on a few sequences
        prev = float(mafd_in[s])
        for k in range(nframes - 1):
            sc, fl, prev = M.step(want[0][k * nseq + s], prev, 8, 2, 8, 10.0)
            assert (want[1][k * nseq + s], want[2][k * nseq + s]) == (M.bits32(sc), fl)
        assert want[3][s] == M.bits64(prev)
    assert 0 < sum(want[2]) < npairs
    assert run_dev(args, npairs, nseq, buf, mafd_in) == want
    # and with nothing but the flags asked for: the sums then live in the launch's table alone
    got = run_dev(args, npairs, nseq, buf, mafd_in, outputs=("flags",))
    assert got[2] == want[2] and set(got[0]) == {S.SENT64} and set(got[3]) == {S.SENT64}


def test_a_sum_past_32_bits():
    """4096 x 4128 at 8 bits, all 0 against all 255: 4,311,613,440"""
    torch = _torch()
    W, H = 4096, 4128
    d_buf = torch.zeros(2 * W * H, dtype=torch.uint8, device="cuda:0")
    d_buf[W * H:] = 255
    buf = np.zeros(2 * W * H, np.uint8)
    buf[W * H:] = 255
    got = run_dev((0, 8, W, H, W, W * H, 2, 0, 1, 50.0), 1, 1, buf, d_buf=d_buf)
    total = W * H * 255
    assert total == 4311613440 and total > 1 << 32
    sc, fl, m = M.step(total, 0.0, W, H, 8, 50.0)
    assert got == ([total], [M.bits32(sc)], [fl], [M.bits64(m)]) and fl == 1


@pytest.mark.parametrize("depth", [8, 10])
def test_1080p(depth):
    px = 2 if depth > 8 else 1
    W, H, n = 1920, 1080, 4
    rng = np.random.default_rng(depth)
    stride = (W + 24) * px
    fp = stride * H + 160
    buf = S.aligned_bytes(16 + (n - 1) * fp + (H - 1) * stride + W * px, rng=rng)
    buf[16 + 2 * fp:] >>= 2                            # a cut before picture 2
    args = (16, depth, W, H, stride, fp, n, 0, 1, 10.0)
    want = _host(buf, args, n - 1, 1)
    assert 1 in want[2]
    assert run_dev(args, n - 1, 1, buf) == want


def test_two_calls_chained_on_the_device_through_mafd_out():
    torch = _torch()
    from ffmpeg_amd import me
    c = next(x for x in S.cases(8) if x.nframes == 6 and x.nseq == 3 and x.width >= 63)
    want = c.host()
    d_buf = torch.from_numpy(c.buf).cuda()
    d_carry = [torch.full((c.nseq,), 7.0, dtype=torch.float64, device="cuda:0") for _ in range(2)]
    d_in = None if c.mafd_in is None else torch.from_numpy(c.mafd_in).cuda()
    d_sad = torch.zeros(c.npairs, dtype=torch.int64, device="cuda:0")
    d_score = torch.zeros(c.npairs, dtype=torch.int32, device="cuda:0")
    d_flags = torch.full((c.npairs,), 9, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    cut = 2                                             # pictures 0..2, then 2..5, nothing between the calls but the stream
    a = list(c.args(d_buf.data_ptr()))
    a[6] = cut + 1
    me.scene_sequence(*a, mafd_in=d_in, mafd_out=d_carry[0], sad_out=d_sad, score_out=d_score, flags_out=d_flags)
    a = list(c.args(d_buf.data_ptr() + cut * c.frame_pitch))
    a[6] = c.nframes - cut
    o = cut * c.nseq
    me.scene_sequence(*a, mafd_in=d_carry[0], mafd_out=d_carry[1], sad_out=d_sad.data_ptr() + 8 * o, score_out=d_score.data_ptr() + 4 * o,
                      flags_out=d_flags.data_ptr() + o)
    torch.cuda.synchronize()
    got = ([int(v) for v in d_sad.cpu().numpy()], [int(v) for v in d_score.cpu().numpy().view(np.uint32)], [int(v) for v in d_flags.cpu().numpy()],
           [int(v) for v in d_carry[1].cpu().numpy().view(np.uint64)])
    assert got == tuple(want)


@pytest.mark.parametrize("action", [1, 2])
def test_interp_sequence_scd_with_the_flags_of_the_device(action):
    """detection, then interpolation, on the device; the same two calls on the host.  Random pictures: the first pair of a sequence
    differs from nothing before it and is flagged, the second is not"""
    torch = _torch()
    from ffmpeg_amd import me
    import test_me_scene_cpu as T
    c = T.scd_call()
    scene = (c.src[0].a.ctypes.data + K.GUARD, 8, c.W, c.H, c.stride[0], c.fpitch[0], c.nframes, c.spitch[0], c.nseq, 10.0)
    flags = np.full((c.nframes - 1) * c.nseq, 9, np.uint8)
    me.scene_sequence_host(*scene, flags_out=flags)
    assert sorted(set(flags)) == [0, 1]
    want, _ = T._scd_host(c, flags, action)
    assert any(not np.array_equal(w, p) for w, p in zip(want, c.host()[0]))
    src = [torch.from_numpy(b.a).cuda() for b in c.src]
    fields = [torch.from_numpy(b.a).cuda() for b in c.fields]
    dst = [torch.from_numpy(b.a).cuda() for b in c.dst]
    d_flags = torch.full((flags.size,), 9, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    me.scene_sequence(src[0].data_ptr() + K.GUARD, *scene[1:], flags_out=d_flags)
    me.interp_sequence_scd(*c.args(me, [t.data_ptr() for t in src], [t.data_ptr() for t in dst], [t.data_ptr() for t in fields]), d_flags, action)
    torch.cuda.synchronize()
    assert np.array_equal(d_flags.cpu().numpy(), flags)
    got = [t.cpu().numpy() for t in dst]
    c.check_guards(got)
    for i in range(c.nplanes):
        assert np.array_equal(got[i], want[i]), "plane %d" % i
    # and without flags the existing face's bytes
    me.interp_sequence_scd(*c.args(me, [t.data_ptr() for t in src], [t.data_ptr() for t in dst], [t.data_ptr() for t in fields]), None, action)
    torch.cuda.synchronize()
    for i in range(c.nplanes):
        assert np.array_equal(dst[i].cpu().numpy(), c.host()[0][i])
