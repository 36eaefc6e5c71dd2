"""The scene-change detection on the CPU: ffhip_me_scene_sequence_host() (kernels/me_scene_rules.h in a plain loop) against
tests/me_scene_model.py (the rule text of include/ffhip.h in numpy int64 sums, Python floats and np.float32), every sum exactly and every
float and double as a bit pattern, over the calls of tests/me_scene_cases.py; the carry, the threshold's edge, the conversion to float,
a sum past 2^32; the refusals, each alone with its text, in both faces.  And ffhip_me_interp_sequence_scd_host(): without flags the
existing host face byte for byte, with flags a model of both actions."""
import ctypes as C
import math

import numpy as np
import pytest

import me_interp_cases as K
import me_scene_cases as S
import me_scene_model as M
from ffmpeg_amd import _lib, me


# ---- the host face equals the model -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", S.DEPTHS)
@pytest.mark.parametrize("width", S.WIDTHS)
def test_host_face_equals_the_model(width, depth):
    seen = 0
    for c in S.cases(depth):
        if c.width != width:
            continue
        got, want = c.host(), c.model()
        for what, g, w in zip(("sad", "score", "flags", "mafd_out"), got, want):
            assert g == w, "%s: %s differs: %r, the model has %r" % (c.name, what, g, w)
        seen += 1
    assert seen == len(S.HEIGHTS) * len(S.PADS)


def test_the_sweep_reaches_both_flags_and_both_carries():
    flags = [f for d in S.DEPTHS for c in S.cases(d) for f in c.model()[2]]
    assert 0 in flags and 1 in flags
    assert any(c.mafd_in is None for c in S.cases(8)) and any(c.mafd_in is not None for c in S.cases(8))
    assert {c.frame_pitch % 16 == 0 for c in S.cases(8)} == {True, False}


def _flat(width, height, depth, levels):
    """one sequence of flat pictures, or of the given sample arrays"""
    dt = np.uint16 if depth > 8 else np.uint8
    pics = [np.full((height, width), v, dt) if np.isscalar(v) else v.astype(dt).reshape(height, width) for v in levels]
    return np.ascontiguousarray(np.stack(pics)), pics


def _run(buf, depth, width, height, nframes, threshold, mafd_in=None, outputs=("sad", "score", "flags", "mafd")):
    px = 2 if depth > 8 else 1
    o = S.Outputs(nframes - 1, 1)
    sad, score, flags, mafd = o.addresses()
    me.scene_sequence_host(buf, depth, width, height, width * px, width * height * px, nframes, 0, 1, threshold, mafd_in=mafd_in,
                           mafd_out=mafd if "mafd" in outputs else None, sad_out=sad if "sad" in outputs else None,
                           score_out=score if "score" in outputs else None, flags_out=flags if "flags" in outputs else None)
    return o


def _with_sum(n, total):
    """n samples that sum to `total`, as evenly as possible"""
    a = np.full(n, total // n, np.int64)
    a[:total - a.sum()] += 1
    assert a.sum() == total and a.max() <= 255
    return a


def test_the_carry_joins_two_calls():
    for c in [x for d in S.DEPTHS for x in S.cases(d) if x.nframes == 6][:12]:
        want = c.host()
        cut = 3                                          # pictures 0..3, then 3..5
        got = [[], [], [], None]
        carry = c.mafd_in
        for first, n in ((0, cut + 1), (cut, c.nframes - cut)):
            cin = carry
            o = S.Outputs((n - 1) * c.nseq, c.nseq)
            sad, score, flags, mafd = o.addresses()
            a = list(c.args(c.buf.ctypes.data + first * c.frame_pitch))
            a[6] = n
            me.scene_sequence_host(*a, mafd_in=cin, mafd_out=mafd, sad_out=sad, score_out=score, flags_out=flags)
            r = o.results()
            for k in range(3):
                got[k] += r[k]
            got[3] = r[3]
            carry = np.array(r[3], np.uint64).view(np.float64).copy()
        assert tuple(got) == tuple(want), c.name


def test_any_output_may_be_left_out():
    buf, pics = _flat(16, 4, 8, [0, 9, 200])
    full = _run(buf, 8, 16, 4, 3, 10.0).results()
    for keep in (("sad",), ("score",), ("flags",), ("flags", "mafd")):
        r = _run(buf, 8, 16, 4, 3, 10.0, outputs=keep).results()
        for k, what in enumerate(("sad", "score", "flags", "mafd")):
            if what in keep:
                assert r[k] == full[k]
            else:
                assert all(v in (S.SENT64, S.SENT32, S.SENT8) for v in r[k])


def test_the_threshold_edge():
    """160 x 160, sad 655360: mafd = 655360 * 100 / 25600 / 256 = 10.0 exactly, so is the score; flagged at 10.0, not at the next double"""
    buf, _ = _flat(160, 160, 8, [0, _with_sum(160 * 160, 655360)])
    r = _run(buf, 8, 160, 160, 2, 10.0).results()
    assert r[0] == [655360] and r[1] == [M.bits32(10.0)] and r[2] == [1] and r[3] == [M.bits64(10.0)]
    assert _run(buf, 8, 160, 160, 2, math.nextafter(10.0, math.inf)).results()[2] == [0]


def test_the_conversion_to_float_is_part_of_the_rule():
    """1280 x 720, sad 23592959: mafd is below 10 as a double and the score is 10.0f; one less and the score is the float below 10"""
    for sad, flag in ((23592959, 1), (23592958, 0)):
        buf, _ = _flat(1280, 720, 8, [0, _with_sum(1280 * 720, sad)])
        r = _run(buf, 8, 1280, 720, 2, 10.0).results()
        mafd = M.mafd(sad, 1280, 720, 8)
        assert mafd < 10.0 and r[0] == [sad] and r[3] == [M.bits64(mafd)]
        assert r[1] == [M.bits32(M.score(mafd, 0.0))] and r[2] == [flag]
        assert (r[1] == [M.bits32(10.0)]) == bool(flag)


def test_a_sum_past_32_bits():
    buf, pics = _flat(256, 257, 16, [0, 65535, 0])
    r = _run(buf, 16, 256, 257, 3, 50.0).results()
    total = 256 * 257 * 65535
    assert total > 1 << 32 and r[0] == [total, total]
    assert r == S.model_results([pics], 16, 50.0, None)


def test_no_pairs():
    """nframes <= 1 or nseq == 0: no pair output is written and the carry passes through, in both faces where no device is needed"""
    L = _lib.lib()
    buf = np.zeros(64, np.uint8)
    o = S.Outputs(0, 3)
    sad, score, flags, mafd = o.addresses()
    cin = np.array([1.5, 2.5, -3.0])
    me.scene_sequence_host(buf, 8, 4, 4, 4, 16, 1, 16, 3, 10.0, mafd_in=cin, mafd_out=mafd, sad_out=sad)
    assert o.results()[3] == [M.bits64(v) for v in cin]
    me.scene_sequence_host(buf, 8, 4, 4, 4, 16, 0, 16, 3, 10.0, mafd_out=mafd, sad_out=sad)
    assert o.results()[3] == [0, 0, 0]
    o = S.Outputs(0, 0)
    sad, score, flags, mafd = o.addresses()
    for face in ("host", "dev"):
        a = (buf.ctypes.data, 8, 4, 4, 4, 16, 5, 80, 0, 10.0, None, mafd, sad, None, None)
        assert (L.ffhip_me_scene_sequence_host(*a) if face == "host" else L.ffhip_me_scene_sequence_dev(*a, None)) == 0
        o.results()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
class Args:
    """a small legal call on host memory; a test changes one thing"""

    def __init__(self, depth=8):
        px = 2 if depth > 8 else 1
        self.depth, self.width, self.height, self.nframes, self.nseq, self.threshold = depth, 12, 5, 3, 2, 10.0
        self.stride = 14 * px
        self.frame_pitch = self.stride * 5 + 2
        self.seq_pitch = 2 * self.frame_pitch + self.stride * 5
        self.buf = S.aligned_bytes(2 * self.seq_pitch + 64, fill=3)
        self.frames = self.buf.ctypes.data
        self.mafd_in, self.mafd_out = np.zeros(2), np.zeros(2)
        self.sad, self.score, self.flags = np.zeros(4, np.uint64), np.zeros(4, np.float32), np.zeros(4, np.uint8)

    def call(self, face):
        L = _lib.lib()
        a = (me._ptr(self.frames), self.depth, self.width, self.height, self.stride, self.frame_pitch, self.nframes, self.seq_pitch, self.nseq,
             self.threshold, me._ptr(self.mafd_in), me._ptr(self.mafd_out), me._ptr(self.sad), me._ptr(self.score), me._ptr(self.flags))
        r = L.ffhip_me_scene_sequence_host(*a) if face == "host" else L.ffhip_me_scene_sequence_dev(*a, None)
        return r, L.ffhip_last_error().decode()


def _set(**kw):
    def f(a):
        for k, v in kw.items():
            setattr(a, k, v)
    return f


def _shift(name, by):
    def f(a):
        setattr(a, name, getattr(a, name) + by)
    return f


def _on(out, what):
    """`out` starts at the last byte of `what`"""
    def f(a):
        if what == "frames":
            end = a.seq_pitch + 2 * a.frame_pitch + 4 * a.stride + 12 * (2 if a.depth > 8 else 1)
            setattr(a, out, a.frames + end - 1)
        else:
            big = np.zeros(256, np.uint8)
            n = getattr(a, what).nbytes
            setattr(a, what, big[:n].view(getattr(a, what).dtype))
            setattr(a, out, big[n - 1:n - 1 + 64])
    return f


OVERLAP = "an output (mafd_out, sad_out, score_out, flags_out) overlaps frames, mafd_in or another output"
REFUSALS = [
    ("null-frames", 8, _set(frames=None), "a NULL frames, or sad_out, score_out and flags_out all NULL"),
    ("no-output", 8, _set(sad=None, score=None, flags=None), "a NULL frames, or sad_out, score_out and flags_out all NULL"),
    ("depth-low", 8, _set(depth=7), "depth 7 outside 8..16"),
    ("depth-high", 16, _set(depth=17), "depth 17 outside 8..16"),
    ("width-zero", 8, _set(width=0), "0 x 5: width and height are 1..32768"),
    ("width-large", 8, _set(width=32769, stride=40000), "32769 x 5: width and height are 1..32768"),
    ("height-zero", 8, _set(height=0), "12 x 0: width and height are 1..32768"),
    ("height-large", 8, _set(height=32769), "12 x 32769: width and height are 1..32768"),
    ("negative-nframes", 8, _set(nframes=-1), "a negative nframes or nseq (-1, 2)"),
    ("negative-nseq", 8, _set(nseq=-3), "a negative nframes or nseq (3, -3)"),
    ("stride", 8, _set(stride=11), "stride 11 below the row's 12 bytes"),
    ("stride-16-bit", 10, _set(stride=22), "stride 22 below the row's 24 bytes"),
    ("odd-frames", 10, _shift("frames", 1), "an odd frames address, stride, frame_pitch or seq_pitch"),
    ("odd-stride", 16, _shift("stride", 1), "an odd frames address, stride, frame_pitch or seq_pitch"),
    ("odd-frame-pitch", 12, _shift("frame_pitch", 1), "an odd frames address, stride, frame_pitch or seq_pitch"),
    ("odd-seq-pitch", 9, _shift("seq_pitch", 1), "an odd frames address, stride, frame_pitch or seq_pitch"),
    ("frame-pitch", 8, _set(frame_pitch=69), "frame_pitch 69 < stride * height 70"),
    ("seq-pitch", 8, _shift("seq_pitch", -1), "seq_pitch 213 < (nframes - 1) * frame_pitch + stride * height 214"),
    ("threshold-nan", 8, _set(threshold=float("nan")), "threshold nan is not a number in 0..100"),
    ("threshold-negative", 8, _set(threshold=-0.5), "threshold -0.5 is not a number in 0..100"),
    ("threshold-high", 8, _set(threshold=100.5), "threshold 100.5 is not a number in 0..100"),
    ("sad-on-frames", 8, _on("sad", "frames"), OVERLAP),
    ("score-on-frames", 16, _on("score", "frames"), OVERLAP),
    ("flags-on-mafd-in", 8, _on("flags", "mafd_in"), OVERLAP),
    ("mafd-out-on-mafd-in", 8, _on("mafd_out", "mafd_in"), OVERLAP),
    ("score-on-sad", 8, _on("score", "sad"), OVERLAP),
    ("flags-on-score", 8, _on("flags", "score"), OVERLAP),
    ("mafd-out-on-flags", 8, _on("mafd_out", "flags"), OVERLAP),
    ("pairs", 8, _set(nframes=65537, nseq=32768, frame_pitch=70, seq_pitch=65537 * 70), "2147483648 pairs: more than 2^31 - 1"),
]


@pytest.mark.parametrize("face", ["host", "dev"])
@pytest.mark.parametrize("what", [r[0] for r in REFUSALS])
def test_refusal(what, face):
    """every refusal alone, with its text, before any device check and identically in both faces"""
    _, depth, change, text = next(r for r in REFUSALS if r[0] == what)
    a = Args(depth)
    change(a)
    r, msg = a.call(face)
    assert r == -22 and text in msg and msg.startswith("ffhip_me_scene_sequence_dev / _host: "), (r, msg)


@pytest.mark.parametrize("depth", [8, 10])
def test_the_legal_call_of_the_refusal_tests_runs(depth):
    a = Args(depth)
    assert a.call("host")[0] == 0
    assert list(a.sad) == [0, 0, 0, 0] and list(a.flags) == [0, 0, 0, 0]


# ---- the interpolation that takes the flags ---------------------------------------------------------------------------------------------
def _scd_host(c, scene, action):
    counts = me.interp_sequence_scd_host(*c.args(me, [b.a.ctypes.data for b in c.src], [b.a.ctypes.data for b in c.dst],
                                                 [b.a.ctypes.data for b in c.fields]), scene, action)
    bufs = [b.a.copy() for b in c.dst]
    for b in c.dst:
        b.a[:] = K.FILL
    c.check_guards(bufs)
    return bufs, counts


@pytest.mark.parametrize("name", K.NAMES)
def test_without_flags_the_scd_host_face_is_the_existing_one(name):
    c = K.calls()[name]
    want, wcounts = c.host()
    for action in (me.SCENE_BLEND, me.SCENE_DUP):
        got, counts = _scd_host(c, None, action)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)) and counts == wcounts


SCD_JOBS = [(0, 0, 512, me.MCI), (0, 0, 513, me.MCI), (1, 0, 512, me.MCI), (1, 1, 513, me.MCI), (1, 1, 512, me.BLEND), (0, 1, 1024, me.MCI),
            (1, 1, 0, me.MCI), (0, 0, 341, me.BLEND), (1, 1, 512, me.MCI), (0, 0, 0, me.MCI), (1, 1, 1023, me.MCI)]
SCD_FLAGS = np.array([1, 0, 0, 7], np.uint8)            # pair-major: pair 0 of sequence 0 and pair 1 of sequence 1 are cuts


def scd_call(chroma=(1, 1), mb=16):
    return K.Call("scd", 52, 38, mb, chroma, "random", "ramp", SCD_JOBS, R=16, nseq=2, nframes=3, seed=95)


@pytest.mark.parametrize("action", [me.SCENE_BLEND, me.SCENE_DUP])
@pytest.mark.parametrize("chroma", [(1, 1), (0, 0), None])
def test_flagged_pairs_run_the_scene_action(chroma, action):
    c = scd_call(chroma)
    plain, pcounts = c.host()
    got, counts = _scd_host(c, SCD_FLAGS, action)
    flagged = 0
    for j, (s, p, alpha, mode) in enumerate(c.jobs):
        cut = mode == me.MCI and SCD_FLAGS[p * c.nseq + s]
        want = M.scene_picture(c.picture(s, p), c.picture(s, p + 1), alpha, action) if cut else c.output(j, plain)
        for i, (g, w) in enumerate(zip(c.output(j, got), want)):
            assert np.array_equal(g, w), "job %d %r plane %d" % (j, c.jobs[j], i)
        flagged += bool(cut)
    assert flagged == 7
    per = sum(w * h for w, h in zip(c.pw, c.ph))
    assert counts["samples"] == pcounts["samples"] == per * len(c.jobs)
    assert counts["blend"] == pcounts["blend"] + flagged * per == (flagged + 2) * per


def test_dup_differs_from_blend_and_turns_at_512():
    c = scd_call()
    blend, dup = _scd_host(c, SCD_FLAGS, me.SCENE_BLEND)[0], _scd_host(c, SCD_FLAGS, me.SCENE_DUP)[0]
    A, B = c.picture(0, 0), c.picture(0, 1)
    assert np.array_equal(c.output(0, dup)[0], A[0]) and np.array_equal(c.output(1, dup)[0], B[0])
    assert not np.array_equal(c.output(0, blend)[0], A[0])


def _scd_refusal(face, scene, action, dst_on_scene=False):
    import test_me_interp_cpu as T
    L = _lib.lib()
    a = T.Args()
    if dst_on_scene:
        big = np.zeros(3 * a.dp[2] + 64, np.uint8)
        scene, a.dst[2] = big[:4], big[3:]
    src = C.addressof(a.keep(me.planes(a.src, a.sstride, a.fp, a.sp)))
    dst = C.addressof(a.keep(me.planes(a.dst, a.dstride, a.dp)))
    jobs = C.addressof(a.keep(me.interp_jobs(a.jobs)))
    args = (src, dst, a.nplanes, a.sw, a.sh, a.W, a.H, a.nframes, a.nseq, a.mb, a.R, me._ptr(a.window), me._ptr(a.fwd), me._ptr(a.bwd), jobs,
            len(a.jobs), me._ptr(scene), action)
    r = L.ffhip_me_interp_sequence_scd_host(*args) if face == "host" else L.ffhip_me_interp_sequence_scd_dev(*args, None)
    return r, L.ffhip_last_error().decode()


@pytest.mark.parametrize("face", ["host", "dev"])
def test_scd_refusals(face):
    flags = np.zeros(4, np.uint8)
    for action in (0, 3, -1):
        r, msg = _scd_refusal(face, flags, action)
        assert r == -22 and msg == "ffhip_me_interp_sequence_scd_dev / _host: scene_action %d (1: blend, 2: duplicate)" % action
    r, msg = _scd_refusal(face, flags, me.SCENE_DUP, dst_on_scene=True)
    assert r == -22 and msg == "ffhip_me_interp_sequence_scd_dev / _host: dst overlaps scene"
    if face == "host":
        assert _scd_refusal(face, flags, me.SCENE_DUP)[0] == 0


def test_job_modes_stay_0_or_1_in_the_scd_faces():
    import test_me_interp_cpu as T
    a = T.Args()
    a.jobs[1] = (0, 0, 5, 2)
    src, dst, jobs = me.planes(a.src, a.sstride, a.fp, a.sp), me.planes(a.dst, a.dstride, a.dp), me.interp_jobs(a.jobs)
    r = _lib.lib().ffhip_me_interp_sequence_scd_host(C.addressof(src), C.addressof(dst), 3, 1, 1, a.W, a.H, 3, 2, 16, 8, a.window.ctypes.data,
                                                     a.fwd.ctypes.data, a.bwd.ctypes.data, C.addressof(jobs), 3, None, me.SCENE_DUP)
    assert r == -22 and "mode 2 (0 or 1)" in _lib.lib().ffhip_last_error().decode()
