"""vf_minterpolate's compensation on the CPU: ffhip_me_interp_sequence_host() (kernels/me_interp_rules.h in a plain loop over samples, a
gather that stores no list) against tests/me_interp_model.py (the rule text of include/ffhip.h as the reference's scatter into explicit
lists): every byte and every counter, over the calls of tests/me_interp_cases.py; the refusals, each alone with its text; and a property
that ties the face to the search: a pure shift found by the exhaustive search is interpolated exactly."""
import ctypes as C

import numpy as np
import pytest

import me_interp_cases as K
import me_interp_model as M
from ffmpeg_amd import _lib, me


@pytest.mark.parametrize("name", K.NAMES)
def test_host_face_equals_the_model(name):
    c = K.calls()[name]
    bufs, counts = c.host()                     # checks the guards round every plane, field and output too
    want, wcounts = c.model()
    for j, job in enumerate(c.jobs):
        for i, (got, ref) in enumerate(zip(c.output(j, bufs), want[j])):
            assert np.array_equal(got, ref), "%s: job %d %r plane %d: %d samples differ, first at %s" % (
                name, j, job, i, (got != ref).sum(), np.argwhere(got != ref)[:1].tolist())
    assert counts == wcounts


def test_every_counter_is_reached():
    total = M.new_counts()
    for c in K.calls().values():
        for k, v in c.host()[1].items():
            total[k] += v
    assert all(total[k] > 0 for k in M.COUNTS), total


def test_only_the_pile_up_reaches_the_cap_by_design():
    """about 8 x 8 windows stacked on one pixel against a cap of 16: the reference's nb + 1 >= NB_PIXEL_MVS branch"""
    c = K.calls()["pileup"]
    assert c.model()[1]["capped"] > 0 and c.host()[1]["capped"] == c.model()[1]["capped"]
    lists = M.scatter(c.W, c.H, c.mb, c.R, 0, c.window, c.field_array(0)[0][0], c.field_array(1)[0][0], M.new_counts())
    x, y = K.PILE_AT
    assert len(lists[y][x]) == M.NB_PIXEL_MVS


def test_struct_sizes():
    Planes, Job = me._structs()
    assert C.sizeof(Job) == 16 == _lib.lib().ffhip_me_interp_job_size()
    assert C.sizeof(Planes) == 12 * C.sizeof(C.c_void_p)


@pytest.mark.parametrize("mb", [16, 8])
@pytest.mark.parametrize("d", [(6, -2), (-4, 4), (2, 0)])
def test_a_shift_found_by_the_search_is_interpolated_exactly(mb, d):
    """A noise, B = A moved by an even d: the exhaustive search finds -d (dir 0) and +d (dir 1), and at alpha 512 both entries of every
    contribution read the same sample, so the interior (2 mb + |d| from every border) is A moved by d / 2, exactly"""
    W, H, R = 96, 80, 8
    dx, dy = d
    rng = np.random.default_rng(5)
    A = rng.integers(0, 256, (H, W), dtype=np.uint8)
    B = np.roll(A, (dy, dx), axis=(0, 1))
    lg = {16: 4, 8: 3}[mb]
    per = (W >> lg) * (H >> lg)
    fields = []
    for cur, ref in ((B, A), (A, B)):
        mv, cost = np.zeros(2 * per, np.int16), np.zeros(per, np.uint32)
        me.search_frames_host(me.ESA, np.ascontiguousarray(cur), np.ascontiguousarray(ref), W, H, W, W * H, 1, mb, R, me.SAD, mv, cost)
        fields.append(mv)
    src = np.concatenate([A.reshape(-1), B.reshape(-1)])
    out = np.zeros(W * H, np.uint8)
    me.interp_sequence_host(me.planes([src], [W], [W * H]), me.planes([out], [W], [W * H]), 1, 0, 0, W, H, 2, 1, mb, R, K.window("ramp", mb),
                            fields[0], fields[1], [(0, 0, 512, me.MCI)])
    m = 2 * mb + max(abs(dx), abs(dy))
    want = np.roll(A, (dy // 2, dx // 2), axis=(0, 1))
    assert np.array_equal(out.reshape(H, W)[m:H - m, m:W - m], want[m:H - m, m:W - m])
    assert not np.array_equal(out.reshape(H, W)[m:H - m, m:W - m], A[m:H - m, m:W - m])


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
class Args:
    """a small legal call on host memory; a test changes one thing"""

    def __init__(self):
        self.W, self.H, self.nframes, self.nseq, self.mb, self.R, self.nplanes, self.sw, self.sh = 32, 16, 3, 2, 16, 8, 3, 1, 1
        self.sstride, self.dstride = [40, 20, 20], [32, 16, 16]
        self.fp = [40 * 16, 20 * 8, 20 * 8]
        self.sp = [3 * f for f in self.fp]
        self.dp = [32 * 16, 16 * 8, 16 * 8]
        self.src = [np.zeros(2 * s, np.uint8) for s in self.sp]
        self.jobs = [(0, 0, 100, me.MCI), (1, 1, 1024, me.BLEND), (1, 0, 0, me.MCI)]
        self.dst = [np.zeros(3 * d, np.uint8) for d in self.dp]
        self.window = np.full(1024, 7, np.uint8)
        per = 2
        self.fwd = np.tile(np.array([0, 0, 16, 0], np.int16), 2 * 2)
        self.bwd = self.fwd.copy()
        assert self.fwd.size == 2 * per * 2 * 2
        self.srcp = self.dstp = None

    def call(self, face="host"):
        L = _lib.lib()
        _, Job = me._structs()
        src = self.srcp if self.srcp is not None else C.addressof(self.keep(me.planes(self.src, self.sstride, self.fp, self.sp)))
        dst = self.dstp if self.dstp is not None else C.addressof(self.keep(me.planes(self.dst, self.dstride, self.dp)))
        jobs = None if self.jobs is None else C.addressof(self.keep(me.interp_jobs(self.jobs)))
        a = (src or None, dst or None, self.nplanes, self.sw, self.sh, self.W, self.H, self.nframes, self.nseq, self.mb, self.R,
             me._ptr(self.window), me._ptr(self.fwd), me._ptr(self.bwd), jobs, 0 if self.jobs is None else len(self.jobs))
        r = L.ffhip_me_interp_sequence_host(*a) if face == "host" else L.ffhip_me_interp_sequence_dev(*a, None)
        return r, L.ffhip_last_error().decode()

    def keep(self, o):
        self.kept = getattr(self, "kept", []) + [o]
        return o


def _planes_with(a, which, i, field, value):
    P = me.planes(a.src, a.sstride, a.fp, a.sp) if which == "src" else me.planes(a.dst, a.dstride, a.dp)
    getattr(P, field)[i] = value
    a.keep(P)
    setattr(a, which + "p", C.addressof(P))


def _set(name, value):
    return lambda a: setattr(a, name, value)


def _job(j, t):
    def f(a):
        a.jobs[j] = t
    return f


def _overlap(which):
    def f(a):
        if which == "src":
            end = a.sp[0] + 2 * a.fp[0] + 15 * a.sstride[0] + 32        # plane 0 of the last picture of the last sequence ends here
            big = np.zeros(4 * a.sp[0], np.uint8)
            a.src[0] = big[:2 * a.sp[0]]
            a.dst[0] = big[end - 1:]                      # dst's first byte is src's last
        else:
            big = np.zeros(3 * a.dp[1] + 64, np.uint8)
            big[:32] = a.fwd.view(np.uint8)
            a.bwd = big[:32].view(np.int16)
            a.dst[1] = big[31:]                           # dst's first byte is the field's last
    return f


REFUSALS = [
    ("null-src", _set("srcp", 0), "a NULL src, dst, window or jobs"),
    ("null-dst", _set("dstp", 0), "a NULL src, dst, window or jobs"),
    ("null-window", _set("window", None), "a NULL src, dst, window or jobs"),
    ("null-jobs", _set("jobs", None), "a NULL src, dst, window or jobs"),
    ("null-src-plane", lambda a: _planes_with(a, "src", 2, "base", None), "plane 2 of src is NULL"),
    ("null-dst-plane", lambda a: _planes_with(a, "dst", 1, "base", None), "plane 1 of dst is NULL"),
    ("null-fwd", _set("fwd", None), "a NULL mv_fwd or mv_bwd with an MCI job"),
    ("null-bwd", _set("bwd", None), "a NULL mv_fwd or mv_bwd with an MCI job"),
    ("nplanes-2", _set("nplanes", 2), "nplanes 2 is neither 1 nor 3"),
    ("nplanes-0", _set("nplanes", 0), "nplanes 0 is neither 1 nor 3"),
    ("shift-w", _set("sw", 2), "chroma shifts 2, 1"),
    ("shift-h", _set("sh", -1), "chroma shifts 1, -1"),
    ("mb-size", _set("mb", 32), "mb_size 32 (16 or 8)"),
    ("range-high", _set("R", 257), "mv_range 257 outside 0..256"),
    ("range-negative", _set("R", -1), "mv_range -1 outside 0..256"),
    ("negative-width", _set("W", -1), "a negative width, height, nframes, nseq or njobs"),
    ("negative-height", _set("H", -2), "a negative width, height, nframes, nseq or njobs"),
    ("negative-nframes", _set("nframes", -1), "a negative width, height, nframes, nseq or njobs"),
    ("negative-nseq", _set("nseq", -1), "a negative width, height, nframes, nseq or njobs"),
    ("wide", _set("W", 32769), "32769 x 16: positions of a picture above 32768"),
    ("tall", _set("H", 32770), "32 x 32770: positions of a picture above 32768"),
    ("src-stride", lambda a: _planes_with(a, "src", 0, "stride", 31), "plane 0: a stride (src 31, dst 32) below the plane's width 32"),
    ("dst-stride", lambda a: _planes_with(a, "dst", 2, "stride", 15), "plane 2: a stride (src 20, dst 15) below the plane's width 16"),
    ("frame-pitch", lambda a: _planes_with(a, "src", 1, "frame_pitch", 20 * 8 - 1), "plane 1: src frame_pitch 159 < stride * height 160"),
    ("seq-pitch", lambda a: _planes_with(a, "src", 0, "seq_pitch", 3 * 640 - 1), "plane 0: src seq_pitch 1919 < (nframes - 1) * frame_pitch"),
    ("dst-pitch", lambda a: _planes_with(a, "dst", 0, "frame_pitch", 511), "plane 0: dst frame_pitch 511 < stride * height 512"),
    ("job-seq", _job(1, (2, 0, 0, me.MCI)), "job 1: seq 2 (0..1)"),
    ("job-seq-negative", _job(0, (-1, 0, 0, me.MCI)), "job 0: seq -1 (0..1)"),
    ("job-pair", _job(2, (0, 2, 0, me.BLEND)), "job 2: seq 0 (0..1), pair 2 (0..1)"),
    ("job-pair-negative", _job(2, (0, -1, 0, me.BLEND)), "job 2: seq 0 (0..1), pair -1 (0..1)"),
    ("job-alpha", _job(0, (0, 0, 1025, me.MCI)), "job 0: seq 0 (0..1), pair 0 (0..1), alpha 1025 (0..1024)"),
    ("job-alpha-negative", _job(1, (0, 0, -1, me.MCI)), "alpha -1 (0..1024)"),
    ("job-mode", _job(1, (0, 0, 5, 2)), "job 1: seq 0 (0..1), pair 0 (0..1), alpha 5 (0..1024), mode 2 (0 or 1)"),
    ("dst-on-src", _overlap("src"), "dst overlaps src, mv_fwd or mv_bwd"),
    ("dst-on-field", _overlap("field"), "dst overlaps src, mv_fwd or mv_bwd"),
]


@pytest.mark.parametrize("face", ["host", "dev"])
@pytest.mark.parametrize("what", [r[0] for r in REFUSALS])
def test_refusal(what, face):
    """every refusal alone, with its text, before any device check and identically in both faces"""
    _, change, text = next(r for r in REFUSALS if r[0] == what)
    a = Args()
    change(a)
    r, msg = a.call(face)
    assert r == -22 and text in msg and msg.startswith("ffhip_me_interp_sequence_dev / _host: "), (r, msg)


def test_negative_njobs_is_refused():
    L = _lib.lib()
    a = Args()
    P, D, J = me.planes(a.src, a.sstride, a.fp, a.sp), me.planes(a.dst, a.dstride, a.dp), me.interp_jobs(a.jobs)
    r = L.ffhip_me_interp_sequence_host(C.addressof(P), C.addressof(D), 3, 1, 1, 32, 16, 3, 2, 16, 8, a.window.ctypes.data, a.fwd.ctypes.data,
                                        a.bwd.ctypes.data, C.addressof(J), -1)
    assert r == -22 and "a negative width, height, nframes, nseq or njobs" in L.ffhip_last_error().decode()


def test_the_legal_call_of_the_refusal_tests_runs_and_no_jobs_do_nothing():
    a = Args()
    assert a.call("host")[0] == 0
    assert me.interp_host_counts()["samples"] == 3 * (32 * 16 + 2 * 16 * 8)
    a = Args()
    a.jobs = []
    for d in a.dst:
        d[:] = 9
    assert a.call("host")[0] == 0 and a.call("dev")[0] == 0          # before any device check
    assert all((d == 9).all() for d in a.dst)


def test_blend_jobs_alone_need_no_fields():
    a = Args()
    a.jobs = [(0, 0, 300, me.BLEND)]
    a.fwd = a.bwd = None
    for s in a.src:
        s[:] = np.random.default_rng(3).integers(0, 256, s.size, dtype=np.uint8)
    assert a.call("host")[0] == 0
    A, B = a.src[0][:640].reshape(16, 40)[:, :32].astype(int), a.src[0][640:1280].reshape(16, 40)[:, :32].astype(int)
    assert np.array_equal(a.dst[0][:512].reshape(16, 32), (300 * B + 724 * A + 512) >> 10)
