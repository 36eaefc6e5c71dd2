"""CPU tier of the bilateral compensation (ffhip_me_interp_bilat_sequence_host and the refusals of the device face): the host face
against the scatter model of tests/me_bilat_model.py, written from the rule text of include/ffhip.h, over every byte and counter, on the
calls of tests/me_interp_cases.py (imported, not edited: their direction-0 field is the one field here) — fields random within
mv_range, at +-mv_range, of any int16 (malformed vectors), windows with zeros, 1 and 3 planes, chroma shifts 0 and 1, alphas 0, 1,
341, 512, 1023, 1024 — plus a picture whose right and bottom strips no window reaches, and scene flags with both actions; guard bytes
round every plane, field and output.  Then the textures of tests/test_me_bilat_search_cpu.py, searched by the bilateral search and
interpolated exactly; and every refusal alone with its text.  No device is needed."""
import functools

import numpy as np
import pytest

import ffi
import me_bilat_model as M
import me_interp_cases as K
import me_interp_model as I
import test_me_bilat_search_cpu as B

EINVAL, ENOSYS = -22, -38
WHO = "ffhip_me_interp_bilat_sequence_dev / _host: "


def me():
    from ffmpeg_amd import me
    return me


@functools.lru_cache(maxsize=None)
def calls():
    """name -> (Call, scene flags or None, scene_action)"""
    out = {n: (c, None, 1) for n, c in K.calls().items()}
    jobs = [(0, 0, a, I.MCI) for a in (0, 1, 512, 1023, 1024)]
    # 3 x 2 blocks of 16 reach column 55 and row 39: the strips 56..62 and 40..46 take the empty-list fallback
    out["strips"] = (K.Call("strips", 63, 47, 16, (1, 1), "random", "full", jobs, R=32, seed=95), None, 1)
    out["strips-mb8-y"] = (K.Call("strips-mb8-y", 31, 29, 8, None, "random", "ramp", jobs[1:4], R=9, seed=96), None, 1)
    sj = [(s, p, K.ALPHAS[(s + p + t) % 6], I.BLEND if (s + p + t) % 5 == 4 else I.MCI) for s in range(3) for p in range(3) for t in range(2)]
    flags = (np.arange(9).reshape(3, 3) % 2).astype(np.uint8)         # [pair][seq]
    for action in (1, 2):
        out["scene-%d" % action] = (K.Call("scene-%d" % action, 48, 32, 16, (1, 1), "random", "ramp", sj, R=16, nseq=3, nframes=4, seed=97), flags, action)
    return out


NAMES = tuple(calls())


def bilat_args(c, m, src_addr, dst_addr, field_addr, scene, action):
    a = c.args(m, src_addr, dst_addr, [field_addr, field_addr])
    return a[:12] + (a[12], a[14], None if scene is None else scene.ctypes.data, action)


@functools.lru_cache(maxsize=None)
def host(name):
    """(the output buffers after the host face, its counts); guards and inputs checked"""
    c, scene, action = calls()[name]
    counts = me().interp_bilat_sequence_host(*bilat_args(c, me(), [b.a.ctypes.data for b in c.src], [b.a.ctypes.data for b in c.dst],
                                                         c.fields[0].a.ctypes.data, scene, action))
    bufs = [b.a.copy() for b in c.dst]
    for b in c.dst:
        b.a[:] = K.FILL
    c.check_guards(bufs)
    return bufs, counts


@functools.lru_cache(maxsize=None)
def model(name):
    c, scene, action = calls()[name]
    pics = [[c.picture(s, p) for p in range(c.nframes)] for s in range(c.nseq)]
    return M.interp_bilat_sequence(pics, c.W, c.H, c.sw, c.sh, c.mb, c.R, c.window, c.field_array(0), c.jobs, scene, action)


@pytest.mark.parametrize("name", NAMES)
def test_host_face_equals_the_model(name):
    c = calls()[name][0]
    bufs, counts = host(name)
    want, wcounts = model(name)
    for j in range(len(c.jobs)):
        for i, (got, w) in enumerate(zip(c.output(j, bufs), want[j])):
            assert np.array_equal(got, w), (name, j, i)
    assert counts == wcounts
    assert counts["capped"] == 0


def test_the_calls_reach_what_they_are_for():
    total = I.new_counts()
    for name in NAMES:
        for k, v in model(name)[1].items():
            total[k] += v
    assert total["capped"] == 0 and all(total[k] > 0 for k in ("taken", "zero_weight", "malformed", "fallback", "clipped", "blend"))
    # the strips: every pixel right of column 55 or below row 39 is on the fallback, in every job
    c = calls()["strips"][0]
    assert model("strips")[1]["fallback"] >= len(c.jobs) * (63 * 47 - 56 * 40)
    # both scene actions differ where a pair is flagged
    a, b = host("scene-1")[0], host("scene-2")[0]
    assert any(not np.array_equal(x, y) for x, y in zip(a, b))


# ---- the textures: searched by the bilateral search, interpolated exactly ---------------------------------------------------------------
def _interior(a):
    """the pixels whose (at most four) blocks are all interior blocks of the 6 x 5"""
    return a[24:56, 24:72]


@pytest.mark.parametrize("v,alpha", [((1, 0), 512), ((2, 1), 512), ((-3, 2), 512), ((2, -2), 256)])
@pytest.mark.parametrize("method", B.METHODS, ids=B.IDS)
def test_a_searched_texture_is_interpolated_exactly(method, v, alpha):
    """A(p) = T(p - v), B(p) = T(p + v): at alpha 512 the picture between them is T; at alpha 256, with v = (2, -2), it is T a quarter of
    the way, T(p - v / 2)"""
    w, h, m = B.BW * B.MB, B.BH * B.MB, 8
    A, Bp, _ = B.found_pictures(v)
    mv, _, _ = B.host_pairs(method, A[None], Bp[None], w, h, B.MB, B.RR, None, None)
    field = mv.reshape(B.BH, B.BW, 2)
    for by in range(1, B.BH - 1):
        for bx in range(1, B.BW - 1):
            assert (int(field[by, bx, 0]) - bx * B.MB, int(field[by, bx, 1]) - by * B.MB) == v, (bx, by)
    big = B.texture(np.random.default_rng(ffi.stable_seed("me_bilat_found")), h + 2 * m, w + 2 * m)
    s = (v[0] * (512 - alpha) // 512, v[1] * (512 - alpha) // 512)          # the texture's shift at this instant: exact for these cases
    assert (s[0] * 512, s[1] * 512) == (v[0] * (512 - alpha), v[1] * (512 - alpha))
    want = big[m - s[1]:m - s[1] + h, m - s[0]:m - s[0] + w].astype(np.uint8)
    src = np.stack([A, Bp])
    dst = np.full((h, w), K.FILL, np.uint8)
    M_ = me()
    counts = M_.interp_bilat_sequence_host(M_.planes([src], [w], [w * h]), M_.planes([dst], [w], [w * h]), 1, 0, 0, w, h, 2, 1, B.MB, B.RR,
                                           K.window("ramp", B.MB), mv, [(0, 0, alpha, I.MCI)])
    assert np.array_equal(_interior(dst), _interior(want))
    assert counts["capped"] == 0 and counts["malformed"] == 0


# ---- refusals: identically in both faces, before any device check --------------------------------------------------------------------------
class Args:
    """a legal call of 2 sequences of 3 pictures of 48 x 32, three planes, and what a test changes of it"""

    def __init__(self):
        self.W, self.H, self.nframes, self.nseq, self.mb, self.R = 48, 32, 3, 2, 16, 16
        self.nplanes, self.sw, self.sh = 3, 1, 1
        self.src = [np.zeros(2 * 3 * 48 * 32, np.uint8), np.zeros(2 * 3 * 24 * 16, np.uint8), np.zeros(2 * 3 * 24 * 16, np.uint8)]
        self.dst = [np.zeros(2 * 48 * 32, np.uint8), np.zeros(2 * 24 * 16, np.uint8), np.zeros(2 * 24 * 16, np.uint8)]
        self.sstride, self.dstride = [48, 24, 24], [48, 24, 24]
        self.sframe, self.sseq, self.dframe = [48 * 32, 24 * 16, 24 * 16], [3 * 48 * 32, 3 * 24 * 16, 3 * 24 * 16], [48 * 32, 24 * 16, 24 * 16]
        self.window = np.full(1024, 7, np.uint8)
        self.mv = np.zeros(2 * 2 * 6 * 2, np.int16)
        self.jobs = [(0, 0, 512, I.MCI), (1, 1, 100, I.BLEND)]
        self.scene, self.action = np.zeros(4, np.uint8), 1
        self.null = set()

    def call(self, face):
        from ffmpeg_amd import _lib
        import ctypes as C
        m = me()
        L = _lib.lib()
        ad = lambda a: None if a is None else (a if isinstance(a, int) else a.ctypes.data)
        src = m.planes([ad(a) for a in self.src], self.sstride, self.sframe, self.sseq)
        dst = m.planes([ad(a) for a in self.dst], self.dstride, self.dframe)
        jobs = m.interp_jobs(self.jobs)
        njobs = getattr(self, "njobs", len(self.jobs))
        a = [None if "src" in self.null else C.addressof(src), None if "dst" in self.null else C.addressof(dst), self.nplanes, self.sw, self.sh,
             self.W, self.H, self.nframes, self.nseq, self.mb, self.R, ad(self.window), ad(self.mv), None if "jobs" in self.null else C.addressof(jobs),
             njobs, ad(self.scene), self.action]
        if face == "dev":
            rc = L.ffhip_me_interp_bilat_sequence_dev(*a, None)
        else:
            rc = L.ffhip_me_interp_bilat_sequence_host(*a)
        return rc, L.ffhip_last_error().decode()


def _with(**kw):
    def f(a):
        for k, v in kw.items():
            setattr(a, k, v)
    return f


def _null(what):
    return lambda a: a.null.add(what)


def _plane(which, i, value):
    def f(a):
        getattr(a, which)[i] = value
    return f


def _mv_in_dst(a):
    a.mv = a.dst[0][:96].view(np.int16)


def _scene_in_dst(a):
    a.scene = a.dst[1][:4]


REFUSALS = [
    ("a NULL src", _null("src"), "a NULL src, dst, window or jobs"),
    ("a NULL window", _with(window=None), "a NULL src, dst, window or jobs"),
    ("a NULL jobs", _null("jobs"), "a NULL src, dst, window or jobs"),
    ("nplanes 2", _with(nplanes=2), "nplanes 2 is neither 1 nor 3"),
    ("a NULL plane", _plane("dst", 2, None), "plane 2 of dst is NULL"),
    ("a chroma shift of 2", _with(sw=2), "chroma shifts 2, 1 (0 or 1 each)"),
    ("mb_size 32", _with(mb=32), "mb_size 32 (16 or 8)"),
    ("mv_range 257", _with(R=257), "mv_range 257 outside 0..256"),
    ("a negative nseq", _with(nseq=-1), "a negative width, height, nframes, nseq or njobs"),
    ("a negative njobs", _with(njobs=-1), "a negative width, height, nframes, nseq or njobs"),
    ("a width above 32768", _with(W=32769), "do not fit the int16 vector fields"),
    ("a stride below the width", _plane("sstride", 1, 23), "plane 1: a stride (src 23, dst 24) below the plane's width 24"),
    ("a frame_pitch below the picture", _plane("sframe", 0, 48 * 32 - 1), "plane 0: src frame_pitch 1535 < stride * height 1536"),
    ("a seq_pitch below the sequence", _plane("sseq", 2, 3 * 24 * 16 - 1), "plane 2: src seq_pitch 1151 <"),
    ("a dst frame_pitch below the picture", _plane("dframe", 1, 24 * 16 - 1), "plane 1: dst frame_pitch 383 < stride * height 384"),
    ("a job's pair", _with(jobs=[(0, 0, 0, 0), (0, 2, 0, 0)]), "job 1: seq 0 (0..1), pair 2 (0..1)"),
    ("a job's alpha", _with(jobs=[(0, 0, 1025, 0)]), "job 0: seq 0 (0..1), pair 0 (0..1), alpha 1025 (0..1024)"),
    ("a job's mode", _with(jobs=[(0, 0, 5, 2)]), "mode 2 (0 or 1)"),
    ("a NULL mv with an MCI job", _with(mv=None), "a NULL mv with an MCI job"),
    ("dst overlaps mv", _mv_in_dst, "dst overlaps src, or mv"),
    ("scene_action 3", _with(action=3), "scene_action 3 (1: blend, 2: duplicate)"),
    ("dst overlaps scene", _scene_in_dst, "dst overlaps scene"),
]


@pytest.mark.parametrize("face", ["host", "dev"])
@pytest.mark.parametrize("what", [r[0] for r in REFUSALS])
def test_refusal(what, face):
    _, change, text = next(r for r in REFUSALS if r[0] == what)
    a = Args()
    change(a)
    rc, err = a.call(face)
    assert rc == EINVAL and err.startswith(WHO) and text in err, (rc, err)


def test_the_legal_call_runs_and_what_needs_no_field():
    from ffmpeg_amd import _lib
    a = Args()
    assert a.call("host")[0] == 0
    a = Args()
    a.scene = None                      # scene may be NULL
    assert a.call("host")[0] == 0
    a = Args()
    a.mv, a.jobs = None, [(0, 0, 7, I.BLEND)]
    assert a.call("host")[0] == 0
    a = Args()
    a.jobs = []
    assert a.call("host")[0] == 0 and a.call("dev")[0] == 0      # no jobs: nothing is done, with or without a device
    if _lib.lib().ffhip_device_count() == 0:
        assert Args().call("dev")[0] == ENOSYS
    # the existing faces' texts still name the existing faces
    m = me()
    with pytest.raises(RuntimeError, match="ffhip_me_interp_sequence_dev / _host: mb_size 4"):
        m.interp_sequence_host(m.planes([a.src[0]], [48], [48 * 32]), m.planes([a.dst[0]], [48], [48 * 32]), 1, 0, 0, 48, 32, 2, 1, 4, 16, a.window, a.mv,
                               a.mv, [(0, 0, 0, 0)])
