"""CPU tier of the filter's per-block motion searches (ffhip_me_search_frames_host / ffhip_me_search_batch_dev): the host face runs
kernels/me_search_rules.h — the code the kernel runs — on the CPU, and must equal tests/me_search_model.py, the model written from the
rules text of include/ffhip.h, for every method, metric and block size; the model's counters show that the inputs reach every branch of
the rules.  No device is needed.  tests/test_gpu_me_search.py takes its inputs and references from here."""
import ctypes as C
import collections
import functools

import numpy as np
import pytest

import ffi
import me_search_model as M
from ffi import i16p, ptr
from test_gpu_me import _shifted_pair

EINVAL, ENOSYS = -22, -38
GUARD = 0xA5
NG = 256            # guard bytes on each side

#: (w, h, pad, mb, R) of the issue: a width that is no multiple of mb, R = 0, R = 1, a window larger than the picture
SHAPES = [(64, 48, 0, 16, 7), (52, 36, 1, 16, 5), (40, 40, 0, 8, 3), (72, 56, 0, 16, 0), (64, 64, 0, 8, 1), (96, 80, 3, 16, 32)]
#: every shape at both block sizes (its own first)
CASES = [(w, h, pad, m, R) for (w, h, pad, mb, R) in SHAPES for m in (mb, 24 - mb)]
METHODS = list(range(1, 8))
KINDS = [M.SAD, M.SATD]


def _lib():
    from ffmpeg_amd import _lib
    return _lib.lib()


@functools.lru_cache(maxsize=None)
def pairs(w, h, pad, mb, R):
    """three frame pairs, as tests/test_gpu_me.py::test_esa_frames builds them: shifted texture + noise, one with exactly matching
    blocks, one flat with sparse marks (ties).  -> cur, ref (3, h, stride) uint8, read-only"""
    rng = np.random.default_rng(ffi.stable_seed("me_search", w, h, pad, mb, R))
    stride = w + pad
    curs, refs = [], []
    for f in range(3):
        c, r, _, _ = _shifted_pair(rng, w, h, stride, max(R, 1), flat=(f == 2))
        if f == 1:
            c[:mb * 2, :mb * 2] = r[:mb * 2, :mb * 2]
        curs.append(c)
        refs.append(r)
    cur, ref = np.stack(curs), np.stack(refs)
    cur.setflags(write=False)
    ref.setflags(write=False)
    return cur, ref


@functools.lru_cache(maxsize=None)
def reference(method, kind, w, h, pad, mb, R):
    """the model's vectors and costs of pairs(...), computed once, with the branch counters that run added: (mv, cost, ncosts, Counter)"""
    cur, ref = pairs(w, h, pad, mb, R)
    before = collections.Counter(M.COUNTS)
    mv, cost, n = M.frames(method, cur, ref, w, h, mb, R, kind)
    took = collections.Counter(M.COUNTS)
    took.subtract(before)
    mv.setflags(write=False)
    cost.setflags(write=False)
    return mv, cost, n, took


class Guarded:
    """bytes of `a` between two runs of guard bytes, nothing else: a plane that ends exactly at height * stride ends at the guard"""

    def __init__(self, a):
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        self.buf = np.full(raw.size + 2 * NG, GUARD, np.uint8)
        self.buf[NG:NG + raw.size] = raw
        self.n, self.dtype, self.shape, self.before = raw.size, a.dtype, a.shape, raw.copy()

    @property
    def addr(self):
        return self.buf.ctypes.data + NG

    def body(self):
        return self.buf[NG:NG + self.n].view(self.dtype).reshape(self.shape)

    def guards_intact(self):
        return (self.buf[:NG] == GUARD).all() and (self.buf[NG + self.n:] == GUARD).all()

    def unchanged(self):
        return self.guards_intact() and np.array_equal(self.buf[NG:NG + self.n], self.before)


def host_face(method, kind, cur, ref, w, h, mb, R):
    """ffhip_me_search_frames_host on guarded copies -> mv, cost, (blocks, costs); asserts that nothing outside the outputs changed"""
    nf, _, stride = cur.shape
    bw, bh = w // mb, h // mb
    gc, gr = Guarded(cur), Guarded(ref)
    gm, gk = Guarded(np.full((nf, bh * bw * 2), 0x5A5A, np.int16)), Guarded(np.full((nf, bh * bw), 0x5A5A5A5A, np.uint32))
    L = _lib()
    rc = L.ffhip_me_search_frames_host(method, gc.addr, gr.addr, w, h, stride, h * stride, nf, mb, R, kind, gm.addr, gk.addr)
    assert rc == 0, (rc, L.ffhip_last_error())
    assert gc.unchanged() and gr.unchanged() and gm.guards_intact() and gk.guards_intact()
    blocks, costs = C.c_uint64(), C.c_uint64()
    L.ffhip_me_search_host_counts(C.byref(blocks), C.byref(costs))
    return gm.body().copy(), gk.body().copy(), (blocks.value, costs.value)


@pytest.mark.parametrize("kind", KINDS, ids=["sad", "satd"])
@pytest.mark.parametrize("method", METHODS, ids=[M.NAMES[m] for m in METHODS])
@pytest.mark.parametrize("w,h,pad,mb,R", CASES)
def test_host_face_equals_the_model(w, h, pad, mb, R, method, kind):
    cur, ref = pairs(w, h, pad, mb, R)
    wmv, wcost, wn, _ = reference(method, kind, w, h, pad, mb, R)
    mv, cost, (blocks, costs) = host_face(method, kind, cur, ref, w, h, mb, R)
    assert np.array_equal(cost, wcost)
    assert np.array_equal(mv, wmv)
    assert blocks == 3 * (w // mb) * (h // mb) and costs == wn      # the rules header evaluates what the text says, no more


@pytest.mark.parametrize("kind", KINDS, ids=["sad", "satd"])
@pytest.mark.parametrize("w,h,pad,mb,R", CASES)
def test_method_1_equals_the_oracles_exhaustive_search(w, h, pad, mb, R, kind):
    cur, ref = pairs(w, h, pad, mb, R)
    mv, cost, _ = host_face(M.ESA, kind, cur, ref, w, h, mb, R)
    bw, bh = w // mb, h // mb
    for f in range(3):
        wmv, wcost = np.zeros(bh * bw * 2, np.int16), np.zeros(bh * bw, np.uint32)
        ffi.oracle().ffo_me_esa_frame(ptr(cur[f]), ptr(ref[f]), w + pad, w, h, mb, R, kind, ptr(wmv, i16p), wcost.ctypes.data_as(C.POINTER(C.c_uint32)))
        assert np.array_equal(cost[f], wcost) and np.array_equal(mv[f], wmv), f


def test_the_inputs_reach_every_branch():
    """every counter of the model is non-zero over the inputs of test_host_face_equals_the_model"""
    total = collections.Counter()
    for case in CASES:
        for method in METHODS:
            for kind in KINDS:
                total.update(reference(method, kind, *case)[3])
    assert not [b for b in M.BRANCHES if total[b] <= 0], total


# ---- hand-made cases: one block of a paraboloid plane, whose cost falls towards the one position that matches ---------------------
def _bowl(target, method, R=7, mb=16):
    """64 x 64, the block at (32, 32) holds what the reference holds at 32 + target: -> (mv - (32, 32), cost) of host face and model,
    and the model's counters of that block"""
    yy, xx = np.mgrid[0:64, 0:64]
    ref = ((xx * xx + yy * yy) // 33).astype(np.uint8)[None]
    cur = np.zeros_like(ref)
    tx, ty = 32 + target[0], 32 + target[1]
    cur[0, 32:32 + mb, 32:32 + mb] = ref[0, ty:ty + mb, tx:tx + mb]
    before = collections.Counter(M.COUNTS)
    x, y, c, _ = M.search(method, cur[0], ref[0], 64, 64, mb, R, M.SAD, 32, 32)
    took = collections.Counter(M.COUNTS)
    took.subtract(before)
    mv, cost, _ = host_face(method, M.SAD, cur, ref, 64, 64, mb, R)
    b = 2 * (64 // mb) + 2
    assert (int(mv[0, 2 * b]), int(mv[0, 2 * b + 1]), int(cost[0, b])) == (x, y, c)
    return (x - 32, y - 32), c, took


def test_ntss_minimum_beside_the_unit_ring():
    """the best position is (1, 2): the unit ring of the first iteration beats the large one (step 4) and moves the centre next to it;
    only the closing unit ring round the NEW centre reaches (1, 2).  TSS, with the same steps, ends elsewhere."""
    mv, cost, took = _bowl((1, 2), M.NTSS)
    assert (mv, cost) == ((1, 2), 0) and took["ntss_exit_unit_ring"] == 1 and not took["ntss_exit_large_ring"]
    assert _bowl((1, 2), M.TSS)[:2] != ((1, 2), 0)


def test_ntss_minimum_on_the_large_ring():
    """the best position is (5, 3): the large ring (step 4) beats the unit ring, first = 0, and the search goes on as TSS: steps 2, 1"""
    mv, cost, took = _bowl((5, 3), M.NTSS)
    assert (mv, cost) == ((5, 3), 0) and took["ntss_exit_large_ring"] == 1 and not took["ntss_exit_unit_ring"]


def test_ntss_minimum_at_the_centre():
    mv, cost, took = _bowl((0, 0), M.NTSS)          # cost 0 at the start: no ring at all
    assert (mv, cost) == ((0, 0), 0) and took["zero_cost_start"] == 1 and not took["ntss_exit_centre"]


def test_tdls_halves_twice():
    """the best position is (1, 0): the diamonds of step 4 and of step 2 keep the centre (two halvings), the one of step 1 finds it"""
    mv, cost, took = _bowl((1, 0), M.TDLS)
    assert (mv, cost) == ((1, 0), 0) and took["tdls_centre_moved"] == 1 and took["tdls_centre_kept"] == 3


def test_ds_and_hexbs_walk_and_refine():
    """(7, 6) is several large patterns away: both methods walk there in more than one move, stop when a pattern keeps its centre, and
    end on it exactly after the closing dia1"""
    for method in (M.DS, M.HEXBS):
        mv, cost, took = _bowl((7, 6), method)
        assert took["%s_centre_moved" % M.NAMES[method]] >= 2 and took["%s_centre_kept" % M.NAMES[method]] == 1
        assert (mv, cost) == ((7, 6), 0)


def test_fss_keeps_step_2_while_it_moves():
    mv, cost, took = _bowl((6, 0), M.FSS)
    assert took["fss_centre_moved"] >= 3 and took["fss_centre_kept"] == 2 and mv == (6, 0)


# ---- arguments ------------------------------------------------------------------------------------------------------------------
def _args(**over):
    """a well-formed call on 64 x 48, two frames; buffers are kept alive by the returned dict"""
    a = dict(method=M.HEXBS, width=64, height=48, stride=64, frame_pitch=64 * 48, nframes=2, mb_size=16, search_param=7, cost_kind=M.SAD)
    a["cur"], a["ref"] = np.zeros(2 * 64 * 48, np.uint8), np.zeros(2 * 64 * 48, np.uint8)
    a["mv"], a["cost"] = np.zeros(2 * 12 * 2, np.int16), np.zeros(2 * 12, np.uint32)
    a.update(over)
    return a


def _call(face, a):
    p = lambda v: None if v is None else v.ctypes.data
    args = [a["method"], p(a["cur"]), p(a["ref"]), a["width"], a["height"], a["stride"], a["frame_pitch"], a["nframes"], a["mb_size"],
            a["search_param"], a["cost_kind"], p(a["mv"]), p(a["cost"])]
    L = _lib()
    return L.ffhip_me_search_frames_host(*args) if face == "host" else L.ffhip_me_search_batch_dev(*(args + [None]))


BAD = {"a NULL cur": dict(cur=None), "a NULL ref": dict(ref=None), "a NULL mv_out": dict(mv=None), "a NULL cost_out": dict(cost=None),
       "method 0": dict(method=0), "method 10": dict(method=10), "method -1": dict(method=-1), "mb_size 4": dict(mb_size=4),
       "mb_size 32": dict(mb_size=32), "mb_size 12": dict(mb_size=12), "cost_kind 2": dict(cost_kind=2), "cost_kind -1": dict(cost_kind=-1),
       "a negative width": dict(width=-16), "a negative height": dict(height=-16), "a negative nframes": dict(nframes=-1),
       "a negative search_param": dict(search_param=-1), "stride < width": dict(stride=63), "a negative stride": dict(stride=-64),
       "frame_pitch < stride * height": dict(frame_pitch=64 * 48 - 1)}


@pytest.mark.parametrize("face", ["host", "dev"])
@pytest.mark.parametrize("what", sorted(BAD))
def test_einval(what, face):
    """each refusal alone, on both faces, before any device check (the device face answers the same with or without a device)"""
    assert _call(face, _args()) in ((0,) if face == "host" else (0, ENOSYS))
    a = _args(**BAD[what])
    assert _call(face, a) == EINVAL
    assert not a["mv"].any() if a["mv"] is not None else True


def test_what_is_legal_at_the_edges():
    assert _call("host", _args(frame_pitch=1, nframes=1)) == 0                    # one frame: the pitch is not used
    a = _args(nframes=0, mv=np.full(4, 7, np.int16))
    assert _call("host", a) == 0 and (a["mv"] == 7).all()                         # nothing is done
    a = _args(width=15, mv=np.full(4, 7, np.int16))
    assert _call("host", a) == 0 and (a["mv"] == 7).all()                         # no whole block
    assert _call("host", _args(search_param=0)) == 0
    assert _call("host", _args(search_param=2 ** 31 - 1)) == 0                    # the window and the steps do not overflow
    assert _call("host", _args(width=0, height=0, stride=0)) == 0


@pytest.mark.parametrize("face", ["host", "dev"])
@pytest.mark.parametrize("method,name", [(8, "EPZS"), (9, "UMH")])
def test_epzs_and_umh_are_refused_by_name(method, name, face):
    L = _lib()
    a = _args(method=method, mv=np.full(48, 7, np.int16))
    assert _call(face, a) == ENOSYS and (a["mv"] == 7).all()
    text = L.ffhip_last_error().decode()
    assert name in text and "neighbouring blocks' vectors" in text and "FFHIP_" not in text
    assert _call(face, _args(method=method, cur=None)) == EINVAL                  # the argument checks come first


def test_device_face_without_a_device():
    L = _lib()
    if L.ffhip_device_count() > 0:
        pytest.skip("a HIP device is present: the refusal is not reachable")
    for method in METHODS:
        a = _args(method=method, mv=np.full(48, 7, np.int16))
        assert _call("dev", a) == ENOSYS and (a["mv"] == 7).all()


def test_python_face_on_the_host():
    from ffmpeg_amd import me
    assert (me.ESA, me.TSS, me.TDLS, me.NTSS, me.FSS, me.DS, me.HEXBS, me.EPZS, me.UMH) == tuple(range(1, 10))
    w, h, pad, mb, R = SHAPES[0]
    cur, ref = pairs(w, h, pad, mb, R)
    wmv, wcost, wn, _ = reference(me.DS, me.SATD, w, h, pad, mb, R)
    mv, cost = np.zeros_like(wmv), np.zeros_like(wcost)
    blocks, costs = me.search_frames_host(me.DS, np.ascontiguousarray(cur), np.ascontiguousarray(ref), w, h, w + pad, h * (w + pad), 3, mb, R,
                                          me.SATD, mv, cost)
    assert np.array_equal(mv, wmv) and np.array_equal(cost, wcost) and (blocks, costs) == (36, wn)
    with pytest.raises(RuntimeError, match="UMH"):
        me.search_frames_host(me.UMH, np.ascontiguousarray(cur), np.ascontiguousarray(ref), w, h, w + pad, h * (w + pad), 3, mb, R, me.SAD, mv, cost)
