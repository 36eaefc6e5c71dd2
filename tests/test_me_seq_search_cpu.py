"""CPU tier of the predictive motion searches of whole sequences (ffhip_me_search_pred_sequence_host / _dev): the face is DEFINED as a
loop of calls of the pair face, step k's prev fields being steps k - 1 and k - 2 of its own output (init1 / init2 before them).  So the
reference here is never the new face: it is that loop over the existing ffhip_me_search_pred_frames_host, and the same loop over the
model of tests/me_pred_search_model.py, as test_me_pred_search_cpu.chain() runs it.  Vectors, costs and cost counts must agree.

Whether pair k really read the fields of pairs k - 1 and k - 2 shows only on inputs where nothing else finds the match: made() builds
white-noise sequences whose blocks move so that the accelerator 2 * rel1 - rel2, the collocated vector, or prev1's left, top, right or
bottom neighbour alone reaches a match of cost 0.  No device is needed.  tests/test_gpu_me_seq_search.py takes its inputs and references
from here."""
import collections
import ctypes as C
import functools

import numpy as np
import pytest

import ffi
import me_pred_search_model as M
import test_me_pred_search_cpu as T
from test_me_search_cpu import Guarded

EINVAL, ENOSYS = -22, -38

#: (w, h, pad, mb, R): one block row, two rows, one column, two columns, a padded stride, R = 0, a window larger than the picture
CASES = [(40, 8, 0, 8, 3), (64, 32, 0, 16, 7), (16, 64, 0, 16, 7), (32, 48, 0, 16, 4), (52, 36, 1, 16, 5), (72, 56, 0, 16, 0),
         (96, 80, 3, 16, 32)]
NSEQ, NFRAMES = 3, 6        # what pictures() holds; the calls take the first nseq sequences and the first nframes pictures of it
NSEQS, NFRAMESS = (1, 3), (2, 3, 4, 6)
DIRECTIONS = (0, 1)


def _lib():
    from ffmpeg_amd import _lib
    return _lib.lib()


def origins(w, h, mb):
    """every block's origin as a field of absolute positions, (b_h * b_w * 2,)"""
    return np.array([[(bx * mb, by * mb) for bx in range(w // mb)] for by in range(h // mb)], np.int64).reshape(-1)


@functools.lru_cache(maxsize=None)
def pictures(w, h, pad, mb, R):
    """three sequences of six pictures.  0: a smooth texture that drifts by a changing vector, plus noise of +-1 (test_me_pred_search_cpu
    .chain()'s kind); 1: a rough texture that drifts faster, some blocks frozen; 2: flat with sparse marks that move (ties everywhere).
    And two starting fields of small vectors.  -> frames (3, 6, h, stride) uint8, init1, init2 (3, b_h * b_w * 2) int16, read-only"""
    rng = np.random.default_rng(ffi.stable_seed("me_seq_search", w, h, pad, mb, R))
    stride, m = w + pad, 48
    frames = np.zeros((NSEQ, NFRAMES, h, stride), np.uint8)
    smooth = T.texture(rng, h + 2 * m, w + 2 * m)
    rough = 0.5 * T.texture(rng, h + 2 * m, w + 2 * m) + 0.5 * rng.integers(0, 256, (h + 2 * m, w + 2 * m))
    s = max(1, min(R, 5))
    for q, big in enumerate((smooth, rough)):
        x, y = m, m
        for p in range(NFRAMES):
            x, y = x + int(rng.integers(-s, s + 1)), y + int(rng.integers(-s, s + 1))
            frames[q, p, :, :w] = np.clip(np.round(big[y:y + h, x:x + w] + rng.integers(-1, 2, (h, w))), 0, 255)
            if q == 1 and p:
                frames[q, p, :mb, :mb] = frames[q, p - 1, :mb, :mb]
    for p in range(NFRAMES):
        frames[2, p, :, :w] = 128
        frames[2, p, p % 5::5, (2 * p) % 7:w:7] = 130
    o = origins(w, h, mb)
    init = [np.clip(o + rng.integers(-min(R, 3), min(R, 3) + 1, (NSEQ, o.size)), 0, 32767).astype(np.int16) for _ in range(2)]
    for a in [frames] + init:
        a.setflags(write=False)
    return frames, init[0], init[1]


def pairs_of(frames, k, direction):
    """cur, ref of step k: (nseq, h, stride) each"""
    lo, hi = np.ascontiguousarray(frames[:, k]), np.ascontiguousarray(frames[:, k + 1])
    return (lo, hi) if direction else (hi, lo)


def chained(one_step, frames, direction, init1, init2):
    """THE DEFINITION: one_step(cur, ref, prev1, prev2) -> (mv, cost, n), the pair face over the nseq pairs of a step, chained.
    -> mv (np, nseq, b * 2), cost (np, nseq, b), [n] per step"""
    outs = []
    for k in range(frames.shape[1] - 1):
        prev1 = outs[k - 1][0] if k >= 1 else init1
        prev2 = outs[k - 2][0] if k >= 2 else (init1 if k == 1 else init2)
        cur, ref = pairs_of(frames, k, direction)
        outs.append(one_step(cur, ref, prev1, prev2))
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs]), [o[2] for o in outs]


def chained_host(method, kind, frames, w, h, mb, R, direction, init1, init2):
    """the loop over the existing host face; n = (blocks, costs)"""
    return chained(lambda cur, ref, p1, p2: T.host_face(method, kind, cur, ref, w, h, mb, R, p1, p2), frames, direction, init1, init2)


def chained_model(method, kind, frames, w, h, mb, R, direction, init1, init2):
    """the loop over the model; n = costs"""
    return chained(lambda cur, ref, p1, p2: M.frames(method, cur, ref, w, h, mb, R, kind, p1, p2), frames, direction, init1, init2)


@functools.lru_cache(maxsize=None)
def reference(method, kind, direction, w, h, pad, mb, R):
    """the model's chained run over all of pictures(...), once.  A call over the first nseq sequences and the first nframes pictures is a
    prefix of it: step k reads pictures k and k + 1 and steps k - 1, k - 2, sequence s only itself."""
    frames, i1, i2 = pictures(w, h, pad, mb, R)
    per = (w // mb) * (h // mb)
    mv, cost, ns = np.zeros((NFRAMES - 1, NSEQ, per * 2), np.int16), np.zeros((NFRAMES - 1, NSEQ, per), np.uint32), np.zeros((NFRAMES - 1, NSEQ), np.int64)
    for s in range(NSEQ):       # sequence by sequence, so that the costs evaluated are known per sequence
        m, c, n = chained_model(method, kind, frames[s:s + 1], w, h, mb, R, direction, i1[s:s + 1], i2[s:s + 1])
        mv[:, s:s + 1], cost[:, s:s + 1], ns[:, s] = m, c, n
    for a in (mv, cost, ns):
        a.setflags(write=False)
    return mv, cost, ns


def seq_host(method, kind, frames, w, h, mb, R, direction, init1, init2, face=None):
    """ffhip_me_search_pred_sequence_host on guarded copies of frames (nseq, nframes, h, stride) -> mv (np, nseq, b * 2), cost
    (np, nseq, b), (blocks, costs); asserts that nothing outside the outputs changed"""
    nseq, nframes, _, stride = frames.shape
    per, np_ = (w // mb) * (h // mb), max(nframes - 1, 0)
    gf = Guarded(frames)
    g1, g2 = (None if p is None else Guarded(p) for p in (init1, init2))
    gm, gk = Guarded(np.full((np_, nseq, per * 2), 0x5A5A, np.int16)), Guarded(np.full((np_, nseq, per), 0x5A5A5A5A, np.uint32))
    L = _lib()
    rc = L.ffhip_me_search_pred_sequence_host(method, gf.addr, w, h, stride, h * stride, nframes, nframes * h * stride, nseq, direction, mb, R,
                                              kind, g1 and g1.addr, g2 and g2.addr, gm.addr, gk.addr)
    assert rc == 0, (rc, L.ffhip_last_error())
    assert gf.unchanged() and gm.guards_intact() and gk.guards_intact()
    assert (g1 is None or g1.unchanged()) and (g2 is None or g2.unchanged())
    blocks, costs = C.c_uint64(), C.c_uint64()
    L.ffhip_me_search_host_counts(C.byref(blocks), C.byref(costs))
    return gm.body().copy(), gk.body().copy(), (blocks.value, costs.value)


def calls(case):
    """the (nseq, nframes, frames, init1, init2) of a shape: every count of sequences and pictures the face is run with"""
    frames, i1, i2 = pictures(*case)
    for nseq in NSEQS:
        for nframes in NFRAMESS:
            yield nseq, nframes, np.ascontiguousarray(frames[:nseq, :nframes]), np.ascontiguousarray(i1[:nseq]), np.ascontiguousarray(i2[:nseq])


@pytest.mark.parametrize("direction", DIRECTIONS)
@pytest.mark.parametrize("kind", T.KINDS, ids=["sad", "satd"])
@pytest.mark.parametrize("method", T.METHODS, ids=[M.NAMES[m] for m in T.METHODS])
@pytest.mark.parametrize("w,h,pad,mb,R", CASES)
def test_host_face_equals_the_chained_host_face_equals_the_model(w, h, pad, mb, R, method, kind, direction):
    case = (w, h, pad, mb, R)
    wmv, wcost, wn = reference(method, kind, direction, *case)
    per = (w // mb) * (h // mb)
    for nseq, nframes, frames, i1, i2 in calls(case):
        mv, cost, counts = seq_host(method, kind, frames, w, h, mb, R, direction, i1, i2)
        cmv, ccost, cn = chained_host(method, kind, frames, w, h, mb, R, direction, i1, i2)
        what = (nseq, nframes)
        assert np.array_equal(cost, ccost) and np.array_equal(mv, cmv), what
        assert counts == (sum(n[0] for n in cn), sum(n[1] for n in cn)), what
        assert np.array_equal(cost, wcost[:nframes - 1, :nseq]) and np.array_equal(mv, wmv[:nframes - 1, :nseq]), what
        assert counts == ((nframes - 1) * nseq * per, int(wn[:nframes - 1, :nseq].sum())), what


@pytest.mark.parametrize("direction", DIRECTIONS)
@pytest.mark.parametrize("method", T.METHODS, ids=[M.NAMES[m] for m in T.METHODS])
def test_the_chained_run_of_five_pictures(method, direction):
    """test_me_pred_search_cpu.chain()'s pictures as one sequence, NULL starting fields; direction 0 is the run chain() holds"""
    pics, want = T.chain()
    frames = np.ascontiguousarray(pics[None])
    mv, cost, counts = seq_host(method, M.SAD, frames, 64, 48, 16, 7, direction, None, None)
    cmv, ccost, cn = chained_host(method, M.SAD, frames, 64, 48, 16, 7, direction, None, None)
    assert np.array_equal(mv, cmv) and np.array_equal(cost, ccost) and counts == (48, sum(n[1] for n in cn))
    if direction == 0:
        for k in range(4):
            wmv, wcost, wn = want[method][k]
            assert np.array_equal(mv[k], wmv) and np.array_equal(cost[k], wcost), k
        assert counts[1] == sum(w[2] for w in want[method])
    else:
        mmv, mcost, mn = chained_model(method, M.SAD, frames, 64, 48, 16, 7, direction, None, None)
        assert np.array_equal(mv, mmv) and np.array_equal(cost, mcost) and counts[1] == sum(mn)


# ---- sequences that only the chaining solves ----------------------------------------------------------------------------------------
MADE = (96, 80, 0, 16, 8)       # 6 x 5 blocks: interior blocks, every border, every corner
MADE_NAMES = ["accelerator", "collocated", "neighbours"]


def _fits(v, bx, by, w, h, mb, R):
    x0, x1, y0, y1 = T._window(bx, by, w, h, mb, R)
    return x0 <= bx * mb + v[0] <= x1 and y0 <= by * mb + v[1] <= y1


@functools.lru_cache(maxsize=None)
def made():
    """three sequences of six white-noise pictures, direction 0: block b of picture k + 1 is picture k's content at origin + v_b(k), so
    pair k's block b has one match, of cost 0, and no slope leads to it.
      0  v_b(k) = v0_b + k * e_b, e_b != 0, every target inside the block's window for k = -2 .. 4: only 2 * rel1 - rel2 reaches it
      1  v_b(k) = v_b: the collocated vector reaches it
      2  v_b(k) = v_n(k - 1) of a left, top, right or bottom neighbour n chosen per block and pair (its own where none fits the window)
    init1 / init2 hold the true fields of k = -1 and k = -2 (sequence 2: both the field of k = -1).
    -> frames (3, 6, h, w), init1, init2 (3, b * 2) int16, the vectors (3, 7, b_h, b_w, 2) of k = -2 .. 4, read-only"""
    w, h, _, mb, R = MADE
    bw, bh = w // mb, h // mb
    rng = np.random.default_rng(ffi.stable_seed("me_seq_made"))
    ks = list(range(-2, NFRAMES - 1))
    vec = np.zeros((3, len(ks), bh, bw, 2), np.int64)
    for by in range(bh):
        for bx in range(bw):
            while True:         # sequence 0
                v0, e = rng.integers(-4, 5, 2), rng.integers(-1, 2, 2)
                if e.any() and all(_fits(v0 + k * e, bx, by, w, h, mb, R) for k in ks):
                    break
            vec[0, :, by, bx] = [v0 + k * e for k in ks]
            while True:         # sequence 1
                v = rng.integers(-6, 7, 2)
                if v.any() and _fits(v, bx, by, w, h, mb, R):
                    break
            vec[1, :, by, bx] = v
            while True:         # sequence 2, k = -2 and -1
                v = rng.integers(-5, 6, 2)
                if v.any() and _fits(v, bx, by, w, h, mb, R):
                    break
            vec[2, :2, by, bx] = v
    for i in range(2, len(ks)):
        for by in range(bh):
            for bx in range(bw):
                vec[2, i, by, bx] = vec[2, i - 1, by, bx]
                for j in rng.permutation(4):
                    nx, ny = [(bx - 1, by), (bx, by - 1), (bx + 1, by), (bx, by + 1)][j]
                    if 0 <= nx < bw and 0 <= ny < bh and _fits(vec[2, i - 1, ny, nx], bx, by, w, h, mb, R):
                        vec[2, i, by, bx] = vec[2, i - 1, ny, nx]
                        break
    frames = np.zeros((3, NFRAMES, h, w), np.uint8)
    for s in range(3):
        frames[s, 0] = rng.integers(0, 256, (h, w))
        for k in range(NFRAMES - 1):
            for by in range(bh):
                for bx in range(bw):
                    x, y = bx * mb + vec[s, k + 2, by, bx, 0], by * mb + vec[s, k + 2, by, bx, 1]
                    frames[s, k + 1, by * mb:(by + 1) * mb, bx * mb:(bx + 1) * mb] = frames[s, k, y:y + mb, x:x + mb]
    o = origins(w, h, mb)
    init1 = (vec[:, 1].reshape(3, -1) + o).astype(np.int16)
    init2 = (vec[:, 0].reshape(3, -1) + o).astype(np.int16)
    for a in (frames, init1, init2, vec):
        a.setflags(write=False)
    return frames, init1, init2, vec


@functools.lru_cache(maxsize=None)
def made_reference():
    """the chained model over made(), EPZS, SAD, sequence by sequence, with the counters of the pairs k >= 2 -> mv, cost, [Counter]"""
    frames, i1, i2, _ = made()
    w, h, _, mb, R = MADE
    mvs, costs, took = [], [], []
    for s in range(3):
        t, steps = collections.Counter(), []

        def step(cur, ref, p1, p2):
            before = collections.Counter(M.COUNTS)
            out = M.frames(M.EPZS, cur, ref, w, h, mb, R, M.SAD, p1, p2)
            if len(steps) >= 2:         # pairs k >= 2: both prev fields are outputs of the run
                t.update(M.COUNTS)
                t.subtract(before)
            steps.append(out)
            return out
        mv, cost, _ = chained(step, frames[s:s + 1], 0, i1[s:s + 1], i2[s:s + 1])
        mvs.append(mv)
        costs.append(cost)
        took.append(t)
    mv, cost = np.concatenate(mvs, 1), np.concatenate(costs, 1)
    mv.setflags(write=False)
    cost.setflags(write=False)
    return mv, cost, took


def test_the_made_sequences_need_the_chaining():
    """a condition on the INPUTS, asserted on the CPU with the model: over the pairs k >= 2 the accelerator, the collocated vector and
    prev1's four neighbours each win at least once, every block ends on its match, and without the prev fields every pair k >= 1 comes
    out differently"""
    frames, i1, i2, vec = made()
    w, h, _, mb, R = MADE
    mv, cost, took = made_reference()
    assert took[0]["wins_accelerator"] > 0 and took[1]["wins_collocated"] > 0
    for label in ("prev_left", "prev_top", "prev_right", "prev_bottom"):
        assert took[2]["wins_" + label] > 0, (label, took[2])
    assert not cost.any()
    want = vec[:, 2:].reshape(3, NFRAMES - 1, -1) + origins(w, h, mb)
    assert np.array_equal(mv.astype(np.int64), want.transpose(1, 0, 2))
    for k in range(1, NFRAMES - 1):
        cur, ref = pairs_of(frames, k, 0)
        nmv, ncost, _ = T.host_face(M.EPZS, M.SAD, cur, ref, w, h, mb, R, None, None)
        for s in range(3):
            assert not (np.array_equal(nmv[s], mv[k, s]) and np.array_equal(ncost[s], cost[k, s])), (MADE_NAMES[s], k)


@pytest.mark.parametrize("method", T.METHODS, ids=[M.NAMES[m] for m in T.METHODS])
def test_host_face_on_the_made_sequences(method):
    frames, i1, i2, _ = made()
    w, h, _, mb, R = MADE
    mv, cost, counts = seq_host(method, M.SAD, frames, w, h, mb, R, 0, i1, i2)
    cmv, ccost, cn = chained_host(method, M.SAD, frames, w, h, mb, R, 0, i1, i2)
    assert np.array_equal(mv, cmv) and np.array_equal(cost, ccost) and counts == (sum(n[0] for n in cn), sum(n[1] for n in cn))
    if method == M.EPZS:
        wmv, wcost, _ = made_reference()
        assert np.array_equal(mv, wmv) and np.array_equal(cost, wcost)


# ---- the starting fields ------------------------------------------------------------------------------------------------------------
def test_one_null_starting_field_is_a_field_of_origins():
    case = CASES[1]
    w, h, pad, mb, R = case
    frames, i1, i2 = pictures(*case)
    o = np.tile(origins(w, h, mb).astype(np.int16), (NSEQ, 1))
    for a, b, za, zb in ((None, i2, o, i2), (i1, None, i1, o), (None, None, o, o)):
        got = seq_host(M.EPZS, M.SAD, frames, w, h, mb, R, 0, a, b)
        want = seq_host(M.EPZS, M.SAD, frames, w, h, mb, R, 0, za, zb)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    assert not np.array_equal(seq_host(M.EPZS, M.SAD, frames, w, h, mb, R, 0, None, None)[0], seq_host(M.EPZS, M.SAD, frames, w, h, mb, R, 0, i1, i2)[0])


@pytest.mark.parametrize("frames_of", ["pictures", "made"])
def test_a_call_continues_the_one_before(frames_of):
    """6 pictures == 4 pictures, then 3 that start from the first call's last two steps"""
    if frames_of == "made":
        (frames, i1, i2, _), (w, h, _, mb, R) = made(), MADE
    else:
        (frames, i1, i2), (w, h, _, mb, R) = pictures(*CASES[4]), CASES[4]
    for method in T.METHODS:
        mv, cost, counts = seq_host(method, M.SAD, frames, w, h, mb, R, 0, i1, i2)
        mva, costa, na = seq_host(method, M.SAD, np.ascontiguousarray(frames[:, :4]), w, h, mb, R, 0, i1, i2)
        mvb, costb, nb = seq_host(method, M.SAD, np.ascontiguousarray(frames[:, 3:]), w, h, mb, R, 0, mva[2], mva[1])
        assert np.array_equal(np.concatenate([mva, mvb]), mv) and np.array_equal(np.concatenate([costa, costb]), cost)
        assert (na[0] + nb[0], na[1] + nb[1]) == counts


# ---- arguments ----------------------------------------------------------------------------------------------------------------------
PLANE = 64 * 48


def _args(**over):
    """a well-formed call on 64 x 48: two sequences of three pictures; buffers are kept alive by the returned dict"""
    a = dict(method=M.EPZS, width=64, height=48, stride=64, frame_pitch=PLANE, nframes=3, seq_pitch=3 * PLANE, nseq=2, direction=0, mb_size=16,
             search_param=7, cost_kind=M.SAD)
    a["frames"] = np.zeros(6 * PLANE, np.uint8)
    a["init1"], a["init2"] = np.zeros(2 * 12 * 2, np.int16), np.zeros(2 * 12 * 2, np.int16)
    a["mv"], a["cost"] = np.full(2 * 2 * 12 * 2, 7, np.int16), np.zeros(2 * 2 * 12, np.uint32)
    a.update(over)
    return a


def _call(face, a):
    args = [a["method"], T._addr(a["frames"]), a["width"], a["height"], a["stride"], a["frame_pitch"], a["nframes"], a["seq_pitch"], a["nseq"],
            a["direction"], a["mb_size"], a["search_param"], a["cost_kind"], T._addr(a["init1"]), T._addr(a["init2"]), T._addr(a["mv"]),
            T._addr(a["cost"])]
    L = _lib()
    return L.ffhip_me_search_pred_sequence_host(*args) if face == "host" else L.ffhip_me_search_pred_sequence_dev(*(args + [None]))


def _bad():
    """name -> (overrides, a word of the text).  The overlapping ones carve both arrays out of one buffer."""
    pool = np.zeros(16384, np.int16)
    mv = pool[:96]
    tall = dict(nseq=1, nframes=2, init1=None, init2=None)
    bad = {"a NULL frames": (dict(frames=None), "NULL"), "a NULL mv_out": (dict(mv=None), "NULL"), "a NULL cost_out": (dict(cost=None), "NULL"),
           "mb_size 4": (dict(mb_size=4), "mb_size 4"), "mb_size 32": (dict(mb_size=32), "mb_size 32"),
           "cost_kind 2": (dict(cost_kind=2), "cost_kind 2"), "cost_kind -1": (dict(cost_kind=-1), "cost_kind -1"),
           "a negative width": (dict(width=-16), "negative"), "a negative height": (dict(height=-16), "negative"),
           "a negative nframes": (dict(nframes=-1), "negative"), "a negative search_param": (dict(search_param=-1), "negative"),
           "stride < width": (dict(stride=63), "stride < width"), "a negative stride": (dict(stride=-64), "stride < width"),
           "frame_pitch < stride * height": (dict(frame_pitch=PLANE - 1), "frame_pitch < stride * height"),
           "method 0": (dict(method=0), "method 0 is neither EPZS"), "method 7": (dict(method=7), "method 7 is neither EPZS"),
           "method 10": (dict(method=10), "method 10 is neither EPZS"),
           "a width above 32768": (dict(width=32784, stride=32784, height=16, frame_pitch=16 * 32784, frames=np.zeros(2 * 16 * 32784, np.uint8),
                                        mv=np.zeros(2 * 2049, np.int16), cost=np.zeros(2049, np.uint32), **tall), "32784 x 16"),
           "a height above 32768": (dict(height=32776, width=16, stride=16, frame_pitch=16 * 32776, frames=np.zeros(2 * 16 * 32776, np.uint8),
                                         mv=np.zeros(2 * 2048, np.int16), cost=np.zeros(2048, np.uint32), **tall), "16 x 32776"),
           "mv_out at an odd dword": (dict(mv=pool[1:97]), "4-byte aligned"),
           "direction 2": (dict(direction=2), "direction 2"), "direction -1": (dict(direction=-1), "direction -1"),
           "a negative nseq": (dict(nseq=-1), "negative nseq"),
           "seq_pitch one byte short": (dict(seq_pitch=3 * PLANE - 1), "seq_pitch"),
           "seq_pitch of one picture": (dict(seq_pitch=PLANE), "seq_pitch"),
           "seq_pitch 0": (dict(seq_pitch=0), "seq_pitch"),
           "mv_out overlapping init1": (dict(mv=mv, init1=pool[94:142]), "overlaps"),
           "mv_out overlapping init2": (dict(mv=mv, init2=pool[2:50]), "overlaps"),
           "mv_out equal to init1": (dict(mv=mv, init1=mv), "overlaps"),
           "mv_out overlapping cost_out": (dict(mv=mv, cost=pool[90:186].view(np.uint32)), "overlaps"),
           "mv_out inside frames": (dict(mv=mv, frames=pool.view(np.uint8)[:6 * PLANE]), "overlaps"),
           "mv_out at the last sample of frames": (dict(mv=pool[3 * PLANE - 2:3 * PLANE + 94], frames=pool.view(np.uint8)[:6 * PLANE]), "overlaps"),
           "more blocks than an int counts": (dict(nframes=2 ** 31 - 1, nseq=1, init1=None, init2=None), "2^31 - 1 blocks"),
           "more blocks than an int counts, by sequences": (dict(nseq=2 ** 31 - 1, seq_pitch=3 * PLANE), "2^31 - 1 blocks")}
    return bad


BAD = _bad()


@pytest.mark.parametrize("face", ["host", "dev"])
@pytest.mark.parametrize("what", sorted(BAD))
def test_einval(what, face):
    """each refusal alone, on both faces, before any device check, with its text; nothing is written.  The well-formed call goes to
    the device face only where there is no device: these are host arrays, and a launch would follow their pointers"""
    if face == "host":
        assert _call(face, _args()) == 0
    elif _lib().ffhip_device_count() == 0:
        assert _call(face, _args()) == ENOSYS
    over, word = BAD[what]
    a = _args(**over)
    if a["mv"] is not None:
        a["mv"][:] = 7
    assert _call(face, a) == EINVAL
    text = _lib().ffhip_last_error().decode()
    assert "ffhip_me_search_pred_sequence" in text and word in text and "FFHIP_" not in text, text
    assert a["mv"] is None or (a["mv"] == 7).all()


def test_the_refusals_have_texts_of_their_own():
    texts = set()
    for what in ("a NULL frames", "method 0", "a width above 32768", "mv_out at an odd dword", "direction 2", "a negative nseq",
                 "seq_pitch 0", "mv_out equal to init1", "more blocks than an int counts"):
        assert _call("host", _args(**BAD[what][0])) == EINVAL
        texts.add(_lib().ffhip_last_error().decode())
    assert len(texts) == 9


def test_what_is_legal_at_the_edges():
    pool = np.zeros(4096, np.int16)
    for over in (dict(nframes=0), dict(nframes=1), dict(nseq=0), dict(width=15), dict(height=8), dict(width=0, height=0, stride=0)):
        a = _args(**over)
        assert _call("host", a) == 0 and (a["mv"] == 7).all(), over        # nothing is done
        assert _counts() == (0, 0)
    assert _call("host", _args(nframes=1, frame_pitch=1, seq_pitch=PLANE)) == 0             # one picture: frame_pitch is not used
    assert _call("host", _args(nseq=1, seq_pitch=0)) == 0                                   # one sequence: seq_pitch is not used
    assert _call("host", _args(nframes=0, mv=pool[:96], init1=pool[:48])) == 0              # no blocks: nothing overlaps
    assert _call("host", _args(mv=pool[:96], init1=pool[96:144], init2=pool[144:192])) == 0     # touching is not overlapping
    assert _call("host", _args(init1=pool[:48], init2=pool[:48])) == 0                      # the two inputs may be one field
    assert _call("host", _args(init1=None)) == 0 and _call("host", _args(init2=None)) == 0
    assert _call("host", _args(direction=1)) == 0 and _call("host", _args(method=M.UMH, search_param=2 ** 31 - 1)) == 0
    assert _call("host", _args(search_param=0)) == 0 and _counts()[0] == 2 * 2 * 12


def _counts():
    blocks, costs = C.c_uint64(), C.c_uint64()
    _lib().ffhip_me_search_host_counts(C.byref(blocks), C.byref(costs))
    return blocks.value, costs.value


def test_device_face_without_a_device():
    L = _lib()
    if L.ffhip_device_count() > 0:
        pytest.skip("a HIP device is present: the refusal is not reachable")
    for method in T.METHODS:
        for over in (dict(), dict(nframes=1), dict(nseq=0)):
            a = _args(method=method, **over)
            assert _call("dev", a) == ENOSYS and (a["mv"] == 7).all()


def test_python_face_on_the_host():
    from ffmpeg_amd import me
    case = CASES[4]
    w, h, pad, mb, R = case
    frames, i1, i2 = pictures(*case)
    stride, per = w + pad, (w // mb) * (h // mb)
    for method in T.METHODS:
        for direction in DIRECTIONS:
            wmv, wcost, wn = reference(method, M.SATD, direction, *case)
            mv, cost = np.zeros_like(wmv), np.zeros_like(wcost)
            got = me.search_pred_sequence_host(method, np.array(frames), w, h, stride, h * stride, NFRAMES, NFRAMES * h * stride, NSEQ, direction, mb,
                                               R, me.SATD, np.array(i1), np.array(i2), mv, cost)
            assert np.array_equal(mv, wmv) and np.array_equal(cost, wcost) and got == ((NFRAMES - 1) * NSEQ * per, int(wn.sum()))
    mv, cost = np.zeros((NFRAMES - 1, NSEQ, per * 2), np.int16), np.zeros((NFRAMES - 1, NSEQ, per), np.uint32)
    me.search_pred_sequence_host(me.EPZS, np.array(frames), w, h, stride, h * stride, NFRAMES, NFRAMES * h * stride, NSEQ, 0, mb, R, me.SAD, None,
                                 None, mv, cost)
    assert np.array_equal(mv, chained_host(M.EPZS, M.SAD, frames, w, h, mb, R, 0, None, None)[0])
    with pytest.raises(RuntimeError, match="direction 3"):
        me.search_pred_sequence_host(me.EPZS, np.array(frames), w, h, stride, h * stride, NFRAMES, NFRAMES * h * stride, NSEQ, 3, mb, R, me.SAD,
                                     None, None, mv, cost)


def test_the_two_symbols_are_exported():
    """both libraries export the faces as include/ffhip.h declares them (tests/test_abi.py checks every declaration of the header)"""
    import os
    import re
    import ffmpeg_amd
    root = os.path.dirname(os.path.abspath(ffmpeg_amd.__file__))
    header = open(os.path.join(os.path.dirname(root), "include", "ffhip.h")).read()
    for name in ("ffhip_me_search_pred_sequence_dev", "ffhip_me_search_pred_sequence_host"):
        assert re.search(r"^int %s\(int method, const uint8_t \*frames," % name, header, re.M)
        for lib in ("libffhip.so", "libffhip_measure.so"):
            assert hasattr(C.CDLL(os.path.join(root, lib)), name), (lib, name)
