"""The cells of the VP9 loop filter (kernels/vp9_lf.hip: vp9_lf_line behind k_vp9_loop_filter, k_vp9_lf_frame and the _ssc kernels;
the branch-free vp9_lf_line2 behind k_vp9_lf_frame_wg) as deterministic lists, shared by tests/test_vp9_lf_matrix_cpu.py and
tests/test_gpu_vp9_lf_matrix.py.  Nothing is random but the seeded background of the buffers.

A *cell* is one 16-sample line p7 .. p0 q0 .. q7 built by construction with its width and limits (E, I, H in 8-bit units, scaled by
F = 1 << (bd - 8) as the reference scales them), the label it is built for (none / tap_hev / tap_soft / flat8 / flat16) and the set
of output indices that must change.  lf_model() is loop_filter() of vp9dsp_template.c restated line by line; it takes the name of a
*mutation* — one decision of the rule changed — and MUTATIONS lists them all: the CPU tier shows that every mutation changes some
cell's output on every route, which is the proof that a kernel wrong in that decision would fail.  Eight cells that share width and
limits make a *record* (one 8-line segment: a FFHipVp9Edge of the batch face, a table entry of the frame faces).

Batch routes (the conditions of vp9_lf_lines):
  R1   column edge, every line address on a dword: the wide loads and the per-dword write-back mask
  R2   column edge off the dword grid (an odd record offset or an unaligned base): sample by sample
  R3   row edge
  R4   column edge on a stride off the dword grid: the lines of one record alternate between the wide path (R4w) and the other (R4n)
  Rmix waves of 8 records that hold both directions, the three widths and both column paths
Every record lives in a private TILE_H x TILE_W tile: its 16 x 8 footprint with at least 8 samples of guard all round.

Frame routes: <format><plane>/<col|row> for the formats 420, 444, 422, 440; pictures of 2 x 2 (one of 3 x 2) superblocks whose table
entries are written directly, 16 samples apart along the filter axis, so that every line is filtered once and from its constructed
content.  `waves` pictures compose the 64 lanes of one position for the ballots of vp9_lf_line2; the `mixed` picture has columns and
rows 8 apart and is compared with the oracle only."""
import ctypes as C
import functools
from collections import namedtuple

import numpy as np

import ffi
import vp9_lf_gen as G

DEPTHS = [8, 10, 12]
WD = [4, 8, 16]
LABELS = ["none", "tap_hev", "tap_soft", "flat8", "flat16"]
COUNTS = [1, 7, 8, 9, 31, 32, 33, 129]
TILE_H, TILE_W, PER_ROW = 32, 36, 16
BATCH_ROUTES = ["R1", "R2", "R3", "R4w", "R4n", "Rmix"]
BATCH_GROUPS = ["R1", "R2", "R3", "R4", "Rmix", "counts"]

#: name: what the line is built for; px: p7 .. p0 q0 .. q7; E, I, H in 8-bit units; changed: the output indices that must change
Cell = namedtuple("Cell", "name wd px E I H label changed")
#: eight cells of one width and one set of limits: an 8-line segment
Rec = namedtuple("Rec", "wd E I H cells")

I_TESTS = ["p3p2", "p2p1", "p1p0", "q1q0", "q2q1", "q3q2"]
F8_TESTS = ["p1", "p2", "p3", "q1", "q2", "q3"]
F16_TESTS = ["p4", "p5", "p6", "p7", "q4", "q5", "q6", "q7"]

MUTATIONS = ["lt:I:%d" % k for k in range(6)] + ["lt:E"] + ["lt:F8:%d" % k for k in range(6)] + ["lt:F16:%d" % k for k in range(8)] + \
            ["drop:I:%d" % k for k in range(6)] + ["drop:E"] + ["drop:F8:%d" % k for k in range(6)] + ["drop:F16:%d" % k for k in range(8)] + \
            ["hev:p-only", "hev:q-only", "ge:H:p", "ge:H:q", "noclip:inner", "noclip:outer", "noclip:p0", "noclip:q0", "noclip:p1",
             "noclip:q1", "unsat:f1", "unsat:f2", "round:f1:+1", "round:f1:-1", "round:f2:+1", "round:f2:-1", "round:g:+1", "round:g:-1",
             "round:flat8:+1", "round:flat8:-1", "round:flat16:+1", "round:flat16:-1", "noshift:E", "wd:flat8", "wd:flat16"]


# ---------------------------------------------------------------------------------------------------------------------------
# the model of one line
# ---------------------------------------------------------------------------------------------------------------------------
def lf_model(px, wd, E, I, H, bd, mut=None):
    """loop_filter() of vp9dsp_template.c on one line px[16] = p7 .. p0 q0 .. q7 (below 16 wide only px[4:12] are read).  Returns
    (out[16] as ints, not yet cast to the sample type, label).  mut: one entry of MUTATIONS, the decision that is changed."""
    F, fmax, maxv = 1 << (bd - 8), (1 << (bd - 1)) - 1, (1 << bd) - 1
    E, I, H = E * F, I * F, H * F
    px = [int(v) for v in px]
    out = px[:]
    p3, p2, p1, p0, q0, q1, q2, q3 = px[4:12]

    def le(a, b, site):
        if mut == "drop:" + site:
            return True
        return a < b if mut == "lt:" + site else a <= b

    def rnd(site):
        return 1 if mut == "round:%s:+1" % site else -1 if mut == "round:%s:-1" % site else 0

    diffs = [abs(p3 - p2), abs(p2 - p1), abs(p1 - p0), abs(q1 - q0), abs(q2 - q1), abs(q3 - q2)]
    esum = abs(p0 - q0) * 2 + (abs(p1 - q1) if mut == "noshift:E" else abs(p1 - q1) >> 1)
    if not (all(le(d, I, "I:%d" % k) for k, d in enumerate(diffs)) and le(esum, E, "E")):
        return out, "none"
    inner = [abs(px[6] - p0), abs(px[5] - p0), abs(px[4] - p0), abs(px[9] - q0), abs(px[10] - q0), abs(px[11] - q0)]
    outer = [abs(px[3] - p0), abs(px[2] - p0), abs(px[1] - p0), abs(px[0] - p0), abs(px[12] - q0), abs(px[13] - q0), abs(px[14] - q0),
             abs(px[15] - q0)]
    flat8in = (wd >= 8 or mut == "wd:flat8") and all(le(d, F, "F8:%d" % k) for k, d in enumerate(inner))
    flat8out = (wd >= 16 or mut == "wd:flat16") and all(le(d, F, "F16:%d" % k) for k, d in enumerate(outer))
    if flat8out and flat8in:
        ext = [px[0]] * 7 + px + [px[15]] * 7                       # p7 and q7 repeated: the 7 p7 + 2 p6 + p5 + ... taps as a window
        for c in range(1, 15):
            out[c] = (sum(ext[c:c + 15]) + px[c] + 8 + rnd("flat16")) >> 4
        return out, "flat16"
    if flat8in:
        ext = [p3] * 3 + px[4:12] + [q3] * 3
        for c in range(5, 11):
            out[c] = (sum(ext[c - 4:c + 3]) + px[c] + 4 + rnd("flat8")) >> 3
        return out, "flat8"
    clipf = lambda v: min(max(v, -fmax - 1), fmax)
    clipp = lambda v, site: v if mut == "noclip:" + site else min(max(v, 0), maxv)
    hev_p = abs(p1 - p0) >= H if mut == "ge:H:p" else abs(p1 - p0) > H
    hev_q = abs(q1 - q0) >= H if mut == "ge:H:q" else abs(q1 - q0) > H
    hev = hev_p if mut == "hev:p-only" else hev_q if mut == "hev:q-only" else hev_p or hev_q
    f = 3 * (q0 - p0)
    if hev:
        f += p1 - q1 if mut == "noclip:inner" else clipf(p1 - q1)
    if mut != "noclip:outer":
        f = clipf(f)
    f1 = f + 4 + rnd("f1")
    f2 = f + 3 + rnd("f2")
    f1 = (f1 if mut == "unsat:f1" else min(f1, fmax)) >> 3
    f2 = (f2 if mut == "unsat:f2" else min(f2, fmax)) >> 3
    out[7], out[8] = clipp(p0 + f2, "p0"), clipp(q0 - f1, "q0")
    if hev:
        return out, "tap_hev"
    g = (f1 + 1 + rnd("g")) >> 1
    out[6], out[9] = clipp(p1 + g, "p1"), clipp(q1 - g, "q1")
    return out, "tap_soft"


def _weights(wide):
    """output index -> the 16 tap weights of the flat filter: a window of radius 3 over px[4:12] (7 over px[0:16]) with the ends
    repeated and the centre counted twice; used to build lines whose sums land on a chosen residue"""
    lo, hi, r = (0, 15, 7) if wide else (4, 11, 3)
    W = {}
    for c in range(lo + 1, hi):
        w = [0] * 16
        for t in range(-r, r + 1):
            w[min(max(c + t, lo), hi)] += 1
        w[c] += 1
        W[c] = w
    return W


def _flat_changed(px, wide):
    sh = 4 if wide else 3
    return [c for c, w in _weights(wide).items() if (sum(a * b for a, b in zip(w, px)) + (1 << (sh - 1))) >> sh != px[c]]


# ---------------------------------------------------------------------------------------------------------------------------
# the cells
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cells(bd):
    F, fmax, maxv = 1 << (bd - 8), (1 << (bd - 1)) - 1, (1 << bd) - 1
    out = []

    def rough(v):                                              # an outer sample that is not flat
        return v + 10 * F if v + 10 * F <= maxv else v - 10 * F

    def add(name, wd, p, q, E, I, H, label, changed=None, op=None, oq=None):
        """p = p3 p2 p1 p0, q = q0 q1 q2 q3, op = p7 p6 p5 p4, oq = q4 q5 q6 q7"""
        px = list(op if op is not None else [rough(p[3])] * 4) + list(p) + list(q) + list(oq if oq is not None else [rough(q[0])] * 4)
        assert len(px) == 16 and all(0 <= v <= maxv for v in px), (name, px)
        if changed is None:
            changed = {"none": (), "tap_hev": (7, 8), "tap_soft": (6, 7, 8, 9)}[label] if label in ("none", "tap_hev", "tap_soft") \
                else _flat_changed(px, label == "flat16")
        assert not any(c.name == name for c in out), name
        out.append(Cell(name, wd, tuple(int(v) for v in px), E, I, H, label, frozenset(changed)))

    # ---- mask: each I test at exactly I (the 4-tap runs) and at I + 1 alone (nothing runs); I = 10
    for k, t in enumerate(I_TESTS):
        for extra, label in ((0, "tap_soft"), (1, "none")):
            d = 10 * F + extra
            p, q = [100 * F] * 4, [104 * F] * 4
            for j in ([0], [0, 1], [0, 1, 2])[k] if k < 3 else []:
                p[j] += d
            for j in ([1, 2, 3], [2, 3], [3])[k - 3] if k >= 3 else []:
                q[j] += d
            add("fm_%s_%s" % (t, "eq" if not extra else "plus1"), 4, p, q, 255, 10, 255, label)
    add("fm_fail_flat16", 16, [100 * F + F] + [100 * F] * 3, [164 * F] * 4, 255, 0, 255, "none", op=[100 * F + F] * 4, oq=[164 * F] * 4)
    # ---- mask: 2 |p0 - q0| + (|p1 - q1| >> 1) at exactly E = 20, with the dropped bit set, and one and two above
    for dl, tag, label in ((0, "eq", "tap_soft"), (1, "odd_eq", "tap_soft"), (2, "plus1", "none"), (3, "odd_plus1", "none")):
        add("E_" + tag, 4, [100 * F] * 4, [108 * F] + [108 * F + dl] * 3, 20, 255, 255, label)
    for wd, label in ((4, "tap_soft"), (8, "flat8"), (16, "flat16")):
        add("zero_limits_w%d" % wd, wd, [100 * F] * 4, [100 * F] * 4, 0, 0, 0, label, changed=(), op=[100 * F] * 4, oq=[100 * F] * 4)
    # ---- the largest limits of the batch record: I = 255 met by |p3 - p2| and |p2 - p1| < that, E = 255 met exactly and missed by one
    add("big_limits_eq", 4, [255 * F, 0, 150 * F, 150 * F], [50 * F] + [40 * F] * 3, 255, 255, 255, "tap_soft")
    add("big_limits_E_plus1", 4, [255 * F, 0, 150 * F, 150 * F], [50 * F] + [40 * F - 2] * 3, 255, 255, 255, "none")
    # ---- flat8: each inner comparison at exactly F (flat) and at F + 1 alone (the 4-tap); a step of 64 F moves every output
    A, B = 64 * F, 128 * F
    for wd in (8, 16):
        for k, t in enumerate(F8_TESTS):
            for extra, label in ((0, "flat8"), (1, "tap_soft")):
                d = (F + extra) * (-1 if k & 1 else 1)
                p, q = [A] * 4, [B] * 4
                if k < 3:
                    p[2 - k] += d
                else:
                    q[k - 2] += d
                add("f8_w%d_%s_%s" % (wd, t, "eq" if not extra else "plus1"), wd, p, q, 255, 255, 255, label)
    # ---- flat16: flat8 true, each outer comparison at exactly F and at F + 1 alone (flat8 runs)
    for k, t in enumerate(F16_TESTS):
        for extra, label in ((0, "flat16"), (1, "flat8")):
            d = (F + extra) * (-1 if k & 1 else 1)
            op, oq = [A] * 4, [B] * 4
            if k < 4:
                op[3 - k] += d
            else:
                oq[k - 4] += d
            add("f16_%s_%s" % (t, "eq" if not extra else "plus1"), 16, [A] * 4, [B] * 4, 255, 255, 255, label, op=op, oq=oq)
    add("f16_outer_flat_inner_not", 16, [A, A + F + 1, A, A], [B] * 4, 255, 255, 255, "tap_soft", op=[A] * 4, oq=[B] * 4)
    # ---- width limits
    add("w8_flat16_looking", 8, [A] * 4, [B] * 4, 255, 255, 255, "flat8", op=[A] * 4, oq=[B] * 4)
    add("w4_flat8_looking", 4, [A] * 4, [B] * 4, 255, 255, 255, "tap_soft", op=[A] * 4, oq=[B] * 4)

    # ---- the 4-tap filter: p3 = p2 = p1, q3 = q2 = q1; E = I = 255
    def tap(name, p1, p0, q0, q1, H, label, changed=None):
        add(name, 4, [p1, p1, p1, p0], [q0, q1, q1, q1], 255, 255, H, label, changed)

    P, Q, HF = 100 * F, 110 * F, 4 * F
    tap("hev_neither", P, P, Q, Q, 4, "tap_soft")
    tap("hev_p_only_H_plus1", P + HF + 1, P, Q, Q, 4, "tap_hev")
    tap("hev_q_only_H_plus1", P, P, Q, Q + HF + 1, 4, "tap_hev")
    tap("hev_both", P + HF + 1, P, Q, Q + HF + 1, 4, "tap_hev")
    tap("H_p_eq", P + HF, P, Q, Q, 4, "tap_soft")
    tap("H_q_eq", P, P, Q, Q - HF, 4, "tap_soft")
    tap("H0_soft", P, P, Q, Q, 0, "tap_soft")
    tap("H0_hev", P - 1, P, Q, Q, 0, "tap_hev")
    tap("inner_clip_hi", 250 * F, 120 * F, 100 * F, 10 * F, 4, "tap_hev")       # p1 - q1 > fmax, 3 (q0 - p0) < 0
    tap("inner_clip_lo", 10 * F, 100 * F, 120 * F, 250 * F, 4, "tap_hev")
    tap("outer_clip_hi_fsat_both", P, P, 160 * F, 160 * F, 255, "tap_soft")      # f = fmax: f + 4 and f + 3 saturate
    tap("outer_clip_lo_fmin", 160 * F, 160 * F, P, P, 255, "tap_soft")           # f = -fmax - 1
    tap("fsat_f1_only", 148 * F - 4, P, 140 * F, 140 * F, 0, "tap_hev")          # f = fmax - 3: f + 4 saturates, f + 3 = fmax
    tap("clip_p0_max", maxv, maxv - 1, maxv, maxv - 40 * F, 4, "tap_hev")
    tap("clip_p0_zero", 0, 1, 0, 40 * F, 4, "tap_hev")
    tap("clip_q0_zero", 40 * F, 0, 1, 0, 4, "tap_hev")
    tap("clip_q0_max", maxv - 40 * F, maxv, maxv - 1, maxv, 4, "tap_hev")
    tap("clip_p1_max", maxv - 1, maxv - 20 * F, maxv - 10 * F, maxv - 10 * F, 255, "tap_soft")
    tap("clip_p1_zero", 1, 20 * F, 10 * F, 10 * F, 255, "tap_soft")
    tap("clip_q1_zero", 10 * F, 10 * F, 20 * F, 1, 255, "tap_soft")
    tap("clip_q1_max", maxv - 10 * F, maxv - 10 * F, maxv - 20 * F, maxv - 1, 255, "tap_soft")
    # f1 = 0 / 2 / 3 / -2 / -3: (f1 + 1) >> 1 on odd and even, f + 4 and f + 3 on both sides of a multiple of 8 (sample units)
    tap("f1_0_nothing_moves", P, P, P + 1, P + 1, 255, "tap_soft", changed=())
    tap("f1_2_even", P, P, P + 4, P + 4, 255, "tap_soft")
    tap("f1_3_odd", P, P, P + 7, P + 7, 255, "tap_soft")
    tap("f1_m2_even", P, P, P - 5, P - 5, 255, "tap_soft")
    tap("f1_m3_odd", P, P, P - 7, P - 7, 255, "tap_soft")
    # ---- window rounding: the sum of output p0 on k 8 + 3 / k 8 + 4 (flat8), k 16 + 7 / k 16 + 8 (flat16); the p side at 0 and the
    #      q side at the maximum; constant sides and sides that alternate between the base and F away from it
    for wide, mod, targets in ((0, 8, (3, 4)), (1, 16, (7, 8))):
        w7 = _weights(wide)[7]
        for side in ("zero", "max"):
            for noisy in (0, 1):
                for target in targets:
                    for d in range(1, 64):
                        n = [F if (k & 1) == 0 else 0 for k in range(8)] if noisy else [0] * 8      # p0 and q0 stay on the base
                        n[7] = 0
                        if side == "zero":
                            ps, qs = [n[7 - k] for k in range(8)], [d + n[k] for k in range(8)]
                            ps[7] = 0
                        else:
                            ps, qs = [maxv - d - n[7 - k] for k in range(8)], [maxv - n[k] for k in range(8)]
                        px = ps + qs
                        if sum(a * b for a, b in zip(w7, px if wide else [0] * 4 + px[4:12] + [0] * 4)) % mod == target:
                            break
                    else:
                        raise AssertionError("no step reaches the residue")
                    add("round_%s_%s_%s_%d" % ("f16" if wide else "f8", side, "alt" if noisy else "const", target), 16 if wide else 8,
                        px[4:8], px[8:12], 255, 255, 255, "flat16" if wide else "flat8", op=px[:4] if wide else None,
                        oq=px[12:] if wide else None)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def cell_by_name(bd):
    return {c.name: c for c in cells(bd)}


def _rec(cs):
    cs = list(cs)
    assert len({(c.wd, c.E, c.I, c.H) for c in cs}) == 1 and 1 <= len(cs) <= 8
    cs = [cs[i % len(cs)] for i in range(8)]
    return Rec(cs[0].wd, cs[0].E, cs[0].I, cs[0].H, tuple(cs))


def rot(rec, n):
    """the record with its lines rotated by n"""
    return rec._replace(cells=tuple(rec.cells[(i + n) % 8] for i in range(8)))


@functools.lru_cache(maxsize=None)
def records(bd):
    """every cell in a record: cells grouped by (width, limits), eight to a record, the last of a group filled up from its first"""
    groups = {}
    for c in cells(bd):
        groups.setdefault((c.wd, c.E, c.I, c.H), []).append(c)
    out = []
    for cs in groups.values():
        for at in range(0, len(cs), 8):
            out.append(_rec(cs[at:at + 8]))
    return tuple(out)


def rec_lines(rec):
    return np.array([c.px for c in rec.cells], np.int64)


def rec_model(rec, bd):
    return np.array([lf_model(c.px, rec.wd, rec.E, rec.I, rec.H, bd)[0] for c in rec.cells], np.int64)


def entry(rec, valid=True):
    """the table word of FFHipVp9LfSb / FFHipVp9LfSbC"""
    return (0x80000000 if valid else 0) | WD.index(rec.wd) << 24 | rec.H << 16 | rec.I << 8 | rec.E


@functools.lru_cache(maxsize=None)
def mutation_cells(bd, mut):
    """the names of the cells whose output the mutation changes"""
    return frozenset(c.name for c in cells(bd) if lf_model(c.px, c.wd, c.E, c.I, c.H, bd) != lf_model(c.px, c.wd, c.E, c.I, c.H, bd, mut))


def mutation_caught(bd, names, mut):
    """the cells among `names` whose output the mutation changes"""
    return sorted(mutation_cells(bd, mut) & set(names))


# ---------------------------------------------------------------------------------------------------------------------------
# batch launches
# ---------------------------------------------------------------------------------------------------------------------------
Seg = namedtuple("Seg", "rec dir y x offset route")


class BatchLaunch:
    """One call of vp9.loop_filter_batch.  items: (record, dir, residue, route) — residue: the record's address (base + offset) in
    bytes modulo 4.  k: samples cut off the front of the buffer (the unaligned base: the plane is buf[k * ps:]); stride_mod: added to
    the stride in samples.  buf is the whole byte buffer, plane(buf) the 2-D view of its samples."""

    def __init__(self, bd, name, items, k=0, stride_mod=0, seed=0):
        self.bd, self.name, self.k = bd, name, k
        self.ps = ps = 1 if bd == 8 else 2
        self.ss = PER_ROW * TILE_W + stride_mod
        self.stride = self.ss * ps
        self.rows = (len(items) + PER_ROW - 1) // PER_ROW * TILE_H
        rng = np.random.default_rng(3000 * bd + seed)
        self.buf = np.zeros((k + self.rows * self.ss) * ps, np.uint8)
        self.buf.view(np.uint8 if ps == 1 else np.uint16)[:] = rng.integers(0, 1 << bd, k + self.rows * self.ss)
        plane = self.plane(self.buf)
        self.segs = []
        for i, (rec, d, residue, route) in enumerate(items):
            ty, tx = i // PER_ROW * TILE_H, i % PER_ROW * TILE_W
            y, x = (ty + 16, tx + 12) if d else (ty + 12, tx + 16)
            assert residue % ps == 0
            x += ((residue - (k + y * self.ss + x) * ps) % 4) // ps
            self._put(plane, d, y, x, rec_lines(rec))
            self.segs.append(Seg(rec, d, y, x, (y * self.ss + x) * ps, route))
        self.buf.setflags(write=False)

    def plane(self, buf):
        ps = self.ps
        return buf[self.k * ps:].view(np.uint8 if ps == 1 else np.uint16).reshape(self.rows, self.ss)

    @staticmethod
    def _put(plane, d, y, x, lines):
        if d:
            plane[y - 8:y + 8, x:x + 8] = lines.T
        else:
            plane[y:y + 8, x - 8:x + 8] = lines

    def lines(self, buf, i):
        """the 8 lines x 16 samples of record i"""
        s, plane = self.segs[i], self.plane(buf)
        return plane[s.y - 8:s.y + 8, s.x:s.x + 8].T if s.dir else plane[s.y:s.y + 8, s.x - 8:s.x + 8]

    def foot(self, i):
        s = self.segs[i]
        return (s.y - 8, s.y + 8, s.x, s.x + 8) if s.dir else (s.y, s.y + 8, s.x - 8, s.x + 8)

    def tile(self, i):
        ty, tx = i // PER_ROW * TILE_H, i % PER_ROW * TILE_W
        return ty, ty + TILE_H, tx, tx + TILE_W

    def want_model(self):
        buf = self.buf.copy()
        plane = self.plane(buf)
        for s in self.segs:
            self._put(plane, s.dir, s.y, s.x, rec_model(s.rec, self.bd))
        return buf

    def want_oracle(self):
        O = ffi.oracle()
        buf = self.buf.copy()
        base = buf.ctypes.data + self.k * self.ps
        for s in self.segs:
            r = s.rec
            O.ffo_vp9_loop_filter_bd(self.bd, r.wd, s.dir, C.cast(base + s.offset, ffi.u8p), self.stride, r.E, r.I, r.H)
        return buf

    def edge_records(self, dtype):
        rec = np.zeros(len(self.segs), dtype)
        for i, s in enumerate(self.segs):
            rec[i] = (s.offset, WD.index(s.rec.wd), s.dir, s.rec.E, s.rec.I, s.rec.H, (0, 0, 0))
        return rec

    def first_bad(self, got, want):
        """None, or the first mismatch as text: the record, its route, the cell of the line and its label"""
        bad = np.argwhere(self.plane(got) != self.plane(want))
        head = np.flatnonzero(got[:self.k * self.ps] != want[:self.k * self.ps])
        if not len(bad) and not len(head):
            return None
        if not len(bad):
            return "%s: %d bytes changed in front of the plane" % (self.name, len(head))
        y, x = (int(v) for v in bad[0])
        for i, s in enumerate(self.segs):
            y0, y1, x0, x1 = self.tile(i)
            if y0 <= y < y1 and x0 <= x < x1:
                line, k = (x - s.x, y - s.y + 8) if s.dir else (y - s.y, x - s.x + 8)
                cell = s.rec.cells[line] if 0 <= line < 8 else None
                return "%s: %d mismatches; first in record %d (route %s, %s edge, width %d, E %d I %d H %d), line %d sample %d: cell %s, label %s: " \
                       "got %d, want %d" % (self.name, len(bad), i, line_route(self, i, line) if cell else s.route, "row" if s.dir else "column",
                                            s.rec.wd, s.rec.E, s.rec.I, s.rec.H, line, k, cell.name if cell else "(guard)",
                                            cell.label if cell else "-", int(self.plane(got)[y, x]), int(self.plane(want)[y, x]))
        return "%s: %d mismatches; first at %s, outside every tile" % (self.name, len(bad), (y, x))


def _wide(L, i, line):
    """vp9_lf_lines' `wide` for one line of record i, from the addresses; the device base is assumed to sit on a 16-byte boundary
    before the k samples are cut off"""
    s = L.segs[i]
    return not s.dir and not ((L.k * L.ps + s.offset + line * L.stride) & 3)


def kernel_route(L, i):
    """the route of record i from the kernel's own condition"""
    if L.segs[i].dir:
        return "R3"
    wide = [_wide(L, i, line) for line in range(8)]
    return "R1" if all(wide) else "R2" if not any(wide) else "R4"


def line_route(L, i, line):
    r = kernel_route(L, i)
    return r if r != "R4" else "R4w" if _wide(L, i, line) else "R4n"


_MIX = [(0, 0, "R1"), (0, 1, "R2"), (1, 0, "R3"), (0, 3, "R2"), (0, 0, "R1"), (1, 2, "R3"), (0, 2, "R2"), (1, 1, "R3")]


def _mixed_items(bd, n, start=0):
    """n records in waves of 8 that hold both directions, the three widths and both column paths"""
    by_wd = [[r for r in records(bd) if r.wd == wd] for wd in WD]
    ps = 1 if bd == 8 else 2
    out = []
    for i in range(n):
        j = start + i
        pool = by_wd[j % 3]
        d, res, route = _MIX[j % 8]
        res = res if ps == 1 else (2 if res else 0)
        out.append((rot(pool[(j // 3) % len(pool)], j // 8), d, res, route if d or res else "R1"))
    return out


@functools.lru_cache(maxsize=None)
def batch_launches(bd, group):
    """the launches of one route group at one depth"""
    recs = records(bd)
    ps = 1 if bd == 8 else 2
    mk = lambda name, items, **kw: BatchLaunch(bd, "%s/%s" % (group, name), items, seed=BATCH_GROUPS.index(group) * 41 + len(name) + sum(kw.values()), **kw)
    if group == "R1":
        return [mk("dword", [(r, 0, 0, "R1") for r in recs])]
    if group == "R2":
        res = (1, 2, 3) if ps == 1 else (2,)
        return [mk("offset%d" % m, [(r, 0, m, "R2") for r in recs]) for m in res] + \
               [mk("base%d" % k, [(r, 0, (k * ps) % 4, "R2") for r in recs], k=k) for k in ((1, 2, 3) if ps == 1 else (1,))]
    if group == "R3":
        return [mk("row", [(r, 1, (2 * i) % 4, "R3") for i, r in enumerate(recs)]), mk("row_stride", [(r, 1, 0, "R3") for r in recs], stride_mod=1)]
    if group == "R4":
        return [mk("rot%d" % n, [(rot(r, n), 0, 0, "R4") for r in recs], stride_mod=1) for n in range(4)]
    if group == "Rmix":
        return [mk("waves", _mixed_items(bd, 24 * max(len([r for r in recs if r.wd == wd]) for wd in WD)))]
    assert group == "counts"
    return [mk("n%d" % n, _mixed_items(bd, n, start=5 * ci), k=ci % 2 if ps == 1 else 0) for ci, n in enumerate(COUNTS)]


def batch_missing(launches, route):
    """the cells that no line of `route` holds, over a list of launches"""
    have = set()
    for L in launches:
        for i, s in enumerate(L.segs):
            for line, c in enumerate(s.rec.cells):
                if route == "Rmix" or line_route(L, i, line) == route:
                    have.add(c.name)
    return sorted({c.name for c in cells(launches[0].bd)} - have)


# ---------------------------------------------------------------------------------------------------------------------------
# frame pictures
# ---------------------------------------------------------------------------------------------------------------------------
#: per superblock: column-edge positions, their 8-line segments, row-edge positions, their segments
GEOM = {"Y": (16, 8, 16, 8), "420": (8, 4, 8, 4), "422": (8, 8, 16, 4), "440": (16, 4, 8, 8)}
FORMATS = {"420": (1, 1), "444": (0, 0), "422": (1, 0), "440": (0, 1)}
FRAME_ROUTES = ["%s%s/%s" % (f, p, d) for f in FORMATS for p in "YUV" for d in ("col", "row")]
COMPOSITIONS = [("flat8", "none"), ("flat8", "one"), ("flat8", "all"), ("flat16", "none"), ("flat16", "one"), ("flat16", "all"),
                ("w8 flat", False), ("w8 flat", True), ("invalid beside valid",), ("one valid",)]

#: one entry of one plane: d 0 column / 1 row edge; (y, x): q0 of line 0; lines: rec's cells as placed (rotated per plane)
Place = namedtuple("Place", "plane d y x rec valid")


def _word(fmt, plane, d, p, sg):
    """(table, index) of the entry: table 0 FFHipVp9LfSb, 1 FFHipVp9LfSbC"""
    if plane == 0 or fmt == "444":
        return 0, (d * 16 + p) * 8 + sg
    if fmt == "420":
        return 0, 256 + (d * 8 + p) * 4 + sg
    npc, nsc, npr, nsr = GEOM[fmt]
    return 1, p * nsc + sg if d == 0 else npc * nsc + p * nsr + sg


class FramePic:
    """One picture of sbc x sbr superblocks with hand-written tables.  kind: "col" / "row" — every slot 16 apart along the filter
    axis holds a record, cycling from `start`; "waves_col" / "waves_row" — the luma slots compose the lanes of their position;
    "mixed" — columns and rows 8 apart (oracle only).  planes / before: sample arrays with stride padding; places: what sits where."""

    def __init__(self, bd, fmt, kind, sbc=2, sbr=2, start=0, seed=0):
        self.bd, self.fmt, self.kind, self.sbc, self.sbr = bd, fmt, kind, sbc, sbr
        self.name = "%s/%s%d/%dx%d" % (fmt, kind, start, sbc, sbr)
        self.ss = ss_h, ss_v = FORMATS[fmt]
        self.cols, self.rows = 8 * sbc, 8 * sbr
        dt = np.uint8 if bd == 8 else np.uint16
        rng = np.random.default_rng(5000 * bd + 100 * list(FORMATS).index(fmt) + seed)
        shape = [(64 * sbr, 64 * sbc)] + [((64 >> ss_v) * sbr, (64 >> ss_h) * sbc)] * 2
        self.before = [rng.integers(0, 1 << bd, (h, w + (12 if k == 0 else 4))).astype(dt) for k, (h, w) in enumerate(shape)]
        self.tables = np.zeros((sbr * sbc, 320), np.uint32)
        self.ctables = np.zeros((sbr * sbc, 128), np.uint32)
        self.places = []
        recs = records(bd)
        geoms = [GEOM["Y"], GEOM["Y" if fmt == "444" else fmt]]
        if kind == "mixed":
            self._mixed(recs, geoms)
        else:
            d = int(kind.endswith("row"))
            tabs = [(geoms[0], [0, 1, 2] if fmt == "444" else [0])] + ([] if fmt == "444" else [(geoms[1], [1, 2])])
            for geom, planes in tabs:
                slots = self._slots(geom, d)
                if kind.startswith("waves") and planes[0] == 0:
                    self._compose(slots, geom, d, planes)
                    continue
                for n, (r, c, p, sg) in enumerate(slots):
                    self._place(planes, geom, d, r, c, p, sg, recs[(start + n) % len(recs)])
        for a in self.before:
            a.setflags(write=False)

    def _slots(self, geom, d, step=4, first=4):
        """(superblock row, column, position, segment) of every entry `step` positions apart; none reaches out of the picture"""
        npos, nseg = (geom[0], geom[1]) if d == 0 else (geom[2], geom[3])
        return [(r, c, p, sg) for r in range(self.sbr) for c in range(self.sbc) for p in range(0, npos, step)
                if (c if d == 0 else r) * npos + p >= first for sg in range(nseg)]

    def slot_count(self, plane, d):
        return len(self._slots(GEOM["Y" if plane == 0 or self.fmt == "444" else self.fmt], d))

    def _place(self, planes, geom, d, r, c, p, sg, rec, valid=True, write=True):
        npc, nsc, npr, nsr = geom
        sbh, sbw = 8 * nsc, 4 * npc
        y, x = (r * sbh + 8 * sg, c * sbw + 4 * p) if d == 0 else (r * sbh + 4 * p, c * sbw + 8 * sg)
        tab, idx = _word(self.fmt, planes[0], d, p, sg)
        (self.ctables if tab else self.tables)[r * self.sbc + c, idx] = entry(rec, valid)
        for pl in planes:
            placed = rot(rec, pl)                               # the planes that share a table entry hold the lines in another order
            if write:
                BatchLaunch._put(self.before[pl], d, y, x, rec_lines(placed))
            self.places.append(Place(pl, d, y, x, placed, valid))

    def _compose(self, slots, geom, d, planes):
        """the lanes of one position: the segments of one superblock at one p"""
        bd = self.bd
        by = cell_by_name(bd)
        recs = records(bd)
        taps = [r for r in recs if r.wd == 4]
        flat8_eq = [by["f8_w8_%s_eq" % t] for t in F8_TESTS]
        flat8_plus = [by["f8_w8_%s_plus1" % t] for t in F8_TESTS]
        f16_eq = [by["f16_%s_eq" % t] for t in F16_TESTS]
        f16_plus = [by["f16_%s_plus1" % t] for t in F16_TESTS]
        all8, one8, none8 = _rec(flat8_eq), _rec(flat8_eq[:1] + flat8_plus + flat8_plus[:1]), _rec(flat8_plus)
        all16, one16, none16 = _rec(f16_eq), _rec(f16_eq[:1] + f16_plus[:7]), _rec(f16_plus)
        T = lambda n: taps[n % len(taps)]
        waves = [[T(n) for n in range(8)],                                              # no lane flat8
                 [one8] + [T(n) for n in range(7)],                                     # exactly one lane flat8
                 [all8] * 8,                                                            # all lanes flat8, no 16-wide entry in the wave
                 [none16] * 4 + [T(n) for n in range(4)],                               # 16-wide entries, no lane flat16
                 [T(n) for n in range(3)] + [one16] + [T(n) for n in range(4)],         # exactly one lane flat16
                 [all16] * 8,                                                           # all lanes flat16
                 [all8, all16, all8, none16, all8, T(0), all8, T(1)],                   # width-8 flat lanes beside 16-wide entries
                 [T(0), (all16, False), T(1), (all8, False), all8, (all16, False), T(2), all16],   # invalid entries beside valid ones
                 [None, None, None, all16, None, None, None, None],                     # exactly one valid segment
                 [None, None, (all16, False), None, None, one8, None, None]]
        positions = sorted({(r, c, p) for r, c, p, sg in slots})
        for n, (r, c, p) in enumerate(positions):
            wave = waves[n % len(waves)]
            nseg = geom[1] if d == 0 else geom[3]
            for sg in range(nseg):
                e = wave[(sg + n // len(waves)) % 8]
                if e is None:
                    continue
                rec, valid = e if isinstance(e, tuple) and not isinstance(e, Rec) else (e, True)
                if not valid:                                    # bit 31 clear, every other bit as a 16-wide entry with open limits
                    rec = rec._replace(wd=16, E=255, I=255, H=255)
                self._place(planes, geom, d, r, c, p, sg, rec, valid)

    def _mixed(self, recs, geoms):
        """both directions, entries 8 apart (every other position), reaching into the left and the upper superblock; the column
        entries' lines are written, the row entries filter what they find"""
        n = 0
        for gi, (geom, planes) in enumerate([(geoms[0], [0, 1, 2] if self.fmt == "444" else [0])] + ([] if self.fmt == "444" else [(geoms[1], [1, 2])])):
            for d in (0, 1):
                for r, c, p, sg in self._slots(geom, d, step=2, first=2):
                    rec = recs[(7 * n + gi) % len(recs)]
                    n += 1
                    if rec.wd == 16 and p % 4:
                        continue                                 # 16-wide entries stay 16 apart; these positions stay empty
                    self._place(planes, geom, d, r, c, p, sg, rec, write=(d == 0 and p % 4 == 0))

    def addresses(self, planes, r, c):
        ss_h, ss_v = self.ss
        cw, ch = 64 >> ss_h, 64 >> ss_v
        return [planes[0].ctypes.data + r * 64 * planes[0].strides[0] + c * 64 * planes[0].itemsize] + \
               [p.ctypes.data + r * ch * p.strides[0] + c * cw * p.itemsize for p in planes[1:]]

    def want_oracle(self):
        """run_tables / run_ctables superblock by superblock in raster order"""
        O = ffi.oracle()
        planes = [b.copy() for b in self.before]
        sy, suv = planes[0].strides[0], planes[1].strides[0]
        for r in range(self.sbr):
            for c in range(self.sbc):
                at = self.addresses(planes, r, c)
                tab = self.tables[r * self.sbc + c]
                if self.fmt == "420":
                    G.run_tables(O, tab, self.bd, at, (sy, suv))
                    continue
                luma = tab.copy()
                luma[256:] = 0
                G.run_tables(O, luma, self.bd, (at[0], 0, 0), (sy, 0))
                if self.fmt == "444":
                    G.run_tables(O, luma, self.bd, (at[1], 0, 0), (suv, 0))
                    G.run_tables(O, luma, self.bd, (at[2], 0, 0), (suv, 0))
                else:
                    G.run_ctables(O, self.ctables[r * self.sbc + c], self.bd, at[1:], suv, *self.ss)
        return planes

    def lines(self, planes, pl):
        a, s = planes[pl.plane], pl
        return a[s.y - 8:s.y + 8, s.x:s.x + 8].T if s.d else a[s.y:s.y + 8, s.x - 8:s.x + 8]

    def route(self, pl):
        return "%s%s/%s" % (self.fmt, "YUV"[pl.plane], "row" if pl.d else "col")

    def compositions(self):
        """the COMPOSITIONS that the luma waves of this picture hold, by the model's labels"""
        have = set()
        geom = GEOM["Y"]
        waves = {}
        for pl in self.places:
            if pl.plane == 0:
                waves.setdefault((pl.d, pl.y // 64, pl.x // 64, (pl.x if pl.d == 0 else pl.y) % 64), []).append(pl)
        for (d, r, c, at), pls in waves.items():
            labels = [lf_model(cell.px, p.rec.wd, p.rec.E, p.rec.I, p.rec.H, self.bd)[1] for p in pls if p.valid for cell in p.rec.cells]
            lanes = 64
            n8, n16 = sum(l in ("flat8", "flat16") for l in labels), sum(l == "flat16" for l in labels)
            any16 = any(p.valid and p.rec.wd == 16 for p in pls)
            count = lambda n: "none" if n == 0 else "one" if n == 1 else "all" if n == lanes else None
            if count(n8):
                have.add(("flat8", count(n8)))
            if any16 and count(n16):
                have.add(("flat16", count(n16)))
            if any(p.valid and p.rec.wd == 8 and "flat8" in [lf_model(cell.px, 8, p.rec.E, p.rec.I, p.rec.H, self.bd)[1] for cell in p.rec.cells]
                   for p in pls):
                have.add(("w8 flat", any16))
            nvalid = sum(p.valid for p in pls)
            if nvalid and any(not p.valid for p in pls):
                have.add(("invalid beside valid",))
            if nvalid == 1:
                have.add(("one valid",))
        return have


@functools.lru_cache(maxsize=None)
def frame_pics(bd, fmt):
    """the cell pictures of one format: columns and rows, as many of each as the smallest plane needs to hold every record (the first
    column picture of 3 x 2 superblocks), then the two `waves` pictures"""
    nrec = len(records(bd))
    out = []
    for kind in ("col", "row"):
        start = k = 0
        while start < nrec:
            pic = FramePic(bd, fmt, kind, 3 if k == 0 and kind == "col" else 2, 2, start, seed=k + 10 * (kind == "row"))
            out.append(pic)
            start += min(pic.slot_count(pl, int(kind == "row")) for pl in range(3))
            k += 1
    out += [FramePic(bd, fmt, "waves_col", 3, 2, 0, seed=31), FramePic(bd, fmt, "waves_row", 2, 2, 0, seed=32)]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def mixed_pic(bd, fmt):
    return FramePic(bd, fmt, "mixed", 3, 2, 0, seed=40)


def frame_missing(pics, route):
    """the cells that no valid entry of `route` holds"""
    have = {c.name for P in pics for pl in P.places if pl.valid and P.route(pl) == route for c in pl.rec.cells}
    return sorted({c.name for c in cells(pics[0].bd)} - have)


def compositions_missing(pics, d):
    have = set()
    for P in pics:
        if P.kind == ("waves_row" if d else "waves_col"):
            have |= P.compositions()
    return [c for c in COMPOSITIONS if c not in have]


def missing(launches, route):
    """the (route, cell) pairs that are absent: batch launches for a batch route, frame pictures for a frame route"""
    names = batch_missing(launches, route) if route in BATCH_ROUTES else frame_missing(launches, route)
    return [(route, n) for n in names]
