"""The cells of the HEVC in-loop filter batch kernels (hevc.loop_filter_batch, hevc.sao_batch, hevc.sao_restore_batch:
k_hevc_loop_filter_w, k_hevc_sao, k_hevc_sao16, k_hevc_sao_restore) as deterministic lists, shared by
tests/test_hevc_lf_matrix_cpu.py and tests/test_gpu_hevc_lf_matrix.py.  Nothing is random but seeded sample noise.

Deblocking.  A *segment* is one record: 8 lines of 8 samples p3 .. q3 (chroma: p1 .. q1), two 4-line groups that share beta and
have their own tc / no_p / no_q.  A *cell* is what the filter decides per group — none / strong / weak with (nd_p, nd_q), lines the
weak filter skips, results clipped at 0 or the maximum, tc, the no_p / no_q flags — and is reached by construction (_luma_group,
_chroma_group); its label comes from the numpy model lf_model() alone.  A *route* is what the kernel branches on:
  R1   hevc_lf_hgroup: the 32 records of the wave are all horizontal with base + offset and the stride on the dword grid
       (8-byte grid at 16 bits)
  R2   horizontal in hevc_lf_lines because the wave holds a vertical record (first, a middle or the last of the wave)
  R3   horizontal in hevc_lf_lines because base + offset is off that grid (an odd record offset, or an unaligned base)
  R4   horizontal in hevc_lf_lines because the stride is off that grid while row q0 of every record is on it
  R5   vertical luma, p3 on the grid: the `wide` loads and stores
  R6   vertical luma, p3 off the grid: sample by sample;  R56: a stride off the grid, the lines of one record alternate
  R7v0..3 / R7h0..3  chroma in hevc_lf_lines, vertical / horizontal, by the residue of the record's address (chroma in hgroup is R1)
Every segment lives in a private TILE_H x TILE_W tile: its 8 x 8 footprint with at least 8 samples of guard all round.

SAO.  A block has a private destination slot and a private source slot (its one-sample margin inside), 8 samples of guard all
round.  sao_model() returns the result and the class of every sample (edge: sign sum + 2; band: relative band 0..3, 4 = other)."""
import ctypes as C
from collections import namedtuple

import numpy as np

import ffi
from mc_matrix import _pack

DEPTHS = [8, 10, 12]
COUNTS = [1, 7, 8, 9, 31, 32, 33, 127, 128, 129]
BETA8, TC_TYP, TCS = 64, 6, [0, 1, 6, 24]
TILE_H, TILE_W, PER_ROW = 24, 28, 16
LUMA_MODES = ["none", "strong", "w11", "w12", "w21", "w22"]
LUMA_ROUTES = ["R1", "R2", "R3", "R4", "R5", "R6", "R56"]
CHROMA_ROUTES = ["R1"] + ["R7v%d" % r for r in range(4)] + ["R7h%d" % r for r in range(4)]
LF_GROUPS = ["R1", "R2", "R3", "R4", "R5", "R6", "R7", "counts"]
#: the routes on which a group's launches must reach every cell: (luma, chroma)
LF_GROUP_ROUTES = {"R1": (["R1"], ["R1"]), "R2": (["R2"], []), "R3": (["R3"], []), "R4": (["R4"], []), "R5": (["R5"], []),
                   "R6": (["R6", "R56"], []), "R7": ([], CHROMA_ROUTES[1:]), "counts": ([], [])}

#: one record's construction: cells / tc8 / no_p / no_q per group
Spec = namedtuple("Spec", "chroma cells beta8 tc8 no_p no_q")
#: what the model found in one group; skip: "" / "part" (lines 1 and 2 skipped, 0 and 3 filtered, or the like) / "all"
Label = namedtuple("Label", "mode beta0 tc no_p no_q skip clip0 clipmax changed")
Seg = namedtuple("Seg", "spec vertical y x offset route labels")


def _clip3(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


# ---------------------------------------------------------------------------------------------------------------------------
# deblocking: the model of one segment
# ---------------------------------------------------------------------------------------------------------------------------
def lf_model(lines, chroma, bd, beta8, tc8, no_p, no_q):
    """hevc_{h,v}_loop_filter_{luma,chroma} on lines[8][8] = p3 p2 p1 p0 q0 q1 q2 q3 per line (chroma uses p1 .. q1).
    Returns (the filtered lines, [Label of group 0, Label of group 1])."""
    maxv, sh = (1 << bd) - 1, bd - 8
    out = np.array(lines, np.int64)
    beta = beta8 << sh
    labels = []
    for j in range(2):
        tc, np_, nq = int(tc8[j]) << sh, bool(no_p[j]), bool(no_q[j])
        src = [[int(v) for v in row] for row in out[4 * j:4 * j + 4]]
        res = [row[:] for row in src]
        mode, skipped, clip0, clipmax = "none", 0, False, False

        def put(l, k, v):
            nonlocal clip0, clipmax
            clip0, clipmax = clip0 or v < 0, clipmax or v > maxv
            res[l][k] = _clip3(v, 0, maxv)

        if chroma:
            mode = "chroma"
            if tc > 0:
                for l in range(4):
                    p1, p0, q0, q1 = src[l][2:6]
                    delta = _clip3((((q0 - p0) * 4) + p1 - q1 + 4) >> 3, -tc, tc)
                    if not np_:
                        put(l, 3, p0 + delta)
                    if not nq:
                        put(l, 4, q0 - delta)
        else:
            dp = [abs(r[1] - 2 * r[2] + r[3]) for r in src]
            dq = [abs(r[6] - 2 * r[5] + r[4]) for r in src]
            d0, d3 = dp[0] + dq[0], dp[3] + dq[3]
            if d0 + d3 < beta:
                tc25 = (tc * 5 + 1) >> 1
                strong = all(abs(src[l][0] - src[l][3]) + abs(src[l][7] - src[l][4]) < (beta >> 3) and abs(src[l][3] - src[l][4]) < tc25 and
                             (d << 1) < (beta >> 2) for l, d in ((0, d0), (3, d3)))
                if strong:
                    mode = "strong"
                    t = tc << 1
                    for l in range(4):
                        p3, p2, p1, p0, q0, q1, q2, q3 = src[l]
                        if not np_:
                            res[l][3] = p0 + _clip3(((p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3) - p0, -t, t)
                            res[l][2] = p1 + _clip3(((p2 + p1 + p0 + q0 + 2) >> 2) - p1, -t, t)
                            res[l][1] = p2 + _clip3(((2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3) - p2, -t, t)
                        if not nq:
                            res[l][4] = q0 + _clip3(((p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3) - q0, -t, t)
                            res[l][5] = q1 + _clip3(((p0 + q0 + q1 + q2 + 2) >> 2) - q1, -t, t)
                            res[l][6] = q2 + _clip3(((2 * q3 + 3 * q2 + q1 + q0 + p0 + 4) >> 3) - q2, -t, t)
                else:
                    side = (beta + (beta >> 1)) >> 3
                    nd_p, nd_q = (2 if dp[0] + dp[3] < side else 1), (2 if dq[0] + dq[3] < side else 1)
                    mode = "w%d%d" % (nd_p, nd_q)
                    tc_2 = tc >> 1
                    for l in range(4):
                        p3, p2, p1, p0, q0, q1, q2, q3 = src[l]
                        delta = (9 * (q0 - p0) - 3 * (q1 - p1) + 8) >> 4
                        if abs(delta) >= 10 * tc:
                            skipped += 1
                            continue
                        delta = _clip3(delta, -tc, tc)
                        if not np_:
                            put(l, 3, p0 + delta)
                            if nd_p > 1:
                                put(l, 2, p1 + _clip3((((p2 + p0 + 1) >> 1) - p1 + delta) >> 1, -tc_2, tc_2))
                        if not nq:
                            put(l, 4, q0 - delta)
                            if nd_q > 1:
                                put(l, 5, q1 + _clip3((((q2 + q0 + 1) >> 1) - q1 - delta) >> 1, -tc_2, tc_2))
        out[4 * j:4 * j + 4] = res
        labels.append(Label(mode, beta8 == 0, int(tc8[j]), np_, nq, "" if not skipped else "all" if skipped == 4 else "part", clip0, clipmax,
                            res != src))
    return out, labels


def should_change(lab):
    """what the tests assert of the oracle's output, group by group: True / False, or None where the cell leaves it open"""
    if lab.mode == "none" or lab.tc == 0 or (lab.no_p and lab.no_q):
        return False
    if lab.skip == "all":
        return None
    return True


# ---------------------------------------------------------------------------------------------------------------------------
# deblocking: content by construction
# ---------------------------------------------------------------------------------------------------------------------------
def _luma_group(cell, bd, tc8, rng):
    """4 lines x 8 samples that decide `cell` from lines 0 and 3 (beta8 = BETA8); lines 1 and 2 carry +-1 of noise"""
    sc, maxv = 1 << (bd - 8), (1 << bd) - 1
    tc = tc8 * sc
    tc25 = (5 * tc + 1) >> 1
    B = 100 * sc
    side = (BETA8 * sc + (BETA8 * sc >> 1)) >> 3
    k = side // 2 + 1
    noise = True
    if cell == "none":                                      # d0 + d3 >= beta
        line = [0, 200 * sc] * 4
    elif cell == "strong":                                  # flat sides, a step below (5 tc + 1) >> 1 that still moves p0 and q0
        s = max(2, min(tc25 - 1, 3 * sc))
        line = [B] * 4 + [B + s] * 4
    elif cell in ("w11", "w12", "w21", "w22", "wskip"):     # a step of at least (5 tc + 1) >> 1; curvature k at p1 / q1: nd 1
        B = 20 * sc if cell == "wskip" else B
        step = tc25 + 5 * sc
        line = [B] * 4 + [B + step] * 4
        if cell[1] == "1":
            line[2] += k
        if cell[2] == "1":
            line[5] += k
    elif cell in ("wclip0", "wclipmax"):                    # p side at 0, q a ramp: delta < 0 takes p0 and p1 below 0; and mirrored
        X = 16 * sc
        line = [0, 0, 0, 0, 0, X, 2 * X, 3 * X]
        if cell == "wclipmax":
            line = [maxv - v for v in line]
        noise = False
    else:
        raise ValueError(cell)
    g = np.array([line, line, line, [v + 1 if 0 < v < maxv else v for v in line]], np.int64)
    if cell == "wskip":                                     # |delta| >= 10 tc on lines 1 and 2
        g[1:3, 4:] = g[0, 0] + 30 * tc + 10 * sc           # delta = (6 step + 8) >> 4 on a flat q side
    elif noise:
        g[1:3] = np.clip(g[1:3] + rng.integers(-1, 2, (2, 8)), 0, maxv)
    return g


def _chroma_group(cell, bd, tc8, rng):
    sc, maxv = 1 << (bd - 8), (1 << bd) - 1
    tc = tc8 * sc
    g = rng.integers(0, maxv + 1, (4, 8)).astype(np.int64)  # p3 p2 q2 q3 belong to the guard
    if cell == "step":
        B = 90 * sc + rng.integers(0, 4, (4, 1))
        g[:, 2:4], g[:, 4:6] = B, B + 8 * sc
    else:                                                   # delta = -tc at p0 = 0; mirrored: + tc at the maximum
        g[:, 2:6] = [0, 0, 0, min(maxv, 8 * tc + 8)]
        if cell == "cclipmax":
            g[:, 2:6] = maxv - g[:, 2:6]
    return g


def seg_lines(spec, bd, rng):
    f = _chroma_group if spec.chroma else _luma_group
    return np.concatenate([f(spec.cells[j], bd, spec.tc8[j], rng) for j in range(2)])


def luma_specs():
    T, z, out = TC_TYP, (0, 0), []
    for c in ("none", "strong", "w11", "w12", "w21", "w22", "wskip", "wclip0", "wclipmax"):
        out.append(Spec(0, (c, c), BETA8, (T, T), z, z))
    out.append(Spec(0, ("strong", "w22"), 0, (T, T), z, z))                                  # beta = 0: none
    for tc in TCS:
        for c in ("strong", "w22"):
            out.append(Spec(0, (c, c), BETA8, (tc, tc), z, z))
    out += [Spec(0, ("w22", "w22"), BETA8, (0, 24), z, z), Spec(0, ("w22", "w22"), BETA8, (24, 0), z, z)]
    for c in ("strong", "w22", "w11"):
        for a in range(4):
            for b in range(4):
                out.append(Spec(0, (c, c), BETA8, (T, T), (a & 1, b & 1), (a >> 1, b >> 1)))
    for w in ("w22", "w11"):
        for c0 in ("none", w, "strong"):
            for c1 in ("none", w, "strong"):
                out.append(Spec(0, (c0, c1), BETA8, (T, T), z, z))
    return out


def chroma_specs():
    z, out = (0, 0), []
    for tc in ((0, 0), (0, 5), (5, 0), (5, 5), (1, 24)):
        out.append(Spec(1, ("step", "step"), 0, tc, z, z))
    for a in range(4):
        for b in range(4):
            out.append(Spec(1, ("step", "step"), 0, (5, 7), (a & 1, b & 1), (a >> 1, b >> 1)))
    out += [Spec(1, ("cclip0", "cclipmax"), 0, (5, 5), z, z), Spec(1, ("cclipmax", "cclip0"), 0, (9, 3), z, z)]
    return out


def lf_keys(seg):
    """the coverage keys a segment contributes"""
    keys = []
    l0, l1 = seg.labels
    if seg.spec.chroma:
        keys.append(("ctc", l0.tc > 0, l1.tc > 0))
        for j, l in enumerate(seg.labels):
            if l.tc > 0:
                keys.append(("cno", j, l.no_p, l.no_q))
            keys += [(k,) for k, on in (("cclip0", l.clip0), ("cclipmax", l.clipmax)) if on]
        return keys
    coarse = lambda m: "weak" if m[0] == "w" else m
    keys.append(("pair", coarse(l0.mode), coarse(l1.mode)))
    for j, l in enumerate(seg.labels):
        keys += [("mode", j, l.mode), ("tc", j, l.tc)]
        if l.beta0:
            keys.append(("beta0",))
        if l.mode != "none" and l.tc > 0:
            keys.append(("no", j, l.no_p, l.no_q))
        if l.skip == "part":
            keys.append(("skip", j))
        keys += [(k,) for k, on in (("clip0", l.clip0), ("clipmax", l.clipmax)) if on]
    return keys


def lf_wanted(chroma):
    bools = (False, True)
    if chroma:
        return [("ctc", a, b) for a in bools for b in bools] + [("cno", j, a, b) for j in (0, 1) for a in bools for b in bools] + \
               [("cclip0",), ("cclipmax",)]
    return [("mode", j, m) for j in (0, 1) for m in LUMA_MODES] + [("skip", j) for j in (0, 1)] + [("clip0",), ("clipmax",), ("beta0",)] + \
           [("tc", j, t) for j in (0, 1) for t in TCS] + [("no", j, a, b) for j in (0, 1) for a in bools for b in bools] + \
           [("pair", a, b) for a in ("none", "weak", "strong") for b in ("none", "weak", "strong")]


def lf_missing(launches, route, chroma):
    """the required cells that no segment of `route` reaches, over a list of launches"""
    have = {k for L in launches for s in L.segs if s.route == route and bool(s.spec.chroma) == bool(chroma) for k in lf_keys(s)}
    return sorted(set(lf_wanted(chroma)) - have, key=repr)


# ---------------------------------------------------------------------------------------------------------------------------
# deblocking: launches
# ---------------------------------------------------------------------------------------------------------------------------
class LfLaunch:
    """One call of hevc.loop_filter_batch.  items: (spec, vertical, residue, route) — residue: the record's address (base + offset)
    in samples modulo 4.  k: samples cut off the front of the buffer (the unaligned base: the plane is buf[k * ps:]); stride_mod:
    the stride in samples modulo 4.  buf is the whole byte buffer, plane(buf) the 2-D view of its samples."""

    def __init__(self, bd, name, items, k=0, stride_mod=0, seed=0):
        self.bd, self.name, self.k = bd, name, k
        self.ps = ps = 1 if bd == 8 else 2
        self.ss = PER_ROW * TILE_W + stride_mod
        self.stride = self.ss * ps
        self.rows = (len(items) + PER_ROW - 1) // PER_ROW * TILE_H
        rng = np.random.default_rng(1000 * bd + seed)
        maxv = (1 << bd) - 1
        self.buf = np.zeros((k + self.rows * self.ss) * ps, np.uint8)
        self.buf.view(np.uint8 if ps == 1 else np.uint16)[:] = rng.integers(0, maxv + 1, k + self.rows * self.ss)
        plane = self.plane(self.buf)
        self.segs, self.lines, self.model = [], [], []
        for i, (spec, vertical, residue, route) in enumerate(items):
            ty, tx = i // PER_ROW * TILE_H, i % PER_ROW * TILE_W
            y, x = (ty + 8, tx + 12) if vertical else (ty + 12, tx + 8)
            x += (residue - (k + y * self.ss + x)) % 4
            lines = seg_lines(spec, bd, rng)
            out, labels = lf_model(lines, spec.chroma, bd, spec.beta8, spec.tc8, spec.no_p, spec.no_q)
            self._put(plane, vertical, y, x, lines)
            self.segs.append(Seg(spec, vertical, y, x, (y * self.ss + x) * ps, route, labels))
            self.model.append(out)
        self.buf.setflags(write=False)

    def plane(self, buf):
        ps = self.ps
        return buf[self.k * ps:].view(np.uint8 if ps == 1 else np.uint16).reshape(self.rows, self.ss)

    @staticmethod
    def _put(plane, vertical, y, x, lines):
        if vertical:
            plane[y:y + 8, x - 4:x + 4] = lines
        else:
            plane[y - 4:y + 4, x:x + 8] = lines.T

    def foot(self, i):
        """(y0, y1, x0, x1), end-exclusive: the 8 x 8 samples of segment i"""
        s = self.segs[i]
        return (s.y, s.y + 8, s.x - 4, s.x + 4) if s.vertical else (s.y - 4, s.y + 4, s.x, s.x + 8)

    def tile(self, i):
        ty, tx = i // PER_ROW * TILE_H, i % PER_ROW * TILE_W
        return ty, ty + TILE_H, tx, tx + TILE_W

    def group_region(self, i, j):
        """the samples of group j of segment i"""
        s = self.segs[i]
        if s.vertical:
            return slice(s.y + 4 * j, s.y + 4 * j + 4), slice(s.x - 4, s.x + 4)
        return slice(s.y - 4, s.y + 4), slice(s.x + 4 * j, s.x + 4 * j + 4)

    def want_model(self):
        buf = self.buf.copy()
        plane = self.plane(buf)
        for s, out in zip(self.segs, self.model):
            self._put(plane, s.vertical, s.y, s.x, out)
        return buf

    def want_oracle(self):
        O = ffi.oracle()
        buf = self.buf.copy()
        base = buf.ctypes.data + self.k * self.ps
        for s in self.segs:
            p = s.spec
            O.ffo_hevc_loop_filter_bd(self.bd, p.chroma, int(s.vertical), C.cast(base + s.offset, ffi.u8p), self.stride, p.beta8,
                                      ffi.ptr(np.array(p.tc8, np.int32), ffi.i32p), ffi.ptr(np.array(p.no_p, np.uint8)),
                                      ffi.ptr(np.array(p.no_q, np.uint8)))
        return buf

    def first_bad(self, got, want):
        """None, or the first mismatch as text: the segment, its route and labels"""
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
                f = self.foot(i)
                return "%s: %d mismatches; first in segment %d (%s, route %s, %s, cells %s, labels %s) at row %d column %d of its footprint: " \
                       "got %d, want %d" % (self.name, len(bad), i, "chroma" if s.spec.chroma else "luma", s.route, "vertical" if s.vertical else
                                            "horizontal", s.spec.cells, [tuple(l) for l in s.labels], y - f[0], x - f[2],
                                            int(self.plane(got)[y, x]), int(self.plane(want)[y, x]))
        return "%s: %d mismatches; first at %s, outside every tile" % (self.name, len(bad), (y, x))


def kernel_route(L, i):
    """the route of record i from the kernel's own conditions (k_hevc_loop_filter_w's ballot and hevc_lf_lines' `wide`), restated
    from the addresses; the device base is assumed to sit on a 16-byte boundary before the k samples are cut off"""
    ps = L.ps
    mask = 4 * ps - 1
    base = L.k * ps
    seg = L.segs[i]
    w0 = i // 32 * 32
    wave = L.segs[w0:w0 + 32]
    aligned = lambda s: not ((base + s.offset) & mask)
    hgroup = all(not s.vertical and aligned(s) for s in wave) and not (L.stride & mask)
    res = ((base + seg.offset) // ps) % 4
    if hgroup:
        return "R1"
    if seg.spec.chroma:
        if seg.vertical and L.stride & mask:
            return "R7v*"
        return "R7%s%d" % ("v" if seg.vertical else "h", res)
    if seg.vertical:
        wide = [not ((base + seg.offset + line * L.stride - 4 * ps) & mask) for line in range(8)]
        return "R5" if all(wide) else "R6" if not any(wide) else "R56"
    if not aligned(seg):
        return "R3"
    if L.stride & mask:
        return "R4"
    assert any(s.vertical for s in wave)
    return "R2"


def _mixed(horizontal, verticals):
    """waves of 32 records: 31 horizontal ones and one vertical as the first, a middle or the last record of the wave"""
    out, w = [], 0
    for at in range(0, len(horizontal), 31):
        wave = list(horizontal[at:at + 31])
        wave.insert(min((0, 15, 31)[w % 3], len(wave)), verticals[w % len(verticals)])
        out += wave
        w += 1
    return out


def lf_launches(bd, group):
    """the launches of one route group at one depth"""
    lu, ch = luma_specs(), chroma_specs()
    mk = lambda name, items, **kw: LfLaunch(bd, "%s/%s" % (group, name), items, seed=LF_GROUPS.index(group) * 37 + len(name) + sum(kw.values()), **kw)
    if group == "R1":
        return [mk("hgroup", [(s, 0, 0, "R1") for s in lu + ch])]
    if group == "R2":
        return [mk("mixed", _mixed([(s, 0, 0, "R2") for s in lu], [(s, 1, 0, "R5") for s in lu]))]
    if group == "R3":
        return [mk("offset", [(s, 0, r, "R3") for r in (1, 2, 3) for s in lu])] + \
               [mk("base%d" % k, [(s, 0, k, "R3") for s in lu], k=k) for k in (1, 2, 3)]
    if group == "R4":
        return [mk("stride%d" % m, [(s, 0, 0, "R4") for s in lu], stride_mod=m) for m in (1, 2, 3)]
    if group == "R5":
        return [mk("wide", [(s, 1, 0, "R5") for s in lu])]
    if group == "R6":
        return [mk("offset", [(s, 1, r, "R6") for r in (1, 2, 3) for s in lu]), mk("base", [(s, 1, 1, "R6") for s in lu], k=1),
                mk("stride", [(s, 1, 0, "R56") for s in lu], stride_mod=1)]
    if group == "R7":
        return [mk("v", [(s, 1, r, "R7v%d" % r) for r in range(4) for s in ch]),
                mk("h", [(s, 0, r, "R7h%d" % r) for r in (1, 2, 3) for s in ch]),
                mk("hstride", [(s, 0, 0, "R7h0") for s in ch], stride_mod=1),
                mk("hbase", [(s, 0, 2, "R7h2") for s in ch], k=2),
                mk("hmixed", _mixed([(s, 0, 0, "R7h0") for s in ch], [(s, 1, 0, "R7v0") for s in ch])),
                mk("vstride", [(s, 1, 0, "R7v*") for s in ch], stride_mod=1)]
    assert group == "counts"
    out = []
    pool = [lu[i // 2] if i % 2 == 0 else ch[(i // 2) % len(ch)] for i in range(2 * len(lu))]       # luma and chroma in turn
    for ci, n in enumerate(COUNTS):
        for first in (0, 1):                                                                          # record 0 luma / chroma
            specs = [pool[(2 * ci + first + i) % len(pool)] for i in range(n)]
            assert specs[0].chroma == first
            out.append(mk("n%d_%s_hgroup" % (n, "chroma" if first else "luma"), [(s, 0, 0, "R1") for s in specs]))
            items = [(s, 0, 1 + i % 3, "R7h%d" % (1 + i % 3) if s.chroma else "R3") for i, s in enumerate(specs)]
            out.append(mk("n%d_%s_lines" % (n, "chroma" if first else "luma"), items))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# SAO
# ---------------------------------------------------------------------------------------------------------------------------
#: content: "noise3" three adjacent levels (every sign sum, equal neighbours), "full" the whole range, "ext" mostly 0 and the maximum
SaoBlock = namedtuple("SaoBlock", "edge cls off w h dmod smod content")
PACKED = [(0, -128, 127, -5, 7), (3, 127, -128, 100, -100), (-2, 1, -1, 2, -2), (0, -7, 5, -3, 6)]
BYTEWISE = [(0, -300, 300, -129, 128), (200, 5, -6, 300, -300), (0, 128, -1, 2, -2), (-129, 1, 2, 3, 4)]
CLIP_EDGE = {0: (0, -128, -100, 100, 127), 1: (0, -300, -100, 100, 300)}       # sign sum -2 on a 0, +2 on the maximum
CLIP_BAND = {0: (0, 127, -128, -128, 127), 1: (0, 300, -300, -300, 300)}       # left class 31: band 31 up, band 0 down
LEFTS = [0, 1, 28, 29, 30, 31]
SAO_W8, SAO_H8 = [1, 4, 5, 61, 64], [1, 2, 63, 64]
SAO_WH16 = [1, 2, 17, 33, 64]
SAO_COUNTS = [1, 3, 4, 5]
EO_DX = [(-1, 1), (0, 0), (-1, 1), (1, -1)]
EO_DY = [(0, 0), (-1, 1), (-1, 1), (-1, 1)]


def sao_blocks(bd, edge, bytewise):
    sc = 1 << (bd - 8)
    sets = [tuple(v * sc for v in s) for s in (BYTEWISE if bytewise else PACKED)]
    clip = tuple(v * sc for v in (CLIP_EDGE if edge else CLIP_BAND)[bytewise])
    out = []

    def add(w, h, cls=None, off=None, content=None, at=None):
        i = len(out)
        if cls is None:
            cls = (i + i // 4 + i // 16) % 4 if edge else (LEFTS + [5, 17])[i % 8]
        if content is None:
            content = (("noise3", "ext", "full") if edge else ("full", "ext", "full"))[i % 3]
        if bd == 8:
            dmod, smod = (i if at is None else at) % 4, (i // 4 + i // 16) % 4
        else:
            dmod = 2 * (i % 2)
            smod = 2 - dmod
        out.append(SaoBlock(edge, cls, off or sets[(i + i // 4) % 4], w, h, dmod, smod, content))

    if bd == 8:
        for w in range(1, 65):
            add(w, 64)
        for h in SAO_H8:
            for w in SAO_W8:
                add(w, h)
    else:
        for h in SAO_WH16:
            for w in SAO_WH16:
                add(w, h)
    for w in (32, 30):                                       # whole dwords, and a partial last one
        if edge:
            for eo in range(4):
                add(w, 32, cls=eo, content="noise3")
                add(w, 16, cls=eo, off=clip, content="ext", at=0 if w == 32 else eo)   # both clips with dword and with byte stores
        else:
            for cls in LEFTS:
                add(w, 32, cls=cls, content="full")
            for k in range(4):
                add(w, 16, cls=31, off=clip, content="ext", at=k)
    return out


def sao_model(src, y, x, blk, bd):
    """sao_band_filter / sao_edge_filter of block blk whose first sample is src[y, x].  Returns (result, class of every sample, mask of
    results clipped at 0, mask of results clipped at the maximum); class: sign sum + 2 (edge), min(relative band, 4) (band)"""
    maxv = (1 << bd) - 1
    w, h = blk.w, blk.h
    c = src[y:y + h, x:x + w].astype(np.int64)
    off = np.array(blk.off, np.int64)
    if blk.edge:
        (ax, bx), (ay, by) = EO_DX[blk.cls], EO_DY[blk.cls]
        a = src[y + ay:y + ay + h, x + ax:x + ax + w].astype(np.int64)
        b = src[y + by:y + by + h, x + bx:x + bx + w].astype(np.int64)
        cls = np.sign(c - a) + np.sign(c - b) + 2
        raw = c + off[np.array([1, 2, 0, 3, 4])[cls]]
    else:
        rel = ((c >> (bd - 5)) - blk.cls) & 31
        cls = np.minimum(rel, 4)
        raw = c + np.where(rel < 4, off[1 + np.minimum(rel, 3)], 0)
    return np.clip(raw, 0, maxv), cls, raw < 0, raw > maxv


class SaoLaunch:
    """One call of hevc.sao_batch: dst0 / src planes (sd / ss samples wide), dpos / spos the first sample of every block, dslot /
    sslot the private rectangles"""

    def __init__(self, bd, name, blocks, sd, ss, seed):
        self.bd, self.name, self.blocks, self.sd, self.ss = bd, name, blocks, sd, ss
        self.ps = ps = 1 if bd == 8 else 2
        dt = np.uint8 if ps == 1 else np.uint16
        maxv = (1 << bd) - 1
        rng = np.random.default_rng(2000 * bd + seed)
        dsz = [(b.h + 16, b.w + 16 + 3) for b in blocks]
        ssz = [(b.h + 18, b.w + 18 + 3) for b in blocks]
        dat, drows = _pack(dsz, sd)
        sat, srows = _pack(ssz, ss)
        self.dst0 = rng.integers(0, maxv + 1, (drows, sd)).astype(dt)
        self.src = rng.integers(0, maxv + 1, (srows, ss)).astype(dt)
        self.dpos, self.spos, self.dslot, self.sslot = [], [], [], []
        shift = lambda y, x, stride, mod: next(s for s in range(4) if ((y * stride + x + s) * ps) % 4 == mod)
        for b, (dy, dx), (sy, sx), (dh, dw), (sh, sw) in zip(blocks, dat, sat, dsz, ssz):
            self.dslot.append((dy, dy + dh, dx, dx + dw))
            self.sslot.append((sy, sy + sh, sx, sx + sw))
            py, px = dy + 8, dx + 8
            self.dpos.append((py, px + shift(py, px, sd, b.dmod)))
            py, px = sy + 9, sx + 9
            px += shift(py, px, ss, b.smod)
            self.spos.append((py, px))
            box = (slice(py - 1, py + b.h + 1), slice(px - 1, px + b.w + 1))
            shape = (b.h + 2, b.w + 2)
            if b.content == "noise3":
                self.src[box] = int(rng.integers(1, maxv - 2)) + rng.integers(0, 3, shape)
            elif b.content == "ext":
                self.src[box] = rng.choice(np.array([0, 0, 1, maxv // 2, maxv - 1, maxv, maxv], dt), shape)
        self.model = [sao_model(self.src, y, x, b, bd) for b, (y, x) in zip(blocks, self.spos)]
        self.dst0.setflags(write=False)
        self.src.setflags(write=False)

    def dst_offset(self, i):
        return (self.dpos[i][0] * self.sd + self.dpos[i][1]) * self.ps

    def src_offset(self, i):
        return (self.spos[i][0] * self.ss + self.spos[i][1]) * self.ps

    def d_al(self, i):
        """k_hevc_sao's store kind: whole dwords when the block's first address and the stride allow"""
        return not ((self.dst_offset(i) | (self.sd * self.ps)) & 3)

    def want_model(self):
        want = self.dst0.copy()
        for b, (y, x), m in zip(self.blocks, self.dpos, self.model):
            want[y:y + b.h, x:x + b.w] = m[0]
        return want

    def want_oracle(self):
        O = ffi.oracle()
        want = self.dst0.copy()
        for i, b in enumerate(self.blocks):
            f = O.ffo_hevc_sao_edge_bd if b.edge else O.ffo_hevc_sao_band_bd
            f(self.bd, C.cast(want.ctypes.data + self.dst_offset(i), ffi.u8p), C.cast(self.src.ctypes.data + self.src_offset(i), ffi.u8p),
              self.sd * self.ps, self.ss * self.ps, ffi.ptr(np.array(b.off, np.int16), ffi.i16p), b.cls, b.w, b.h)
        return want

    def inside(self):
        m = np.zeros(self.dst0.shape, bool)
        for b, (y, x) in zip(self.blocks, self.dpos):
            m[y:y + b.h, x:x + b.w] = True
        return m

    def keys(self):
        """the coverage keys of the launch"""
        keys = set()
        for i, (b, m) in enumerate(zip(self.blocks, self.model)):
            _, cls, c0, cm = m
            pos = np.arange(b.w) % 4
            full = (np.arange(b.w) // 4 * 4 + 4 <= b.w) | (self.bd > 8)       # k_hevc_sao: the packed path takes whole dwords only
            for p in range(4):
                col = cls[:, (pos == p) & full]
                for v in np.unique(col):
                    keys.add(("edge", b.cls, int(v) - 2, p) if b.edge else ("band", b.cls, int(v), p))
            al = bool(self.d_al(i)) and self.bd == 8                          # k_hevc_sao16 stores sample by sample
            if c0[:, full].any():
                keys.add(("clip0", al))
            if cm[:, full].any():
                keys.add(("clipmax", al))
            keys |= {("wh", b.w, b.h), ("dmod", b.dmod), ("smod", b.smod), ("dsmod", b.dmod, b.smod)} | {("off", int(v)) for v in b.off}
            if al and (self.sd * self.ps) & 3 == 0:
                keys.add(("dword stores",))
            if self.dst_offset(i) & 3 == 0 and (self.sd * self.ps) & 3:
                keys.add(("odd sd, aligned d0",))
        return keys

    def first_bad(self, got, want):
        bad = np.argwhere(got != want)
        if not len(bad):
            return None
        y, x = (int(v) for v in bad[0])
        for i, (b, s) in enumerate(zip(self.blocks, self.dslot)):
            if s[0] <= y < s[1] and s[2] <= x < s[3]:
                ry, rx = y - self.dpos[i][0], x - self.dpos[i][1]
                cls = int(self.model[i][1][ry, rx]) if 0 <= ry < b.h and 0 <= rx < b.w else None
                return "%s: %d mismatches; first in block %d (%s) at row %d column %d (class %s, dword stores %s): got %d, want %d" % (
                    self.name, len(bad), i, b, ry, rx, cls, bool(self.d_al(i)), int(got[y, x]), int(want[y, x]))
        return "%s: %d mismatches; first at %s, outside every slot" % (self.name, len(bad), (y, x))


def sao_wanted(bd, edge, bytewise):
    sc = 1 << (bd - 8)
    bools = (False, True)
    if bd == 8:
        want = [("wh", w, 64) for w in range(1, 65)] + [("wh", w, h) for w in SAO_W8 for h in SAO_H8] + [("dmod", m) for m in range(4)] + \
               [("smod", m) for m in range(4)] + [("odd sd, aligned d0",), ("dword stores",)] + [(c, al) for c in ("clip0", "clipmax") for al in bools]
        want += [("off", 300), ("off", -300)] if bytewise else [("off", -128), ("off", 127)]
    else:
        want = [("wh", w, h) for w in SAO_WH16 for h in SAO_WH16] + [("dsmod", 0, 2), ("dsmod", 2, 0), ("clip0", False), ("clipmax", False)] + \
               [("off", (300 if bytewise else 127) * sc), ("off", (-300 if bytewise else -128) * sc)]
    if edge:
        want += [("edge", eo, s, p) for eo in range(4) for s in range(-2, 3) for p in range(4)]
    else:
        want += [("band", cls, r, p) for cls in LEFTS for r in range(5) for p in range(4)]
    return want


def sao_missing(launches, bd, edge, bytewise):
    have = set().union(*(L.keys() for L in launches))
    return sorted(set(sao_wanted(bd, edge, bytewise)) - have, key=repr)


def sao_launches(bd, edge, bytewise):
    """the whole list on a destination stride of whole dwords and on an odd one (16 bits: 4 n and 4 n + 2 bytes), then launches of 1, 3,
    4 and 5 blocks (four waves per workgroup)"""
    blocks = sao_blocks(bd, edge, bytewise)
    seed = 10 * edge + bytewise
    name = "%s/%s" % ("edge" if edge else "band", "bytewise" if bytewise else "packed")
    out = [SaoLaunch(bd, name + "/sd4", blocks, 1200, 1301, seed), SaoLaunch(bd, name + "/sdodd", blocks, 1201, 1301, seed + 100)]
    for n in SAO_COUNTS:
        out.append(SaoLaunch(bd, name + "/n%d" % n, blocks[-n:], 200 + n, 211, seed + 200 + n))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# SAO restore
# ---------------------------------------------------------------------------------------------------------------------------
RESTORE_SIZES = [(2, 2), (2, 64), (64, 2)]
RESTORE_COUNTS = [1, 5]


def restore_cases(bd):
    """hevc_restore_case's flag draws on the sizes whose candidate columns / rows coincide (the first, last and last but one are
    the same two), 10 of each"""
    from test_oracle_vs_ref import hevc_restore_case
    rng = np.random.default_rng(700 + bd)
    out = []
    for rep in range(30):
        var, eo, off0, borders, _, _, ve, he, de = hevc_restore_case(rng, rep)
        w, h = RESTORE_SIZES[rep % 3]
        out.append((var, eo, off0 << (bd - 8), borders, w, h, ve, he, de))
    return out


def restore_model(dst, src, bd, case):
    """sao_edge_restore[variant] on dst / src [h][w]: hevc_sao_restore_kind's rule sample by sample.  Returns the result"""
    var, eo, off0, borders, W, H, ve, he, de = case
    HORIZ, VERT, D135, D45 = 0, 1, 2, 3
    b0, b1, b2, b3 = (bool(v) for v in borders)
    maxv = (1 << bd) - 1
    init_x, w = int(eo != VERT and b0), W - int(eo != VERT and b2)
    init_y, h = int(eo != HORIZ and b1), H - int(eo != HORIZ and b3)
    s_ul, s_ur = int(not de[0] and eo == D135 and not b0 and not b1), int(not de[1] and eo == D45 and not b1 and not b2)
    s_lr, s_ll = int(not de[2] and eo == D135 and not b2 and not b3), int(not de[3] and eo == D45 and not b0 and not b3)
    out = dst.copy()
    for y in range(H):
        for x in range(W):
            kind = 0
            if eo != VERT:
                if (b0 and x == 0) or (b2 and x == W - 1):
                    kind = 1
            if eo != HORIZ:
                if (b1 and y == 0 or b3 and y == H - 1) and init_x <= x < w:
                    kind = 1
            if var:
                if ve[0] and eo != VERT and x == 0 and init_y + s_ul <= y < h - s_ll: kind = 2
                if ve[1] and eo != VERT and x == w - 1 and init_y + s_ur <= y < h - s_lr: kind = 2
                if he[0] and eo != HORIZ and y == 0 and init_x + s_ul <= x < w - s_ur: kind = 2
                if he[1] and eo != HORIZ and y == h - 1 and init_x + s_ll <= x < w - s_lr: kind = 2
                if de[0] and eo == D135 and x == 0 and y == 0: kind = 2
                if de[1] and eo == D45 and x == w - 1 and y == 0: kind = 2
                if de[2] and eo == D135 and x == w - 1 and y == h - 1: kind = 2
                if de[3] and eo == D45 and x == 0 and y == h - 1: kind = 2
            if kind == 1:
                out[y, x] = min(max(int(src[y, x]) + off0, 0), maxv)
            elif kind == 2:
                out[y, x] = src[y, x]
    return out
