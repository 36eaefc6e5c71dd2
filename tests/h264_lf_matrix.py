"""The cells of the H.264 in-loop filter as deterministic lists, shared by tests/test_h264_lf_matrix_cpu.py and
tests/test_gpu_h264_lf_matrix.py.  h264dsp_template.c:104-330 is written twice in this tree, both times in kernels/h264_lf_line.h:
lf_line (branching: k_h264_loop_filter, k_h264_loop_filter_hbd, the row kernel k_h264_deblock_frame, k_h264_deblock_c422, the MBAFF
kernels) and db_edge (in registers: k_h264_deblock_skew at every depth, k_h264_deblock_band); every kernel is still a route of its
own here, with its own loads, stores and lane maps.  Nothing here is random but the seeded background of the buffers.

A *cell* is one 8-sample line p3 p2 p1 p0 q0 q1 q2 q3 built by construction with its class (0 luma, 1 chroma, 2 luma intra, 3 chroma
intra), alpha, beta and tc0 in the 8-bit units the decoder passes, the label it is built for and the output indices that must
change.  lf_model() restates the reference line by line with the reference's scaling at the depth; it takes the name of a *mutation*
- one decision changed - and MUTATIONS lists them all: the CPU tier shows that every observable mutation changes some cell on every
route that runs the mutated class, which is the proof that a kernel wrong in that decision would fail.  UNOBSERVABLE lists the
changes that cannot show in any output, with the reason.

Cells that share class, alpha and beta make a *record* (one edge: 4 * inner lines, tc0 per `inner` lines; luma 4, chroma 2, the
MBAFF and 4:2:2 members 1, 2 and 4).  The tc0 bytes of a bS = 4 record are always INTRA_TC0 and must not matter.  rot() moves the
cells over the tc0 slots and lane groups between routes.

Batch routes (the conditions of k_h264_loop_filter), every record in a private 32 x 36 tile with at least 8 samples of guard:
  B1   column edge, every line address on a dword: two dwords in, whole dwords out
  B2   column edge off the dword grid (by the record's offset or by the base pointer): sample by sample
  B3   row edge
  B4   column edge on a stride off the dword grid: the lines of one record alternate between the two paths (B4w / B4n)
  Bmix workgroups of 16 records holding all eight kinds
  members   the 14 (kind, lines per tc0) members of k_h264_loop_filter_hbd, row and column edges
Frame routes: kernel x plane class x (direction, k == 0 | k > 0).  In a *cell picture* only macroblocks with x + y even carry a
live edge, exactly one each, all of one (direction, k class): every line is filtered once and from its constructed content.  The
k == 0 horizontal pictures are tall enough for every hand-off class of the kernel (handoff_class()); `waves` pictures compose the 64
lanes of one db_edge call; the `mixed` picture has every edge live and is compared with the oracle's frame order only.
Object routes: c422_pics() - the cell pictures of an 8 x 16-macroblock 4:2:2 chroma plane for k_h264_deblock_c422; MbaffPic - one
ffhip_h264_mbaff_filter_call() per live macroblock pair and plane, the ordinary and the _mbaff members at both line sizes."""
import ctypes as C
import functools
import itertools
from collections import namedtuple

import numpy as np

import ffi

DEPTHS = [8, 10, 14]
MEMBER_DEPTHS = [8, 9, 10, 12, 14]
CLASSES = ["luma", "chroma", "luma intra", "chroma intra"]
LABELS = ["none", "n00", "n10", "n01", "n11", "n00_tc0zero", "n10_tc0zero", "n01_tc0zero", "n11_tc0zero", "c", "weak", "s00", "s10", "s01",
          "s11", "ci"]
INTRA_TC0 = (-128, -1, 127, 0)
#: the members of test_loop_filter_batch_hbd: (kind, lines per tc0 entry)
MEMBERS = [(0, 4), (1, 4), (1, 2), (4, 4), (5, 4), (5, 2), (2, 2), (3, 2), (3, 1), (3, 4), (6, 2), (7, 2), (7, 1), (7, 4)]
COUNTS = [1, 15, 16, 17, 33]
TILE_H, TILE_W, PER_ROW = 32, 36, 16
BATCH_ROUTES = ["B1", "B2", "B3", "B4w", "B4n", "Bmix"]
BATCH_GROUPS = ["B1", "B2", "B3", "B4", "Bmix", "counts"]
DB_SKEW = 1                                                   # kernels/h264_deblock.hip

#: name; cls; px = p3 .. q3; alpha, beta, tc0 in 8-bit units; label; changed: the output indices that must change
Cell = namedtuple("Cell", "name cls px alpha beta tc0 label changed")
#: 4 * inner cells of one class, alpha and beta; tc0[g] belongs to lines g * inner .. g * inner + inner - 1
Rec = namedtuple("Rec", "cls alpha beta inner tc0 cells")

SITES = {"a": (0, 1, 2, 3), "bp": (0, 1, 2, 3), "bq": (0, 1, 2, 3), "ap": (0, 2), "aq": (0, 2), "strong": (2,)}
_ROUND = {"delta": (0, 1), "avg": (0,), "wp0": (2, 3), "wq0": (2, 3), "sp0": (2,), "sp1": (2,), "sp2": (2,), "sq0": (2,), "sq1": (2,),
          "sq2": (2,)}
#: mutation -> the classes whose filter it changes
MUT_CLASSES = {}
for _s, _c in SITES.items():
    for _m in ("le", "drop", "signed+", "signed-"):
        MUT_CLASSES["%s:%s" % (_m, _s)] = _c
MUT_CLASSES.update({"tc0:le0": (0,), "tcinc:drop:p": (0,), "tcinc:drop:q": (0,), "tcinc:always:p": (0,), "tcinc:always:q": (0,),
                    "p1clip:drop": (0,), "q1clip:drop": (0,), "p1clip:tc": (0,), "q1clip:tc": (0,), "dclip:drop": (0, 1), "dclip:tc0": (0,),
                    "pixclip:p0:lo": (0, 1), "pixclip:p0:hi": (0, 1), "pixclip:q0:lo": (0, 1), "pixclip:q0:hi": (0, 1),
                    "delta:truncdiv": (0, 1), "intra:tc0": (2, 3), "kind4only": (2, 3), "beta0:noskip": (0, 1, 2, 3),
                    "alpha0:noskip": (0, 1, 2, 3), "p3:drop": (2,), "q3:drop": (2,)})
for _s, _c in _ROUND.items():
    MUT_CLASSES["round:%s:+1" % _s] = MUT_CLASSES["round:%s:-1" % _s] = _c
#: the depth mistakes: the same as the rule at 8 bits, required above
DEPTH_MUTATIONS = {"depth:alpha": (0, 1, 2, 3), "depth:beta": (0, 1, 2, 3), "depth:tc0": (0,), "depth:tc0_late": (0,), "depth:ctc": (1,),
                   "depth:strong": (2,), "depth:max255": (0, 1)}
MUT_CLASSES.update(DEPTH_MUTATIONS)
MUTATIONS = list(MUT_CLASSES)
#: changes of the rule that no output can show, and why; the CPU tier asserts that no cell differs and checks the reason
UNOBSERVABLE = {"drop:tc_orig_guard": "p1 + clip3(x, -0, 0) == p1: with tc0 == 0 the guarded store writes the value it read",
                "ctc:lt0": "tc == 0 clips delta to 0, and ((tc0 - 1) << sh) + 1 == 0 only for sh == 0, tc0 == 0"}


# ---------------------------------------------------------------------------------------------------------------------------
# the model of one line
# ---------------------------------------------------------------------------------------------------------------------------
def lf_model(px, cls, alpha8, beta8, tc0, bd, mut=None, kind=None):
    """h264dsp_template.c:104-330 on one line px[8] = p3 p2 p1 p0 q0 q1 q2 q3 at depth bd.  Returns (out[8] as ints, not yet cast to
    the sample type, label, the set of changed indices).  mut: one entry of MUTATIONS / UNOBSERVABLE; kind: the record's kind byte,
    read by the mutation `kind4only` alone (the frame faces read kind >= 4 as bS = 4)."""
    sh = bd - 8
    maxv = 255 if mut == "depth:max255" else (1 << bd) - 1
    alpha = alpha8 if mut == "depth:alpha" else alpha8 << sh
    beta = beta8 if mut == "depth:beta" else beta8 << sh
    if mut == "beta0:noskip" and beta8 == 0:
        beta = 1 << 20                                            # a kernel that reads beta == 0 as "no limit"
    if mut == "alpha0:noskip" and alpha8 == 0:
        alpha = 1 << 20
    px = [int(v) for v in px]
    out = px[:]
    p3, p2, p1, p0, q0, q1, q2, q3 = px

    def done(label):
        return out, label, frozenset(k for k in range(8) if out[k] != px[k])

    def lt(a, b, t, site):
        if mut == "drop:" + site:
            return True
        d = a - b if mut == "signed+:" + site else b - a if mut == "signed-:" + site else abs(a - b)
        return d <= t if mut == "le:" + site else d < t

    def rnd(site):
        return 1 if mut == "round:%s:+1" % site else -1 if mut == "round:%s:-1" % site else 0

    clip3 = lambda v, lo, hi: lo if v < lo else hi if v > hi else v
    if mut == "kind4only" and cls >= 2 and kind not in (None, 4):
        cls -= 2
    if cls >= 2 and mut == "intra:tc0" and (tc0 < 0 if cls == 2 else tc0 <= 0):
        return done("none")
    if not (lt(p0, q0, alpha, "a") and lt(p1, p0, beta, "bp") and lt(q1, q0, beta, "bq")):
        return done("none")
    if cls == 3:
        out[3] = (2 * p1 + p0 + q1 + 2 + rnd("wp0")) >> 2
        out[4] = (2 * q1 + q0 + p1 + 2 + rnd("wq0")) >> 2
        return done("ci")
    if cls == 2:
        limit = ((alpha8 >> 2) + 2) << sh if mut == "depth:strong" else (alpha >> 2) + 2
        if not lt(p0, q0, limit, "strong"):
            out[3] = (2 * p1 + p0 + q1 + 2 + rnd("wp0")) >> 2
            out[4] = (2 * q1 + q0 + p1 + 2 + rnd("wq0")) >> 2
            return done("weak")
        ap, aq = lt(p2, p0, beta, "ap"), lt(q2, q0, beta, "aq")
        if ap:
            out[3] = (p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4 + rnd("sp0")) >> 3
            out[2] = (p2 + p1 + p0 + q0 + 2 + rnd("sp1")) >> 2
            out[1] = (2 * (p2 if mut == "p3:drop" else p3) + 3 * p2 + p1 + p0 + q0 + 4 + rnd("sp2")) >> 3
        else:
            out[3] = (2 * p1 + p0 + q1 + 2 + rnd("wp0")) >> 2
        if aq:
            out[4] = (p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4 + rnd("sq0")) >> 3
            out[5] = (p0 + q0 + q1 + q2 + 2 + rnd("sq1")) >> 2
            out[6] = (2 * (q2 if mut == "q3:drop" else q3) + 3 * q2 + q1 + q0 + p0 + 4 + rnd("sq2")) >> 3
        else:
            out[4] = (2 * q1 + q0 + p1 + 2 + rnd("wq0")) >> 2
        return done("s%d%d" % (ap, aq))
    x8 = (q0 - p0) * 4 + (p1 - q1) + 4 + rnd("delta")
    raw = -((-x8) >> 3) if mut == "delta:truncdiv" and x8 < 0 else x8 >> 3
    pix = lambda v, site: v if (mut == "pixclip:%s:lo" % site and v < 0) or (mut == "pixclip:%s:hi" % site and v > maxv) else clip3(v, 0, maxv)
    if cls == 1:
        tc = tc0 << sh if mut == "depth:ctc" else ((tc0 - 1) << sh) + 1
        if tc < 0 if mut == "ctc:lt0" else tc <= 0:
            return done("none")
        delta = raw if mut == "dclip:drop" else clip3(raw, -tc, tc)
        out[3], out[4] = pix(p0 + delta, "p0"), pix(q0 - delta, "q0")
        return done("c")
    t0 = tc0 if mut in ("depth:tc0", "depth:tc0_late") else tc0 * (1 << sh)
    if t0 <= 0 if mut == "tc0:le0" else t0 < 0:
        return done("none")
    ap, aq = lt(p2, p0, beta, "ap"), lt(q2, q0, beta, "aq")
    tc = t0
    avg = (p0 + q0 + 1 + rnd("avg")) >> 1
    tcl = (t0 << sh) if mut == "depth:tc0_late" else t0           # the limit of the p1 / q1 corrections
    for side, on, k2, k1 in (("p", ap, 1, 2), ("q", aq, 6, 5)):
        if on:
            if t0 or mut == "drop:tc_orig_guard":
                c = ((px[k2] + avg) >> 1) - px[k1]
                lim = None if mut == side + "1clip:drop" else (t0 + ap + aq) if mut == side + "1clip:tc" else tcl
                out[k1] = px[k1] + (c if lim is None else clip3(c, -lim, lim))
            if mut != "tcinc:drop:" + side:
                tc += 1
        elif mut == "tcinc:always:" + side:
            tc += 1
    if mut == "depth:tc0_late":
        tc <<= sh
    lim = t0 if mut == "dclip:tc0" else tc
    delta = raw if mut == "dclip:drop" else clip3(raw, -lim, lim)
    out[3], out[4] = pix(p0 + delta, "p0"), pix(q0 - delta, "q0")
    return done("n%d%d%s" % (ap, aq, "" if t0 else "_tc0zero"))


def _formulas(px):
    """the eight formulas of the bS = 4 filter as sums before the shift: name -> (sum, shift, output index)"""
    p3, p2, p1, p0, q0, q1, q2, q3 = px
    return {"sp0": (p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4, 3, 3), "sp1": (p2 + p1 + p0 + q0 + 2, 2, 2), "sp2": (2 * p3 + 3 * p2 + p1 + p0 + q0 + 4, 3, 1),
            "sq0": (p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4, 3, 4), "sq1": (p0 + q0 + q1 + q2 + 2, 2, 5), "sq2": (2 * q3 + 3 * q2 + q1 + q0 + p0 + 4, 3, 6),
            "wp0": (2 * p1 + p0 + q1 + 2, 2, 3), "wq0": (2 * q1 + q0 + p1 + 2, 2, 4)}


def _intra_changed(px, label):
    """the indices the bS = 4 filter of that label changes, from the formulas alone"""
    use = {"weak": ("wp0", "wq0"), "ci": ("wp0", "wq0"), "s00": ("wp0", "wq0"), "s10": ("sp0", "sp1", "sp2", "wq0"),
           "s01": ("wp0", "sq0", "sq1", "sq2"), "s11": ("sp0", "sp1", "sp2", "sq0", "sq1", "sq2"), "none": ()}[label]
    f = _formulas(px)
    return frozenset(k for s, sh, k in (f[n] for n in use) if s >> sh != px[k])


_DEFAULT = {"none": (), "n00": (3, 4), "n10": (2, 3, 4), "n01": (3, 4, 5), "n11": (2, 3, 4, 5), "n00_tc0zero": (), "n10_tc0zero": (3, 4),
            "n01_tc0zero": (3, 4), "n11_tc0zero": (3, 4), "c": (3, 4)}
_SWAP = {"n10": "n01", "n01": "n10", "s10": "s01", "s01": "s10", "n10_tc0zero": "n01_tc0zero", "n01_tc0zero": "n10_tc0zero"}


# ---------------------------------------------------------------------------------------------------------------------------
# the cells
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cells(bd):
    sh = bd - 8
    F, maxv = 1 << sh, (1 << bd) - 1
    A8, B8 = 40, 10
    A, B, P = A8 * F, B8 * F, 100 * F
    out = []
    far = lambda v: v + 24 * F if v + 24 * F <= maxv else v - 24 * F

    def add(name, cls, px, alpha8, beta8, tc0, label, changed=None, mirror=None):
        """mirror: the name of the cell with the sides exchanged"""
        assert len(px) == 8 and all(0 <= v <= maxv for v in px), (name, px)
        if changed is None:
            changed = _intra_changed(px, label) if cls >= 2 else _DEFAULT[label]
        assert not any(c.name == name for c in out), name
        out.append(Cell(name, cls, tuple(int(v) for v in px), alpha8, beta8, tc0, label, frozenset(changed)))
        if mirror:
            add(mirror, cls, px[::-1], alpha8, beta8, tc0, _SWAP.get(label, label), frozenset(7 - k for k in changed))

    def line(cls, p0, q0, dp1=0, dq1=0, dp2=0, dq2=0, p3=None, q3=None):
        p2, q2 = p0 + dp2, q0 + dq2
        if p3 is None:
            p3 = far(p2) if cls == 2 else p2
        if q3 is None:
            q3 = far(q2) if cls == 2 else q2
        return [p3, p2, p0 + dp1, p0, q0, q0 + dq1, q2, q3]

    # ---- all four classes: the three gate differences at t - 1 (passes alone) and at t (fails alone), p > q and p < q
    for cls in range(4):
        c = ("l", "c", "li", "ci")[cls]
        t = 3 if cls < 2 else 0
        for sg, st in ((1, "pgt"), (-1, "plt")):
            add("%s_gate_a_pass_%s" % (c, st), cls, line(cls, P, P - sg * (A - 1)), A8, B8, t, ("n11", "c", "weak", "ci")[cls])
            add("%s_gate_a_fail_%s" % (c, st), cls, line(cls, P, P - sg * A), A8, B8, t, "none")
            add("%s_gate_bp_pass_%s" % (c, st), cls, line(cls, P, P + 6 * F, dp1=sg * (B - 1)), A8, B8, t, ("n11", "c", "s11", "ci")[cls],
                mirror="%s_gate_bq_pass_%s" % (c, st))
            add("%s_gate_bp_fail_%s" % (c, st), cls, line(cls, P, P + 6 * F, dp1=sg * B), A8, B8, t, "none", mirror="%s_gate_bq_fail_%s" % (c, st))
        add("%s_alpha255_inside" % c, cls, line(cls, maxv, F), 255, B8, t, ("n11", "c", "weak", "ci")[cls])
        add("%s_alpha255_at" % c, cls, line(cls, maxv, F - 1), 255, B8, t, "none")
        add("%s_beta0" % c, cls, line(cls, P, P + 6 * F), A8, 0, t, "none")
        add("%s_alpha0" % c, cls, line(cls, P, P + 6 * F), 0, B8, t, "none")
        add("%s_beta0_alpha255" % c, cls, line(cls, P, P), 255, 0, t, "none")
    # ---- luma and chroma normal: the sum 4 (q0 - p0) + (p1 - q1) + 4, the pixel clips, lines that change one side only
    NO = B + F                                                     # |p2 - p0| that fails beta
    for cls in (0, 1):
        c, lab = ("l", "n00") if cls == 0 else ("c", "c")
        for S in (-12, -9, -8, -5, -4, -1, 0, 3, 4, 7, 8):
            d = (S - 4) >> 2
            e = S - 4 - 4 * d
            add("%s_sum_%d" % (c, S), cls, line(cls, P, P + d, dp1=e + d, dp2=NO, dq2=NO), A8, B8, 3, lab, (3, 4) if S >> 3 else ())
        hi = [maxv - 1 - NO] * 2 + [maxv, maxv - 1, maxv, maxv - (B - 1)] + [maxv - NO] * 2
        add("%s_clip_p0_hi" % c, cls, hi, A8, B8, 3, lab, mirror="%s_clip_q0_hi" % c)
        lo = [NO] * 2 + [B - 1, 0, 1, 0] + [1 + NO] * 2
        add("%s_clip_q0_lo" % c, cls, lo, A8, B8, 3, lab, mirror="%s_clip_p0_lo" % c)
        add("%s_only_p0" % c, cls, [NO] * 2 + [B - 1, 0, 0, 0] + [NO] * 2, A8, B8, 3, lab, (3,), mirror="%s_only_q0" % c)
    # ---- luma normal
    for t in (-128, -1, 0, 1, 25, 127):
        add("l_tc0_%d" % t, 0, line(0, P, P + 6 * F), A8, B8, t, "none" if t < 0 else "n11" if t else "n11_tc0zero")
    for sg, st in ((1, "pgt"), (-1, "plt")):
        for ok, tag in ((1, "m1"), (0, "eq")):
            for other in (1, 0):
                add("l_ap_%s_%s_aq%d" % (tag, st, other), 0, line(0, P, P + 6 * F, dp2=sg * (B - 1 if ok else B), dq2=0 if other else NO), A8, B8, 3,
                    "n%d%d" % (ok, other), mirror="l_aq_%s_%s_ap%d" % (tag, st, other))
    for ap in (0, 1):
        for aq in (0, 1):
            add("l_tc0zero_%d%d" % (ap, aq), 0, line(0, P, P + 6 * F, dp2=0 if ap else NO, dq2=0 if aq else NO), A8, B8, 0, "n%d%d_tc0zero" % (ap, aq))
    for k in (0, 1, 2):                                            # delta's raw value at -tc - 1, -tc, tc, tc + 1 for tc = tc0 + k
        tc = 3 * F + k
        for r, tag in ((-tc - 1, "below"), (-tc, "lo"), (tc, "hi"), (tc + 1, "above")):
            add("l_delta_k%d_%s" % (k, tag), 0, line(0, P, P + 2 * r, dp2=0 if k >= 1 else NO, dq2=0 if k >= 2 else NO), A8, B8, 3, "n%d%d" % (k >= 1, k >= 2))
    for g, tag in ((3 * F + 1, "below"), (3 * F, "lo"), (-3 * F, "hi"), (-3 * F - 1, "above")):        # the p1 correction is -g
        add("l_p1corr_%s" % tag, 0, line(0, P, P + 4 * F, dp1=g, dp2=-2 * F), A8, B8, 3, "n11", mirror="l_q1corr_%s" % tag)
    for d0 in (0, 1):                                              # p0 + q0 even / odd, p2 + avg even / odd; tc0 = 25: nothing clips
        for d2 in (0, 1):
            add("l_avg_%s_p2%s" % ("odd" if d0 else "even", "odd" if d0 != d2 else "even"), 0,
                line(0, P, P + 4 * F + d0, dp1=-3, dp2=-2 * F + d2), A8, B8, 25, "n11", mirror="l_avg_%s_q2%s" % ("odd" if d0 else "even", "odd" if d0 != d2 else "even"))
    # ---- chroma normal: p2 q2 far away, they must not matter
    for t in (-128, 0, 1, 2, 127):
        add("c_tc0_%d" % t, 1, line(1, P, P + 6 * F, dp2=50 * F, dq2=-50 * F), A8, B8, t, "none" if t <= 0 else "c")
    tc = 2 * F + 1
    for r, tag in ((-tc - 1, "below"), (-tc, "lo"), (tc, "hi"), (tc + 1, "above")):
        add("c_delta_%s" % tag, 1, line(1, P, P + 2 * r, dp2=50 * F, dq2=-50 * F), A8, B8, 3, "c")
    # ---- luma intra
    for a8 in (4, 5, 6, 7, 255):
        limit = ((a8 * F) >> 2) + 2
        for sg, st in ((1, "pgt"), (-1, "plt")):
            add("li_alpha%d_limit_m1_%s" % (a8, st), 2, line(2, P, P - sg * (limit - 1)), a8, B8, 0, "s11")
            add("li_alpha%d_limit_%s" % (a8, st), 2, line(2, P, P - sg * limit), a8, B8, 0, "weak")
    for ap in (0, 1):
        for aq in (0, 1):
            add("li_sides_%d%d" % (ap, aq), 2, line(2, P, P + 2, dp2=0 if ap else NO, dq2=0 if aq else NO), A8, B8, 0, "s%d%d" % (ap, aq))
    for sg, st in ((1, "pgt"), (-1, "plt")):
        for ok, tag in ((1, "m1"), (0, "eq")):
            add("li_ap_%s_%s" % (tag, st), 2, line(2, P, P + 2, dp2=sg * (B - 1 if ok else B)), A8, B8, 0, "s%d1" % ok, mirror="li_aq_%s_%s" % (tag, st))
    add("li_weak_above_limit", 2, line(2, P, P + 10 * F + 2), A8, B8, 0, "weak")
    add("li_p3_q3_far", 2, line(2, P, P + 2, p3=P + 60 * F, q3=P - 60 * F), A8, B8, 0, "s11")
    # each formula on every residue of its divisor, the samples at 0 and at the maximum
    for form, div in (("sp0", 8), ("sp1", 4), ("sp2", 8), ("wp0", 4)):
        for cls in ((2, 3) if form == "wp0" else (2,)):
            for side in ("zero", "max"):
                for r in range(div):
                    for o in itertools.product(range(4), repeat=6):
                        if min(o[:4]) != 0:
                            continue
                        gap = 10 * F + 5 if form == "wp0" else 0          # the weak form: |p0 - q0| at or above the strong limit
                        v = [o[0], o[1], o[2], o[3], gap + o[4], gap + o[5], gap + o[4], gap + o[4]]
                        if side == "max":
                            v = [maxv - x for x in v]
                        s, shf, k = _formulas(v)[form]
                        if (s - (1 << (shf - 1))) % div == r:
                            break
                    else:
                        raise AssertionError("no line reaches the residue")
                    c = "li" if cls == 2 else "ci"
                    add("%s_%s_%s_r%d" % (c, form, side, r), cls, v, A8, B8, 0, ("weak" if cls == 2 else "ci") if form == "wp0" else "s11",
                        mirror="%s_%s_%s_r%d" % (c, form.replace("p", "q"), side, r))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def cell_by_name(bd):
    return {c.name: c for c in cells(bd)}


def fill(cls, bd):
    """a line that no alpha, beta or tc0 filters: |p0 - q0| is the largest there is"""
    m = (1 << bd) - 1
    return Cell("fill", cls, (0, 0, 0, 0, m, m, m, m), 0, 0, 0, "none", frozenset())


@functools.lru_cache(maxsize=None)
def records(bd, cls, inner=None):
    """every cell of the class in a record of 4 * inner lines: cells grouped by (alpha, beta); of a bS < 4 class by tc0 into runs of
    `inner` lines, four runs to a record; spare lines hold fill()"""
    inner = inner or (2 if cls & 1 else 4)
    groups = {}
    for c in cells(bd):
        if c.cls == cls:
            groups.setdefault((c.alpha, c.beta), []).append(c)
    F = fill(cls, bd)
    out = []
    for (a, b), cs in groups.items():
        if cls >= 2:
            runs = [(INTRA_TC0[k % 4], cs[at:at + inner]) for k, at in enumerate(range(0, len(cs), inner))]
        else:
            runs = []
            for t in sorted({c.tc0 for c in cs}):
                ct = [c for c in cs if c.tc0 == t]
                runs += [(t, ct[at:at + inner]) for at in range(0, len(ct), inner)]
        runs = [(t, list(r) + [F] * (inner - len(r))) for t, r in runs]
        while len(runs) % 4:
            runs.append((INTRA_TC0[len(runs) % 4] if cls >= 2 else 0, [F] * inner))
        for at in range(0, len(runs), 4):
            four = runs[at:at + 4]
            out.append(Rec(cls, a, b, inner, INTRA_TC0 if cls >= 2 else tuple(t for t, r in four), tuple(c for t, r in four for c in r)))
    return tuple(out)


def rot(rec, n):
    """the record with its runs moved n slots on and the lines of a run rotated by n; the tc0 bytes of a bS = 4 record stay"""
    i = rec.inner
    runs = [rec.cells[g * i:(g + 1) * i] for g in range(4)]
    runs = [runs[(g + n) % 4] for g in range(4)]
    runs = [tuple(r[(k + n) % i] for k in range(i)) for r in runs]
    tc0 = rec.tc0 if rec.cls >= 2 else tuple(rec.tc0[(g + n) % 4] for g in range(4))
    return rec._replace(tc0=tc0, cells=tuple(c for r in runs for c in r))


def rec_lines(rec):
    return np.array([c.px for c in rec.cells], np.int64)


def rec_model(rec, bd):
    return np.array([lf_model(c.px, rec.cls, rec.alpha, rec.beta, rec.tc0[k // rec.inner], bd)[0] for k, c in enumerate(rec.cells)], np.int64)


def rec_triples(rec, kind=None):
    """(cell name, the tc0 of its slot, the record's kind byte): what decides a line's output besides the cell itself"""
    return [(c.name, rec.tc0[k // rec.inner], kind) for k, c in enumerate(rec.cells) if c.name != "fill"]


@functools.lru_cache(maxsize=None)
def _line_differs(bd, name, tc0, kind, mut):
    c = cell_by_name(bd)[name]
    return lf_model(c.px, c.cls, c.alpha, c.beta, tc0, bd)[0] != lf_model(c.px, c.cls, c.alpha, c.beta, tc0, bd, mut, kind)[0]


def mutation_caught(bd, triples, mut, cls):
    """the lines of class `cls` among `triples` whose output the mutation changes"""
    by = cell_by_name(bd)
    return sorted(t for t in set(triples) if by[t[0]].cls == cls and _line_differs(bd, t[0], t[1], t[2], mut))


def kind_of(cls, col):
    """FFHIP_H264_LF_*: bit 0 the edge is vertical (a column edge, the h_ member), bit 1 chroma, bit 2 bS = 4"""
    return int(col) | (cls & 1) << 1 | (cls >> 1) << 2


def oracle():
    O = ffi.oracle()
    O.ffo_h264_loop_filter.argtypes = [C.c_int, ffi.u8p, C.c_ssize_t, C.c_int, C.c_int, ffi.i8p]
    O.ffo_h264_loop_filter_bd.argtypes = [C.c_int, C.c_int, C.c_int, ffi.u8p, C.c_ssize_t, C.c_int, C.c_int, ffi.i8p]
    O.ffo_h264_deblock_frame.argtypes = [ffi.u8p, C.c_ssize_t, C.c_int, C.c_int, C.c_void_p]
    O.ffo_h264_deblock_frame_chroma.argtypes = [ffi.u8p, C.c_ssize_t, C.c_int, C.c_int, C.c_void_p]
    O.ffo_h264_deblock_frame_bd.argtypes = [C.c_int, C.c_int, ffi.u8p, C.c_ssize_t, C.c_int, C.c_int, C.c_void_p]
    O.ffo_h264_deblock_frame_c422_bd.argtypes = [C.c_int, ffi.u8p, C.c_ssize_t, C.c_int, C.c_int, C.c_void_p]
    return O


# ---------------------------------------------------------------------------------------------------------------------------
# batch launches
# ---------------------------------------------------------------------------------------------------------------------------
Seg = namedtuple("Seg", "rec col y x offset route")


class BatchLaunch:
    """One call of ffhip_h264_loop_filter_batch_dev (face "b8") or ..._dev_hbd (face "hbd": FFHipH264Edge.pad = lines per tc0).
    items: (record, column edge?, residue, route) - residue: the address of line 0 (base + offset) in bytes modulo 4.  k: samples
    cut off the front of the buffer (the unaligned base: the plane is buf[k * ps:]); stride_mod: added to the stride in samples."""

    def __init__(self, bd, name, items, k=0, stride_mod=0, seed=0, face=None):
        self.bd, self.name, self.k = bd, name, k
        self.face = face or ("b8" if bd == 8 else "hbd")
        self.ps = ps = 1 if bd == 8 else 2
        self.ss = PER_ROW * TILE_W + stride_mod
        self.stride = self.ss * ps
        self.rows = (len(items) + PER_ROW - 1) // PER_ROW * TILE_H
        rng = np.random.default_rng(7000 * bd + seed)
        self.buf = np.zeros((k + self.rows * self.ss) * ps, np.uint8)
        self.buf.view(np.uint8 if ps == 1 else np.uint16)[:] = rng.integers(0, 1 << bd, k + self.rows * self.ss)
        plane = self.plane(self.buf)
        self.segs = []
        for i, (rec, col, residue, route) in enumerate(items):
            ty, tx = i // PER_ROW * TILE_H, i % PER_ROW * TILE_W
            y, x = (ty + 8, tx + 13) if col else (ty + 16, tx + 8)
            assert residue % ps == 0
            x += ((residue - (k + y * self.ss + x) * ps) % 4) // ps
            self._put(plane, col, y, x, rec_lines(rec))
            self.segs.append(Seg(rec, col, y, x, (y * self.ss + x) * ps, route))
        self.buf.setflags(write=False)

    def plane(self, buf):
        ps = self.ps
        return buf[self.k * ps:].view(np.uint8 if ps == 1 else np.uint16).reshape(self.rows, self.ss)

    @staticmethod
    def _put(plane, col, y, x, lines):
        n = len(lines)
        if col:
            plane[y:y + n, x - 4:x + 4] = lines
        else:
            plane[y - 4:y + 4, x:x + n] = lines.T

    def lines(self, buf, i):
        """the lines x 8 samples of record i"""
        s, plane = self.segs[i], self.plane(buf)
        n = 4 * s.rec.inner
        return plane[s.y:s.y + n, s.x - 4:s.x + 4] if s.col else plane[s.y - 4:s.y + 4, s.x:s.x + n].T

    def foot(self, i):
        s = self.segs[i]
        n = 4 * s.rec.inner
        return (s.y, s.y + n, s.x - 4, s.x + 4) if s.col else (s.y - 4, s.y + 4, s.x, s.x + n)

    def tile(self, i):
        ty, tx = i // PER_ROW * TILE_H, i % PER_ROW * TILE_W
        return ty, ty + TILE_H, tx, tx + TILE_W

    def kind(self, i):
        return kind_of(self.segs[i].rec.cls, self.segs[i].col)

    def want_model(self):
        buf = self.buf.copy()
        plane = self.plane(buf)
        for s in self.segs:
            self._put(plane, s.col, s.y, s.x, rec_model(s.rec, self.bd))
        return buf

    def want_oracle(self, plain=None):
        """plain: the 8-bit functions of oracle/ffo_h264.c (the members with the default lines per tc0 only); default: at 8 bits where
        they apply"""
        O = oracle()
        buf = self.buf.copy()
        base = buf.ctypes.data + self.k * self.ps
        for i, s in enumerate(self.segs):
            r = s.rec
            tc0 = np.array(r.tc0, np.int8)
            use_plain = self.bd == 8 and r.inner == (2 if r.cls & 1 else 4) if plain is None else plain
            if use_plain:
                O.ffo_h264_loop_filter(self.kind(i), C.cast(base + s.offset, ffi.u8p), self.stride, r.alpha, r.beta, ffi.ptr(tc0, ffi.i8p))
            else:
                O.ffo_h264_loop_filter_bd(self.bd, self.kind(i), r.inner, C.cast(base + s.offset, ffi.u8p), self.stride, r.alpha, r.beta, ffi.ptr(tc0, ffi.i8p))
        return buf

    def edge_records(self):
        rec = np.zeros(len(self.segs), ffi.EDGE_DTYPE)
        for i, s in enumerate(self.segs):
            rec[i] = (s.offset, self.kind(i), s.rec.alpha, s.rec.beta, s.rec.inner if self.face == "hbd" else 0, s.rec.tc0)
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
                line, k = (y - s.y, x - s.x + 4) if s.col else (x - s.x, y - s.y + 4)
                cell = s.rec.cells[line] if 0 <= line < 4 * s.rec.inner else None
                return "%s: %d mismatches; first in record %d (route %s, kind %d, %s edge, alpha %d beta %d tc0 %s, %d lines per tc0), line %d sample %d: " \
                       "cell %s, label %s: got %d, want %d" % (self.name, len(bad), i, line_route(self, i, line) if cell else s.route, self.kind(i),
                                                               "column" if s.col else "row", s.rec.alpha, s.rec.beta, list(s.rec.tc0), s.rec.inner, line, k,
                                                               cell.name if cell else "(guard)", cell.label if cell else "-",
                                                               int(self.plane(got)[y, x]), int(self.plane(want)[y, x]))
        return "%s: %d mismatches; first at %s, outside every tile" % (self.name, len(bad), (y, x))


def _wide(L, i, line):
    """k_h264_loop_filter's dword condition for one line of record i, from the addresses; the device base is assumed to sit on a
    16-byte boundary before the k samples are cut off"""
    s = L.segs[i]
    return bool(s.col) and not ((L.k * L.ps + s.offset + line * L.stride) & 3)


def kernel_route(L, i):
    """the route of record i from the kernel's own condition"""
    if not L.segs[i].col:
        return "B3"
    wide = [_wide(L, i, line) for line in range(4 * L.segs[i].rec.inner)]
    return "B1" if all(wide) else "B2" if not any(wide) else "B4"


def line_route(L, i, line):
    r = kernel_route(L, i)
    return r if r != "B4" else "B4w" if _wide(L, i, line) else "B4n"


@functools.lru_cache(maxsize=None)
def all_records(bd):
    """the records of the four classes at their plain lines per tc0"""
    return tuple(r for cls in range(4) for r in records(bd, cls))


_MIX = [(1, 0, "B1"), (1, 1, "B2"), (0, 0, "B3"), (1, 3, "B2"), (1, 0, "B1"), (0, 2, "B3"), (1, 2, "B2"), (0, 1, "B3")]


def _mixed_items(bd, n, start=0):
    """n records in workgroups of 16 that hold all eight kinds: the four classes in turn, the direction changing every four"""
    by = [records(bd, cls) for cls in range(4)]
    ps = 1 if bd == 8 else 2
    out = []
    for i in range(n):
        j = start + i
        pool = by[j % 4]
        col = (j // 4) % 2
        res = (j // 8) % 4 if col else (2 * j) % 4
        res = res if ps == 1 else res & 2
        out.append((rot(pool[(j // 8) % len(pool)], j // 16), col, res, ("B1" if res == 0 else "B2") if col else "B3"))
    return out


@functools.lru_cache(maxsize=None)
def batch_launches(bd, group):
    """the launches of one route group at one depth"""
    recs = all_records(bd)
    ps = 1 if bd == 8 else 2
    mk = lambda name, items, **kw: BatchLaunch(bd, "%s/%s" % (group, name), items, seed=BATCH_GROUPS.index(group) * 41 + len(name) + sum(kw.values()), **kw)
    if group == "B1":
        return [mk("dword", [(rot(r, i), 1, 0, "B1") for i, r in enumerate(recs)])]
    if group == "B2":
        res = (1, 2, 3) if ps == 1 else (2,)
        return [mk("offset%d" % m, [(rot(r, m), 1, m, "B2") for r in recs]) for m in res] + \
               [mk("base%d" % k, [(rot(r, k + 1), 1, (k * ps) % 4, "B2") for r in recs], k=k) for k in ((1, 2, 3) if ps == 1 else (1,))]
    if group == "B3":
        return [mk("row", [(rot(r, i), 0, (ps * i) % 4, "B3") for i, r in enumerate(recs)]), mk("row_stride", [(rot(r, 2), 0, 0, "B3") for r in recs], stride_mod=1)]
    if group == "B4":
        # line i of a record sits at residue + i * stride: over the residues every line takes the dword path once
        return [mk("res%d" % n, [(rot(r, n * ps // 4), 1, (n * ps) % 4, "B4") for r in recs], stride_mod=1) for n in range(4)]
    if group == "Bmix":
        return [mk("workgroups", _mixed_items(bd, 16 * max(len(records(bd, cls)) for cls in range(4))))]
    assert group == "counts"
    return [mk("n%d" % n, _mixed_items(bd, n, start=5 * ci), k=ci % 2 if ps == 1 else 0) for ci, n in enumerate(COUNTS)]


@functools.lru_cache(maxsize=None)
def member_launches(bd):
    """the 14 members of k_h264_loop_filter_hbd, one launch each: every record of the member's class at its lines per tc0"""
    out = []
    for n, (kind, inner) in enumerate(MEMBERS):
        cls = (kind >> 1 & 1) | (kind >> 2 & 1) << 1
        recs = records(bd, cls, inner)
        items = [(rot(r, i + n), kind & 1, (2 * i) % 4, "B1") for i, r in enumerate(recs)]
        L = BatchLaunch(bd, "members/kind%d_inner%d" % (kind, inner), items, seed=500 + n, face="hbd")
        L.segs = [s._replace(route=kernel_route(L, i)) for i, s in enumerate(L.segs)]
        out.append(L)
    return out


def batch_triples(launches, route):
    """the (cell, tc0, kind) triples on the lines of `route`, over a list of launches"""
    have = set()
    for L in launches:
        for i, s in enumerate(L.segs):
            for line, t in enumerate(zip(s.rec.cells, (s.rec.tc0[k // s.rec.inner] for k in range(4 * s.rec.inner)))):
                if t[0].name != "fill" and (route in ("Bmix", "any") or line_route(L, i, line) == route):
                    have.add((t[0].name, t[1], L.kind(i)))
    return have


def batch_missing(launches, route, classes=range(4)):
    """the cells that no line of `route` holds"""
    have = {t[0] for t in batch_triples(launches, route)}
    return sorted({c.name for c in cells(launches[0].bd) if c.cls in classes} - have)


# ---------------------------------------------------------------------------------------------------------------------------
# frame pictures
# ---------------------------------------------------------------------------------------------------------------------------
KERNELS = ["skew", "band", "row"]
FRAME_DK = ["V0", "Vn", "H0", "Hn"]                             # direction (V: vertical edges, dir 0) x (k == 0 | k > 0)
HANDOFF = {"skew": ("same wave", "other wave", "other workgroup"), "band": ("inside the band", "across bands"), "row": ("every row",)}
COMPOSITIONS = ["bS<4 only", "bS=4 all fail", "bS=4 one passes", "all pass", "bS=4 beside filtered bS<4", "bS=4 beside filtered bS<4, tc0 127 -128"]

#: one live record: macroblock (mx, my), dir 0 vertical / 1 horizontal edge k, the record as placed, the kind byte of the table
Place = namedtuple("Place", "mx my dir k rec kind")


def frame_kernel(bd, chroma, plane_addr, stride, pitch, edges_addr=0, old=0):
    """the kernel deblock_frames() (kernels/h264_deblock.hip) launches, from the addresses and FFHIP_DEBLOCK_OLD; None: rejected"""
    aligned = not ((plane_addr | stride | pitch) & 3)
    if chroma and not aligned:
        return None
    amask = 7 if chroma and bd == 8 else 15
    skew = (not old or bd > 8) and not ((plane_addr | stride | pitch) & amask) and not (edges_addr & 15)
    if bd > 8 and not skew:
        return None
    if skew:
        return "skew"
    return "band" if aligned and not (old == 1 and not chroma) else "row"


def handoff_class(kernel, bd, chroma, my, nframes=1, mb_h=1):
    """how the row above macroblock row my (> 0) reaches it: the launch arithmetic of deblock_frames() and the kernels' constants.
    skew: Q = 64 / (macroblock side) rows per wave, 4 waves per workgroup (3 for 16-bit luma: the LDS strip) on consecutive bands;
    band: 4 rows per band unless nframes * mb_h > 2048 (16); row kernel: a workgroup per row"""
    assert my > 0
    if kernel == "row":
        return "every row"
    if kernel == "band":
        bw = 16 if nframes * mb_h > 2048 else 4
        return "inside the band" if my % bw else "across bands"
    Q = 8 if chroma else 4
    wpb = 3 if bd > 8 and not chroma else 4
    return "same wave" if my % Q else "other wave" if (my // Q) % wpb else "other workgroup"


class FramePic:
    """One plane of mb_w x mb_h macroblocks (16 x 16 luma, 8 x 8 chroma samples) with a hand-written edge table.  kind: one of
    FRAME_DK - a cell picture; "wavesV" / "wavesH" - compositions of db_edge's lanes on edge k = 1; "mixed" - every edge live.
    before: the samples (no stride padding: embed() adds it); edges: the table; places: what sits where."""

    def __init__(self, bd, chroma, kind, mb_w, mb_h, start=0, seed=0, c422=False):
        """c422: a 4:2:2 chroma plane - 8 x 16 macroblocks of six records, the vertical edges x = 0, 4 (16 lines, tc0 per 4), then the
        horizontal ones y = 0, 4, 8, 12 (8 columns, tc0 per 2)"""
        self.bd, self.chroma, self.kind, self.mb_w, self.mb_h, self.c422 = bd, chroma, kind, mb_w, mb_h, c422
        self.name = "%s/%s%d/%dx%d" % ("chroma 4:2:2" if c422 else "chroma" if chroma else "luma", kind, start, mb_w, mb_h)
        self.MB, self.ne = (8, 2) if chroma else (16, 4)
        self.MBW, self.MBH, self.nek = (8, 16, (2, 4)) if c422 else (self.MB, self.MB, (self.ne, self.ne))
        self.classes = (1, 3) if chroma else (0, 2)
        rng = np.random.default_rng(9000 * bd + 100 * chroma + 1000 * c422 + seed)
        self.before = rng.integers(0, 1 << bd, (mb_h * self.MBH, mb_w * self.MBW)).astype(np.uint8 if bd == 8 else np.uint16)
        n = mb_w * mb_h * sum(self.nek)
        self.edges = np.zeros(n, ffi.EDGE_DTYPE)
        # dead records: alpha == 0 or beta == 0, everything else alive and varied
        i = np.arange(n)
        self.edges["kind"] = i % 8
        self.edges["alpha"], self.edges["beta"] = 0, 18
        self.edges["alpha"][i % 5 == 2] = 40
        self.edges["beta"][i % 5 == 2] = 0
        self.edges["tc0"] = np.array([3, 0, -1, 25], np.int8)
        self.edges["offset"] = 12345 - 77 * i                            # ignored by the frame faces
        self.places = []
        self.recs = [r for cls in self.classes for r in records(bd, cls)]
        #: the records of the vertical and of the horizontal edges: as many lines as the macroblock is high / wide
        self.recs_d = [[r for cls in self.classes for r in records(bd, cls, 4)], self.recs] if c422 else [self.recs, self.recs]
        if kind == "mixed":
            self._mixed(rng)
        elif kind.startswith("waves"):
            self._waves(int(kind == "wavesH"))
        else:
            self._cells(int(kind[0] == "H"), kind[1] == "0", start)
        self.before.setflags(write=False)

    def slots(self, d, k0):
        """the live macroblocks of a cell picture in raster order: x + y even, not on the picture edge that is never filtered"""
        return [(mx, my) for my in range(self.mb_h) for mx in range(self.mb_w)
                if (mx + my) % 2 == 0 and not (k0 and (my if d else mx) == 0)]

    def index(self, mx, my, d, k):
        if self.c422:
            return (my * self.mb_w + mx) * 6 + (2 + k if d else k)
        return ((my * self.mb_w + mx) * 2 + d) * self.ne + k

    def _rect(self, a, mx, my, d, k):
        """the lines x 8 samples of an edge as a view of plane a: line = row for a vertical edge, column for a horizontal one"""
        W, H = self.MBW, self.MBH
        if d == 0:
            return a[my * H:(my + 1) * H, mx * W + 4 * k - 4:mx * W + 4 * k + 4]
        return a[my * H + 4 * k - 4:my * H + 4 * k + 4, mx * W:(mx + 1) * W].T

    def put(self, mx, my, d, k, rec, kind, write=True):
        self.edges[self.index(mx, my, d, k)] = (-1 - mx, kind, rec.alpha, rec.beta, 0, rec.tc0)
        if write:
            lines = rec_lines(rec)
            assert len(lines) == (self.MBW if d else self.MBH)
            self._rect(self.before, mx, my, d, k)[:] = lines
        self.places.append(Place(mx, my, d, k, rec, kind))

    def _kind(self, rec, n):
        """the frame faces read kind >= 4 as bS = 4 and ignore bits 0 / 1"""
        return (4 if rec.cls >= 2 else 0) + n % 4

    def _special(self):
        """three records for the rare hand-off rows: p2 p1 p0 change (strong), p1 p0 change, p0 alone"""
        want = (("s11", "n11", "n00") if not self.chroma else ("ci", "c", "c"))
        return [next(r for r in self.recs_d[1] if any(c.label == lab and {1, 2, 3} & c.changed for c in r.cells)) for lab in want]

    def _cells(self, d, k0, start):
        slots = self.slots(d, k0)
        rare = self._special()
        recs = self.recs_d[d]
        n = start
        for i, (mx, my) in enumerate(slots):
            k = 0 if k0 else 1 + i % (self.nek[d] - 1)
            if d == 1 and k0 and not self.c422 and handoff_class("skew", self.bd, self.chroma, my) == "other workgroup":
                rec = rare[mx // 2 % 3]
            else:
                rec = rot(recs[n % len(recs)], n // len(recs) + i)
                n += 1
            self.put(mx, my, d, k, rec, self._kind(rec, i))
        self.used = n - start

    def _waves(self, d):
        """edge k = 1 of every macroblock of the chosen anti-diagonals: the lanes of one db_edge call are the lines of macroblocks
        (s - q * DB_SKEW, band * Q + q), q = 0 .. Q - 1"""
        bd, Q = self.bd, 64 // self.MB
        ncls, icls = self.classes
        F = fill(icls, bd)
        norm = [r for r in records(bd, ncls) if sum(c.label not in ("none",) and bool(c.changed) for c in r.cells) >= 2]
        intr = [r for r in records(bd, icls) if r.alpha == 40]
        passing = [c for r in intr for c in r.cells if c.changed]
        allpass = [Rec(icls, 40, 10, intr[0].inner, INTRA_TC0, tuple(passing[(j * 5 + i) % len(passing)] for i in range(self.MB))) for j in range(Q)]
        allfail = Rec(icls, 40, 10, intr[0].inner, INTRA_TC0, (F,) * self.MB)
        onepass = Rec(icls, 40, 10, intr[0].inner, INTRA_TC0, (F,) * 5 + (passing[0],) + (F,) * (self.MB - 6))
        N = lambda j: norm[j % len(norm)]
        comps = [[N(j) for j in range(Q)],
                 [allfail, N(0)] * (Q // 2),
                 [N(j) for j in range(Q - 1)] + [onepass],
                 allpass,
                 [N(1), allpass[0]] + [N(j) for j in range(2, Q)],
                 [N(3), allpass[1]._replace(tc0=(127, -128, 127, -128))] + [N(j) for j in range(4, Q + 2)]]
        diags = [(band, s) for band in range(self.mb_h // Q) for s in range((Q - 1) * DB_SKEW, self.mb_w)]
        assert len(diags) >= len(comps)
        self.diags = {}
        for n, (band, s) in enumerate(diags[:len(comps) * (len(diags) // len(comps))]):
            comp = comps[n % len(comps)]
            for q in range(Q):
                rec = comp[(q + n // len(comps)) % Q]
                if rec.cls < 2:
                    rec = rot(rec, n + q)
                self.put(s - q * DB_SKEW, band * Q + q, d, 1, rec, self._kind(rec, n + q))
            self.diags[(band, s)] = COMPOSITIONS[n % len(comps)]

    def lanes(self, band, s):
        """(class, label) of the 64 lanes of the db_edge call of edge k = 1 at wave step s of a band, from the launch arithmetic"""
        Q = 64 // self.MB
        at = {(p.mx, p.my): p for p in self.places}
        out = []
        for q in range(Q):
            p = at.get((s - q * DB_SKEW, band * Q + q))
            for k in range(self.MB):
                if p is None:
                    out.append((None, "none", 0))
                else:
                    c = p.rec.cells[k]
                    o, label, ch = lf_model(c.px, p.rec.cls, p.rec.alpha, p.rec.beta, p.rec.tc0[k // p.rec.inner], self.bd)
                    out.append((p.rec.cls, label, p.rec.tc0[k // p.rec.inner]))
        return out

    def _mixed(self, rng):
        """every edge live, kinds mixed, the first column and row included; smooth content so that neighbouring edges filter what
        their neighbours wrote"""
        bd, MB = self.bd, self.MB
        F = 1 << (bd - 8)
        h, w = self.before.shape
        base = np.kron(rng.integers(20 * F, 230 * F, (h // 8 + 1, w // 8 + 1)), np.ones((8, 8), np.int64))[:h, :w]
        self.before[:] = np.clip(base + rng.integers(-6 * F, 6 * F + 1, (h, w)), 0, (1 << bd) - 1)
        n = len(self.edges)
        i = np.arange(n)
        self.edges["kind"] = np.where(i % 3 == 0, 4 + i % 4, i % 4)
        self.edges["alpha"] = np.array([255, 40, 20, 0, 80, 6])[i % 6]
        self.edges["beta"] = np.array([18, 10, 6, 12, 0, 15, 3])[i % 7]
        self.edges["tc0"] = np.array([[3, 0, -1, 25], [1, 2, 3, 4], [127, -128, 0, 1], [0, 0, 5, 13]], np.int8)[i % 4]

    # ---- buffers ---------------------------------------------------------------------------------------------------------
    def embed(self, pad, seed=0):
        """the plane with `pad` samples of seeded stride padding"""
        h, w = self.before.shape
        rng = np.random.default_rng(seed + pad)
        a = rng.integers(0, 1 << self.bd, (h, w + pad)).astype(self.before.dtype)
        a[:, :w] = self.before
        return a

    def want_oracle(self, pad=0, plain=None):
        """the oracle's frame order on embed(pad); plain: the 8-bit functions of oracle/ffo_h264.c, default at 8 bits"""
        O = oracle()
        a = self.embed(pad)
        e = self.edges.copy()
        if self.c422:
            O.ffo_h264_deblock_frame_c422_bd(self.bd, C.cast(a.ctypes.data, ffi.u8p), a.strides[0], self.mb_w, self.mb_h, e.ctypes.data)
        elif (self.bd == 8) if plain is None else plain:
            (O.ffo_h264_deblock_frame_chroma if self.chroma else O.ffo_h264_deblock_frame)(ffi.ptr(a), a.strides[0], self.mb_w, self.mb_h, e.ctypes.data)
        else:
            O.ffo_h264_deblock_frame_bd(self.bd, int(self.chroma), C.cast(a.ctypes.data, ffi.u8p), a.strides[0], self.mb_w, self.mb_h, e.ctypes.data)
        return a

    def want_model(self, pad=0):
        a = self.embed(pad)
        for p in self.places:
            self._rect(a, p.mx, p.my, p.dir, p.k)[:] = rec_model(p.rec, self.bd)
        return a

    def lines(self, a, p):
        return self._rect(a, p.mx, p.my, p.dir, p.k)

    def dk(self, p):
        return "VH"[p.dir] + ("0" if p.k == 0 else "n")

    def first_bad(self, got, want, kernel):
        for p in self.places:
            a, b = self.lines(got, p), self.lines(want, p)
            rows = np.flatnonzero((a != b).any(axis=1))
            if len(rows):
                line = int(rows[0])
                c = p.rec.cells[line]
                return "%s: route %s/%s/%s, macroblock (%d, %d) edge %d, kind %d alpha %d beta %d tc0 %s, line %d: cell %s, label %s: got %s, want %s" % (
                    self.name, kernel, "chroma" if self.chroma else "luma", self.dk(p), p.mx, p.my, p.k, p.kind, p.rec.alpha, p.rec.beta, list(p.rec.tc0),
                    line, c.name, c.label, a[line].tolist(), b[line].tolist())
        bad = np.argwhere(got != want)
        return "%s (%s): %d mismatches outside every live edge, first at %s" % (self.name, kernel, len(bad), bad[0].tolist()) if len(bad) else None

    def triples(self, dk=None):
        return {t for p in self.places if dk in (None, self.dk(p)) for t in rec_triples(p.rec, p.kind)}


@functools.lru_cache(maxsize=None)
def frame_pics(bd, chroma):
    """the cell pictures of one plane class, all of one geometry (so that they also run as the pictures of one launch): 8 macroblocks
    across and 34 (chroma: 66) down, which the k == 0 horizontal route needs for the hand-off between workgroups of the skew
    kernel; per (direction, k class) as many as hold every record"""
    mb_w, mb_h = 8, 66 if chroma else 34
    out = []
    for j, dk in enumerate(FRAME_DK):
        P = FramePic(bd, chroma, dk, mb_w, mb_h, 0, seed=j)
        assert P.used >= len(P.recs), (dk, P.used, len(P.recs))
        out.append(P)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def waves_pics(bd, chroma):
    mb_w, mb_h = (12, 16) if chroma else (8, 8)
    return (FramePic(bd, chroma, "wavesV", mb_w, mb_h, 0, seed=21), FramePic(bd, chroma, "wavesH", mb_w, mb_h, 0, seed=22))


@functools.lru_cache(maxsize=None)
def mixed_pic(bd, chroma):
    return FramePic(bd, chroma, "mixed", 7, 19 if chroma else 18, 0, seed=30)


@functools.lru_cache(maxsize=None)
def c422_pics(bd, plane):
    """the cell pictures of one 4:2:2 chroma plane (1 Cb, 2 Cr) for k_h264_deblock_c422: a workgroup per macroblock row, so every row of
    the k == 0 horizontal picture is handed off through memory"""
    out = []
    for j, dk in enumerate(FRAME_DK):
        P = FramePic(bd, 1, dk, 8, 7, 0, seed=40 + 4 * plane + j, c422=True)
        assert P.used >= len(P.recs_d[int(dk[0] == "H")]), (dk, P.used)
        out.append(P)
    return tuple(out) + (FramePic(bd, 1, "mixed", 5, 4, 0, seed=60 + plane, c422=True),)


def frame_missing(pics, dk, classes):
    """the cells of the plane's classes that no live record of the (direction, k class) holds"""
    have = {t[0] for P in pics for t in P.triples(dk)}
    return sorted({c.name for c in cells(pics[0].bd) if c.cls in classes} - have)


def handoff_missing(pics, kernel, nframes=1):
    """(hand-off class, what must change) pairs absent from the k == 0 horizontal route: the p side of that edge belongs to the row above"""
    have = set()
    for P in pics:
        for p in P.places:
            if p.dir == 1 and p.k == 0:
                cl = handoff_class(kernel, P.bd, P.chroma, p.my, nframes, P.mb_h)
                for c in p.rec.cells:
                    have.add((cl, tuple(sorted(c.changed & {1, 2, 3}))))
    need = [(3,)] if pics[0].chroma else [(1, 2, 3), (2, 3), (3,)]
    return [(cl, n) for cl in HANDOFF[kernel] for n in need if (cl, n) not in have]


def compositions(P):
    """the COMPOSITIONS the diagonals of a waves picture hold, by the model's labels of the 64 lanes"""
    have = set()
    for (band, s), name in P.diags.items():
        L = P.lanes(band, s)
        is4 = [c is not None and c >= 2 for c, lab, t in L]
        passing = [i4 and lab != "none" for i4, (c, lab, t) in zip(is4, L)]
        filtered = [not i4 and lab != "none" for i4, (c, lab, t) in zip(is4, L)]
        if not any(is4) and any(filtered):
            have.add(COMPOSITIONS[0])
        if any(is4) and not any(passing):
            have.add(COMPOSITIONS[1])
        if sum(passing) == 1:
            have.add(COMPOSITIONS[2])
        if all(passing):
            have.add(COMPOSITIONS[3])
        nmb4 = sum(any(is4[q * P.MB:(q + 1) * P.MB]) for q in range(64 // P.MB))
        if nmb4 == 1 and any(passing) and sum(any(filtered[q * P.MB:(q + 1) * P.MB]) for q in range(64 // P.MB)) == 64 // P.MB - 1:
            have.add(COMPOSITIONS[5] if {t for i4, (c, lab, t) in zip(is4, L) if i4} == {127, -128} else COMPOSITIONS[4])
    return have


# ---------------------------------------------------------------------------------------------------------------------------
# the MBAFF object route: ffhip_h264_mbaff_filter_call() / ffhip_h264_mbaff_flush()
# ---------------------------------------------------------------------------------------------------------------------------
CALL_FIELD, CALL_MBAFF = 1, 2                                   # FFHIP_H264_LF_CALL_*
#: one dsp call: plane 0 / 1 / 2; the macroblock it is recorded for; (y, x): q0 of line 0; col: a vertical edge (lines are rows);
#: flags: CALL_FIELD (twice the line size) | CALL_MBAFF (the 8 / 4-line member)
Call = namedtuple("Call", "plane mb_x mb_y y x col flags rec")


class MbaffPic:
    """One frame of mb_w x mb_h macroblocks (mb_h even) whose filter calls are written directly.  Only macroblock pairs with x + pair row
    even carry a call, exactly one per plane, inside the pair or (column edge k = 0) reaching into the dead pair on its left: footprints
    are disjoint and the calls commute, so the oracle runs them call by call.  Ordinary members at the frame's and at twice the line
    size, the _mbaff members (luma 8 lines, tc0 per 2; chroma 4, tc0 per 1) likewise."""

    def __init__(self, bd, mb_w=8, mb_h=34, seed=0):
        self.bd, self.mb_w, self.mb_h = bd, mb_w, mb_h
        dt = np.uint8 if bd == 8 else np.uint16
        rng = np.random.default_rng(11000 * bd + seed)
        self.before = [rng.integers(0, 1 << bd, (mb_h * 16, mb_w * 16)).astype(dt)] + \
                      [rng.integers(0, 1 << bd, (mb_h * 8, mb_w * 8)).astype(dt) for _ in range(2)]
        self.calls = []
        live = [(x, p) for p in range(mb_h // 2) for x in range(mb_w) if (x + p) % 2 == 0]
        for plane in range(3):
            c = int(plane > 0)
            W, H = (8, 16) if c else (16, 32)                    # the pair on this plane
            n = H // 2                                           # lines of an ordinary member = the macroblock's height
            full = [r for cls in ((1, 3) if c else (0, 2)) for r in records(bd, cls, 2 if c else 4)]
            half = [r for cls in ((1, 3) if c else (0, 2)) for r in records(bd, cls, 1 if c else 2)]
            todo = [(r, 0) for r in full] + [(r, CALL_MBAFF) for r in half]
            assert len(todo) <= len(live), (plane, len(todo), len(live))
            for i, (x, p) in enumerate(live):
                rec, fl = todo[(i + 7 * plane) % len(todo)]
                rec = rot(rec, i + plane)
                j = i // len(todo) + i
                field = (j >> 1) & 1
                stl = 2 if field else 1
                parity = j & 1
                nl = len(rec.cells)
                if fl or (j >> 2) & 1 == 0:                      # a column edge: k = 0 reaches into the dead pair on the left
                    k = (j // 8) % (W // 4)
                    if k == 0 and x == 0:
                        k = 1
                    if field:
                        y0 = parity + (2 * nl if fl and (j >> 3) & 1 else 0)         # the _mbaff member's second half of the field
                    else:
                        y0 = nl * ((j >> 3) % (H // nl))
                    self.calls.append(Call(plane, x, 2 * p + (parity if field else int(y0 >= n)), H * p + y0, W * x + 4 * k, 1, fl | field, rec))
                else:                                            # a row edge inside the pair
                    up = 2 if c else 4
                    rows = [r for r in range(0, H, 4) if r - up * stl >= 0] if not field else [r for r in range(4, n, 4) if r - up >= 0]
                    r = rows[(j >> 3) % len(rows)]
                    y0 = parity + 2 * r if field else r
                    self.calls.append(Call(plane, x, 2 * p + (parity if field else int(y0 >= n)), H * p + y0, W * x, 0, field, rec))
                self._rect(self.before[plane], self.calls[-1])[:] = rec_lines(rec)
        for a in self.before:
            a.setflags(write=False)

    @staticmethod
    def _rect(a, c):
        """the lines x 8 samples of a call as a view of plane a"""
        stl = 2 if c.flags & CALL_FIELD else 1
        n = len(c.rec.cells)
        if c.col:
            return a[c.y:c.y + n * stl:stl, c.x - 4:c.x + 4]
        return a[c.y - 4 * stl:c.y + 4 * stl:stl, c.x:c.x + n].T

    def in_tile(self, c):
        """mbaff_place_call() (csrc/h264_mbaff.hip): the call lies in the tile of its pair - the pair, AB lines above, 4 columns left"""
        ch = int(c.plane > 0)
        W, H, AB = (8, 16, 4) if ch else (16, 32, 8)
        stl = 2 if c.flags & CALL_FIELD else 1
        tl, tc = c.y - (H * (c.mb_y // 2) - AB), c.x - (W * c.mb_x - 4)
        if tc < 4 or tc & 3:
            return False
        if c.col:
            return tl >= 0 and tl + (len(c.rec.cells) - 1) * stl < H + AB and tc < W + 4
        up, down = (2, 1) if ch else (4, 3)
        return not c.flags & CALL_MBAFF and tl - up * stl >= 0 and tl + down * stl < H + AB and tc + len(c.rec.cells) <= W + 4

    def embed(self, pad):
        out = []
        for k, b in enumerate(self.before):
            a = np.random.default_rng(pad + k).integers(0, 1 << self.bd, (b.shape[0], b.shape[1] + (pad if k == 0 else pad // 2))).astype(b.dtype)
            a[:, :b.shape[1]] = b
            out.append(a)
        return out

    def edge(self, c, stride):
        """the FFHipH264Edge of the call at the plane's line size"""
        e = np.zeros(1, ffi.EDGE_DTYPE)
        e[0] = (c.y * stride + c.x * (1 if self.bd == 8 else 2), kind_of(c.rec.cls, c.col), c.rec.alpha, c.rec.beta, c.flags, c.rec.tc0)
        return e

    def want_oracle(self, pad=0):
        O = oracle()
        planes = self.embed(pad)
        for c in self.calls:
            a = planes[c.plane]
            stl = 2 if c.flags & CALL_FIELD else 1
            O.ffo_h264_loop_filter_bd(self.bd, kind_of(c.rec.cls, c.col), c.rec.inner, C.cast(a.ctypes.data + c.y * a.strides[0] + c.x * a.itemsize, ffi.u8p),
                                      a.strides[0] * stl, c.rec.alpha, c.rec.beta, ffi.ptr(np.array(c.rec.tc0, np.int8), ffi.i8p))
        return planes

    def want_model(self, pad=0):
        planes = self.embed(pad)
        for c in self.calls:
            self._rect(planes[c.plane], c)[:] = rec_model(c.rec, self.bd)
        return planes

    def first_bad(self, got, want):
        for c in self.calls:
            a, b = self._rect(got[c.plane], c), self._rect(want[c.plane], c)
            rows = np.flatnonzero((a != b).any(axis=1))
            if len(rows):
                line = int(rows[0])
                x = c.rec.cells[line]
                return "MBAFF plane %d macroblock (%d, %d), %s edge, flags %d, alpha %d beta %d tc0 %s, line %d: cell %s, label %s: got %s, want %s" % (
                    c.plane, c.mb_x, c.mb_y, "column" if c.col else "row", c.flags, c.rec.alpha, c.rec.beta, list(c.rec.tc0), line, x.name, x.label,
                    a[line].tolist(), b[line].tolist())
        bad = [(k, np.argwhere(g != w)[0].tolist()) for k, (g, w) in enumerate(zip(got, want)) if (g != w).any()]
        return "MBAFF: mismatches outside every call, first at plane %d %s" % bad[0] if bad else None


@functools.lru_cache(maxsize=None)
def mbaff_pic(bd):
    return MbaffPic(bd)
