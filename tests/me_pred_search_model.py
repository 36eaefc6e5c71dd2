"""A numpy model of the filter's two predictive motion searches (EPZS, UMH), written from the rules text of
ffhip_me_search_pred_batch_dev() in include/ffhip.h — sequential COST_MV / COST_P_MV over plain Python lists, the d loops run in full —
and not from kernels/me_search_pred_rules.h, which restates the same text as a step machine with an ordered minimum and bounded d
loops.  The rules are restated, not checked against libavfilter/motion_estimation.c.

COUNTS counts every branch of the rules a search takes, so that a test can show that its inputs reach all of them."""
import collections

import numpy as np

from me_search_model import DIA1, HEX2, SAD, SATD, Block  # noqa: F401

EPZS, UMH = 8, 9
NAMES = {EPZS: "epzs", UMH: "umh"}

HEX4 = [(-4, -2), (-4, -1), (-4, 0), (-4, 1), (-4, 2), (4, -2), (4, -1), (4, 0), (4, 1), (4, 2), (-2, 3), (0, 4), (2, 3), (-2, -3), (0, -4),
        (2, -3)]

COUNTS = collections.Counter()
PREDICTORS = ["median", "zero", "left", "top", "topright", "topleft", "collocated", "accelerator", "prev_left", "prev_top", "prev_right",
              "prev_bottom"]
UMH_PHASES = ["cross", "raster", "rings", "hex2", "dia1"]
#: the counters a set of inputs has to reach (tests/test_me_pred_search_cpu.py::test_the_inputs_reach_every_branch)
BRANCHES = (["wins_" + p for p in PREDICTORS] + ["median_n%d" % n for n in (1, 2, 3, 4)] +
            ["umh_%s_%s" % (p, k) for p in UMH_PHASES for k in ("moved", "kept")] + ["epzs_dia1_moved", "epzs_dia1_kept"] +
            ["cross_with_vertical_arm", "cross_without_vertical_arm", "no_rings"] +
            ["refused_" + p for p in ("predictor", "epzs_dia1", "cross", "rings", "hex2", "umh_dia1")] +
            ["tie_keeps_earlier", "tie_keeps_best"])


class PredBlock(Block):
    """one block's search: Block's cost and window; cost_min starts as "none yet", and the macros count into this module's COUNTS"""

    memo = None

    def __init__(self, *a):
        super().__init__(*a)
        self.ncost = 0                  # Block evaluated the origin: the predictive searches do not
        self.cost_min = None
        self.memo = {}
        self.phase = "predictor"
        self.taker = None               # the label of the candidate that took the minimum last

    def cost(self, x, y):
        if self.memo is None:
            return super().cost(x, y)
        if (x, y) not in self.memo:
            self.memo[x, y] = super().cost(x, y)
            self.ncost -= 1
        self.ncost += 1                 # a duplicate is evaluated again
        return self.memo[x, y]

    def cost_mv(self, x, y, label=None):
        c = self.cost(x, y)
        if self.cost_min is None or c < self.cost_min:
            self.cost_min, self.mv, self.won, self.taker = c, (x, y), True, label
        elif c == self.cost_min:
            COUNTS["tie_keeps_earlier" if self.won else "tie_keeps_best"] += 1

    def cost_p_mv(self, x, y, label=None):
        if self.x_min <= x <= self.x_max and self.y_min <= y <= self.y_max:
            self.cost_mv(x, y, label)
        else:
            COUNTS["refused_" + self.phase] += 1

    def begin(self, phase):
        """a new list of candidates: none of them holds the minimum yet"""
        self.phase, self.won = phase, False
        return self.mv


def _mid(a, b, c):
    return sorted((a, b, c))[1]


def search(method, cur, ref, width, height, mb, R, kind, bx, by, field, prev1, prev2):
    """Block (bx, by).  field: the current pair's absolute positions so far, (b_h, b_w, 2); prev1, prev2: the same of the two previous
    pairs, or None.  -> (mv x, mv y, cost, costs evaluated)"""
    log2mb = {16: 4, 8: 3}[mb]
    b_w, b_h = width >> log2mb, height >> log2mb
    x_mb, y_mb = bx << log2mb, by << log2mb
    b = PredBlock(cur, ref, width, height, mb, R, kind, x_mb, y_mb)

    def rel(f, x, y):
        """block (x, y)'s relative vector in field f: position minus block origin, in Python's integers"""
        if f is None:
            return (0, 0)
        return (int(f[y, x, 0]) - (x << log2mb), int(f[y, x, 1]) - (y << log2mb))

    # ---- the predictor lists, appended as the text appends them -------------------------------------------------------------------
    p0, p1 = [("zero", (0, 0))], []
    if bx > 0:
        p0.append(("left", rel(field, bx - 1, by)))
    if method == EPZS:
        if by > 0:
            p0.append(("top", rel(field, bx, by - 1)))
        if by > 0 and bx + 1 < b_w:
            p0.append(("topright", rel(field, bx + 1, by - 1)))
    else:
        if by > 0:
            p0.append(("top", rel(field, bx, by - 1)))
            if bx + 1 < b_w:
                p0.append(("topright", rel(field, bx + 1, by - 1)))
            elif bx > 0:
                p0.append(("topleft", rel(field, bx - 1, by - 1)))
    n = len(p0)
    COUNTS["median_n%d" % n] += 1
    if n == 4:
        median = tuple(_mid(p0[1][1][i], p0[2][1][i], p0[3][1][i]) for i in (0, 1))
    elif n == 3:
        median = tuple(_mid(0, p0[1][1][i], p0[2][1][i]) for i in (0, 1))
    elif n == 2:
        median = p0[1][1]
    else:
        median = (0, 0)
    if method == EPZS:
        r1, r2 = rel(prev1, bx, by), rel(prev2, bx, by)
        p0.append(("collocated", r1))
        p1.append(("accelerator", (2 * r1[0] - r2[0], 2 * r1[1] - r2[1])))
        if bx > 0:
            p1.append(("prev_left", rel(prev1, bx - 1, by)))
        if by > 0:
            p1.append(("prev_top", rel(prev1, bx, by - 1)))
        if bx + 1 < b_w:
            p1.append(("prev_right", rel(prev1, bx + 1, by)))
        if by + 1 < b_h:
            p1.append(("prev_bottom", rel(prev1, bx, by + 1)))

    # ---- the predictors ------------------------------------------------------------------------------------------------------------
    b.begin("predictor")
    for label, (vx, vy) in [("median", median)] + p0 + p1:
        b.cost_p_mv(x_mb + vx, y_mb + vy, label)
    COUNTS["wins_" + b.taker] += 1

    def moved(name, centre):
        COUNTS["%s_%s" % (name, "moved" if b.mv != centre else "kept")] += 1
        return b.mv != centre

    if method == EPZS:
        while True:
            x, y = b.begin("epzs_dia1")
            for dx, dy in DIA1:
                b.cost_p_mv(x + dx, y + dy)
            if not moved("epzs_dia1", (x, y)):
                break
        return b.mv[0], b.mv[1], b.cost_min, b.ncost

    # ---- UMH -------------------------------------------------------------------------------------------------------------------------
    x, y = b.begin("cross")
    for d in range(1, R + 1, 2):
        b.cost_p_mv(x - d, y)
        b.cost_p_mv(x + d, y)
        if d <= R // 2:
            COUNTS["cross_with_vertical_arm"] += 1
            b.cost_p_mv(x, y - d)
            b.cost_p_mv(x, y + d)
        else:
            COUNTS["cross_without_vertical_arm"] += 1
    moved("umh_cross", (x, y))
    cx, cy = b.begin("raster")
    for y in range(max(b.y_min, cy - 2), min(cy + 2, b.y_max) + 1):
        for x in range(max(b.x_min, cx - 2), min(cx + 2, b.x_max) + 1):
            b.cost_mv(x, y)
    moved("umh_raster", (cx, cy))
    x, y = b.begin("rings")
    if R // 4 < 1:
        COUNTS["no_rings"] += 1
    for d in range(1, R // 4 + 1):
        for dx, dy in HEX4[1:]:
            b.cost_p_mv(x + dx * d, y + dy * d)
    moved("umh_rings", (x, y))
    while True:
        x, y = b.begin("hex2")
        for dx, dy in HEX2:
            b.cost_p_mv(x + dx, y + dy)
        if not moved("umh_hex2", (x, y)):
            break
    b.begin("umh_dia1")
    for dx, dy in DIA1:
        b.cost_p_mv(x + dx, y + dy)
    moved("umh_dia1", (x, y))
    return b.mv[0], b.mv[1], b.cost_min, b.ncost


def frames(method, cur, ref, width, height, mb, R, kind, prev1=None, prev2=None):
    """cur, ref: (nframes, height, stride) uint8; prev1, prev2: int16 (nframes, b_h * b_w * 2) or None.  The blocks of a pair in raster
    order.  -> mv int16 (nframes, b_h * b_w * 2), cost uint32 (nframes, b_h * b_w), the costs evaluated"""
    log2mb = {16: 4, 8: 3}[mb]
    b_w, b_h = width >> log2mb, height >> log2mb
    nf = cur.shape[0]
    mv = np.zeros((nf, b_h * b_w * 2), np.int16)
    cost = np.zeros((nf, b_h * b_w), np.uint32)
    n = 0
    for f in range(nf):
        field = mv[f].reshape(b_h, b_w, 2)
        q1 = None if prev1 is None else prev1[f].reshape(b_h, b_w, 2)
        q2 = None if prev2 is None else prev2[f].reshape(b_h, b_w, 2)
        for by in range(b_h):
            for bx in range(b_w):
                x, y, c, k = search(method, cur[f], ref[f], width, height, mb, R, kind, bx, by, field, q1, q2)
                field[by, bx] = (x, y)
                cost[f, by * b_w + bx] = c
                n += k
    return mv, cost, n
