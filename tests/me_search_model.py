"""A numpy model of the filter's per-block motion searches (ESA, TSS, TDLS, NTSS, FSS, DS, HEXBS), written from the rules text of
ffhip_me_search_batch_dev() in include/ffhip.h — sequential COST_MV / COST_P_MV, as the text has them — and not from
kernels/me_search_rules.h, which restates the same text as a step machine with an ordered minimum.  The rules are restated, not checked
against libavfilter/motion_estimation.c.

COUNTS counts every branch of the rules a search takes, so that a test can show that its inputs reach all of them."""
import collections

import numpy as np

ESA, TSS, TDLS, NTSS, FSS, DS, HEXBS = range(1, 8)
NAMES = {ESA: "esa", TSS: "tss", TDLS: "tdls", NTSS: "ntss", FSS: "fss", DS: "ds", HEXBS: "hexbs"}
SAD, SATD = 0, 1

SQR1 = [(0, -1), (0, 1), (-1, 0), (1, 0), (-1, -1), (-1, 1), (1, -1), (1, 1)]
DIA1 = [(-1, 0), (0, -1), (1, 0), (0, 1)]
DIA2 = [(-2, 0), (-1, -1), (0, -2), (1, -1), (2, 0), (1, 1), (0, 2), (-1, 1)]
HEX2 = [(-2, 0), (-1, -2), (-1, 2), (1, -2), (1, 2), (2, 0)]

COUNTS = collections.Counter()
#: the counters a set of inputs has to reach (tests/test_me_search_cpu.py::test_the_inputs_reach_every_branch)
BRANCHES = (["zero_cost_start", "window_refused", "picture_refused", "tie_keeps_earlier", "tie_keeps_centre",
             "ntss_exit_centre", "ntss_exit_unit_ring", "ntss_exit_large_ring"] +
            ["%s_centre_%s" % (NAMES[m], k) for m in range(TSS, HEXBS + 1) for k in ("kept", "moved")])

_H8 = np.array([[1]])
for _ in range(3):
    _H8 = np.block([[_H8, _H8], [_H8, -_H8]])


class Block:
    """one block's search: the cost, the window and the two macros"""

    def __init__(self, cur, ref, width, height, mb, R, kind, x_mb, y_mb):
        log2mb = {16: 4, 8: 3}[mb]
        b_w, b_h = width >> log2mb, height >> log2mb
        self.cur = cur[y_mb:y_mb + mb, x_mb:x_mb + mb].astype(np.int64)
        self.ref, self.mb, self.kind, self.R = ref, mb, kind, R
        self.x_mb, self.y_mb = x_mb, y_mb
        self.lim_x, self.lim_y = (b_w - 1) << log2mb, (b_h - 1) << log2mb
        self.x_min, self.x_max = max(0, x_mb - R), min(x_mb + R, self.lim_x)
        self.y_min, self.y_max = max(0, y_mb - R), min(y_mb + R, self.lim_y)
        self.ncost = 0
        self.won = False        # a candidate of the running iteration holds the minimum (for the tie counters)
        self.mv = (x_mb, y_mb)
        self.cost_min = self.cost(x_mb, y_mb)

    def cost(self, x, y):
        self.ncost += 1
        assert 0 <= x and 0 <= y and x + self.mb <= self.ref.shape[1] and y + self.mb <= self.ref.shape[0]
        d = self.cur - self.ref[y:y + self.mb, x:x + self.mb].astype(np.int64)
        if self.kind == SAD:
            return int(np.abs(d).sum())
        hm = np.kron(np.eye(self.mb // 8, dtype=np.int64), _H8)      # the 8x8 transform of every 8x8 block
        return int(np.abs(hm @ d @ hm).sum())

    def cost_mv(self, x, y):
        c = self.cost(x, y)
        if c < self.cost_min:
            self.cost_min, self.mv, self.won = c, (x, y), True
        elif c == self.cost_min:
            COUNTS["tie_keeps_earlier" if self.won else "tie_keeps_centre"] += 1

    def raster_scan(self):
        """COST_MV over the window in raster order, in closed form (the costs of a 65 x 65 window one by one would take minutes):
        the first minimum in raster order, taken only if it is strictly below cost_min"""
        win = self.ref[self.y_min:self.y_max + self.mb, self.x_min:self.x_max + self.mb].astype(np.int64)
        d = self.cur - np.lib.stride_tricks.sliding_window_view(win, (self.mb, self.mb))
        if self.kind == SATD:
            hm = np.kron(np.eye(self.mb // 8, dtype=np.int64), _H8)
            d = hm @ d @ hm
        costs = np.abs(d).sum((2, 3))
        self.ncost += costs.size
        i = int(np.argmin(costs))
        if costs.flat[i] < self.cost_min:
            self.cost_min, self.mv = int(costs.flat[i]), (self.x_min + i % costs.shape[1], self.y_min + i // costs.shape[1])

    def cost_p_mv(self, x, y):
        if self.x_min <= x <= self.x_max and self.y_min <= y <= self.y_max:
            self.cost_mv(x, y)
        elif abs(x - self.x_mb) <= self.R and abs(y - self.y_mb) <= self.R:
            COUNTS["picture_refused"] += 1      # within +-R of the block: it is the picture limit that cuts it off
        else:
            COUNTS["window_refused"] += 1

    def ring(self, table, centre, step=1, same_iteration=False):
        self.won = self.won and same_iteration
        for dx, dy in table:
            self.cost_p_mv(centre[0] + dx * step, centre[1] + dy * step)


def search(method, cur, ref, width, height, mb, R, kind, x_mb, y_mb):
    """-> (mv x, mv y, cost, costs evaluated)"""
    b = Block(cur, ref, width, height, mb, R, kind, x_mb, y_mb)
    name = NAMES[method]

    def moved(centre):
        COUNTS["%s_centre_%s" % (name, "moved" if b.mv != centre else "kept")] += 1
        return b.mv != centre

    if b.cost_min == 0:
        COUNTS["zero_cost_start"] += 1
    elif method == ESA:
        b.raster_scan()
    elif method == TSS:
        step = (R + 1) >> 1
        while True:
            c = b.mv
            b.ring(SQR1, c, step)
            moved(c)
            step >>= 1
            if step <= 0:
                break
    elif method in (TDLS, FSS):
        step = (R + 1) >> 1 if method == TDLS else 2
        while True:
            c = b.mv
            b.ring(DIA1 if method == TDLS else SQR1, c, step)
            if not moved(c):
                step >>= 1
            if step <= 0:
                break
    elif method == NTSS:
        step, first = (R + 1) >> 1, True
        while True:
            c = b.mv
            b.ring(SQR1, c, step)
            if first:
                b.ring(SQR1, c, 1, same_iteration=True)         # round the same (x, y), not round the updated mv
                if b.mv == c:
                    COUNTS["ntss_exit_centre"] += 1
                    moved(c)
                    break
                if abs(c[0] - b.mv[0]) <= 1 and abs(c[1] - b.mv[1]) <= 1:
                    COUNTS["ntss_exit_unit_ring"] += 1
                    moved(c)
                    b.ring(SQR1, b.mv, 1)
                    break
                COUNTS["ntss_exit_large_ring"] += 1
                first = False
            moved(c)
            step >>= 1
            if step <= 0:
                break
    else:
        assert method in (DS, HEXBS)
        while True:
            c = b.mv
            b.ring(DIA2 if method == DS else HEX2, c)
            if not moved(c):
                break
        b.ring(DIA1, c)
    return b.mv[0], b.mv[1], b.cost_min, b.ncost


def frames(method, cur, ref, width, height, mb, R, kind):
    """cur, ref: (nframes, height, stride) uint8.  -> mv int16 (nframes, b_h * b_w * 2), cost uint32 (nframes, b_h * b_w), the costs
    evaluated"""
    log2mb = {16: 4, 8: 3}[mb]
    b_w, b_h = width >> log2mb, height >> log2mb
    nf = cur.shape[0]
    mv = np.zeros((nf, b_h * b_w * 2), np.int16)
    cost = np.zeros((nf, b_h * b_w), np.uint32)
    n = 0
    for f in range(nf):
        for by in range(b_h):
            for bx in range(b_w):
                x, y, c, k = search(method, cur[f], ref[f], width, height, mb, R, kind, bx << log2mb, by << log2mb)
                i = by * b_w + bx
                mv[f, 2 * i], mv[f, 2 * i + 1], cost[f, i] = x, y, c
                n += k
    return mv, cost, n
