"""A numpy model of the bilateral motion search (vf_minterpolate's me_mode=bilat: EPZS or UMH under the overlapped bilateral cost),
written from the rule text of ffhip_me_search_bilat_batch_dev() in include/ffhip.h and not from kernels/me_search_bilat_rules.h or
kernels/me_search_pred_rules.h.  The search is restated here — sequential COST_MV / COST_P_MV over plain Python lists, the d loops run
in full — because the block of tests/me_pred_search_model.py fixes its cost when it is made, before a median exists.  The rules are
restated, not checked against libavfilter/vf_minterpolate.c."""
import numpy as np

from me_pred_search_model import HEX4
from me_search_model import DIA1, HEX2

EPZS, UMH = 8, 9
NAMES = {EPZS: "epzs", UMH: "umh"}


def clip(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def window(width, height, mb, R, x_mb, y_mb):
    """x_min, x_max, y_min, y_max of the block at (x_mb, y_mb)"""
    log2mb = {16: 4, 8: 3}[mb]
    lim_x, lim_y = ((width >> log2mb) - 1) << log2mb, ((height >> log2mb) - 1) << log2mb
    return max(0, x_mb - R), min(x_mb + R, lim_x), max(0, y_mb - R), min(y_mb + R, lim_y)


def place(o, p, w_min, w_max, h):
    """one axis: the centre c and the clamped half-displacement d of candidate position p of the block with origin o"""
    lo, hi = w_min + h, w_max - h
    assert lo <= hi
    c = clip(o, lo, hi)
    r = min(c - lo, hi - c)
    return c, clip(p - c, -r, r)


def sbad(A, B, width, height, mb, R, x_mb, y_mb, X, Y):
    """the sum over the overlapped window of twice the block size; every read is asserted to lie in the width x height plane"""
    h = mb // 2
    x_min, x_max, y_min, y_max = window(width, height, mb, R, x_mb, y_mb)
    cx, dx = place(x_mb, X, x_min, x_max, h)
    cy, dy = place(y_mb, Y, y_min, y_max, h)
    ax, ay, bx, by = cx + dx - h, cy + dy - h, cx - dx - h, cy - dy - h
    for x0, y0 in ((ax, ay), (bx, by)):
        assert 0 <= x0 and x0 + 2 * mb <= width and 0 <= y0 and y0 + 2 * mb <= height
    a = A[ay:ay + 2 * mb, ax:ax + 2 * mb].astype(np.int64)
    b = B[by:by + 2 * mb, bx:bx + 2 * mb].astype(np.int64)
    return int(np.abs(a - b).sum())


def cost(A, B, width, height, mb, R, x_mb, y_mb, X, Y, pred):
    return (sbad(A, B, width, height, mb, R, x_mb, y_mb, X, Y) + 64 * (abs(X - x_mb - pred[0]) + abs(Y - y_mb - pred[1]))) & 0xFFFFFFFF


def _mid(a, b, c):
    return sorted((a, b, c))[1]


class Block:
    """one block's search: the window, the cost with its fixed predictor, COST_MV and COST_P_MV"""

    def __init__(self, A, B, width, height, mb, R, x_mb, y_mb, pred):
        self.args = (A, B, width, height, mb, R, x_mb, y_mb)
        self.pred = pred
        self.x_min, self.x_max, self.y_min, self.y_max = window(width, height, mb, R, x_mb, y_mb)
        self.mv, self.cost_min, self.ncost, self.memo = (x_mb, y_mb), None, 0, {}

    def cost(self, x, y):
        self.ncost += 1                 # a duplicate is evaluated again
        if (x, y) not in self.memo:
            self.memo[x, y] = cost(*self.args, x, y, self.pred)
        return self.memo[x, y]

    def cost_mv(self, x, y):
        c = self.cost(x, y)
        if self.cost_min is None or c < self.cost_min:
            self.cost_min, self.mv = c, (x, y)

    def cost_p_mv(self, x, y):
        if self.x_min <= x <= self.x_max and self.y_min <= y <= self.y_max:
            self.cost_mv(x, y)


def search(method, A, B, width, height, mb, R, bx, by, field, prev1, prev2):
    """Block (bx, by).  field: the current pair's absolute positions so far, (b_h, b_w, 2); prev1, prev2: the same of the two previous
    pairs, or None.  -> (mv x, mv y, cost, costs evaluated)"""
    log2mb = {16: 4, 8: 3}[mb]
    b_w, b_h = width >> log2mb, height >> log2mb
    x_mb, y_mb = bx << log2mb, by << log2mb

    def rel(f, x, y):
        if f is None:
            return (0, 0)
        return (int(f[y, x, 0]) - (x << log2mb), int(f[y, x, 1]) - (y << log2mb))

    p0, p1 = [(0, 0)], []
    if bx > 0:
        p0.append(rel(field, bx - 1, by))
    if by > 0:
        p0.append(rel(field, bx, by - 1))
        if bx + 1 < b_w:
            p0.append(rel(field, bx + 1, by - 1))
        elif method == UMH and bx > 0:
            p0.append(rel(field, bx - 1, by - 1))
    n = len(p0)
    if n == 4:
        median = tuple(_mid(p0[1][i], p0[2][i], p0[3][i]) for i in (0, 1))
    elif n == 3:
        median = tuple(_mid(0, p0[1][i], p0[2][i]) for i in (0, 1))
    elif n == 2:
        median = p0[1]
    else:
        median = (0, 0)
    if method == EPZS:
        r1, r2 = rel(prev1, bx, by), rel(prev2, bx, by)
        p0.append(r1)
        p1.append((2 * r1[0] - r2[0], 2 * r1[1] - r2[1]))
        if bx > 0:
            p1.append(rel(prev1, bx - 1, by))
        if by > 0:
            p1.append(rel(prev1, bx, by - 1))
        if bx + 1 < b_w:
            p1.append(rel(prev1, bx + 1, by))
        if by + 1 < b_h:
            p1.append(rel(prev1, bx, by + 1))

    b = Block(A, B, width, height, mb, R, x_mb, y_mb, median)      # pred is fixed before the first cost
    for vx, vy in [median] + p0 + p1:
        b.cost_p_mv(x_mb + vx, y_mb + vy)

    if method == EPZS:
        while True:
            x, y = b.mv
            for dx, dy in DIA1:
                b.cost_p_mv(x + dx, y + dy)
            if b.mv == (x, y):
                break
        return b.mv[0], b.mv[1], b.cost_min, b.ncost

    x, y = b.mv
    for d in range(1, R + 1, 2):
        b.cost_p_mv(x - d, y)
        b.cost_p_mv(x + d, y)
        if d <= R // 2:
            b.cost_p_mv(x, y - d)
            b.cost_p_mv(x, y + d)
    cx, cy = b.mv
    for y in range(max(b.y_min, cy - 2), min(cy + 2, b.y_max) + 1):
        for x in range(max(b.x_min, cx - 2), min(cx + 2, b.x_max) + 1):
            b.cost_mv(x, y)
    x, y = b.mv
    for d in range(1, R // 4 + 1):
        for dx, dy in HEX4[1:]:
            b.cost_p_mv(x + dx * d, y + dy * d)
    while True:
        x, y = b.mv
        for dx, dy in HEX2:
            b.cost_p_mv(x + dx, y + dy)
        if b.mv == (x, y):
            break
    for dx, dy in DIA1:
        b.cost_p_mv(x + dx, y + dy)
    return b.mv[0], b.mv[1], b.cost_min, b.ncost


def frames(method, A, B, width, height, mb, R, prev1=None, prev2=None):
    """A, B: (nframes, height, stride) uint8; prev1, prev2: int16 (nframes, b_h * b_w * 2) or None.  The blocks of a pair in raster
    order.  -> mv int16 (nframes, b_h * b_w * 2), cost uint32 (nframes, b_h * b_w), the costs evaluated"""
    log2mb = {16: 4, 8: 3}[mb]
    b_w, b_h = width >> log2mb, height >> log2mb
    nf = A.shape[0]
    mv = np.zeros((nf, b_h * b_w * 2), np.int16)
    cost_out = np.zeros((nf, b_h * b_w), np.uint32)
    n = 0
    for f in range(nf):
        field = mv[f].reshape(b_h, b_w, 2)
        q1 = None if prev1 is None else prev1[f].reshape(b_h, b_w, 2)
        q2 = None if prev2 is None else prev2[f].reshape(b_h, b_w, 2)
        for by in range(b_h):
            for bx in range(b_w):
                x, y, c, k = search(method, A[f], B[f], width, height, mb, R, bx, by, field, q1, q2)
                field[by, bx] = (x, y)
                cost_out[f, by * b_w + bx] = c
                n += k
    return mv, cost_out, n


def sequence(method, pics, width, height, mb, R, init1=None, init2=None):
    """THE DEFINITION of the sequence face: the loop of pair calls.  pics: (nseq, nframes, height, stride); init1, init2: (nseq, b * 2)
    or None.  -> mv (np, nseq, b * 2), cost (np, nseq, b), costs evaluated"""
    outs, n = [], 0
    for k in range(pics.shape[1] - 1):
        prev1 = outs[k - 1][0] if k >= 1 else init1
        prev2 = outs[k - 2][0] if k >= 2 else (init1 if k == 1 else init2)
        m, c, i = frames(method, np.ascontiguousarray(pics[:, k]), np.ascontiguousarray(pics[:, k + 1]), width, height, mb, R, prev1, prev2)
        outs.append((m, c))
        n += i
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs]), n


# ---- the bilateral compensation (ffhip_me_interp_bilat_sequence_dev), from the rule text of include/ffhip.h ----------------------------
# A scatter into explicit per-pixel lists, block by block, as tests/me_interp_model.py is; what the text takes over from the existing
# interpolation rule "from its step 5 on" — the two entries, the fallback, the averages, the blend — is that model's code.
def scatter_bilat(W, H, mb, mv_range, alpha, window, field, counts):
    """bilateral_obmc() for every block in raster order: lists[y][x] = [(ref, weight, dx, dy), ...], two entries per contribution"""
    import me_interp_model as I
    log2mb = {16: 4, 8: 3}[mb]
    b_w, b_h = W >> log2mb, H >> log2mb
    h = mb // 2
    lists = [[[] for _ in range(W)] for _ in range(H)]
    for by in range(b_h):
        for bx in range(b_w):
            vx = int(field[by][bx][0]) - (bx << log2mb)
            vy = int(field[by][bx][1]) - (by << log2mb)
            if abs(vx) > mv_range or abs(vy) > mv_range:
                counts["malformed"] += 1
                continue
            sx, sy = (bx << log2mb) - h, (by << log2mb) - h         # the vector does not shift the window
            x0, x1 = clip(sx, 0, W - 1), clip(sx + 2 * mb, 0, W - 1)
            y0, y1 = clip(sy, 0, H - 1), clip(sy + 2 * mb, 0, H - 1)
            mx, my = 2 * vx, 2 * vy
            ax, ay = I.tdiv(mx * alpha), I.tdiv(my * alpha)
            ex, ey = I.tdiv(-mx * (1024 - alpha)), I.tdiv(-my * (1024 - alpha))
            for y in range(y0, y1):
                for x in range(x0, x1):
                    w = int(window[(x - sx) + (y - sy) * 2 * mb])
                    if w == 0:
                        counts["zero_weight"] += 1
                        continue
                    pm = lists[y][x]
                    if len(pm) + 1 >= I.NB_PIXEL_MVS:
                        counts["capped"] += 1          # never: at most four blocks reach a pixel
                        continue
                    counts["taken"] += 1
                    for ref, weight, dx, dy in ((0, w * (1024 - alpha), ax, ay), (1, w * alpha, ex, ey)):
                        cx, cy = clip(dx, -x, W - 1 - x), clip(dy, -y, H - 1 - y)
                        counts["clipped"] += (cx, cy) != (dx, dy)
                        pm.append((ref, weight, cx, cy))
            # every list is at most four contributions long
    assert max(len(p) for row in lists for p in row) <= 8
    return lists


def interp_bilat_sequence(pics, W, H, sw, sh, mb, mv_range, window, mv, jobs, scene=None, scene_action=1):
    """pics[s][p] = a picture's planes; mv[k][s] = the field of pair k of sequence s; jobs = (seq, pair, alpha, mode); scene[k][s]: a
    flagged pair's MCI jobs run scene_action (1: the blend, 2: picture A when alpha <= 512, else B).  -> ([job j's planes], counts)"""
    import me_interp_model as I
    counts = I.new_counts()
    out = []
    for seq, pair, alpha, mode in jobs:
        A, B = pics[seq][pair], pics[seq][pair + 1]
        cut = mode == I.MCI and scene is not None and scene[pair][seq]
        if mode == I.BLEND or cut:
            a = alpha if not (cut and scene_action == 2) else (0 if alpha <= 512 else 1024)
            out.append(I.blend(A, B, a, counts))
            continue
        lists = scatter_bilat(W, H, mb, mv_range, alpha, window, mv[pair][seq], counts)
        out.append(I.frame_data(A, B, W, H, sw, sh, alpha, lists, counts))
    return out, counts
