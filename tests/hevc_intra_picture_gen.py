"""Synthetic HEVC pictures for the intra reconstruction wavefront (ffhip_hevc_intra_pictures_dev) and a sequential model of it.

The generator builds a picture the way a decoder meets it when the intra stage runs: random CTB quadtrees (CUs of 8 to 64 luma
samples, NxN 4x4 luma PUs at 8x8, transform trees split down to 4x4 with a largest TB of 32), intra and inter CUs mixed (the inter
ones already reconstructed: random samples), the chroma transform-block rules of every chroma format (4:2:0 / 4:2:2 chroma 4x4 after
the fourth luma 4x4, 4:2:2 chroma as square pairs, 4:4:4 like luma), random modes with and without residuals, slices, tiles and
constrained_intra_pred_flag.  The intra areas start as random garbage, which a correct reconstruction never reads.

Availability masks come from a decoding-order index per 4x4 luma block (6.4.1 z-scan availability: CTBs in tile-scan order, z-order
inside), the slice and tile of each CTB and, under constrained intra prediction, the prediction mode of the neighbour — not from
"the sample is in the plane": inter samples later in decoding order are in the plane and must be substituted.

The model reconstructs the records one by one in decoding order with hevc_pred_ref's substitution, filtering and prediction, adds the
residuals and clips."""
import numpy as np

import hevc_pred_ref as R

FLAG_CORNER, FLAG_STRONG, FLAG_NO_SMOOTH, FLAG_CHROMA444 = 2, 4, 8, 16   # FFHIP_HEVC_INTRA_* (include/ffhip.h)
TU_FIELDS = ("x", "y", "res_offset", "avail_left", "avail_top", "log2_size", "mode", "flags", "c_idx_unit")


def _zorder(n):
    """z-scan index of each cell of an n x n grid (n a power of two), [y, x]"""
    z = np.zeros((n, n), np.int64)
    for y in range(n):
        for x in range(n):
            v = 0
            for b in range(n.bit_length()):
                v |= ((x >> b) & 1) << (2 * b) | ((y >> b) & 1) << (2 * b + 1)
            z[y, x] = v
    return z


def _bounds(n, k, rng):
    """k sorted parts of range(n): their start indices"""
    if k <= 1 or n < 2:
        return [0]
    return [0] + sorted(rng.choice(np.arange(1, n), min(k, n) - 1, replace=False).tolist())


class Picture:
    """One generated picture.  planes[p]: the plane at launch (int64, [h, w]); recs[p]: its records in decoding order, each a dict
    with the FFHipHevcIntraTU fields plus 'ctb' (raster CTB address) and 'order' (decoding-order index of the block's position);
    res[p]: the plane's int16 residuals."""

    def __init__(self, rng, width, height, log2_ctb, bd, cfi, p_intra=1.0, tiles=(1, 1), slices=1, cip=False, strong=None,
                 no_smooth=None, p_res=0.5, modes=None, p_nxn=0.3, inter_rows=()):
        assert width % 8 == 0 and height % 8 == 0
        self.rng, self.W, self.H, self.log2_ctb, self.bd, self.cfi, self.cip = rng, width, height, log2_ctb, bd, cfi, cip
        self.C = C = 1 << log2_ctb
        self.ctb_w, self.ctb_h = (width + C - 1) // C, (height + C - 1) // C
        self.nplanes = 3 if cfi else 1
        self.hs = [0] + [int(cfi in (1, 2))] * 2
        self.vs = [0] + [int(cfi == 1)] * 2
        self.strong = bool(rng.integers(2)) if strong is None else strong
        self.no_smooth = bool(rng.integers(4) == 0) if no_smooth is None else no_smooth
        self.modes = modes
        self.inter_rows = frozenset(inter_rows)                    # CTB rows whose CUs are all inter: rows without a record
        mx = (1 << bd) - 1

        # ---- tiles, tile-scan order, slices ----
        cols, rows = _bounds(self.ctb_w, tiles[0], rng), _bounds(self.ctb_h, tiles[1], rng)
        self.tile = np.zeros((self.ctb_h, self.ctb_w), np.int64)
        ts_list = []
        ce, re_ = cols + [self.ctb_w], rows + [self.ctb_h]
        for ti in range(len(rows)):
            for tj in range(len(cols)):
                self.tile[re_[ti]:re_[ti + 1], ce[tj]:ce[tj + 1]] = ti * len(cols) + tj
                for y in range(re_[ti], re_[ti + 1]):
                    for x in range(ce[tj], ce[tj + 1]):
                        ts_list.append(y * self.ctb_w + x)
        self.ts_order = ts_list                                  # raster CTB addresses in decoding order
        nctb = self.ctb_w * self.ctb_h
        starts = set(_bounds(nctb, slices, rng))
        self.slice = np.zeros(nctb, np.int64)
        s = -1
        for ts, a in enumerate(ts_list):
            s += ts in starts
            self.slice[a] = s

        # ---- decoding-order index per 4x4 luma block ----
        g = C // 4
        z = _zorder(g)
        H4, W4 = self.ctb_h * g, self.ctb_w * g
        self.order = np.zeros((H4, W4), np.int64)
        for ts, a in enumerate(ts_list):
            cy, cx = divmod(a, self.ctb_w)
            self.order[cy * g:(cy + 1) * g, cx * g:(cx + 1) * g] = ts * g * g + z
        self.intra = np.zeros((H4, W4), bool)

        # ---- planes at launch: garbage everywhere, inter CUs overwrite theirs ----
        self.planes = []
        for p in range(self.nplanes):
            self.planes.append(rng.integers(0, mx + 1, (height >> self.vs[p], width >> self.hs[p])).astype(np.int64))

        # ---- the CU trees, in decoding order ----
        self.p_intra, self.p_res, self.p_nxn = p_intra, p_res, p_nxn
        self.tu_list = []                                          # (plane, x, y, log2, mode, has_res) in decoding order per plane
        for a in ts_list:
            cy, cx = divmod(a, self.ctb_w)
            self._cu_tree(a, cx * C, cy * C, log2_ctb)
        self._make_records()

    # ---- coding quadtree ----
    def _cu_tree(self, a, x, y, log2):
        if x >= self.W or y >= self.H:
            return
        s = 1 << log2
        split = log2 > 3 and (x + s > self.W or y + s > self.H or self.rng.random() < 0.5)
        if split:
            h = s // 2
            for dy in (0, h):
                for dx in (0, h):
                    self._cu_tree(a, x + dx, y + dy, log2 - 1)
            return
        if (y >> self.log2_ctb) in self.inter_rows or self.rng.random() >= self.p_intra:
            self.intra[y >> 2:(y + s) >> 2, x >> 2:(x + s) >> 2] = False
            for p in range(self.nplanes):   # already reconstructed by MC and the residual add
                hs, vs = self.hs[p], self.vs[p]
                self.planes[p][y >> vs:(y + s) >> vs, x >> hs:(x + s) >> hs] = self.rng.integers(0, 1 << self.bd, (s >> vs, s >> hs))
            return
        self.intra[y >> 2:(y + s) >> 2, x >> 2:(x + s) >> 2] = True
        nxn = log2 == 3 and self.rng.random() < self.p_nxn
        lmodes = [self._mode() for _ in range(4 if nxn else 1)]
        cmodes = [self._mode() for _ in range(4 if nxn and self.cfi == 3 else 1)]
        self._tu_tree(a, x, y, x, y, log2, 0, 0, nxn, lmodes, cmodes, x, y, log2)

    def _mode(self):
        if self.modes is not None:
            return int(self.rng.choice(self.modes))
        r = self.rng.random()
        return int(self.rng.choice([0, 1, 10, 26])) if r < 0.4 else int(self.rng.integers(0, 35))

    # ---- transform tree ----
    def _tu_tree(self, a, x, y, xb, yb, log2, depth, blk, nxn, lmodes, cmodes, cux, cuy, cu_log2):
        split = log2 > 5 or (nxn and depth == 0) or (log2 > 2 and self.rng.random() < 0.4)
        if split:
            h = 1 << (log2 - 1)
            for i, (dy, dx) in enumerate(((0, 0), (0, h), (h, 0), (h, h))):
                self._tu_tree(a, x + dx, y + dy, x, y, log2 - 1, depth + 1, i, nxn, lmodes, cmodes, cux, cuy, cu_log2)
            return
        q = 0
        if nxn:   # the PU (quadrant of the 8x8 CU) this TB lies in
            q = ((y - cuy) >= 4) * 2 + ((x - cux) >= 4)
        self.tu_list.append((a, 0, x, y, log2, lmodes[q]))
        if not self.cfi:
            return
        cm = cmodes[q if len(cmodes) == 4 else 0]
        if self.cfi == 3:
            for p in (1, 2):
                self.tu_list.append((a, p, x, y, log2, cm))
        elif log2 > 2:
            for p in (1, 2):
                self._chroma(a, p, x, y, log2 - 1, cm)
        elif blk == 3:   # 4x4 luma: the chroma of the parent 8x8 after its fourth block
            for p in (1, 2):
                self._chroma(a, p, xb, yb, 2, cm)

    def _chroma(self, a, p, xl, yl, log2c, mode):
        """chroma blocks of log2c at the luma position (xl, yl), 4:2:0 or 4:2:2 (two square blocks, the top one first)"""
        xc, yc = xl >> 1, yl >> self.vs[p]
        self.tu_list.append((a, p, xc, yc, log2c, mode))
        if self.cfi == 2:
            self.tu_list.append((a, p, xc, yc + (1 << log2c), log2c, mode))

    # ---- availability and records ----
    def available(self, xc, yc, xn, yn):
        """6.4.1 + 8.4.4.2.2 for the luma positions of the current block (xc, yc) and a neighbouring sample (xn, yn)"""
        if xn < 0 or yn < 0 or xn >= self.W or yn >= self.H:
            return False
        if self.order[yn >> 2, xn >> 2] >= self.order[yc >> 2, xc >> 2]:
            return False
        C = self.log2_ctb
        an, ac = (yn >> C) * self.ctb_w + (xn >> C), (yc >> C) * self.ctb_w + (xc >> C)
        if self.slice[an] != self.slice[ac] or self.tile.flat[an] != self.tile.flat[ac]:
            return False
        return not self.cip or bool(self.intra[yn >> 2, xn >> 2])

    def masks(self, p, x0, y0, N):
        hs, vs = self.hs[p], self.vs[p]
        luh, luv = 2 - hs, 2 - vs
        uh, uv = 1 << luh, 1 << luv
        xc, yc = x0 << hs, y0 << vs
        al = sum(1 << i for i in range((2 * N) >> luv) if self.available(xc, yc, (x0 - 1) << hs, (y0 + i * uv) << vs))
        at = sum(1 << j for j in range((2 * N) >> luh) if self.available(xc, yc, (x0 + j * uh) << hs, (y0 - 1) << vs))
        corner = self.available(xc, yc, (x0 - 1) << hs, (y0 - 1) << vs)
        return al, at, corner, luh, luv

    def _make_records(self):
        self.recs = [[] for _ in range(self.nplanes)]
        res = [[] for _ in range(self.nplanes)]
        nres = [0] * self.nplanes
        base_flags = (FLAG_STRONG if self.strong else 0) | (FLAG_NO_SMOOTH if self.no_smooth else 0) | (FLAG_CHROMA444 if self.cfi == 3 else 0)
        for a, p, x, y, log2, mode in self.tu_list:
            N = 1 << log2
            al, at, corner, luh, luv = self.masks(p, x, y, N)
            off = -1
            if self.rng.random() < self.p_res:
                amp = (1 << self.bd) if self.rng.random() < 0.2 else (1 << (self.bd - 3))
                res[p].append(self.rng.integers(-amp, amp + 1, N * N).astype(np.int16))
                off = nres[p]
                nres[p] += N * N
            self.recs[p].append(dict(x=x, y=y, res_offset=off, avail_left=al, avail_top=at, log2_size=log2, mode=mode,
                                     flags=base_flags | (FLAG_CORNER if corner else 0), c_idx_unit=p | luh << 2 | luv << 4, ctb=a,
                                     order=int(self.order[(y << self.vs[p]) >> 2, (x << self.hs[p]) >> 2])))
        self.res = [np.concatenate(r) if r else np.zeros(16, np.int16) for r in res]

    # ---- what the device face takes ----
    def pack(self, p, recs=None, dtype=None):
        """(records sorted by raster CTB as a structured array, int32 CTB starts) of plane p; recs: another record list (dicts)"""
        recs = self.recs[p] if recs is None else recs
        nctb = self.ctb_w * self.ctb_h
        idx = sorted(range(len(recs)), key=lambda i: recs[i]["ctb"])        # stable: decoding order inside a CTB is kept
        arr = np.zeros(len(recs), dtype)
        for j, i in enumerate(idx):
            arr[j] = tuple(recs[i][f] for f in TU_FIELDS)
        counts = np.bincount(np.array([recs[i]["ctb"] for i in idx], np.int64), minlength=nctb) if recs else np.zeros(nctb, np.int64)
        starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        return arr, starts


def model(pic, recs=None):
    """the picture's planes after intra reconstruction: records in decoding order (CTBs in tile-scan order), each predicted from the
    planes as reconstructed so far (hevc_pred_ref), plus its residual, clipped"""
    out = [pl.copy() for pl in pic.planes]
    mx = (1 << pic.bd) - 1
    for p in range(pic.nplanes):
        rl = pic.recs[p] if recs is None else recs[p]
        rank = {a: i for i, a in enumerate(pic.ts_order)}
        for r in sorted(rl, key=lambda r: rank[r["ctb"]]):       # stable: the order inside a CTB is the record order
            reconstruct(out[p], r, pic.res[p], pic.bd)
    for p in range(pic.nplanes):
        assert out[p].min() >= 0 and out[p].max() <= mx
    return out


def gather_line(plane, x0, y0, N):
    """the raw reference line of a block: 4N + 1 samples bottom-left to top-right; samples outside the plane read 0"""
    h, w = plane.shape
    line = np.zeros(4 * N + 1, np.int64)
    ys = y0 + np.arange(2 * N)
    ok = (ys < h) & (x0 >= 1)
    left = np.zeros(2 * N, np.int64)
    left[ok] = plane[ys[ok], x0 - 1]
    xs = x0 + np.arange(2 * N)
    ok = (xs < w) & (y0 >= 1)
    top = np.zeros(2 * N, np.int64)
    top[ok] = plane[y0 - 1, xs[ok]]
    corner = plane[y0 - 1, x0 - 1] if x0 >= 1 and y0 >= 1 else 0
    line[:2 * N] = left[::-1]
    line[2 * N] = corner
    line[2 * N + 1:] = top
    return line


def reconstruct(plane, r, res, bd):
    """one record, in place"""
    N = 1 << r["log2_size"]
    x0, y0, cu = r["x"], r["y"], r["c_idx_unit"]
    c_idx, luh, luv = cu & 3, (cu >> 2) & 3, (cu >> 4) & 3
    avail = R.availability(N, r["avail_left"], r["avail_top"], r["flags"] & FLAG_CORNER, luh, luv)
    line = R.substitute(gather_line(plane, x0, y0, N), avail, bd)
    line = R.filter_line(line, N, r["mode"], c_idx, bd, strong=bool(r["flags"] & FLAG_STRONG),
                         smoothing_disabled=bool(r["flags"] & FLAG_NO_SMOOTH), chroma444=bool(r["flags"] & FLAG_CHROMA444))
    pred = R.predict(line, N, r["mode"], c_idx, bd)
    if r["res_offset"] >= 0:
        pred = pred + res[r["res_offset"]:r["res_offset"] + N * N].astype(np.int64).reshape(N, N)
    plane[y0:y0 + N, x0:x0 + N] = np.clip(pred, 0, (1 << bd) - 1)
