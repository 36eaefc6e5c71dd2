"""Synthetic VP9 inter frames for the inter reconstruction face (ffhip_vp9_inter_frames_dev) and a sequential model of it.

The generator builds what a decoder holds when the inter stage runs: 1..3 random references of the frame's size; a random superblock
partition down to 4x4 (forced splits at the frame's edges as the decoder's, so blocks may overhang the decoded area); intra holes;
inter blocks with every filter, single or compound references and MVs mostly small, some far past every edge; skip, or TUs of every
size the block allows (the lossless WHT in lossless frames) that start inside the decoded area, as inter_recon's loops give them.
Frame sizes need not be multiples of 8 or 64.  The planes start as random garbage: what no prediction covers must survive.

The model runs each prediction record in decoding order by gathering its reference window with clamped coordinates (what
emulated_edge_mc gives mc_luma_unscaled / mc_chroma_unscaled) and calling the oracle's pinned ffo_vp9_mc_bd (put, then avg), then the
TUs through ffo_vp9_itxfm_add_bd (ffo_vp9_itxfm_add at 8 bits) in inter_recon's order, on the covered samples, clipped to the decoded
area.  route="pad" is the second path: the oracle's MC straight on references padded with np.pad(mode="edge") (the batch faces'
route; valid while no window leaves the border)."""
import ctypes as C

import numpy as np

import ffi

#: enum BlockSize: (w, h) in luma samples, BS_64x64 .. BS_4x4
BS_DIMS = [(64, 64), (64, 32), (32, 64), (32, 32), (32, 16), (16, 32), (16, 16), (16, 8), (8, 16), (8, 8), (8, 4), (4, 8), (4, 4)]
BS_OF = {d: i for i, d in enumerate(BS_DIMS)}
PRED_FIELDS = ("x", "y", "w", "h", "filter", "flags", "ref", "mv")
TU_FIELDS = ("x", "y", "coeff_offset", "tx", "txtp", "dc_only")
BORDER = 96


def rounded_div(a, b):
    """ROUNDED_DIV: half away from zero, then C division (towards zero)"""
    n = a + (b >> 1) if a >= 0 else a - (b >> 1)
    q = abs(n) // b
    return q if n >= 0 else -q


def _div2(a, b):
    return [rounded_div(a[0] + b[0], 2), rounded_div(a[1] + b[1], 2)]


def _div4(a, b, c, d):
    return [rounded_div(a[0] + b[0] + c[0] + d[0], 4), rounded_div(a[1] + b[1] + c[1] + d[1], 4)]


def block_preds(bs, row, col, mv, comp, ref, filt, ss_h, ss_v):
    """a restatement of vp9_mc_template.h's calls for one block: a list of record dicts (PRED_FIELDS); mv = [sub][ref][x, y]"""
    out = []
    nr = 2 if comp else 1

    def emit(chroma, x, y, w, h, pick):
        mvs = [[0, 0], [0, 0]]
        refs = [0, 0]
        for r in range(nr):
            mvs[r] = [int(v) for v in pick(r)]
            refs[r] = int(ref[r])
        out.append(dict(x=x, y=y, w=w, h=h, filter=filt, flags=(1 if comp else 0) | (2 if chroma else 0), ref=refs, mv=mvs))

    sub = lambda s: (lambda r: mv[s][r])
    d2 = lambda a, b: (lambda r: _div2(mv[a][r], mv[b][r]))
    ly, lx, cy, cx = row << 3, col << 3, row << (3 - ss_v), col << (3 - ss_h)
    if bs < 10:
        w, h = BS_DIMS[bs]
        emit(False, lx, ly, w, h, sub(0))
        emit(True, cx, cy, w >> ss_h, h >> ss_v, sub(0))
    elif bs == 10:                                   # 8x4
        emit(False, lx, ly, 8, 4, sub(0))
        emit(False, lx, ly + 4, 8, 4, sub(2))
        if ss_v:
            emit(True, cx, row << 2, 8 >> ss_h, 4, d2(0, 2))
        else:
            emit(True, cx, ly, 8 >> ss_h, 4, sub(0))
            emit(True, cx, ly + 4, 8 >> ss_h, 4, d2(0, 2) if ss_h else sub(2))
    elif bs == 11:                                   # 4x8
        emit(False, lx, ly, 4, 8, sub(0))
        emit(False, lx + 4, ly, 4, 8, sub(1))
        if ss_h:
            emit(True, col << 2, cy, 4, 8 >> ss_v, d2(0, 1))
        else:
            emit(True, lx, cy, 4, 8 >> ss_v, sub(0))
            emit(True, lx + 4, cy, 4, 8 >> ss_v, sub(1))
    else:                                            # 4x4
        for s, (dx, dy) in enumerate(((0, 0), (4, 0), (0, 4), (4, 4))):
            emit(False, lx + dx, ly + dy, 4, 4, sub(s))
        if ss_h and ss_v:
            emit(True, col << 2, row << 2, 4, 4, lambda r: _div4(mv[0][r], mv[1][r], mv[2][r], mv[3][r]))
        elif ss_v:
            emit(True, lx, row << 2, 4, 4, d2(0, 2))
            emit(True, lx + 4, row << 2, 4, 4, d2(1, 3))
        elif ss_h:
            emit(True, col << 2, ly, 4, 4, d2(0, 1))
            emit(True, col << 2, ly + 4, 4, 4, d2(1, 2))
        else:
            for s, (dx, dy) in enumerate(((0, 0), (4, 0), (0, 4), (4, 4))):
                emit(True, lx + dx, ly + dy, 4, 4, sub(s))
    return out


class InterFrame:
    """One generated frame.  refs[r][p]: reference planes of the real size (int64); planes[p]: the destination planes (decoded area) at
    launch; preds: record dicts in decoding order (plus 'sb'); tus[p]: TU dicts (plus 'sb'); coeffs[p]: int32 coefficients; blocks:
    (bs, row, col, kind) per block, kind 'inter' / 'intra'."""

    def __init__(self, rng, width, height, bd, ss_h, ss_v, nrefs=None, refs=None, p_intra=0.15, p_skip=0.25, p_comp=0.35, p_far=0.04,
                 p_edge=0.08, lossless=False, min_log2=2, smooth=False, mv_range=64, p_txtp=0.15):
        self.rng, self.W, self.H, self.bd, self.ss_h, self.ss_v = rng, width, height, bd, ss_h, ss_v
        self.cols, self.rows = (width + 7) >> 3, (height + 7) >> 3
        self.sb_w, self.sb_h = (self.cols + 7) >> 3, (self.rows + 7) >> 3
        self.hs, self.vs = [0, ss_h, ss_h], [0, ss_v, ss_v]
        self.maxv = (1 << bd) - 1
        self.dw = [(self.cols * 8) >> s for s in self.hs]
        self.dh = [(self.rows * 8) >> s for s in self.vs]
        self.rw = [(width + s) >> s for s in self.hs]
        self.rh = [(height + s) >> s for s in self.vs]
        self.p_intra, self.p_skip, self.p_comp, self.p_far, self.p_edge = p_intra, p_skip, p_comp, p_far, p_edge
        self.lossless, self.min_log2, self.smooth, self.mv_range, self.p_txtp = lossless, min_log2, smooth, mv_range, p_txtp
        if refs is None:
            n = int(rng.integers(1, 4)) if nrefs is None else nrefs
            refs = [[self._content((self.rh[p], self.rw[p])) for p in range(3)] for _ in range(n)]
        self.refs = refs
        self.nrefs = len(refs)
        self.planes = [rng.integers(0, self.maxv + 1, (self.dh[p], self.dw[p])).astype(np.int64) for p in range(3)]
        self.field = rng.integers(-40, 41, (self.sb_h + 1, self.sb_w + 1, 2))
        self.preds, self.tus, self.blocks = [], [[], [], []], []
        self._co = [[], [], []]
        self._nco = [0, 0, 0]
        for sy in range(self.sb_h):
            for sx in range(self.sb_w):
                self._part(sy * self.sb_w + sx, sy * 8, sx * 8, 3)
        self.coeffs = [np.concatenate(c).astype(np.int32) if c else np.zeros(16, np.int32) for c in self._co]

    def _content(self, shape):
        """a reference plane: smooth gradients plus noise, with some extreme samples"""
        h, w = shape
        yy, xx = np.mgrid[0:h, 0:w]
        f = self.rng.uniform(0.01, 0.3, 2)
        a = (np.sin(xx * f[0]) + np.cos(yy * f[1]) + 2) / 4 * self.maxv + self.rng.normal(0, self.maxv / 12, shape)
        a[self.rng.random(shape) < 0.02] = self.maxv
        a[self.rng.random(shape) < 0.02] = 0
        return np.clip(np.rint(a), 0, self.maxv).astype(np.int64)

    # ---- partition (decode_sb: a half outside the frame forces the split) ----
    def _part(self, sb, row, col, lvl):
        """lvl 3: 64x64 .. 0: 8x8; row / col in 8-sample units"""
        if row >= self.rows or col >= self.cols:
            return
        n = 1 << lvl
        hb = n >> 1
        rng = self.rng
        if lvl == 0:
            kind = rng.choice(["none", "h", "v", "split"]) if self.min_log2 <= 2 else "none"
            self._block(sb, {"none": 9, "h": 10, "v": 11, "split": 12}[str(kind)], row, col)
            return
        below, right = row + hb >= self.rows, col + hb >= self.cols
        if below and right:
            kind = "split"
        elif below:
            kind = rng.choice(["h", "split"])
        elif right:
            kind = rng.choice(["v", "split"])
        else:
            big = 2 + lvl >= self.min_log2
            kind = rng.choice(["none", "h", "v", "split"], p=[0.3, 0.15, 0.15, 0.4]) if big else "none"
        s = 8 * n
        if kind == "none":
            self._block(sb, BS_OF[(s, s)], row, col)
        elif kind == "h":
            self._block(sb, BS_OF[(s, s // 2)], row, col)
            if not below:
                self._block(sb, BS_OF[(s, s // 2)], row + hb, col)
        elif kind == "v":
            self._block(sb, BS_OF[(s // 2, s)], row, col)
            if not right:
                self._block(sb, BS_OF[(s // 2, s)], row, col + hb)
        else:
            for dr, dc in ((0, 0), (0, hb), (hb, 0), (hb, hb)):
                self._part(sb, row + dr, col + dc, lvl - 1)

    def _mv(self, row, col, w, h):
        rng = self.rng
        if self.smooth:
            f = self.field[row >> 3, col >> 3]
            return [int(f[0] + rng.integers(-3, 4)), int(f[1] + rng.integers(-3, 4))]
        r = rng.random()
        if r < self.p_far:                              # anywhere in int16: far past every edge
            return [int(v) for v in rng.integers(-32768, 32768, 2)]
        if r < self.p_far + self.p_edge:                # just across an edge of the frame
            x, y = col * 8, row * 8
            return [int(((rng.integers(-40, 8) - x) if rng.random() < 0.5 else (self.W - x - w + rng.integers(-8, 40))) * 8
                        + rng.integers(0, 8)),
                    int(((rng.integers(-40, 8) - y) if rng.random() < 0.5 else (self.H - y - h + rng.integers(-8, 40))) * 8
                        + rng.integers(0, 8))]
        return [int(v) for v in rng.integers(-self.mv_range, self.mv_range + 1, 2)]

    def _block(self, sb, bs, row, col):
        rng = self.rng
        w, h = BS_DIMS[bs]
        if rng.random() < self.p_intra:
            self.blocks.append((bs, row, col, "intra"))
            return
        self.blocks.append((bs, row, col, "inter"))
        comp = rng.random() < self.p_comp
        ref = [int(rng.integers(0, self.nrefs)), int(rng.integers(0, self.nrefs))] if comp else [int(rng.integers(0, self.nrefs)), 0]
        filt = int(rng.integers(0, 4))
        mv = [[self._mv(row, col, w, h), self._mv(row, col, w, h)] for _ in range(4)]
        mv = [[[int(np.clip(v, -32768, 32767)) for v in m] for m in s] for s in mv]
        if bs < 10:
            mv = [mv[0]] * 4                             # >= 8x8: one vector (the decoder copies it to every sub-block)
        for rec in block_preds(bs, row, col, mv, comp, ref, filt, self.ss_h, self.ss_v):
            rec["sb"] = sb
            self.preds.append(rec)
        if rng.random() < self.p_skip:
            return
        self._tus(sb, bs, row, col)

    # ---- inter_recon's transform loops ----
    def _tus(self, sb, bs, row, col):
        rng = self.rng
        w, h = BS_DIMS[bs]
        w8, h8 = max(w, 8), max(h, 8)                    # sub-8x8 blocks occupy an 8x8 area
        maxtx = min(3, int(np.log2(min(w, h))) - 2)
        tx = 0 if self.lossless else int(rng.integers(0, maxtx + 1))
        uvw, uvh = max(4, w8 >> self.ss_h), max(4, h8 >> self.ss_v)
        uvtx = 0 if self.lossless else min(tx, int(np.log2(min(uvw, uvh))) - 2)
        end_x, end_y = min(2 * (self.cols - col), w8 // 4), min(2 * (self.rows - row), h8 // 4)   # 4-sample units
        for p in range(3):
            t = tx if p == 0 else uvtx
            ex, ey = (end_x, end_y) if p == 0 else (end_x >> self.ss_h, end_y >> self.ss_v)
            step = 1 << t
            x0, y0 = (col * 8) >> self.hs[p], (row * 8) >> self.vs[p]
            for yy in range(0, ey, step):
                for xx in range(0, ex, step):
                    self._tu(sb, p, x0 + 4 * xx, y0 + 4 * yy, t)

    def _tu(self, sb, p, x, y, t):
        rng = self.rng
        r = rng.random()
        if r < 0.2:
            return                                       # eob 0: no call
        N = 4 << t
        dc = r < 0.4
        co = np.zeros(N * N, np.int64)
        if dc:
            co[0] = rng.integers(-(1 << (self.bd + 2)), 1 << (self.bd + 2))
        else:
            k = int(rng.integers(1, min(N * N, 40) + 1))
            amp = 1 << (self.bd + (3 if rng.random() < 0.2 else 0))
            pos = rng.integers(0, min(N * N, 64), k)
            co[pos] = rng.integers(-amp, amp + 1, k)
        lim = 32767 if self.bd == 8 else (1 << 20)
        self._co[p].append(np.clip(co, -lim, lim))
        txtp = 0 if (self.lossless or rng.random() >= self.p_txtp) else int(rng.integers(1, 4))
        self.tus[p].append(dict(x=x, y=y, coeff_offset=self._nco[p], tx=4 if self.lossless else t, txtp=txtp, dc_only=int(dc), sb=sb))
        self._nco[p] += N * N

    # ---- what the device face takes ----
    def pack(self, recs, dtype, fields):
        """(records sorted by raster superblock as a structured array, int32 superblock starts)"""
        nsb = self.sb_w * self.sb_h
        idx = sorted(range(len(recs)), key=lambda i: recs[i]["sb"])
        arr = np.zeros(len(recs), dtype)
        for j, i in enumerate(idx):
            for f in fields:
                arr[j][f] = recs[i][f]
        counts = np.bincount(np.array([recs[i]["sb"] for i in idx], np.int64), minlength=nsb) if recs else np.zeros(nsb, np.int64)
        return arr, np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)

    def coeff_array(self, p):
        return self.coeffs[p].astype(np.int16 if self.bd == 8 else np.int32)


# ---- the model ----
_O = None


def _oracle():
    global _O
    if _O is None:
        _O = ffi.oracle()
    return _O


def rec_geometry(fr, rec, p, r):
    """(x', y', mx, my) of record `rec` in plane p for its reference r: the integer origin and the phases in sixteenths"""
    mvx, mvy = rec["mv"][r]
    if p == 0:
        return rec["x"] + (mvx >> 3), rec["y"] + (mvy >> 3), (mvx & 7) << 1, (mvy & 7) << 1
    mx, my = mvx * (1 << (1 - fr.ss_h)), mvy * (1 << (1 - fr.ss_v))
    return rec["x"] + (mx >> 4), rec["y"] + (my >> 4), mx & 15, my & 15


def window(ref, xi, yi, w, h):
    """reference samples rows yi - 3 .. yi + h + 4, columns xi - 3 .. xi + w + 4, coordinates clamped to the plane"""
    H, W = ref.shape
    ys = np.clip(np.arange(yi - 3, yi + h + 5), 0, H - 1)
    xs = np.clip(np.arange(xi - 3, xi + w + 5), 0, W - 1)
    return ref[np.ix_(ys, xs)]


_PADDED = {}


def padded(ref, dt):
    """the reference plane with a BORDER-sample edge-replicated border, as samples of type dt (cached per plane)"""
    key = (id(ref), dt)
    if key not in _PADDED or _PADDED[key][0] is not ref:
        _PADDED[key] = (ref, np.ascontiguousarray(np.pad(ref, BORDER, mode="edge").astype(dt)))
    return _PADDED[key][1]


def predict(fr, rec, p, route="clamp", refs=None):
    """the oracle's prediction of one record in plane p (put from ref[0], then avg from ref[1] when compound): a (h, w) int64 block"""
    O = _oracle()
    refs = fr.refs if refs is None else refs
    dt = np.uint8 if fr.bd == 8 else np.uint16
    ps = np.dtype(dt).itemsize
    w, h = rec["w"], rec["h"]
    out = np.zeros((h, w), dt)
    for r in range(2 if rec["flags"] & 1 else 1):
        xi, yi, mx, my = rec_geometry(fr, rec, p, r)
        ref = refs[rec["ref"][r]][p]
        if route == "clamp":
            win = np.ascontiguousarray(window(ref, xi, yi, w, h).astype(dt))
            at = (3 * win.shape[1] + 3) * ps
        else:
            assert -BORDER + 3 <= xi and xi + w + 5 <= ref.shape[1] + BORDER and -BORDER + 3 <= yi and yi + h + 5 <= ref.shape[0] + BORDER, \
                "window outside the border"
            win = padded(ref, dt)
            at = ((yi + BORDER) * win.shape[1] + xi + BORDER) * ps
        O.ffo_vp9_mc_bd(fr.bd, rec["filter"], r, ffi.ptr(out), w * ps, C.cast(win.ctypes.data + at, ffi.u8p), win.shape[1] * ps, w, h, mx, my)
    return out.astype(np.int64)


def tu_add(fr, t, blk, p):
    """itxfm_add[tx][txtp] of TU t on the (N, N) int64 block blk (a copy), returned"""
    O = _oracle()
    N = 4 if t["tx"] == 4 else 4 << t["tx"]
    co = fr.coeffs[p][t["coeff_offset"]:t["coeff_offset"] + N * N]
    eob = 1 if t["dc_only"] else N * N
    if fr.bd == 8:
        b = np.ascontiguousarray(blk.astype(np.uint8))
        c = np.ascontiguousarray(co.astype(np.int16))
        O.ffo_vp9_itxfm_add(t["tx"], t["txtp"], ffi.ptr(b), N, ffi.ptr(c, ffi.i16p), eob)
    else:
        b = np.ascontiguousarray(blk.astype(np.uint16))
        c = np.ascontiguousarray(co.astype(np.int32))
        O.ffo_vp9_itxfm_add_bd(fr.bd, t["tx"], t["txtp"], ffi.ptr(b), 2 * N, ffi.ptr(c, ffi.i32p), eob)
    return b.astype(np.int64)


def model(fr, preds=None, tus=None, planes=None, route="clamp"):
    """the planes after inter reconstruction: per superblock every record predicted, then every TU added to the covered samples
    (records of a plane of a superblock are disjoint, so decoding order within it does not matter), the covered samples inside the
    decoded area written"""
    preds = fr.preds if preds is None else preds
    tus = fr.tus if tus is None else tus
    src = fr.planes if planes is None else planes
    out = [pl.copy() for pl in src]
    for p in range(3):
        Cw, Ch = 64 >> fr.hs[p], 64 >> fr.vs[p]
        canvas = np.zeros((fr.sb_h * Ch, fr.sb_w * Cw), np.int64)
        cov = np.zeros(canvas.shape, bool)
        chroma = int(p > 0)
        for rec in preds:
            if (rec["flags"] >> 1) & 1 != chroma:
                continue
            x, y, w, h = rec["x"], rec["y"], rec["w"], rec["h"]
            canvas[y:y + h, x:x + w] = predict(fr, rec, p, route)
            cov[y:y + h, x:x + w] = True
        for t in tus[p]:
            N = 4 if t["tx"] == 4 else 4 << t["tx"]
            x, y = t["x"], t["y"]
            m = cov[y:y + N, x:x + N]
            if not m.any():
                continue
            blk = canvas[y:y + N, x:x + N]
            new = tu_add(fr, t, blk.copy(), p)
            blk[m] = new[m]
        dh, dw = fr.dh[p], fr.dw[p]        # the decoded area (planes may be larger)
        c = cov[:dh, :dw]
        out[p][:dh, :dw][c] = canvas[:dh, :dw][c]
    return out
