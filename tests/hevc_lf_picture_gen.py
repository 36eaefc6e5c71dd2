"""Synthetic HEVC pictures for the in-loop filter face (ffhip_hevc_loop_filter_pictures_dev), its sequential model, and an
independent restatement of H.265 8.7.2.5 / 8.7.3.

The generator builds what a decoder holds when the in-loop filters run: a reconstructed picture of blocky content (so that the
filters act), tiles, slices (contiguous in tile-scan order) with their own beta / tC offsets, some with deblocking disabled and some
with slice_loop_filter_across_slices_enabled_flag 0; random CU quadtrees with intra, inter and bypass (PCM / transquant-bypass)
CUs, QpY per CU from -6 * (bd - 8) to 51, transform and prediction splits inside CUs; the boundary strengths the decoder derives
from them (2 on intra-CU edges, 0 / 1 / 2 on TU / PU edges, 0 across a slice or tile edge the flags forbid and on the edges of a
slice with deblocking disabled); SAO off / band / edge over all four classes per CTB and component, and the sao_edge_restore
flags by the standard's rule for neighbours in other slices and tiles.

The model drives the oracle's pinned per-call functions in the reference's order: ffo_hevc_loop_filter_bd over every vertical
edge of the picture, then every horizontal one (deblocking_filter_CTB's operands: beta, two tC, no_p / no_q per 8-line unit),
then per CTB and component ffo_hevc_sao_band_bd or ffo_hevc_sao_edge_bd + ffo_hevc_sao_edge_restore_bd from the deblocked picture,
then the bypass samples' deblocked values.  The restatement decides per sample from the slice and tile maps and shares nothing
with the model but the tables of the standard."""
import ctypes as C

import numpy as np

import ffi

# H.265 Table 8-12 (beta', tC') and Table 8-10 (QpC of qPi 30..43 for ChromaArrayType 1)
BETA = [0] * 16 + [6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 20, 22, 24, 26, 28, 30, 32, 34, 36, 38, 40, 42, 44, 46, 48, 50, 52,
                   54, 56, 58, 60, 62, 64]
TC = [0] * 18 + [1] * 9 + [2] * 4 + [3] * 4 + [4] * 3 + [5, 5, 6, 6, 7, 8, 9, 10, 11, 13, 14, 16, 18, 20, 22, 24]
QPC = [29, 30, 31, 32, 33, 33, 34, 34, 35, 35, 36, 36, 37, 37]
assert len(BETA) == 52 and len(TC) == 54
EO_DX = ((-1, 1), (0, 0), (-1, 1), (1, -1))
EO_DY = ((0, 0), (-1, 1), (-1, 1), (-1, 1))


def clip(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def chroma_qp(qpi, cfi):
    if cfi != 1:
        return min(qpi, 51)
    return qpi if qpi < 30 else qpi - 6 if qpi > 43 else QPC[qpi - 30]


class LfPicture:
    """One generated picture.  src[p]: the reconstructed planes (int64); bs_ver / bs_hor: (H / 4, W / 4) uint8; qp / bypass: the
    min-CB grid; ctbs: per raster CTB a dict of FFHipHevcLfCtb fields; slice_of / tile_of: per raster CTB; slices: dicts."""

    def __init__(self, rng, width, height, log2_ctb, bd, cfi, log2_min_cb=3, tiles=(1, 1), nslices=2, p_bypass=0.08, p_intra=0.3,
                 deblock=True, sao=True, lf_across_tiles=None, cqp=None):
        assert width % (1 << log2_min_cb) == 0 and height % (1 << log2_min_cb) == 0   # whole min CBs, as the standard requires
        self.rng, self.W, self.H, self.log2_ctb, self.bd, self.cfi, self.lmc = rng, width, height, log2_ctb, bd, cfi, log2_min_cb
        self.C = C_ = 1 << log2_ctb
        self.ctb_w, self.ctb_h = -(-width // C_), -(-height // C_)
        self.nplanes = 3 if cfi else 1
        self.hs = [0] + [int(cfi in (1, 2))] * 2
        self.vs = [0] + [int(cfi == 1)] * 2
        self.maxv = (1 << bd) - 1
        self.src = [self._content((height >> self.vs[p], width >> self.hs[p])) for p in range(self.nplanes)]
        # the chroma offsets keep qPi <= 57, where filter.c's Clip3(0, 57, .) and the standard's Table 8-10 agree
        self.cb_qp_offset, self.cr_qp_offset = cqp if cqp is not None else (int(rng.integers(-12, 7)), int(rng.integers(-12, 7)))

        # ---- tiles, tile scan, slices contiguous in tile scan ----
        nctb = self.ctb_w * self.ctb_h
        cols = self._bounds(self.ctb_w, tiles[0])
        rows = self._bounds(self.ctb_h, tiles[1])
        self.tile_of = np.zeros(nctb, np.int64)
        ts = []
        for ty in range(len(rows) - 1):
            for tx in range(len(cols) - 1):
                for y in range(rows[ty], rows[ty + 1]):
                    for x in range(cols[tx], cols[tx + 1]):
                        self.tile_of[y * self.ctb_w + x] = ty * (len(cols) - 1) + tx
                        ts.append(y * self.ctb_w + x)
        self.lf_across_tiles = bool(rng.integers(0, 2)) if lf_across_tiles is None else lf_across_tiles
        self.tiles_enabled = len(ts) and (len(cols) > 2 or len(rows) > 2)
        nslices = max(1, min(nslices, nctb))
        cuts = sorted(rng.choice(np.arange(1, nctb), nslices - 1, replace=False).tolist()) if nslices > 1 else []
        self.slice_of = np.zeros(nctb, np.int64)
        for i, a in enumerate(ts):
            self.slice_of[a] = sum(1 for c in cuts if c <= i)
        self.slices = []
        for i in range(nslices):
            off = rng.integers(-6, 7, 2) * 2
            self.slices.append(dict(beta_offset=int(off[0]), tc_offset=int(off[1]), deblock_off=bool(rng.random() < 0.2),
                                    across=bool(rng.random() < 0.5), sao_luma=bool(rng.random() < 0.85), sao_chroma=bool(rng.random() < 0.85)))
        if not deblock:
            for s in self.slices:
                s["deblock_off"] = True
        if not sao:
            for s in self.slices:
                s["sao_luma"] = s["sao_chroma"] = False

        # ---- CU quadtrees: QpY, bypass, intra, and the TU / PU edges on the 8 x 8 grid ----
        self.nb_w, self.nb_h = -(-width // (1 << log2_min_cb)), -(-height // (1 << log2_min_cb))
        self.qp = np.zeros((self.nb_h, self.nb_w), np.int64)
        self.bypass = np.zeros((self.nb_h, self.nb_w), np.uint8)
        self.cu = -np.ones((height // 4, width // 4), np.int64)        # CU id per 4 x 4
        self.intra = np.zeros((height // 4, width // 4), bool)
        self.inner_v = np.zeros((height // 4, width // 4), np.int64)   # 1 TU edge, 2 PU edge (inside a CU) at this 4 x 4's left
        self.inner_h = np.zeros((height // 4, width // 4), np.int64)
        self._ncu = 0
        for a in range(nctb):
            cy, cx = divmod(a, self.ctb_w)
            self._cu_tree(cx * C_, cy * C_, log2_ctb, p_bypass, p_intra)
        self._bs()
        self._sao()

    # ---- content ----
    def _content(self, shape):
        """blocky: a gradient, per-4x4 steps of a few levels and noise, so that every filter decision occurs"""
        h, w = shape
        rng, s = self.rng, 1 << (self.bd - 8)
        y, x = np.mgrid[0:h, 0:w]
        base = (x * rng.integers(0, 3) + y * rng.integers(0, 3) + rng.integers(40, 200)) * s
        step = np.kron(rng.integers(-6, 7, (-(-h // 4), -(-w // 4))) * rng.integers(1, 5), np.ones((4, 4), np.int64))[:h, :w] * s
        noise = rng.integers(-1, 2, (h, w)) * s
        out = base + step + noise
        wild = rng.random((h, w)) < 0.01
        out[wild] = rng.integers(0, self.maxv + 1, int(wild.sum()))
        return np.clip(out, 0, self.maxv).astype(np.int64)

    @staticmethod
    def _bounds(n, k):
        k = max(1, min(k, n))
        return [i * n // k for i in range(k + 1)]

    def _cu_tree(self, x, y, log2, p_bypass, p_intra):
        if x >= self.W or y >= self.H:
            return
        s = 1 << log2
        if log2 > self.lmc and (x + s > self.W or y + s > self.H or self.rng.random() < 0.55):
            h = s // 2
            for dy in (0, h):
                for dx in (0, h):
                    self._cu_tree(x + dx, y + dy, log2 - 1, p_bypass, p_intra)
            return
        rng, m = self.rng, 1 << self.lmc
        q = int(rng.integers(-6 * (self.bd - 8), 52))
        byp = int(rng.random() < p_bypass)
        self.qp[y // m:(y + s) // m, x // m:(x + s) // m] = q
        self.bypass[y // m:(y + s) // m, x // m:(x + s) // m] = byp
        y4, x4, n4 = y // 4, x // 4, s // 4
        self.cu[y4:y4 + n4, x4:x4 + n4] = self._ncu
        self._ncu += 1
        intra = rng.random() < p_intra
        self.intra[y4:y4 + n4, x4:x4 + n4] = intra
        # inner edges: a random transform split down to 8 x 8, and for inter CUs a PU split (2NxN / Nx2N / AMP)
        self._tu_split(x, y, s)
        if not intra and s >= 16:
            k = rng.integers(0, 4)
            if k == 1:
                self.inner_h[y4 + n4 // 2, x4:x4 + n4] = 2
            elif k == 2:
                self.inner_v[y4:y4 + n4, x4 + n4 // 2] = 2
            elif k == 3 and s >= 32:
                self.inner_v[y4:y4 + n4, x4 + n4 // 4] = 2                    # nLx2N: only its 8-grid part counts

    def _tu_split(self, x, y, s):
        if s <= 8 or self.rng.random() < 0.5:
            return
        h = s // 2
        y4, x4 = y // 4, x // 4
        self.inner_v[y4:y4 + s // 4, x4 + h // 4] = np.maximum(self.inner_v[y4:y4 + s // 4, x4 + h // 4], 1)
        self.inner_h[y4 + h // 4, x4:x4 + s // 4] = np.maximum(self.inner_h[y4 + h // 4, x4:x4 + s // 4], 1)
        for dy in (0, h):
            for dx in (0, h):
                self._tu_split(x + dx, y + dy, h)

    def ctb_at(self, x, y):
        return (y >> self.log2_ctb) * self.ctb_w + (x >> self.log2_ctb)

    def _edge_bs(self, xq, yq, xp, yp, inner):
        """the bS of the segment whose q0,0 is luma (xq, yq) and whose p side holds (xp, yp)"""
        rng = self.rng
        aq, ap = self.ctb_at(xq, yq), self.ctb_at(xp, yp)
        sl = self.slices[self.slice_of[aq]]
        if sl["deblock_off"]:
            return 0
        if self.slice_of[aq] != self.slice_of[ap] and not sl["across"]:
            return 0
        if self.tile_of[aq] != self.tile_of[ap] and not self.lf_across_tiles:
            return 0
        cu_edge = self.cu[yq >> 2, xq >> 2] != self.cu[yp >> 2, xp >> 2]
        if self.intra[yq >> 2, xq >> 2] or self.intra[yp >> 2, xp >> 2]:
            return 2 if (cu_edge or inner) else 0
        if cu_edge or inner:
            return int(rng.choice([0, 1, 2], p=[0.3, 0.5, 0.2]))
        return 0

    def _bs(self):
        W, H = self.W, self.H
        self.bs_ver = np.zeros((H // 4, W // 4), np.uint8)
        self.bs_hor = np.zeros((H // 4, W // 4), np.uint8)
        for y in range(0, H, 4):
            for x in range(8, W, 8):
                self.bs_ver[y >> 2, x >> 2] = self._edge_bs(x, y, x - 1, y, self.inner_v[y >> 2, x >> 2])
        for y in range(8, H, 8):
            for x in range(0, W, 4):
                self.bs_hor[y >> 2, x >> 2] = self._edge_bs(x, y, x, y - 1, self.inner_h[y >> 2, x >> 2])

    def _available(self, a, b):
        """may SAO of a sample of CTB a use a neighbour in CTB b (H.265 8.7.3.2: slices by tile-scan order, tiles)"""
        sa, sb = self.slice_of[a], self.slice_of[b]
        if sa != sb:
            later = sa if sa > sb else sb
            if not self.slices[later]["across"]:
                return False
        if self.tile_of[a] != self.tile_of[b] and not self.lf_across_tiles:
            return False
        return True

    def _sao(self):
        rng, sc = self.rng, 1 << (self.bd - min(self.bd, 10))
        lim = (1 << (min(self.bd, 10) - 5)) - 1
        self.ctbs = []
        for a in range(self.ctb_w * self.ctb_h):
            cy, cx = divmod(a, self.ctb_w)
            sl = self.slices[self.slice_of[a]]
            r = dict(beta_offset=sl["beta_offset"], tc_offset=sl["tc_offset"], sao_type=[0, 0, 0], sao_class=[0, 0, 0],
                     sao_offset_val=np.zeros((3, 5), np.int64))
            for c in range(self.nplanes):
                if not (sl["sao_chroma"] if c else sl["sao_luma"]) or rng.random() < 0.25:
                    continue
                t = int(rng.integers(1, 3))
                r["sao_type"][c] = t
                mags = rng.integers(0, lim + 1, 4)
                if t == 1:
                    r["sao_class"][c] = int(rng.integers(0, 32))
                    r["sao_offset_val"][c, 1:] = mags * rng.choice([-1, 1], 4) * sc
                else:
                    r["sao_class"][c] = int(rng.integers(0, 4))
                    r["sao_offset_val"][c, 1:] = np.array([mags[0], mags[1], -mags[2], -mags[3]]) * sc
            # the restore flags: neighbouring CTBs whose samples SAO must not use
            nb = lambda dx, dy: (0 <= cx + dx < self.ctb_w and 0 <= cy + dy < self.ctb_h and
                                 not self._available(a, (cy + dy) * self.ctb_w + cx + dx))
            ve = nb(-1, 0) | nb(1, 0) << 1
            he = nb(0, -1) | nb(0, 1) << 1
            de = nb(-1, -1) | nb(1, -1) << 1 | nb(1, 1) << 2 | nb(-1, 1) << 3
            r.update(vert_edge=int(ve), horiz_edge=int(he), diag_edge=int(de), restore=int(bool(ve | he | de) or rng.random() < 0.3))
            self.ctbs.append(r)

    # ---- what the face takes ----
    def ctb_table(self, dtype):
        t = np.zeros(len(self.ctbs), dtype)
        for i, r in enumerate(self.ctbs):
            for k in ("beta_offset", "tc_offset", "sao_type", "sao_class", "restore", "vert_edge", "horiz_edge", "diag_edge", "sao_offset_val"):
                t[i][k] = r[k]
        return t

    def borders(self, a):
        cy, cx = divmod(a, self.ctb_w)
        return [int(cx == 0), int(cy == 0), int(cx == self.ctb_w - 1), int(cy == self.ctb_h - 1)]

    def bypass_at(self, x, y):
        return bool(self.bypass[y >> self.lmc, x >> self.lmc])

    def bypass_mask(self, p):
        """per sample of plane p: does it lie in a bypass CU"""
        ph, pw = self.H >> self.vs[p], self.W >> self.hs[p]
        ys = (np.arange(ph) << self.vs[p]) >> self.lmc
        xs = (np.arange(pw) << self.hs[p]) >> self.lmc
        return self.bypass[ys[:, None], xs[None, :]] != 0


# ================================================================================================================================
# the model: the oracle's per-call functions in the reference's order
# ================================================================================================================================
def _oracle():
    L = ffi.oracle()
    assert L is not None, "the oracle library is not built"
    return L


def _dt(bd):
    return np.uint8 if bd == 8 else np.uint16


def _ptr(a, y, x):
    return C.cast(a.ctypes.data + (y * a.shape[1] + x) * a.itemsize, C.POINTER(C.c_uint8))


def _tc_luma(qpl, bs, tc_offset):
    return TC[clip(qpl + 2 * (bs - 1) + (tc_offset & -2), 0, 53)]


def edges(pic):
    """deblocking_filter_CTB's calls over the whole picture: per direction a list of (plane, vertical, chroma, x, y, beta, tc[2],
    no_p[2], no_q[2]) in plane samples, one per 8-line unit with some segment filtered.  Vertical edges first, then horizontal."""
    W, H, out = pic.W, pic.H, []
    bsv = lambda m, x, y: int(m[y >> 2, x >> 2]) if y < pic.H and x < pic.W else 0
    qp = lambda x, y: int(pic.qp[y >> pic.lmc, x >> pic.lmc])
    byp = lambda x, y: int(pic.bypass_at(x, y))
    for vertical in (True, False):
        m = pic.bs_ver if vertical else pic.bs_hor
        calls = []
        # luma: 8-line units at (x, y); segments at +0 and +4 along the edge
        for y in range(0 if vertical else 8, H, 8):
            for x in range(8 if vertical else 0, W, 8):
                segs = [(x, y), (x, y + 4)] if vertical else [(x, y), (x + 4, y)]
                bs = [bsv(m, sx, sy) for sx, sy in segs]
                bs = [b if b in (1, 2) else 0 for b in bs]
                if not any(bs):
                    continue
                px, py = (x - 1, y) if vertical else (x, y - 1)
                qpl = (qp(px, py) + qp(x, y) + 1) >> 1
                R = pic.ctbs[pic.ctb_at(x, y)]
                beta = BETA[clip(qpl + R["beta_offset"], 0, 51)]
                tc = [_tc_luma(qpl, b, R["tc_offset"]) if b else 0 for b in bs]
                nop = [byp(sx - vertical, sy - (not vertical)) for sx, sy in segs]
                noq = [byp(sx, sy) for sx, sy in segs]
                calls.append((0, vertical, False, x, y, beta, tc, nop, noq))
        for p in range(1, pic.nplanes):
            h, v = 1 << pic.hs[p], 1 << pic.vs[p]
            off = pic.cb_qp_offset if p == 1 else pic.cr_qp_offset
            for y in range(0 if vertical else 8 * v, H, 8 * v):
                for x in range(8 * h if vertical else 0, W, 8 * h):
                    segs = [(x, y), (x, y + 4 * v)] if vertical else [(x, y), (x + 4 * h, y)]
                    bs = [bsv(m, sx, sy) for sx, sy in segs]
                    if 2 not in bs:
                        continue
                    R = pic.ctbs[pic.ctb_at(x, y)]
                    tc, nop, noq = [], [], []
                    for (sx, sy), b in zip(segs, bs):
                        if b != 2:
                            tc.append(0), nop.append(0), noq.append(0)
                            continue
                        px, py = (sx - 1, sy) if vertical else (sx, sy - 1)
                        qpl = (qp(px, py) + qp(sx, sy) + 1) >> 1
                        qpc = chroma_qp(clip(qpl + off, 0, 57), pic.cfi)
                        tc.append(TC[clip(qpc + 2 + R["tc_offset"], 0, 53)])
                        nop.append(byp(px, py)), noq.append(byp(sx, sy))
                    calls.append((p, vertical, True, x >> pic.hs[p], y >> pic.vs[p], 0, tc, nop, noq))
        out.append(calls)
    return out


def deblock(pic, planes=None):
    """the deblocked planes (int64), by ffo_hevc_loop_filter_bd over edges(pic)"""
    L, bd = _oracle(), pic.bd
    src = pic.src if planes is None else planes
    work = [np.ascontiguousarray(s.astype(_dt(bd))) for s in src]
    for calls in edges(pic):
        for p, vertical, chroma, x, y, beta, tc, nop, noq in calls:
            a = work[p]
            L.ffo_hevc_loop_filter_bd(bd, int(chroma), int(vertical), _ptr(a, y, x), a.shape[1] * a.itemsize, beta,
                                      (C.c_int32 * 2)(*tc), (C.c_uint8 * 2)(*nop), (C.c_uint8 * 2)(*noq))
    return [a.astype(np.int64) for a in work]


def sao_blocks(pic):
    """sao_filter_CTB's work: (plane, ctb, x0, y0, w, h, type, class, offsets) per CTB and component with SAO applied"""
    out = []
    for a in range(pic.ctb_w * pic.ctb_h):
        cy, cx = divmod(a, pic.ctb_w)
        R = pic.ctbs[a]
        for p in range(pic.nplanes):
            t, k = R["sao_type"][p], R["sao_class"][p]
            if not ((t == 1 and k < 32) or (t == 2 and k < 4)):
                continue
            cw, ch = pic.C >> pic.hs[p], pic.C >> pic.vs[p]
            x0, y0 = cx * cw, cy * ch
            w, h = min(cw, (pic.W >> pic.hs[p]) - x0), min(ch, (pic.H >> pic.vs[p]) - y0)
            out.append((p, a, x0, y0, w, h, t, k, [int(v) for v in R["sao_offset_val"][p]]))
    return out


def model(pic, planes=None):
    """the filtered planes (int64): deblocking, then SAO + sao_edge_restore + the bypass copy-back per CTB and component"""
    L, bd = _oracle(), pic.bd
    dbk = deblock(pic, planes)
    out = [d.copy() for d in dbk]
    # the deblocked planes with a 1-sample border, so that the edge filter's reads at the picture border stay in bounds
    pads = [np.ascontiguousarray(np.pad(d, 1, mode="edge").astype(_dt(bd))) for d in dbk]
    masks = [pic.bypass_mask(p) for p in range(pic.nplanes)]
    for p, a, x0, y0, w, h, t, k, ov in sao_blocks(pic):
        pad = pads[p]
        blk = np.ascontiguousarray(np.zeros((h, w), _dt(bd)))
        ss, sd = pad.shape[1] * pad.itemsize, w * blk.itemsize
        offs = (C.c_int16 * 5)(*ov)
        if t == 1:
            L.ffo_hevc_sao_band_bd(bd, _ptr(blk, 0, 0), _ptr(pad, y0 + 1, x0 + 1), sd, ss, offs, k, w, h)
        else:
            L.ffo_hevc_sao_edge_bd(bd, _ptr(blk, 0, 0), _ptr(pad, y0 + 1, x0 + 1), sd, ss, offs, k, w, h)
            R = pic.ctbs[a]
            bits = lambda v, n: (C.c_uint8 * n)(*[(v >> i) & 1 for i in range(n)])
            L.ffo_hevc_sao_edge_restore_bd(bd, R["restore"], _ptr(blk, 0, 0), _ptr(pad, y0 + 1, x0 + 1), sd, ss, k, ov[0],
                                           (C.c_int * 4)(*pic.borders(a)), w, h, bits(R["vert_edge"], 2), bits(R["horiz_edge"], 2),
                                           bits(R["diag_edge"], 4))
        m = masks[p][y0:y0 + h, x0:x0 + w]
        out[p][y0:y0 + h, x0:x0 + w] = np.where(m, dbk[p][y0:y0 + h, x0:x0 + w], blk.astype(np.int64))
    return out


# ================================================================================================================================
# the restatement: H.265 8.7.2.5 and 8.7.3 per segment and per sample, nothing shared with the model but the tables
# ================================================================================================================================
def restate(pic):
    bd, maxv = pic.bd, pic.maxv
    rec = [s.copy() for s in pic.src]
    sc = 1 << (bd - 8)

    def qp(x, y):
        return int(pic.qp[y >> pic.lmc, x >> pic.lmc])

    def bs_of(vertical, x, y):
        b = int((pic.bs_ver if vertical else pic.bs_hor)[y >> 2, x >> 2])
        return b if b in (1, 2) else 0

    def line(a, vertical, X, Y, k):      # sample k of the line through (X, Y): k < 0 p side, k >= 0 q side
        return (Y, X + k) if vertical else (Y + k, X)

    for vertical in (True, False):
        # luma: every 4-line segment on the 8 x 8 grid (8.7.2.5.3 decisions, 8.7.2.5.6 / 8.7.2.5.7 filtering)
        a = rec[0]
        segs = ([(x, y) for y in range(0, pic.H, 4) for x in range(8, pic.W, 8)] if vertical else
                [(x, y) for y in range(8, pic.H, 8) for x in range(0, pic.W, 4)])
        new = a.copy()
        for X, Y in segs:
            bS = bs_of(vertical, X, Y)
            if not bS:
                continue
            P = (X - 1, Y) if vertical else (X, Y - 1)
            qpl = (qp(*P) + qp(X, Y) + 1) >> 1
            R = pic.ctbs[pic.ctb_at(X, Y)]
            beta = BETA[clip(qpl + R["beta_offset"], 0, 51)] * sc
            tc = TC[clip(qpl + 2 * (bS - 1) + R["tc_offset"], 0, 53)] * sc
            lines = [(X, Y + d) if vertical else (X + d, Y) for d in range(4)]
            px = lambda i, k: int(a[line(a, vertical, *lines[i], -k - 1)])      # p_k of line i
            qx = lambda i, k: int(a[line(a, vertical, *lines[i], k)])
            dp0, dp3 = abs(px(0, 2) - 2 * px(0, 1) + px(0, 0)), abs(px(3, 2) - 2 * px(3, 1) + px(3, 0))
            dq0, dq3 = abs(qx(0, 2) - 2 * qx(0, 1) + qx(0, 0)), abs(qx(3, 2) - 2 * qx(3, 1) + qx(3, 0))
            d = dp0 + dq0 + dp3 + dq3
            if d >= beta:
                continue

            def dsam(i, dpq):
                return (2 * dpq < (beta >> 2) and abs(px(i, 3) - px(i, 0)) + abs(qx(i, 0) - qx(i, 3)) < (beta >> 3) and
                        abs(px(i, 0) - qx(i, 0)) < ((5 * tc + 1) >> 1))
            dE = 2 if dsam(0, dp0 + dq0) and dsam(3, dp3 + dq3) else 1
            dEp = (dp0 + dp3) < ((beta + (beta >> 1)) >> 3)
            dEq = (dq0 + dq3) < ((beta + (beta >> 1)) >> 3)
            nop = pic.bypass_at(*P)
            noq = pic.bypass_at(X, Y)
            for i in range(4):
                p = [px(i, k) for k in range(4)]
                q = [qx(i, k) for k in range(4)]
                pn, qn = list(p), list(q)
                if dE == 2:
                    pn[0] = clip((p[2] + 2 * p[1] + 2 * p[0] + 2 * q[0] + q[1] + 4) >> 3, p[0] - 2 * tc, p[0] + 2 * tc)
                    pn[1] = clip((p[2] + p[1] + p[0] + q[0] + 2) >> 2, p[1] - 2 * tc, p[1] + 2 * tc)
                    pn[2] = clip((2 * p[3] + 3 * p[2] + p[1] + p[0] + q[0] + 4) >> 3, p[2] - 2 * tc, p[2] + 2 * tc)
                    qn[0] = clip((p[1] + 2 * p[0] + 2 * q[0] + 2 * q[1] + q[2] + 4) >> 3, q[0] - 2 * tc, q[0] + 2 * tc)
                    qn[1] = clip((p[0] + q[0] + q[1] + q[2] + 2) >> 2, q[1] - 2 * tc, q[1] + 2 * tc)
                    qn[2] = clip((p[0] + q[0] + q[1] + 3 * q[2] + 2 * q[3] + 4) >> 3, q[2] - 2 * tc, q[2] + 2 * tc)
                else:
                    delta = (9 * (q[0] - p[0]) - 3 * (q[1] - p[1]) + 8) >> 4
                    if abs(delta) >= tc * 10:
                        continue
                    delta = clip(delta, -tc, tc)
                    pn[0] = clip(p[0] + delta, 0, maxv)
                    qn[0] = clip(q[0] - delta, 0, maxv)
                    if dEp:
                        pn[1] = clip(p[1] + clip((((p[2] + p[0] + 1) >> 1) - p[1] + delta) >> 1, -(tc >> 1), tc >> 1), 0, maxv)
                    if dEq:
                        qn[1] = clip(q[1] + clip((((q[2] + q[0] + 1) >> 1) - q[1] - delta) >> 1, -(tc >> 1), tc >> 1), 0, maxv)
                for k in range(3):
                    if not nop:
                        new[line(a, vertical, *lines[i], -k - 1)] = pn[k]
                    if not noq:
                        new[line(a, vertical, *lines[i], k)] = qn[k]
        rec[0] = new
        # chroma (8.7.2.5.5): edges on the 8-sample chroma grid, bS 2, 4-line groups at the luma segment they sit on
        for c in range(1, pic.nplanes):
            a, hs, vs = rec[c], pic.hs[c], pic.vs[c]
            pw, ph = a.shape[1], a.shape[0]
            off = pic.cb_qp_offset if c == 1 else pic.cr_qp_offset
            new = a.copy()
            segs = ([(x, y) for y in range(0, ph, 4) for x in range(8, pw, 8)] if vertical else
                    [(x, y) for y in range(8, ph, 8) for x in range(0, pw, 4)])
            for X, Y in segs:
                xl, yl = X << hs, Y << vs
                if bs_of(vertical, xl, yl) != 2:
                    continue
                P = (xl - 1, yl) if vertical else (xl, yl - 1)
                qpi = ((qp(*P) + qp(xl, yl) + 1) >> 1) + off
                qpc = chroma_qp(qpi, pic.cfi)
                tc = TC[clip(qpc + 2 + pic.ctbs[pic.ctb_at(xl, yl)]["tc_offset"], 0, 53)] * sc
                for d in range(4):
                    xx, yy = (X, Y + d) if vertical else (X + d, Y)
                    g = lambda k: int(a[line(a, vertical, xx, yy, k)])
                    delta = clip((((g(0) - g(-1)) << 2) + g(-2) - g(1) + 4) >> 3, -tc, tc)
                    if not pic.bypass_at(*P):
                        new[line(a, vertical, xx, yy, -1)] = clip(g(-1) + delta, 0, maxv)
                    if not pic.bypass_at(xl, yl):
                        new[line(a, vertical, xx, yy, 0)] = clip(g(0) - delta, 0, maxv)
            rec[c] = new

    # SAO (8.7.3) per sample
    out = [r.copy() for r in rec]
    for c in range(pic.nplanes):
        a, hs, vs = rec[c], pic.hs[c], pic.vs[c]
        ph, pw = a.shape
        for Y in range(ph):
            for X in range(pw):
                xl, yl = X << hs, Y << vs
                ctb = pic.ctb_at(xl, yl)
                R = pic.ctbs[ctb]
                t, k, ov = R["sao_type"][c], R["sao_class"][c], R["sao_offset_val"][c]
                if t not in (1, 2) or pic.bypass_at(xl, yl):
                    continue
                v = int(a[Y, X])
                if t == 1:
                    if k > 31:
                        continue
                    band = ((v >> (bd - 5)) - k) & 31
                    out[c][Y, X] = clip(v + (int(ov[band + 1]) if band < 4 else 0), 0, maxv)
                    continue
                if k > 3:
                    continue
                idx, ok = 2, True
                for j in range(2):
                    nx, ny = X + EO_DX[k][j], Y + EO_DY[k][j]
                    if not (0 <= nx < pw and 0 <= ny < ph):
                        ok = False
                        break
                    if ctb != pic.ctb_at(nx << hs, ny << vs) and not pic._available(ctb, pic.ctb_at(nx << hs, ny << vs)):
                        ok = False
                        break
                    n = int(a[ny, nx])
                    idx += (v > n) - (v < n)
                if not ok:
                    continue                            # edgeIdx 0: SaoOffsetVal[0] = 0
                idx = {0: 1, 1: 2, 2: 0, 3: 3, 4: 4}[idx]
                out[c][Y, X] = clip(v + int(ov[idx]), 0, maxv)
    return out
