"""Synthetic HEVC P/B pictures for the inter reconstruction face (ffhip_hevc_inter_pictures_dev) and a sequential model of it.

The generator builds what a decoder holds when the inter stage runs: a DPB of 1..16 random reference pictures, slices (contiguous
raster CTB ranges) with their own reference lists and weight tables, P or B, weighted or not; random CTB quadtrees of inter, intra
and PCM CUs; every partition mode of an inter CU (2Nx2N, 2NxN, Nx2N, NxN at the minimum CB above 8x8, the four AMP modes above
the minimum CB; no bi-prediction for 8x4 / 4x8, as the standard has it); MVs mostly small, some pointing far past every edge;
inter transform trees (largest TB 32) with the chroma TU rules of every chroma format, with and without residuals.  The planes
start as random garbage: what no PU covers must survive.

The model predicts each PU of each plane in decoding order by gathering its reference window with clamped coordinates (H.265
8.5.3.3.3.1 / .2, what emulated_edge_mc gives the reference decoder) and calling the oracle's pinned ffo_hevc_mc_bd /
ffo_hevc_mc_w_bd in hevcdec.c's order (uni / uni_w; list 0 into the 14-bit intermediate, then bi / bi_w with list 1), then adds
the TU residuals to the covered samples and clips."""
import ctypes as C

import numpy as np

import ffi

PART_MODES = ("2Nx2N", "2NxN", "Nx2N", "NxN", "2NxnU", "2NxnD", "nLx2N", "nRx2N")
PU_FIELDS = ("x", "y", "w", "h", "flags", "ref_idx", "slice", "mv")


def part_boxes(mode, s):
    """the PUs (x, y, w, h) of an s x s CU, relative to the CU, in decoding order (hevcdec.c hls_coding_unit)"""
    h, q = s // 2, s // 4
    return {"2Nx2N": [(0, 0, s, s)], "2NxN": [(0, 0, s, h), (0, h, s, h)], "Nx2N": [(0, 0, h, s), (h, 0, h, s)],
            "NxN": [(0, 0, h, h), (h, 0, h, h), (0, h, h, h), (h, h, h, h)],
            "2NxnU": [(0, 0, s, q), (0, q, s, s - q)], "2NxnD": [(0, 0, s, s - q), (0, s - q, s, q)],
            "nLx2N": [(0, 0, q, s), (q, 0, s - q, s)], "nRx2N": [(0, 0, s - q, s), (s - q, 0, q, s)]}[mode]


class InterPicture:
    """One generated picture.  refs[slot][p]: the DPB planes (int64); planes[p]: the planes at launch; pus: PU dicts in decoding order
    (FFHipHevcInterPU fields plus 'ctb' and 'part'); tus[p]: TU dicts (plus 'ctb'); res[p]: int16 residuals; slices: INTER_SLICE
    dicts; kind: per 4x4 luma block 0 outside, 1 inter, 2 intra, 3 PCM."""

    def __init__(self, rng, width, height, log2_ctb, bd, cfi, nrefs=4, nslices=2, p_inter=0.8, p_pcm=0.1, p_res=0.6, p_far=0.05,
                 slice_types=None, weighted=None, min_cb=3, smooth=False, refs=None, p_bi=None):
        assert width % 8 == 0 and height % 8 == 0
        self.rng, self.W, self.H, self.log2_ctb, self.bd, self.cfi = rng, width, height, log2_ctb, bd, cfi
        self.C = C_ = 1 << log2_ctb
        self.ctb_w, self.ctb_h = (width + C_ - 1) // C_, (height + C_ - 1) // C_
        self.nplanes = 3 if cfi else 1
        self.hs = [0] + [int(cfi in (1, 2))] * 2
        self.vs = [0] + [int(cfi == 1)] * 2
        self.maxv = (1 << bd) - 1
        self.min_cb, self.p_inter, self.p_pcm, self.p_res, self.p_far, self.smooth = min_cb, p_inter, p_pcm, p_res, p_far, smooth
        self.p_bi = p_bi                       # B slices: the share of bi-predicted PUs (None: a third)
        shapes = [(height >> self.vs[p], width >> self.hs[p]) for p in range(self.nplanes)]
        if refs is None:
            refs = [[self._content(sh) for sh in shapes] for _ in range(nrefs)]
        self.refs = refs
        self.nrefs = len(refs)
        self.planes = [rng.integers(0, self.maxv + 1, sh).astype(np.int64) for sh in shapes]

        # ---- slices: contiguous raster CTB ranges, each with its lists and weights ----
        nctb = self.ctb_w * self.ctb_h
        nslices = max(1, min(nslices, nctb))
        starts = [0] + sorted(rng.choice(np.arange(1, nctb), nslices - 1, replace=False).tolist()) if nslices > 1 else [0]
        self.ctb_slice = np.zeros(nctb, np.int64)
        for i, s in enumerate(starts):
            self.ctb_slice[s:] = i
        self.slices = [self._slice(i, slice_types, weighted) for i in range(nslices)]

        # ---- MV field for smooth pictures: one vector per 64x64 area plus noise ----
        self.field = rng.integers(-48, 49, (2, (height >> 6) + 2, (width >> 6) + 2, 2))

        self.kind = np.zeros((self.ctb_h * C_ // 4, self.ctb_w * C_ // 4), np.int64)
        self.pus, self.tus = [], [[] for _ in range(self.nplanes)]
        self._res = [[] for _ in range(self.nplanes)]
        self._nres = [0] * self.nplanes
        for a in range(nctb):
            cy, cx = divmod(a, self.ctb_w)
            self._cu_tree(a, cx * C_, cy * C_, log2_ctb)
        self.res = [np.concatenate(r) if r else np.zeros(16, np.int16) for r in self._res]

    def _content(self, shape):
        """a reference plane: smooth gradients plus noise, with some extreme samples"""
        h, w = shape
        yy, xx = np.mgrid[0:h, 0:w]
        f = self.rng.uniform(0.01, 0.2, 2)
        base = (np.sin(xx * f[0]) + np.cos(yy * f[1]) + 2) / 4 * self.maxv
        a = base + self.rng.normal(0, self.maxv / 16, shape)
        a[self.rng.random(shape) < 0.02] = self.maxv
        a[self.rng.random(shape) < 0.02] = 0
        return np.clip(np.rint(a), 0, self.maxv).astype(np.int64)

    def _slice(self, i, slice_types, weighted):
        rng = self.rng
        st = (slice_types[i % len(slice_types)] if slice_types else rng.choice(["P", "B"]))
        wtd = bool(rng.integers(2)) if weighted is None else bool(weighted)
        nr = [int(rng.integers(1, 17)), int(rng.integers(1, 17)) if st == "B" else 0]
        s = dict(type=st, ref=np.zeros((2, 16), np.int64), num_ref=nr, weighted=int(wtd), luma_log2_denom=int(rng.integers(0, 8)),
                 chroma_log2_denom=int(rng.integers(0, 8)), luma_weight=np.zeros((2, 16), np.int64), luma_offset=np.zeros((2, 16), np.int64),
                 chroma_weight=np.zeros((2, 16, 2), np.int64), chroma_offset=np.zeros((2, 16, 2), np.int64))
        for l in range(2):
            s["ref"][l, :nr[l]] = rng.integers(0, self.nrefs, nr[l])
            if wtd:
                s["luma_weight"][l] = (1 << s["luma_log2_denom"]) + rng.integers(-128, 128, 16)
                s["luma_offset"][l] = rng.integers(-128, 128, 16)
                s["chroma_weight"][l] = (1 << s["chroma_log2_denom"]) + rng.integers(-128, 128, (16, 2))
                s["chroma_offset"][l] = rng.integers(-128, 128, (16, 2))
        return s

    # ---- coding quadtree ----
    def _cu_tree(self, a, x, y, log2):
        if x >= self.W or y >= self.H:
            return
        s = 1 << log2
        split = log2 > 3 and (x + s > self.W or y + s > self.H or (log2 > self.min_cb and self.rng.random() < 0.45))
        if split:
            h = s // 2
            for dy in (0, h):
                for dx in (0, h):
                    self._cu_tree(a, x + dx, y + dy, log2 - 1)
            return
        r = self.rng.random()
        k = 1 if r < self.p_inter else 3 if r < self.p_inter + self.p_pcm else 2
        self.kind[y >> 2:(y + s) >> 2, x >> 2:(x + s) >> 2] = k
        if k != 1:
            return
        modes = ["2Nx2N", "2NxN", "Nx2N"]
        if log2 == self.min_cb and log2 > 3:
            modes.append("NxN")
        if log2 > self.min_cb:
            modes += ["2NxnU", "2NxnD", "nLx2N", "nRx2N"]
        mode = str(self.rng.choice(modes))
        for (dx, dy, w, h) in part_boxes(mode, s):
            self.pus.append(self._pu(a, x + dx, y + dy, w, h, mode))
        self._tu_tree(a, x, y, x, y, log2, 0)

    def _mv(self, x, y, w, h):
        rng = self.rng
        if self.smooth:
            return [int(v) + int(rng.integers(-4, 5)) for v in self.field[0, y >> 6, x >> 6]]
        r = rng.random()
        if r < self.p_far:          # anywhere in the int16 range: far past every edge
            return [int(v) for v in rng.integers(-32768, 32768, 2)]
        if r < 3 * self.p_far + 0.1:   # just across an edge of the picture
            return [int((rng.integers(-40, 8) - x) * 4 if rng.random() < 0.5 else (self.W - x - w + rng.integers(-8, 40)) * 4)
                    + int(rng.integers(0, 4)),
                    int((rng.integers(-40, 8) - y) * 4 if rng.random() < 0.5 else (self.H - y - h + rng.integers(-8, 40)) * 4)
                    + int(rng.integers(0, 4))]
        return [int(v) for v in rng.integers(-64, 65, 2)]

    def _mv_clipped(self, x, y, w, h):
        return [int(np.clip(v, -32768, 32767)) for v in self._mv(x, y, w, h)]

    def _pu(self, a, x, y, w, h, mode):
        rng = self.rng
        sl = int(self.ctb_slice[a])
        S = self.slices[sl]
        if S["type"] == "P":
            flags = 1
        else:
            bi = (rng.random() < 1 / 3) if self.p_bi is None else (rng.random() < self.p_bi)
            flags = 3 if bi and w + h != 12 else int(rng.choice([1, 2]))
        ref_idx = [int(rng.integers(0, S["num_ref"][l])) if flags >> l & 1 else 0 for l in range(2)]
        mv = [self._mv_clipped(x, y, w, h) if flags >> l & 1 else [0, 0] for l in range(2)]
        return dict(x=x, y=y, w=w, h=h, flags=flags, ref_idx=ref_idx, slice=sl, mv=mv, ctb=a, part=mode)

    # ---- transform tree (largest TB 32) ----
    def _tu_tree(self, a, x, y, xb, yb, log2, blk):
        split = log2 > 5 or (log2 > 2 and self.rng.random() < 0.4)
        if split:
            h = 1 << (log2 - 1)
            for i, (dy, dx) in enumerate(((0, 0), (0, h), (h, 0), (h, h))):
                self._tu_tree(a, x + dx, y + dy, x, y, log2 - 1, i)
            return
        self._tu(a, 0, x, y, log2)
        if not self.cfi:
            return
        for p in (1, 2):
            if self.cfi == 3:
                self._tu(a, p, x, y, log2)
            elif log2 > 2:
                self._chroma(a, p, x, y, log2 - 1)
            elif blk == 3:   # 4x4 luma: the chroma of the parent 8x8 after its fourth block
                self._chroma(a, p, xb, yb, 2)

    def _chroma(self, a, p, xl, yl, log2c):
        xc, yc = xl >> 1, yl >> self.vs[p]
        self._tu(a, p, xc, yc, log2c)
        if self.cfi == 2:
            self._tu(a, p, xc, yc + (1 << log2c), log2c)

    def _tu(self, a, p, x, y, log2):
        r = self.rng.random()
        if r < 0.2:
            return           # cbf 0 and no record
        off = -1
        if r < 0.2 + self.p_res * 0.8:
            N = 1 << log2
            amp = (1 << self.bd) if self.rng.random() < 0.2 else (1 << (self.bd - 3))
            self._res[p].append(self.rng.integers(-amp, amp + 1, N * N).astype(np.int16))
            off = self._nres[p]
            self._nres[p] += N * N
        self.tus[p].append(dict(x=x, y=y, res_offset=off, log2_size=log2, ctb=a))

    # ---- what the device face takes ----
    def slice_table(self, dtype):
        t = np.zeros(len(self.slices), dtype)
        for i, s in enumerate(self.slices):
            for f in ("ref", "num_ref", "weighted", "luma_log2_denom", "chroma_log2_denom", "luma_weight", "luma_offset", "chroma_weight",
                      "chroma_offset"):
                t[i][f] = s[f]
        return t

    def pack(self, recs, dtype, fields):
        """(records sorted by raster CTB as a structured array, int32 CTB starts)"""
        nctb = self.ctb_w * self.ctb_h
        idx = sorted(range(len(recs)), key=lambda i: recs[i]["ctb"])
        arr = np.zeros(len(recs), dtype)
        for j, i in enumerate(idx):
            for f in fields:
                arr[j][f] = recs[i][f]
        counts = np.bincount(np.array([recs[i]["ctb"] for i in idx], np.int64), minlength=nctb) if recs else np.zeros(nctb, np.int64)
        return arr, np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


# ---- the model ----
_O = None


def _oracle():
    global _O
    if _O is None:
        _O = ffi.oracle()
    return _O


def chroma_mv(mv, hs, vs):
    """chroma_mc_uni / chroma_mc_bi: (integer offset x, y; eighth-sample phases mx, my)"""
    return mv[0] >> (2 + hs), mv[1] >> (2 + vs), (mv[0] & ((4 << hs) - 1)) << (1 - hs), (mv[1] & ((4 << vs) - 1)) << (1 - vs)


def pu_geometry(pic, pu, p, l):
    """(bx, by, bw, bh, xi, yi, mx, my) of PU `pu` in plane p for list l"""
    hs, vs = pic.hs[p], pic.vs[p]
    bx, by, bw, bh = pu["x"] >> hs, pu["y"] >> vs, pu["w"] >> hs, pu["h"] >> vs
    mv = pu["mv"][l]
    if p == 0:
        return bx, by, bw, bh, bx + (mv[0] >> 2), by + (mv[1] >> 2), mv[0] & 3, mv[1] & 3
    dx, dy, mx, my = chroma_mv(mv, hs, vs)
    return bx, by, bw, bh, bx + dx, by + dy, mx, my


def window(ref, xi, yi, bw, bh, before, taps):
    """the reference samples rows yi - before .. and columns xi - before .., (bh + taps - 1) x (bw + taps - 1), clamped to the plane"""
    h, w = ref.shape
    ys = np.clip(np.arange(yi - before, yi - before + bh + taps - 1), 0, h - 1)
    xs = np.clip(np.arange(xi - before, xi - before + bw + taps - 1), 0, w - 1)
    return ref[np.ix_(ys, xs)]


def predict_pu(pic, pu, p, refs=None):
    """the oracle's prediction of one PU in plane p: a (bh, bw) int64 block"""
    O = _oracle()
    refs = pic.refs if refs is None else refs
    bd, chroma = pic.bd, int(p > 0)
    dt = np.uint8 if bd == 8 else np.uint16
    ps = np.dtype(dt).itemsize
    taps, before = (4, 1) if chroma else (8, 3)
    S = pic.slices[pu["slice"]]
    wtd = S["weighted"]
    denom = S["chroma_log2_denom"] if p else S["luma_log2_denom"]

    def wo(l):
        ri = pu["ref_idx"][l]
        if p:
            return int(S["chroma_weight"][l][ri][p - 1]), int(S["chroma_offset"][l][ri][p - 1])
        return int(S["luma_weight"][l][ri]), int(S["luma_offset"][l][ri])

    def src(l):
        bx, by, bw, bh, xi, yi, mx, my = pu_geometry(pic, pu, p, l)
        win = np.ascontiguousarray(window(refs[S["ref"][l][pu["ref_idx"][l]]][p], xi, yi, bw, bh, before, taps).astype(dt))
        stride = win.shape[1] * ps
        return win, C.cast(win.ctypes.data + (before * win.shape[1] + before) * ps, ffi.u8p), stride, bw, bh, mx, my

    out = np.zeros((pu["h"] >> pic.vs[p], pu["w"] >> pic.hs[p]), dt)
    if pu["flags"] == 3:
        w0, sp0, st0, bw, bh, mx0, my0 = src(0)
        tmp = np.zeros((64, 64), np.int16)
        O.ffo_hevc_mc_bd(bd, chroma, 0, tmp.ctypes.data, 0, sp0, st0, bh, mx0, my0, bw)
        w1, sp1, st1, bw, bh, mx1, my1 = src(1)
        (wx0, o0), (wx1, o1) = (wo(0), wo(1)) if wtd else ((0, 0), (0, 0))
        O.ffo_hevc_mc_w_bd(bd, chroma, 4 if wtd else 3, ffi.ptr(out), bw * ps, sp1, st1, ffi.ptr(tmp, ffi.i16p), bh, denom, wx0, wx1, o0 + o1,
                           mx1, my1, bw)
    else:
        l = pu["flags"] >> 1
        win, sp, st, bw, bh, mx, my = src(l)
        if wtd:
            wx, o = wo(l)
            O.ffo_hevc_mc_w_bd(bd, chroma, 2, ffi.ptr(out), bw * ps, sp, st, None, bh, denom, wx, 0, o, mx, my, bw)
        else:
            O.ffo_hevc_mc_bd(bd, chroma, 1, out.ctypes.data, bw * ps, sp, st, bh, mx, my, bw)
    return out.astype(np.int64)


def model(pic, pus=None, tus=None, planes=None):
    """the planes after inter reconstruction: every PU predicted (decoding order; PUs are disjoint), then every TU's residual added
    to the covered samples of its plane and clipped"""
    pus = pic.pus if pus is None else pus
    tus = pic.tus if tus is None else tus
    out = [pl.copy() for pl in (pic.planes if planes is None else planes)]
    for p in range(pic.nplanes):
        cov = np.zeros(out[p].shape, bool)
        for pu in pus:
            hs, vs = pic.hs[p], pic.vs[p]
            bx, by, bw, bh = pu["x"] >> hs, pu["y"] >> vs, pu["w"] >> hs, pu["h"] >> vs
            out[p][by:by + bh, bx:bx + bw] = predict_pu(pic, pu, p)
            cov[by:by + bh, bx:bx + bw] = True
        for t in tus[p]:
            if t["res_offset"] < 0:
                continue
            N = 1 << t["log2_size"]
            x, y = t["x"], t["y"]
            r = pic.res[p][t["res_offset"]:t["res_offset"] + N * N].astype(np.int64).reshape(N, N)
            blk = out[p][y:y + N, x:x + N]
            m = cov[y:y + N, x:x + N]
            blk[m] = np.clip(blk[m] + r[m], 0, pic.maxv)
    return out
