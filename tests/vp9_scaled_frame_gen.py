"""Synthetic VP9 inter frames with references of another size for ffhip_vp9_inter_frames_scaled_dev, and a sequential model of it.

ScaledFrame is vp9_inter_frame_gen.InterFrame with each reference at a size of its own (ref_sizes, luma).  A block takes the SCALED
template when its first reference is scaled, or it is compound and its second one is (inter_recon); its records then come from
block_preds_scaled(), a restatement of that template (the 4x4 branch for every sub-8x8 block, MVs copied as decode_mode does for
8x4 / 4x8).  The model follows mc_luma_scaled / mc_chroma_scaled: the MV clipped to the call's box, the scaled origin and phase, a
window of the reference gathered with coordinates clamped to its real size (what emulated_edge_mc gives), then the oracle's
ffo_vp9_smc_bd; calls from a reference of the frame's size, and records of the unscaled template, take vp9_inter_frame_gen's route.
The TUs follow as vp9_inter_frame_gen.model.  route="pad" is the second path: ffo_vp9_smc_bd / ffo_vp9_mc_bd straight on references
padded with np.pad(mode="edge"), valid while every window stays inside the border."""
import ctypes as C

import numpy as np

import ffi
import vp9_inter_frame_gen as G

SCALED = 4
BORDER = 200          # the MV clip keeps a scaled window within ~150 samples of a 2x reference; unscaled windows need near MVs


def ref_scale(W, H, rw, rh):
    """vp9.c: (scale[2], step[2]) of a reference, scale 0 when it has the frame's size"""
    if (rw, rh) == (W, H):
        return (0, 0), (0, 0)
    assert 2 * W >= rw and 2 * H >= rh and W <= 16 * rw and H <= 16 * rh, "reference size outside the 2x / 16x limits"
    sc = ((rw << 14) // W, (rh << 14) // H)
    return sc, ((16 * sc[0]) >> 14, (16 * sc[1]) >> 14)


def block_preds_scaled(bs, row, col, mv, comp, ref, filt, ss_h, ss_v):
    """a restatement of vp9_mc_template.h's SCALED instantiation for one block: record dicts with 'box' (px, py, pw, ph)"""
    out = []
    nr = 2 if comp else 1

    def emit(chroma, x, y, w, h, box, pick):
        mvs, refs = [[0, 0], [0, 0]], [0, 0]
        for r in range(nr):
            mvs[r] = [int(v) for v in pick(r)]
            refs[r] = int(ref[r])
        px, py, pw, ph = box
        out.append(dict(x=x, y=y, w=w, h=h, filter=filt, flags=(1 if comp else 0) | (2 if chroma else 0) | SCALED, ref=refs, mv=mvs,
                        box=[px | py << 4, (pw.bit_length() - 1) | (ph.bit_length() - 1) << 4]))

    sub = lambda s: (lambda r: mv[s][r])
    d2 = lambda a, b: (lambda r: G._div2(mv[a][r], mv[b][r]))
    ly, lx, cy, cx = row << 3, col << 3, row << (3 - ss_v), col << (3 - ss_h)
    if bs < 10:
        w, h = G.BS_DIMS[bs]
        emit(False, lx, ly, w, h, (0, 0, w, h), sub(0))
        emit(True, cx, cy, w >> ss_h, h >> ss_v, (0, 0, w >> ss_h, h >> ss_v), sub(0))
        return out
    for s, (dx, dy) in enumerate(((0, 0), (4, 0), (0, 4), (4, 4))):
        emit(False, lx + dx, ly + dy, 4, 4, (dx, dy, 8, 8), sub(s))
    cw, ch = 8 >> ss_h, 8 >> ss_v
    if ss_h and ss_v:
        emit(True, cx, cy, 4, 4, (0, 0, 4, 4), lambda r: G._div4(mv[0][r], mv[1][r], mv[2][r], mv[3][r]))
    elif ss_v:
        emit(True, cx, cy, 4, 4, (0, 0, cw, ch), d2(0, 2))
        emit(True, cx + 4, cy, 4, 4, (4, 0, cw, ch), d2(1, 3))
    elif ss_h:
        emit(True, cx, cy, 4, 4, (0, 0, cw, ch), d2(0, 1))
        emit(True, cx, cy + 4, 4, 4, (0, 4, cw, ch), d2(1, 2))
    else:
        for s, (dx, dy) in enumerate(((0, 0), (4, 0), (0, 4), (4, 4))):
            emit(True, cx + dx, cy + dy, 4, 4, (dx, dy, cw, ch), sub(s))
    return out


class ScaledFrame(G.InterFrame):
    """An InterFrame whose references have the luma sizes ref_sizes (one per reference).  scale[r], step[r] per reference; records
    carry 'box' ([0, 0] for the unscaled template)."""

    def __init__(self, rng, width, height, bd, ss_h, ss_v, ref_sizes, **kw):
        self.ref_sizes = [tuple(int(v) for v in s) for s in ref_sizes]
        self.scale, self.step = zip(*[ref_scale(width, height, rw, rh) for rw, rh in self.ref_sizes])
        self.rng, self.maxv = rng, (1 << bd) - 1
        refs = [[self._content(((rh + (ss_v if p else 0)) >> (ss_v if p else 0), (rw + (ss_h if p else 0)) >> (ss_h if p else 0)))
                 for p in range(3)] for rw, rh in self.ref_sizes]
        super().__init__(rng, width, height, bd, ss_h, ss_v, refs=refs, **kw)

    def scaled(self, r):
        return self.scale[r] != (0, 0)

    def _block(self, sb, bs, row, col):
        rng = self.rng
        w, h = G.BS_DIMS[bs]
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
            mv = [mv[0]] * 4
        elif bs == 10:                                   # decode_mode: 8x4 copies mv[0] to [1] and mv[2] to [3]
            mv = [mv[0], mv[0], mv[2], mv[2]]
        elif bs == 11:                                   # 4x8: mv[0] to [2], mv[1] to [3]
            mv = [mv[0], mv[1], mv[0], mv[1]]
        if self.scaled(ref[0]) or (comp and self.scaled(ref[1])):
            recs = block_preds_scaled(bs, row, col, mv, comp, ref, filt, self.ss_h, self.ss_v)
        else:
            recs = G.block_preds(bs, row, col, mv, comp, ref, filt, self.ss_h, self.ss_v)
            for rec in recs:
                rec["box"] = [0, 0]
        for rec in recs:
            rec["sb"] = sb
            self.preds.append(rec)
        if rng.random() < self.p_skip:
            return
        self._tus(sb, bs, row, col)


PRED_FIELDS = G.PRED_FIELDS + ("box",)


# ---- the model ----
def scaled_geometry(fr, rec, p, r):
    """(x', y', mx & 15, my & 15, dx, dy) of a SCALED-template record in plane p from its scaled reference r: mc_luma_scaled /
    mc_chroma_scaled (vp9recon.c)"""
    ri = rec["ref"][r]
    sc, st = fr.scale[ri], fr.step[ri]
    smv = lambda n, d: (n * sc[d]) >> 14
    b0, b1 = rec["box"]
    px, py, pw, ph = b0 & 15, b0 >> 4, 1 << (b1 & 15), 1 << (b1 >> 4)
    x, y = rec["x"], rec["y"]
    clip = lambda v, lo, hi: min(max(v, lo), hi)
    pos = []
    for d, (c, o, bsz, n, sub, v) in enumerate(((x, px, pw, fr.cols, fr.hs[p], rec["mv"][r][0]),
                                                (y, py, ph, fr.rows, fr.vs[p], rec["mv"][r][1]))):
        if sub:
            m = clip(v, -(c + bsz - o + 4) * 16, (n * 4 - c + o + 3) * 16)
            pos.append(smv(m, d) + (smv(c * 16, d) & ~15) + (smv(c * 32, d) & 15))
        else:
            m = clip(v, -(c + bsz - o + 4) * 8, (n * 8 - c + o + 3) * 8)
            pos.append(smv(m * 2, d) + smv(c * 16, d))
    return pos[0] >> 4, pos[1] >> 4, pos[0] & 15, pos[1] & 15, st[0], st[1]


_PADDED = {}


def padded(ref, dt):
    key = (id(ref), dt)
    if key not in _PADDED or _PADDED[key][0] is not ref:
        _PADDED[key] = (ref, np.ascontiguousarray(np.pad(ref, BORDER, mode="edge").astype(dt)))
    return _PADDED[key][1]


def _source(ref, dt, route, xi, yi, x_hi, y_hi):
    """(array, byte offset of sample (xi, yi), stride in bytes) reading rows yi - 3 .. y_hi and columns xi - 3 .. x_hi"""
    ps = np.dtype(dt).itemsize
    if route == "clamp":
        H, W = ref.shape
        ys = np.clip(np.arange(yi - 3, y_hi + 1), 0, H - 1)
        xs = np.clip(np.arange(xi - 3, x_hi + 1), 0, W - 1)
        win = np.ascontiguousarray(ref[np.ix_(ys, xs)].astype(dt))
        return win, (3 * win.shape[1] + 3) * ps, win.shape[1] * ps
    assert xi - 3 >= -BORDER and yi - 3 >= -BORDER and x_hi < ref.shape[1] + BORDER and y_hi < ref.shape[0] + BORDER, \
        "window outside the border"
    pad = padded(ref, dt)
    return pad, ((yi + BORDER) * pad.shape[1] + xi + BORDER) * ps, pad.shape[1] * ps


def predict(fr, rec, p, route="clamp"):
    """one record in plane p: per reference, put then avg, each call by the scaled rule when the record is of the SCALED template and
    that reference is scaled, by the unscaled rule otherwise"""
    O = G._oracle()
    dt = np.uint8 if fr.bd == 8 else np.uint16
    w, h = rec["w"], rec["h"]
    out = np.zeros((h, w), dt)
    op = ffi.ptr(out)
    ps = np.dtype(dt).itemsize
    for r in range(2 if rec["flags"] & 1 else 1):
        ri = rec["ref"][r]
        ref = fr.refs[ri][p]
        if rec["flags"] & SCALED and fr.scaled(ri):
            xi, yi, mx, my, dx, dy = scaled_geometry(fr, rec, p, r)
            x_hi, y_hi = xi + (((w - 1) * dx + mx) >> 4) + 4, yi + (((h - 1) * dy + my) >> 4) + 4
            src, at, st = _source(ref, dt, route, xi, yi, x_hi, y_hi)
            O.ffo_vp9_smc_bd(fr.bd, rec["filter"], r, op, w * ps, C.cast(src.ctypes.data + at, ffi.u8p), st, w, h, mx, my, dx, dy)
        else:
            xi, yi, mx, my = G.rec_geometry(fr, rec, p, r)
            src, at, st = _source(ref, dt, route, xi, yi, xi + w + 4, yi + h + 4)
            O.ffo_vp9_mc_bd(fr.bd, rec["filter"], r, op, w * ps, C.cast(src.ctypes.data + at, ffi.u8p), st, w, h, mx, my)
    return out.astype(np.int64)


def model(fr, preds=None, tus=None, planes=None, route="clamp"):
    """vp9_inter_frame_gen.model with this module's predict: every record of a plane predicted, the TUs added to the covered samples,
    the covered samples inside the decoded area written"""
    preds = fr.preds if preds is None else preds
    tus = fr.tus if tus is None else tus
    src = fr.planes if planes is None else planes
    out = [pl.copy() for pl in src]
    for p in range(3):
        Cw, Ch = 64 >> fr.hs[p], 64 >> fr.vs[p]
        canvas = np.zeros((fr.sb_h * Ch, fr.sb_w * Cw), np.int64)
        cov = np.zeros(canvas.shape, bool)
        for rec in preds:
            if (rec["flags"] >> 1) & 1 != int(p > 0):
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
            new = G.tu_add(fr, t, blk.copy(), p)
            blk[m] = new[m]
        dh, dw = fr.dh[p], fr.dw[p]
        c = cov[:dh, :dw]
        out[p][:dh, :dw][c] = canvas[:dh, :dw][c]
    return out


#: (frame size, reference sizes): both limits (2:1 down, 1:16 up), 3:2, 2:3, unequal horizontal and vertical ratios, odd sizes, and
#: a reference of the frame's size beside a scaled one
RATIOS = [
    ((64, 48), [(128, 96)]),                 # 2x down, the LDS-heavy end
    ((128, 96), [(8, 6)]),                   # 16x up
    ((96, 64), [(144, 96), (96, 64)]),       # 3:2 and unscaled
    ((120, 84), [(80, 56)]),                 # 2:3
    ((100, 70), [(150, 47), (61, 139)]),     # unequal ratios, odd sizes
    ((77, 53), [(111, 77), (77, 53), (39, 27)]),
]
