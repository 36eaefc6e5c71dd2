"""Synthetic HEVC pictures for the boundary-strength face (ffhip_hevc_boundary_strengths_pictures_dev / _host) and two independent
models of the rule include/ffhip.h states (H.265 8.7.2.3 / 8.7.2.4; restated, not checked against the reference's source).

The generator builds what a decoder holds after parsing a picture: tiles, slices (contiguous in tile-scan order) with their own
reference lists over a few DPB slots (the same slot under different ref_idx, different slots under the same ref_idx) and flag pairs;
per CTB a CU quadtree with intra and inter CUs, every partition mode (AMP included), transform trees to depth 2 with random luma
cbf; motion per PU drawn from a small pool and from earlier PUs (copied, lists swapped, MVs moved by 3 or 4 quarter samples, the
same picture in both lists), so that every branch of the motion rule occurs on real neighbours.  mvf is filled per PU, tu through
ffhip_hevc_bs_mark_tu.

Model A (model_a) is the per-segment rule, vectorised over the maps the face takes; it also names the rule that decided each
segment (the CLS_* classes).  Model B (model_b) is the decoder-order walk over the generator's TU list: per TU its left and top
sides, then every 8-sample line inside it by the motion rule only.  They share no code."""
import numpy as np

from ffmpeg_amd import hevc

PARTS = ("2Nx2N", "2NxN", "Nx2N", "NxN", "2NxnU", "2NxnD", "nLx2N", "nRx2N")

# what decided a segment (model A)
(CLS_OFF_GRID, CLS_DISABLED, CLS_SLICE, CLS_TILE, CLS_INTRA, CLS_CBF, CLS_MIXED, CLS_SLOTS, CLS_MV, CLS_EQUAL, CLS_BI1_0, CLS_BI1_1,
 CLS_BI2_0, CLS_BI2_1, CLS_BI3_0, CLS_BI3_1, CLS_BI_OTHER, CLS_BAD_SLICE, CLS_INTRA_INSIDE) = range(19)


def part_rects(part, x, y, s):
    h, q = s // 2, s // 4
    return {"2Nx2N": [(x, y, s, s)], "2NxN": [(x, y, s, h), (x, y + h, s, h)], "Nx2N": [(x, y, h, s), (x + h, y, h, s)],
            "NxN": [(x, y, h, h), (x + h, y, h, h), (x, y + h, h, h), (x + h, y + h, h, h)],
            "2NxnU": [(x, y, s, q), (x, y + q, s, s - q)], "2NxnD": [(x, y, s, s - q), (x, y + s - q, s, q)],
            "nLx2N": [(x, y, q, s), (x + q, y, s - q, s)], "nRx2N": [(x, y, s - q, s), (x + s - q, y, q, s)]}[part]


class BsPicture:
    """One generated picture.  mvf: (H / 4, W / 4) of hevc.BS_MVF_DTYPE; tu: the same grid, uint8; ctb_slice / ctb_tile: uint16 per
    raster CTB; slices: hevc.BS_SLICE_DTYPE table; across_tiles; tus: (x, y, log2, cbf, ctb) in decoding order; parts: the partition
    modes used."""

    def __init__(self, rng, width, height, log2_ctb, tiles=(1, 1), nslices=1, nslots=3, p_intra=0.25, across_tiles=None):
        assert width % 8 == 0 and height % 8 == 0
        self.rng, self.W, self.H, self.log2_ctb = rng, width, height, log2_ctb
        self.C = C_ = 1 << log2_ctb
        self.ctb_w, self.ctb_h = -(-width // C_), -(-height // C_)
        self.w4, self.h4 = width // 4, height // 4
        nctb = self.ctb_w * self.ctb_h
        # ---- tiles, tile scan, slices contiguous in tile scan ----
        cols, rows = self._bounds(self.ctb_w, tiles[0]), self._bounds(self.ctb_h, tiles[1])
        self.ctb_tile = np.zeros(nctb, np.uint16)
        scan = []
        for ty in range(len(rows) - 1):
            for tx in range(len(cols) - 1):
                for y in range(rows[ty], rows[ty + 1]):
                    for x in range(cols[tx], cols[tx + 1]):
                        self.ctb_tile[y * self.ctb_w + x] = ty * (len(cols) - 1) + tx
                        scan.append(y * self.ctb_w + x)
        self.across_tiles = bool(rng.integers(0, 2)) if across_tiles is None else bool(across_tiles)
        nslices = max(1, min(nslices, nctb))
        cuts = sorted(rng.choice(np.arange(1, nctb), nslices - 1, replace=False).tolist()) if nslices > 1 else []
        self.ctb_slice = np.zeros(nctb, np.uint16)
        for i, a in enumerate(scan):
            self.ctb_slice[a] = sum(1 for c in cuts if c <= i)
        self.slices = np.zeros(nslices, hevc.BS_SLICE_DTYPE)
        for s in self.slices:
            for l in range(2):
                n = int(rng.integers(2, 5))
                s["num_ref"][l] = n
                s["ref"][l][:n] = rng.integers(0, nslots, n)
                s["ref"][l][n:] = 200 + l                      # never read by a well-formed unit
            s["flags"] = (hevc.BS_SLICE_DEBLOCK_OFF if rng.random() < 0.2 else 0) | (hevc.BS_SLICE_ACROSS if rng.random() < 0.5 else 0)
        # ---- the MV pool: a base vector and neighbours 3 and 4 quarter samples away ----
        b = rng.integers(-60, 61, 2)
        self.pool = [tuple(int(v) for v in b + d) for d in ((0, 0), (3, 0), (4, 0), (0, -3), (0, 4), (3, 3), (-37, 22))]
        self.mvf = np.zeros((self.h4, self.w4), hevc.BS_MVF_DTYPE)
        self.tu = np.zeros((self.h4, self.w4), np.uint8)
        self.tus, self.parts, self._recent = [], set(), []
        for a in scan:
            cy, cx = divmod(a, self.ctb_w)
            self._slice = self.slices[self.ctb_slice[a]]
            self._ctb = a
            self._cu_tree(cx * C_, cy * C_, log2_ctb, p_intra)

    @staticmethod
    def _bounds(n, k):
        k = max(1, min(k, n))
        return [i * n // k for i in range(k + 1)]

    def _cu_tree(self, x, y, log2, p_intra):
        if x >= self.W or y >= self.H:
            return
        s = 1 << log2
        if log2 > 3 and (x + s > self.W or y + s > self.H or self.rng.random() < 0.5):
            for dy in (0, s // 2):
                for dx in (0, s // 2):
                    self._cu_tree(x + dx, y + dy, log2 - 1, p_intra)
            return
        rng = self.rng
        if rng.random() >= p_intra:
            part = PARTS[int(rng.integers(0, 8 if s >= 16 else 3))]
            self.parts.add(part)
            for k, (px, py, pw, ph) in enumerate(part_rects(part, x, y, s)):
                self.mvf[py // 4:(py + ph) // 4, px // 4:(px + pw) // 4] = self._motion(sibling=k > 0)
        # the transform tree: a 64-sample CU splits at once; two more levels at random, down to 4 x 4
        self._tu_tree(x, y, log2, 0)

    def _tu_tree(self, x, y, log2, depth):
        if log2 > 5 or (log2 > 2 and depth < 2 and self.rng.random() < 0.45):
            h = 1 << (log2 - 1)
            for dy in (0, h):
                for dx in (0, h):
                    self._tu_tree(x + dx, y + dy, log2 - 1, depth + (log2 <= 5))
            return
        cbf = int(self.rng.random() < 0.3)
        hevc.bs_mark_tu(self.tu, x, y, log2, cbf)
        self.tus.append((x, y, log2, cbf, self._ctb))

    def _ref_idx(self, l, slot):
        """a ref_idx of the current slice's list l that names DPB slot `slot`, or None"""
        n = int(self._slice["num_ref"][l])
        hits = [i for i in range(n) if self._slice["ref"][l][i] == slot]
        return hits[int(self.rng.integers(0, len(hits)))] if hits else None

    def _motion(self, sibling=False):
        """one PU's mvf record: from the pool, or derived from a recent PU's (slot, mv) pairs (sibling: mostly from the PU just
        before it, its neighbour inside the CU)"""
        rng, S = self.rng, self._slice
        pick = lambda: self.pool[int(rng.integers(0, len(self.pool)))]
        mot = None                                                   # [(slot, mv) or None per list]
        if self._recent and rng.random() < 0.6:
            m = list(self._recent[-1 if sibling and rng.random() < 0.7 else int(rng.integers(0, len(self._recent)))])
            k = rng.random()
            if k < 0.5:
                m = [m[1], m[0]]                                     # lists swapped
            elif k < 0.75:
                d = [(3, 0), (4, 0), (0, 3), (0, -4)][int(rng.integers(0, 4))]
                l = int(rng.integers(0, 2))
                if m[l]:
                    m[l] = (m[l][0], (m[l][1][0] + d[0], m[l][1][1] + d[1]))
            mot = m
        if mot is None:
            kind = int(rng.integers(1, 5)) % 4 or 3                  # bi-prediction twice as often
            mot = [None, None]
            for l in range(2):
                if kind >> l & 1:
                    mot[l] = (int(S["ref"][l][int(rng.integers(0, S["num_ref"][l]))]), pick())
            if kind == 3 and rng.random() < 0.4:
                mot[1] = (mot[0][0], mot[1][1])                      # the same picture in both lists, if list 1 has it
        rec = np.zeros((), hevc.BS_MVF_DTYPE)
        final = [None, None]
        for l in range(2):
            if mot[l] is None:
                continue
            ri = self._ref_idx(l, mot[l][0])
            if ri is None:                                           # this slice's list does not hold the slot: any of its own
                ri = int(rng.integers(0, S["num_ref"][l]))
            rec["pred_flag"] |= 1 << l
            rec["ref_idx"][l] = ri
            rec["mv"][l] = mot[l][1]
            final[l] = (int(S["ref"][l][ri]), mot[l][1])
        if not rec["pred_flag"]:
            return self._motion(sibling)
        for l in range(2):                                           # the unused list holds noise the rule must not read
            if final[l] is None:
                rec["ref_idx"][l] = -1
                rec["mv"][l] = rng.integers(-500, 500, 2)
        self._recent = (self._recent + [tuple(final)])[-6:]
        return rec

    def maps(self, pad=0, guard=0x5A):
        """the face's arguments as numpy arrays (strides `pad` entries wider than the picture): a dict for
        hevc.boundary_strengths_pictures_host(), with the outputs filled with `guard`"""
        mvf = np.zeros((self.h4, self.w4 + pad), hevc.BS_MVF_DTYPE)
        mvf[:, :self.w4] = self.mvf
        tu = np.zeros((self.h4, self.w4 + pad), np.uint8)
        tu[:, :self.w4] = self.tu
        out = lambda: np.full((self.h4 + 2, self.w4 + pad), guard, np.uint8)   # a guard row above and below
        ver, hor = out(), out()
        return dict(mvf=mvf, tu=tu, ctb_slice=self.ctb_slice, ctb_tile=self.ctb_tile if self.ctb_tile.any() else None, slices=self.slices,
                    bs_ver=ver[1:], bs_hor=hor[1:], _ver=ver, _hor=hor, mvf_stride=self.w4 + pad, tu_stride=self.w4 + pad,
                    bs_stride=self.w4 + pad, nslices=len(self.slices), loop_filter_across_tiles=self.across_tiles)


# ================================================================================================================================
# model A: the per-segment rule, vectorised over the maps the face takes
# ================================================================================================================================
def model_a(mvf, tu, ctb_slice, ctb_tile, slices, across_tiles, log2_ctb):
    """(bs_ver, bs_hor, cls_ver, cls_hor) of (h4, w4) maps.  mvf: BS_MVF_DTYPE (h4, w4); tu: uint8; ctb_slice / ctb_tile: per raster
    CTB (ctb_tile may be None); slices: BS_SLICE_DTYPE table."""
    h4, w4 = tu.shape
    lu = log2_ctb - 2
    ctb_w = -(-w4 // (1 << lu))
    uy, ux = np.mgrid[0:h4, 0:w4]
    ctb = (uy >> lu) * ctb_w + (ux >> lu)
    sl = np.asarray(ctb_slice, np.int64)[ctb]
    tile = np.asarray(ctb_tile, np.int64)[ctb] if ctb_tile is not None else np.zeros_like(sl)
    ok = sl < len(slices)
    sl_c = np.where(ok, sl, 0)
    flags = np.where(ok, slices["flags"].astype(np.int64)[sl_c], 0)
    pred = mvf["pred_flag"].astype(np.int64)
    pred = np.where(pred > 3, 0, pred)
    # the picture each list names: a DPB slot, or -1 for one "different from every other"
    pic = []
    for l in range(2):
        ri = mvf["ref_idx"][..., l].astype(np.int64)
        n = slices["num_ref"].astype(np.int64)[sl_c, l]
        good = ok & ((pred >> l & 1) == 1) & (ri >= 0) & (ri < n) & (n <= 16)
        pic.append(np.where(good, slices["ref"].astype(np.int64)[sl_c, l, np.clip(ri, 0, 15)], -1))
    mv = mvf["mv"].astype(np.int64)
    cbf = (tu >> 2 & 1).astype(bool)
    out = []
    for d in range(2):
        sh = (lambda a: np.roll(a, 1, axis=1)) if d == 0 else (lambda a: np.roll(a, 1, axis=0))      # the p side of every unit
        u = ux if d == 0 else uy
        on = (u > 0) & (u % 2 == 0)
        same = lambda a, b: (a == b) & (a >= 0)
        far = lambda a, b: (np.abs(a[..., 0] - b[..., 0]) >= 4) | (np.abs(a[..., 1] - b[..., 1]) >= 4)
        qp, pp = pred, sh(pred)
        A0, A1, B0, B1 = pic[0], pic[1], sh(pic[0]), sh(pic[1])
        a0, a1, b0, b1 = mv[:, :, 0], mv[:, :, 1], sh(mv[:, :, 0]), sh(mv[:, :, 1])
        d00, d11, d10, d01 = far(b0, a0), far(b1, a1), far(b1, a0), far(b0, a1)
        bi = (qp == 3) & (pp == 3)
        c1 = same(A0, B0) & same(A0, A1) & same(B0, B1)
        c2 = ~c1 & same(A0, B0) & same(A1, B1)
        c3 = ~c1 & ~c2 & same(A0, B1) & same(A1, B0)
        r1, r2, r3 = (d00 | d11) & (d10 | d01), d00 | d11, d10 | d01
        uni = ((qp == 1) | (qp == 2)) & ((pp == 1) | (pp == 2))
        qs, ps_ = np.where(qp == 1, A0, A1), np.where(pp == 1, B0, B1)
        qm = np.where((qp == 1)[..., None], a0, a1)
        pm = np.where((pp == 1)[..., None], b0, b1)
        uslots = ~same(qs, ps_)
        umv = far(pm, qm)
        intra_one = (qp == 0) ^ (pp == 0)
        intra_both = (qp == 0) & (pp == 0)
        # rule 6, then the earlier rules written over it in reverse order
        cls = np.full((h4, w4), CLS_MIXED, np.int64)                 # one bi, one uni
        bs = np.ones((h4, w4), np.int64)
        def put(mask, value, c):
            bs[mask] = value[mask] if isinstance(value, np.ndarray) else value
            cls[mask] = c[mask] if isinstance(c, np.ndarray) else c
        put(uni, np.where(uslots | umv, 1, 0), np.where(uslots, CLS_SLOTS, np.where(umv, CLS_MV, CLS_EQUAL)))
        put(bi, 1, CLS_BI_OTHER)
        put(bi & c3, r3.astype(np.int64), np.where(r3, CLS_BI3_1, CLS_BI3_0))
        put(bi & c2, r2.astype(np.int64), np.where(r2, CLS_BI2_1, CLS_BI2_0))
        put(bi & c1, r1.astype(np.int64), np.where(r1, CLS_BI1_1, CLS_BI1_0))
        put(intra_one, 2, CLS_INTRA)
        put(intra_both, 0, CLS_INTRA_INSIDE)
        edge = (tu >> d & 1).astype(bool)
        put(edge & (cbf | sh(cbf)), 1, CLS_CBF)
        put(edge & ((qp == 0) | (pp == 0)), 2, CLS_INTRA)
        put((tile != sh(tile)) & (not across_tiles), 0, CLS_TILE)
        put((sl != sh(sl)) & ((flags & 2) == 0), 0, CLS_SLICE)
        put((flags & 1) == 1, 0, CLS_DISABLED)
        put(~ok, 0, CLS_BAD_SLICE)
        put(~on, 0, CLS_OFF_GRID)
        out.append((bs.astype(np.uint8), cls))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def model_a_of(pic):
    return model_a(pic.mvf, pic.tu, pic.ctb_slice, pic.ctb_tile, pic.slices, pic.across_tiles, pic.log2_ctb)


# ================================================================================================================================
# model B: the decoder-order walk, per transform unit
# ================================================================================================================================
def _b_motion(cur, nb):
    """cur / nb: (pred_flag, [picture of L0, of L1], [mv of L0, of L1]) of two inter or intra units"""
    def apart(m, n):
        return abs(m[0] - n[0]) >= 4 or abs(m[1] - n[1]) >= 4
    if cur[0] == 0 and nb[0] == 0:
        return 0
    if cur[0] == 0 or nb[0] == 0:
        return 2
    if cur[0] == 3 and nb[0] == 3:
        (A0, A1), (B0, B1) = cur[1], nb[1]
        if A0 == B0 and A0 == A1 and B0 == B1:
            if (apart(nb[2][0], cur[2][0]) or apart(nb[2][1], cur[2][1])) and (apart(nb[2][1], cur[2][0]) or apart(nb[2][0], cur[2][1])):
                return 1
            return 0
        if A0 == B0 and A1 == B1:
            return int(apart(nb[2][0], cur[2][0]) or apart(nb[2][1], cur[2][1]))
        if A0 == B1 and A1 == B0:
            return int(apart(nb[2][1], cur[2][0]) or apart(nb[2][0], cur[2][1]))
        return 1
    if cur[0] == 3 or nb[0] == 3:
        return 1
    lc, ln = cur[0] - 1, nb[0] - 1                                  # pred_flag 1 -> list 0, 2 -> list 1
    if cur[1][lc] != nb[1][ln]:
        return 1
    return int(apart(cur[2][lc], nb[2][ln]))


def model_b(pic):
    """(bs_ver, bs_hor) by visiting pic.tus in decoding order.  For well-formed pictures (the generator's)."""
    ver = np.zeros((pic.h4, pic.w4), np.uint8)
    hor = np.zeros((pic.h4, pic.w4), np.uint8)
    cbf_done = np.zeros((pic.h4, pic.w4), bool)                      # luma cbf of the TUs decoded so far
    lc = pic.log2_ctb

    def unit(x4, y4):
        f = pic.mvf[y4, x4]
        S = pic.slices[pic.ctb_slice[(y4 * 4 >> lc) * pic.ctb_w + (x4 * 4 >> lc)]]
        pf = int(f["pred_flag"])
        pics = [int(S["ref"][l][f["ref_idx"][l]]) if pf >> l & 1 else None for l in range(2)]
        return pf, pics, [tuple(int(v) for v in f["mv"][l]) for l in range(2)]

    for x0, y0, log2, cbf, ctb in pic.tus:
        n4 = 1 << (log2 - 2)
        bx, by = x0 // 4, y0 // 4
        cbf_done[by:by + n4, bx:bx + n4] = bool(cbf)
        sl = pic.slices[pic.ctb_slice[ctb]]
        if sl["flags"] & 1:
            continue
        for vertical, out in ((True, ver), (False, hor)):
            across = x0 if vertical else y0
            # the TU's own side
            if across > 0 and across % 8 == 0:
                nx, ny = (x0 - 1, y0) if vertical else (x0, y0 - 1)
                nctb = (ny >> lc) * pic.ctb_w + (nx >> lc)
                allowed = True
                if pic.ctb_slice[nctb] != pic.ctb_slice[ctb] and not sl["flags"] & 2:
                    allowed = False
                if pic.ctb_tile[nctb] != pic.ctb_tile[ctb] and not pic.across_tiles:
                    allowed = False
                if allowed:
                    for i in range(n4):
                        qx, qy = (bx, by + i) if vertical else (bx + i, by)
                        px, py = (qx - 1, qy) if vertical else (qx, qy - 1)
                        cur, nb = unit(qx, qy), unit(px, py)
                        if cur[0] == 0 or nb[0] == 0:
                            v = 2
                        elif cbf or cbf_done[py, px]:
                            v = 1
                        else:
                            v = _b_motion(cur, nb)
                        out[qy, qx] = v
            # the 8-sample lines inside the TU: prediction-block edges, if any
            for k in range(2, n4, 2):                                # a TU of 16 samples or more starts on the 8-sample grid
                for i in range(n4):
                    qx, qy = (bx + k, by + i) if vertical else (bx + i, by + k)
                    px, py = (qx - 1, qy) if vertical else (qx, qy - 1)
                    out[qy, qx] = _b_motion(unit(qx, qy), unit(px, py))
    return ver, hor


# ================================================================================================================================
# the picture set of the CPU and GPU tiers: (width, height, log2_ctb, tiles, nslices, npics)
# ================================================================================================================================
SET = [(8, 8, 4, (1, 1), 1, 1), (16, 8, 5, (1, 1), 1, 1), (8, 24, 6, (1, 1), 1, 1), (24, 40, 4, (2, 2), 3, 3), (72, 56, 4, (3, 2), 4, 17),
       (136, 88, 5, (2, 2), 3, 3), (200, 136, 6, (2, 1), 2, 1), (264, 200, 6, (3, 2), 4, 3), (416, 240, 5, (3, 2), 4, 3),
       (640, 360, 4, (3, 2), 4, 1), (1920, 1080, 6, (3, 2), 4, 1)]
_SETS = {}


def picture_set(i):
    """the pictures of SET[i], generated once per process from a seed of their own"""
    if i not in _SETS:
        W, H, lc, tiles, ns, n = SET[i]
        rng = np.random.default_rng(9100 + i)
        _SETS[i] = [BsPicture(rng, W, H, lc, tiles=tiles, nslices=1 + (ns - 1 + k) % ns if n > 1 else ns) for k in range(n)]
    return _SETS[i]
