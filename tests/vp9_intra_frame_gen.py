"""Synthetic VP9 frames for the intra reconstruction face (ffhip_vp9_intra_frames_dev) and a sequential model of it.

The generator builds what a decoder holds when the intra stage runs.  Keyframes take the superblock partition of vp9_inter_frame_gen
(forced splits at the frame's edges, sub-8x8 blocks) with every block intra: all ten coded modes (four per sub-8x8 block), every tx
the block allows and the uvtx that follows from it, skip, eob 1 (dc only), random coefficients, lossless frames and tile columns.
Inter frames are an InterFrame whose inter model output fills the planes; its intra holes become the records.  Frame sizes need not
be multiples of 8 or 64, and the planes start as random garbage: what no record covers must survive.

The model (model()) runs the records of each plane in decoding order with the plane-coordinate rules of include/ffhip.h (availability,
check_intra_mode's mode conversion, the edge clamps and substitutes), builds each block's left / top edge lines on the host from the
plane as reconstructed so far, and calls the oracle's ffo_vp9_intra_pred_bd and ffo_vp9_itxfm_add_bd (ffo_vp9_itxfm_add at 8 bits);
the block's samples inside the decoded area are written back.

The pointer form (pointer_model()) is the second route: the decoder's own intra_recon / check_intra_mode transcribed with frame
buffers, overhang buffers and intra_pred_data, from the decoded blocks (IntraFrame.decoded) rather than the records.  Its equality
with model() is the evidence that the plane-coordinate restatement is right."""
import ctypes as C

import numpy as np

import ffi
import vp9_inter_frame_gen as vg

BS_DIMS = vg.BS_DIMS
#: ff_vp9_bwh_tab[1] (libavcodec/vp9data.c) in 8-sample units: sub-8x8 blocks count as 8x8
BWH8 = [(8, 8), (8, 4), (4, 8), (4, 4), (4, 2), (2, 4), (2, 2), (2, 1), (1, 2), (1, 1), (1, 1), (1, 1), (1, 1)]
#: ff_vp9_intra_txfm_type[coded mode]
INTRA_TXFM_TYPE = [2, 1, 0, 0, 3, 2, 1, 2, 1, 3]
REC_FIELDS = ("x", "y", "coeff_offset", "tx", "mode", "txtp", "flags")
RESIDUAL, DC_ONLY, HAVE_RIGHT = 1, 2, 4

# check_intra_mode's mode_conv[mode][have_left][have_top]
VERT, HOR, DC, DDL, DDR, VR, HD, VL, HU, TM, LEFT_DC, TOP_DC, DC_128, DC_127, DC_129 = range(15)
MODE_CONV = [
    [[DC_127, VERT], [DC_127, VERT]],
    [[DC_129, DC_129], [HOR, HOR]],
    [[DC_128, TOP_DC], [LEFT_DC, DC]],
    [[DC_127, DDL], [DC_127, DDL]],
    [[DDR, DDR], [DDR, DDR]],
    [[VR, VR], [VR, VR]],
    [[HD, HD], [HD, HD]],
    [[DC_127, VL], [DC_127, VL]],
    [[DC_129, DC_129], [HU, HU]],
    [[DC_129, VERT], [HOR, TM]],
]


def block_records(plane, bs, tx, row, col, mode, skip, eob, lossless, cols, rows, ss_h, ss_v):
    """a restatement of intra_recon's loops for one block in one plane: record dicts (REC_FIELDS) with coeff_offset = 16 n"""
    hs, vs = (ss_h, ss_v) if plane else (0, 0)
    bw, bh = BWH8[bs]
    w4, h4 = (bw << 1) >> hs, (bh << 1) >> vs
    end_x, end_y = min(2 * (cols - col), bw << 1) >> hs, min(2 * (rows - row), bh << 1) >> vs
    step1d, step = 1 << tx, 1 << (2 * tx)
    x0, y0 = (col * 8) >> hs, (row * 8) >> vs
    out, n = [], 0
    for y in range(0, end_y, step1d):
        for x in range(0, end_x, step1d):
            m = int(mode[y * 2 + x if (plane == 0 and bs > 9 and tx == 0) else 0])
            e = 0 if skip else int(eob[n])
            out.append(dict(x=x0 + 4 * x, y=y0 + 4 * y, coeff_offset=16 * n, tx=4 if lossless else tx, mode=m,
                            txtp=INTRA_TXFM_TYPE[m] if plane == 0 else 0,
                            flags=(RESIDUAL if e else 0) | (DC_ONLY if e == 1 else 0) | (HAVE_RIGHT if x < w4 - 1 else 0)))
            n += step
    return out


def tile_starts(sb_w, log2_tile_cols):
    """set_tile_offset (vp9.c): the first superblock column of each tile column"""
    return [min((i * sb_w) >> log2_tile_cols, sb_w) for i in range(1 << log2_tile_cols)]


class IntraFrame:
    """One generated frame: planes[p] (decoded area, int64) at launch, recs[p] record dicts in decoding order (plus 'sb'),
    coeffs[p] int32 coefficients, log2_tile_cols; inter: the InterFrame it came from (its intra holes are the records)."""

    def __init__(self, rng, width, height, bd, ss_h, ss_v, lossless=False, log2_tile_cols=0, inter=False, p_skip=0.2, p_intra=0.05,
                 min_log2=2, modes=None):
        self.rng, self.W, self.H, self.bd, self.ss_h, self.ss_v = rng, width, height, bd, ss_h, ss_v
        self.lossless, self.log2_tile_cols = lossless, log2_tile_cols
        self.p_skip, self.modes = p_skip, modes
        if inter:
            fr = vg.InterFrame(rng, width, height, bd, ss_h, ss_v, p_intra=p_intra, min_log2=min_log2, lossless=lossless)
            self.planes = vg.model(fr)
        else:
            fr = vg.InterFrame(rng, width, height, bd, ss_h, ss_v, refs=[], p_intra=1.0, min_log2=min_log2)
            self.planes = [pl.copy() for pl in fr.planes]
        self.inter = fr
        self.cols, self.rows, self.sb_w, self.sb_h = fr.cols, fr.rows, fr.sb_w, fr.sb_h
        self.hs, self.vs, self.dw, self.dh, self.maxv = fr.hs, fr.vs, fr.dw, fr.dh, fr.maxv
        self.recs, self._co = [[], [], []], [[], [], []]
        self._nco = [0, 0, 0]
        self.decoded = []   # per intra block, what the decoder holds for intra_recon (pointer_model's input)
        for bs, row, col, kind in fr.blocks:
            if kind == "intra":
                self._block(bs, row, col)
        self.coeffs = [np.concatenate(c).astype(np.int32) if c else np.zeros(16, np.int32) for c in self._co]

    def _mode(self):
        return int(self.rng.integers(0, 10)) if self.modes is None else int(self.rng.choice(self.modes))

    def _block(self, bs, row, col):
        rng = self.rng
        w, h = BS_DIMS[bs]
        sb = (row >> 3) * self.sb_w + (col >> 3)
        maxtx = 0 if bs > 9 else min(3, int(np.log2(min(w, h))) - 2)
        tx = 0 if self.lossless else int(rng.integers(0, maxtx + 1))
        w8, h8 = max(w, 8), max(h, 8)
        uvw, uvh = max(4, w8 >> self.ss_h), max(4, h8 >> self.ss_v)
        uvtx = 0 if self.lossless else min(tx, int(np.log2(min(uvw, uvh))) - 2)
        skip = rng.random() < self.p_skip
        mode = [self._mode() for _ in range(4)]
        uvmode = self._mode()
        blk = dict(bs=bs, row=row, col=col, tx=tx, uvtx=uvtx, mode=mode, uvmode=uvmode, skip=skip, eob=[], base=[])
        self.decoded.append(blk)
        for p in range(3):
            t = tx if p == 0 else uvtx
            N = 4 << t
            eob = rng.choice([0, 1, 2, N * N], 256).tolist()
            recs = block_records(p, bs, t, row, col, mode if p == 0 else [uvmode], skip, eob, self.lossless, self.cols, self.rows,
                                 self.ss_h, self.ss_v)
            hs, vs = self.hs[p], self.vs[p]
            area = max(1, (BWH8[bs][0] * 8 >> hs) * (BWH8[bs][1] * 8 >> vs))
            base = self._nco[p]
            blk["eob"].append(eob)
            blk["base"].append(base)
            co = np.zeros(max(area, max([r["coeff_offset"] for r in recs] + [0]) + N * N), np.int64)
            for r in recs:
                if r["flags"] & RESIDUAL:
                    o = r["coeff_offset"]
                    if r["flags"] & DC_ONLY:
                        co[o] = rng.integers(-(1 << (self.bd + 2)), 1 << (self.bd + 2))
                    else:
                        k = int(rng.integers(1, min(N * N, 40) + 1))
                        amp = 1 << (self.bd + (3 if rng.random() < 0.2 else 0))
                        pos = rng.integers(0, min(N * N, 64), k)
                        co[o + pos] = rng.integers(-amp, amp + 1, k)
                r["coeff_offset"] += base
                r["sb"] = sb
                self.recs[p].append(r)
            lim = 32767 if self.bd == 8 else (1 << 20)
            self._co[p].append(np.clip(co, -lim, lim))
            self._nco[p] += len(co)

    def pack(self, p, recs=None):
        """(records of plane p sorted by raster superblock, decoding order kept within one, as a structured array; int32 superblock
        starts)"""
        dtype = np.dtype([("x", np.uint16), ("y", np.uint16), ("coeff_offset", np.int32), ("tx", np.uint8), ("mode", np.uint8),
                          ("txtp", np.uint8), ("flags", np.uint8)])
        recs = self.recs[p] if recs is None else recs
        nsb = self.sb_w * self.sb_h
        idx = sorted(range(len(recs)), key=lambda i: recs[i]["sb"])        # stable: decoding order within a superblock
        arr = np.zeros(len(recs), dtype)
        for j, i in enumerate(idx):
            for f in REC_FIELDS:
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


def well_formed(fr, p, r):
    """the kernel's record checks (include/ffhip.h); r carries 'sb'"""
    tx, mode, txtp, fl, x, y = r["tx"], r["mode"], r["txtp"], r["flags"], r["x"], r["y"]
    if tx > 4 or mode > 9 or txtp > 3 or fl & ~7 or (fl & DC_ONLY and not fl & RESIDUAL):
        return False
    N = 4 if tx == 4 else 4 << tx
    Cw, Ch = 64 >> fr.hs[p], 64 >> fr.vs[p]
    sy, sx = divmod(r["sb"], fr.sb_w)
    cx0, cy0 = sx * Cw, sy * Ch
    if (x | y) & (N - 1) or x < cx0 or x + N > cx0 + Cw or y < cy0 or y + N > cy0 + Ch or x >= fr.dw[p] or y >= fr.dh[p]:
        return False
    return not (N == 4 and fl & HAVE_RIGHT and x + 8 > cx0 + Cw)


def edges(fr, P, p, r, tiles=True):
    """(converted mode, left[N] as intra_pred reads it, top[-1 .. max(N, 8) - 1]) of record r from plane P (int64, decoded area)"""
    tx, x, y = r["tx"], r["x"], r["y"]
    N = 4 if tx == 4 else 4 << tx
    base = 128 << (fr.bd - 8)
    dw, dh = fr.dw[p], fr.dh[p]
    sbx = x // (64 >> fr.hs[p])
    ts = max(s for s in tile_starts(fr.sb_w, fr.log2_tile_cols) if s <= sbx) if tiles else 0
    have_top, have_left = y > 0, x > (ts * 64) >> fr.hs[p]
    have_right = bool(r["flags"] & HAVE_RIGHT)
    mode = MODE_CONV[r["mode"]][int(have_left)][int(have_top)]
    nt = max(N, 8)
    top = np.full(nt + 1, base - 1, np.int64)             # top[0] is the corner
    if have_top:
        top[1:N + 1] = P[y - 1, np.minimum(np.arange(x, x + N), dw - 1)]
        top[0] = P[y - 1, x - 1] if have_left else base + 1
        if N == 4:
            top[5:9] = P[y - 1, x + 4:x + 8] if (have_right and x + 8 <= dw) else top[4]
    elif N == 4:
        top[5:9] = top[4]
    if have_left:
        col = P[np.minimum(np.arange(y, y + N), dh - 1), x - 1]
        left = col.copy() if mode == HU else col[::-1].copy()
    else:
        left = np.full(N, base + 1, np.int64)
    return mode, left, top


def reconstruct(fr, p, r, mode, left, top, P):
    """intra_pred[tx][mode] from the edge lines, then itxfm_add when the record has a residual: an (N, N) int64 block"""
    O = _oracle()
    tx = r["tx"]
    N = 4 if tx == 4 else 4 << tx
    dt = np.uint8 if fr.bd == 8 else np.uint16
    ps = np.dtype(dt).itemsize
    blk = np.zeros((N, N), dt)
    lb = np.ascontiguousarray(left.astype(dt))
    tb = np.zeros(len(top) + 8, dt)
    tb[:len(top)] = top
    O.ffo_vp9_intra_pred_bd(C.c_int(fr.bd), C.c_int(0 if tx == 4 else tx), C.c_int(mode), ffi.ptr(blk), C.c_ssize_t(N * ps),
                            ffi.ptr(lb), C.cast(tb.ctypes.data + ps, ffi.u8p))
    out = blk.astype(np.int64)
    if r["flags"] & RESIDUAL:
        t = dict(tx=tx, txtp=r["txtp"], coeff_offset=r["coeff_offset"], dc_only=1 if r["flags"] & DC_ONLY else 0)
        out = vg.tu_add(fr, t, out, p)
    return out


def model(fr, recs=None, planes=None, tiles=True):
    """the planes (decoded area) after intra reconstruction: each plane's well-formed records in decoding order (superblocks in raster
    order, records in list order within one), each block's samples inside the decoded area written back"""
    recs = fr.recs if recs is None else recs
    out = [pl.copy() for pl in (fr.planes if planes is None else planes)]
    for p in range(3):
        P = out[p]
        dw, dh = fr.dw[p], fr.dh[p]
        for r in sorted(recs[p], key=lambda r: r["sb"]):
            if not well_formed(fr, p, r):
                continue
            mode, left, top = edges(fr, P, p, r, tiles)
            blk = reconstruct(fr, p, r, mode, left, top, P)
            x, y = r["x"], r["y"]
            N = blk.shape[0]
            h, w = min(N, dh - y), min(N, dw - x)
            P[y:y + h, x:x + w] = blk[:h, :w]
    return out


# ---- the pointer form: intra_recon / check_intra_mode as the reference runs them ----
class _Ptr:
    """a sample pointer: a flat sample array and an index into it"""

    def __init__(self, buf, off):
        self.buf, self.off = buf, off

    def __add__(self, k):
        return _Ptr(self.buf, self.off + k)

    def __getitem__(self, i):
        return int(self.buf[self.off + i])

    def __setitem__(self, i, v):
        self.buf[self.off + i] = v

    def same(self, o):
        return self.buf is o.buf and self.off == o.off

    def addr(self):
        return self.buf.ctypes.data + self.off * self.buf.itemsize


def pointer_model(fr, pad=(0, 8), scribble=True):
    """the planes (decoded area) after the reference's intra reconstruction, transcribed in pointer form from libavcodec's
    ff_vp9_decode_block (vp9block.c: the 128-byte-stride overhang buffers td->tmp_y / tmp_uv when a block crosses the linesize or the
    last block row, and the copy-back of the visible part), intra_recon and check_intra_mode (vp9recon.c: dst_edge / dst_inner, the
    top == topleft test, the n_px_have copies and replications) and decode_tiles (vp9.c: s->intra_pred_data, the pre-loop-filter
    bottom line of each superblock row).  Frames have a linesize of the decoded width plus pad[0] (luma) / pad[1] (chroma) samples
    and garbage rows below; with `scribble` each finished superblock row is overwritten with garbage (what the loop filter does to
    it before the next row is decoded) and restored at the end, so a read that should have come from intra_pred_data shows."""
    O = _oracle()
    bd, rng = fr.bd, np.random.default_rng(fr.W * 7 + fr.H)
    dt = np.uint8 if bd == 8 else np.uint16
    bpp = np.dtype(dt).itemsize
    base_v = 128 << (bd - 8)
    ss_h, ss_v, cols, rows = fr.ss_h, fr.ss_v, fr.cols, fr.rows
    ls = [fr.dw[p] + pad[min(p, 1)] for p in range(3)]              # linesize, samples
    frame = []
    for p in range(3):
        a = rng.integers(0, fr.maxv + 1, (fr.dh[p] + 72, ls[p])).astype(dt)
        a[:fr.dh[p], :fr.dw[p]] = fr.planes[p]
        frame.append(a.reshape(-1))
    tmp = [rng.integers(0, fr.maxv + 1, 64 * (128 // bpp)).astype(dt) for _ in range(3)]   # tmp_y, tmp_uv[0], tmp_uv[1]
    ipd = [np.zeros(fr.dw[p] + 64, dt) for p in range(3)]           # intra_pred_data[p], 8 samples of slack in front
    IPD0 = 8
    starts = tile_starts(fr.sb_w, fr.log2_tile_cols)
    a_buf, l_buf = np.zeros(96 // bpp, dt), np.zeros(64 // bpp, dt)   # LOCAL_ALIGNED_32(uint8_t, a_buf, [96]), l[64]

    def check_intra_mode(mode, dst_edge, stride_edge, dst_inner, stride_inner, col, x, w, row, y, tx, p, ss_h_, ss_v_, tile_col_start):
        have_top = row > 0 or y > 0
        have_left = col > tile_col_start or x > 0
        have_right = x < w - 1
        mode = MODE_CONV[mode][int(have_left)][int(have_top)]
        needs_left = mode in (HOR, DC, DDR, VR, HD, HU, TM, LEFT_DC)
        needs_top = mode in (VERT, DC, DDL, DDR, VR, HD, VL, TM, TOP_DC)
        needs_topleft = mode in (DDR, VR, HD, TM)
        needs_topright = mode in (DDL, VL)
        invert_left = mode == HU
        a = _Ptr(a_buf, 32 // bpp)                                     # &a_buf[32] (bytes)
        l = _Ptr(l_buf, 0)
        if needs_top:
            n_px_need, n_px_have = 4 << tx, (((cols - col) << (1 - ss_h_)) - x) * 4
            n_px_need_tr = 4 if (tx == 0 and needs_topright and have_right) else 0
            top = topleft = None
            if have_top:
                at_sbrow_top = not (row & 7) and not y
                ipd_ptr = _Ptr(ipd[p], IPD0 + col * (8 >> ss_h_) + x * 4)
                top = ipd_ptr if at_sbrow_top else dst_edge + (-stride_edge) if y == 0 else dst_inner + (-stride_inner)
                if have_left:
                    topleft = ipd_ptr if at_sbrow_top else dst_edge + (-stride_edge) if (y == 0 or x == 0) else dst_inner + (-stride_inner)
            if (have_top and (not needs_topleft or (have_left and top.same(topleft))) and (tx != 0 or not needs_topright or have_right)
                    and n_px_need + n_px_need_tr <= n_px_have):
                a = top
            else:
                if have_top:
                    if n_px_need <= n_px_have:
                        for i in range(n_px_need):
                            a[i] = top[i]
                    else:
                        for i in range(n_px_have):
                            a[i] = top[i]
                        for i in range(n_px_have, n_px_need):
                            a[i] = a[n_px_have - 1]
                else:
                    for i in range(n_px_need):
                        a[i] = base_v - 1
                if needs_topleft:
                    a[-1] = topleft[-1] if (have_left and have_top) else base_v + (1 if have_top else -1)
                if tx == 0 and needs_topright:
                    if have_top and have_right and n_px_need + n_px_need_tr <= n_px_have:
                        for i in range(4):
                            a[4 + i] = top[4 + i]
                    else:
                        for i in range(4):
                            a[4 + i] = a[3]
        if needs_left:
            if have_left:
                n_px_need, n_px_have = 4 << tx, (((rows - row) << (1 - ss_v_)) - y) * 4
                d, st = (dst_edge, stride_edge) if x == 0 else (dst_inner, stride_inner)
                if invert_left:
                    for i in range(min(n_px_need, n_px_have)):
                        l[i] = d[i * st - 1]
                    for i in range(n_px_have, n_px_need):
                        l[i] = l[n_px_have - 1]
                else:
                    for i in range(min(n_px_need, n_px_have)):
                        l[n_px_need - 1 - i] = d[i * st - 1]
                    for i in range(max(n_px_need - n_px_have, 0)):
                        l[i] = l[n_px_need - n_px_have]
            else:
                for i in range(4 << tx):
                    l[i] = base_v + 1
        return mode, a, l

    def itxfm_add(tx, txtp, dst, stride, p, off, eob):
        N = 4 if tx == 4 else 4 << tx
        co = fr.coeffs[p][off:off + N * N]
        if bd == 8:
            c = np.ascontiguousarray(co.astype(np.int16))
            O.ffo_vp9_itxfm_add(tx, txtp, C.cast(dst.addr(), ffi.u8p), stride * bpp, ffi.ptr(c, ffi.i16p), eob)
        else:
            c = np.ascontiguousarray(co.astype(np.int32))
            O.ffo_vp9_itxfm_add_bd(bd, tx, txtp, C.cast(dst.addr(), ffi.u8p), stride * bpp, ffi.ptr(c, ffi.i32p), eob)

    def intra_recon(b, dst, stride, dst_r_base, tile_col_start):
        row, col, bs = b["row"], b["col"], b["bs"]
        w4, h4 = BWH8[bs][0] << 1, BWH8[bs][1] << 1
        end_x, end_y = min(2 * (cols - col), w4), min(2 * (rows - row), h4)
        lossless = fr.lossless
        btx, buvtx = b["tx"], b["uvtx"]
        tx, uvtx = 4 * lossless + btx, 4 * lossless + buvtx
        for p in range(3):
            t, ttx = (btx, tx) if p == 0 else (buvtx, uvtx)
            pw4, pex, pey = (w4, end_x, end_y) if p == 0 else (w4 >> ss_h, end_x >> ss_h, end_y >> ss_v)
            sh, sv = (0, 0) if p == 0 else (ss_h, ss_v)
            step1d, step = 1 << t, 1 << (2 * t)
            d, d_r = dst[p], dst_r_base[p]
            n = 0
            for y in range(0, pey, step1d):
                ptr, ptr_r = d, d_r
                for x in range(0, pex, step1d):
                    if p == 0:
                        mode = b["mode"][y * 2 + x if (bs > 9 and btx == 0) else 0]
                        txtp = INTRA_TXFM_TYPE[mode]
                    else:
                        mode, txtp = b["uvmode"], 0
                    eob = 0 if b["skip"] else b["eob"][p][n]
                    mode, a, l = check_intra_mode(mode, ptr_r, ls[p], ptr, stride[p], col, x, pw4, row, y, t, p, sh, sv, tile_col_start)
                    O.ffo_vp9_intra_pred_bd(C.c_int(bd), C.c_int(t), C.c_int(mode), C.cast(ptr.addr(), ffi.u8p),
                                            C.c_ssize_t(stride[p] * bpp), C.cast(l.addr(), ffi.u8p), C.cast(a.addr(), ffi.u8p))
                    if eob:
                        N = 4 << t
                        itxfm_add(ttx, txtp, ptr, stride[p], p, b["base"][p] + 16 * n, 1 if eob == 1 else N * N)
                    ptr, ptr_r, n = ptr + 4 * step1d, ptr_r + 4 * step1d, n + step
                d_r = d_r + 4 * step1d * ls[p]
                d = d + 4 * step1d * stride[p]

    def decode_block(b, tile_col_start):
        row, col, bs = b["row"], b["col"], b["bs"]
        w4, h4 = BWH8[bs]
        yoff, uvoff = row * 8 * ls[0] + col * 8, (row * 8 >> ss_v) * ls[1] + (col * 8 >> ss_h)
        emu0 = (col + w4) * 8 * bpp > ls[0] * bpp or row + h4 > rows
        emu1 = ((col + w4) * 8 >> ss_h) * bpp > ls[1] * bpp or row + h4 > rows
        dst_r = [_Ptr(frame[0], yoff), _Ptr(frame[1], uvoff), _Ptr(frame[2], uvoff)]
        dst = [_Ptr(tmp[0], 0) if emu0 else dst_r[0]] + [(_Ptr(tmp[p], 0) if emu1 else dst_r[p]) for p in (1, 2)]
        stride = [128 // bpp if emu0 else ls[0]] + [128 // bpp if emu1 else ls[1]] * 2
        intra_recon(b, dst, stride, dst_r, tile_col_start)
        for p, emu in ((0, emu0), (1, emu1), (2, emu1)):              # the visible part back (s->dsp.mc copies)
            if not emu:
                continue
            sh, sv = (0, 0) if p == 0 else (ss_h, ss_v)
            w, h = min(cols - col, w4) * 8 >> sh, min(rows - row, h4) * 8 >> sv
            for r in range(h):
                frame[p][dst_r[p].off + r * ls[p]:dst_r[p].off + r * ls[p] + w] = tmp[p][r * (128 // bpp):r * (128 // bpp) + w]

    # decode_tiles: superblock rows; within one, the tile columns left to right, each its superblocks' blocks in decoding order
    by_sb = {}
    for b in fr.decoded:
        by_sb.setdefault((b["row"] >> 3) * fr.sb_w + (b["col"] >> 3), []).append(b)
    saved = []
    for sy in range(fr.sb_h):
        for sx in range(fr.sb_w):
            tcs = max(s for s in starts if s <= sx) << 3
            for b in by_sb.get(sy * fr.sb_w + sx, []):
                decode_block(b, tcs)
        if sy + 1 < fr.sb_h:                                          # row + 8 < s->rows
            for p in range(3):
                r63 = ((sy * 64) >> (fr.vs[p])) + (64 >> fr.vs[p]) - 1
                ipd[p][IPD0:IPD0 + fr.dw[p]] = frame[p][r63 * ls[p]:r63 * ls[p] + fr.dw[p]]
                if scribble:                                          # the loop filter changes the finished row
                    r0, r1 = (sy * 64) >> fr.vs[p], r63 + 1
                    seg = slice(r0 * ls[p], r1 * ls[p])
                    saved.append((p, seg, frame[p][seg].copy()))
                    frame[p][seg] = rng.integers(0, fr.maxv + 1, r1 * ls[p] - r0 * ls[p]).astype(dt)
    for p, seg, v in saved:
        frame[p][seg] = v
    return [frame[p].reshape(-1, ls[p])[:fr.dh[p], :fr.dw[p]].astype(np.int64) for p in range(3)]
