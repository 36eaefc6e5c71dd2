"""The cells of the motion-compensation batch kernels (hevc.mc_batch / hevc.mc_w_batch / vp9.mc_batch) as deterministic block
lists, shared by tests/test_mc_matrix_cpu.py and tests/test_gpu_mc_matrix.py.

A *cell* is what the kernels branch on: width, height, (mx, my), the source address modulo 4, the destination address modulo 4, for
HEVC bi / bi_w the address of the other list's block modulo 4, for VP9 put / avg.  hevc_cells() and vp9_cells() enumerate them
without any random choice; only sample values (and HEVC's weights, drawn by weights() from a fixed seed) are random.

lay_out() gives every block a private source slot and a private destination slot:
  source       the reference's exact footprint — the block plus the filter's margin, and that margin only on an axis whose fraction
               is non-zero — with SLACK_Y rows above and below and SLACK_X samples left and right that belong to no other block.
               SLACK_X is 16, not 8: the matrix-core kernels load a 16 x 16 block's footprint in aligned 16-byte chunks, up to 15
               bytes either side of it; k_hevc_mc reads up to 3 bytes and k_vp9_mc 1 byte to its right.
  destination  64 rows of the full width of 64 plus DSLACK samples all round (put_hevc_*: 64 int16 rows of pitch 64 with DSLACK
               elements before and after).  Tests compare the WHOLE destination buffer, so a store that leaves its block shows up.
"""
import ctypes as C
from collections import namedtuple

import numpy as np

import ffi

HEVC_WIDTHS = [2, 4, 6, 8, 12, 16, 24, 32, 48, 64]
HEVC_HEIGHTS = [2, 4, 6, 8, 12, 16, 24, 32, 48, 64]
VP9_WIDTHS = [4, 8, 16, 32, 64]
VP9_HEIGHTS = [1, 2, 3, 4, 8, 16, 32, 33, 64]
CLASSES = ["copy", "h", "v", "hv"]
SLACK_Y, SLACK_X, DSLACK = 8, 16, 8

#: w, h, mx, my; smod / dmod / s2mod: the addresses modulo 4 (source: bytes at 8 bits; destination: bytes, int16 units for put_hevc_*;
#: src2: int16 units); avg, filt: VP9 only; wt: HEVC's (denom, wx0, wx1, ox)
Cell = namedtuple("Cell", "w h mx my smod dmod s2mod avg filt wt")


def weights(rng, rep):
    """(denom, wx0, wx1, ox): slice-header ranges mixed with tests/checkasm/hevc_pel.c's ladders"""
    if rep % 3 == 0:
        return int(rng.choice([0, 7, 12])), int(rng.choice([0, 128, 255])), int(rng.choice([0, 128, 255])), int(rng.choice([0, 255]))
    d = int(rng.integers(0, 8))
    return d, (1 << d) + int(rng.integers(-128, 128)), (1 << d) + int(rng.integers(-128, 128)), int(rng.integers(-256, 255))


def klass(c):
    return CLASSES[(1 if c.mx else 0) + (2 if c.my else 0)]


def covers(cells, key, wanted):
    """every value of `wanted` occurs as key(cell)"""
    return set(wanted) <= {key(c) for c in cells}


def missing(cells, key, wanted):
    return sorted(set(wanted) - {key(c) for c in cells})


def _fractions(cls, k, nf):
    """the k-th non-zero fraction (pair) of a class: 1 .. nf - 1 in turn, hv walking all (nf - 1)^2 pairs"""
    m = nf - 1
    if cls == "copy":
        return 0, 0
    if cls == "h":
        return 1 + k % m, 0
    if cls == "v":
        return 0, 1 + k % m
    return 1 + k % m, 1 + (k // m) % m


def hevc_cells(chroma, mode):
    """1600 blocks: every (w, h) x class x source address modulo 4, the non-zero fractions in turn per width; then every (mx, my) pair
    for every width (64 pairs for chroma, 16 for luma — which also leaves the luma batch no multiple of 64 records)"""
    nf = 8 if chroma else 4
    rng = np.random.default_rng(1000 + 10 * chroma + mode)
    cells = []
    for w in HEVC_WIDTHS:
        k = {cls: 0 for cls in CLASSES}
        for h in HEVC_HEIGHTS:
            for cls in CLASSES:
                for smod in range(4):
                    i = len(cells)
                    mx, my = _fractions(cls, k[cls], nf)
                    k[cls] += 1
                    cells.append(Cell(w, h, mx, my, smod, (i + i // 4) % 4, (i + i // 16) % 4, 0, 0, weights(rng, i)))
    for wi, w in enumerate(HEVC_WIDTHS):
        for mx in range(nf):
            for my in range(nf):
                i = len(cells)
                h = HEVC_HEIGHTS[(i + wi) % len(HEVC_HEIGHTS)]
                cells.append(Cell(w, h, mx, my, i % 4, (i + i // 4) % 4, (i + i // 16) % 4, 0, 0, weights(rng, i)))
    return cells


def vp9_cells(filt):
    """360 blocks: every (w, h) x class x put / avg with the source address modulo 4 in turn; then the 16 x 16 grid of (mx, my) for
    every width with heights and avg in turn"""
    cells = []
    for wi, w in enumerate(VP9_WIDTHS):
        k = {cls: 0 for cls in CLASSES}
        for hi, h in enumerate(VP9_HEIGHTS):
            for ci, cls in enumerate(CLASSES):
                for avg in (0, 1):
                    mx, my = _fractions(cls, k[cls], 16)
                    if cls == "hv":
                        my = 1 + (7 * k[cls] + k[cls] // 15) % 15
                    k[cls] += 1
                    cells.append(Cell(w, h, mx, my, (hi + ci + avg + wi) % 4, (3 * hi + wi) % 4, 0, avg, filt, None))
    for wi, w in enumerate(VP9_WIDTHS):
        for my in range(16):
            for mx in range(16):
                i = len(cells)
                h = VP9_HEIGHTS[(i + wi + my) % len(VP9_HEIGHTS)]
                cells.append(Cell(w, h, mx, my, i % 4, (i + i // 4) % 4, 0, (i + my + wi) & 1, filt, None))
    return cells


def hevc_margin(chroma):
    """(samples before, samples after) a block on an axis with a non-zero fraction: the 8-tap and 4-tap windows"""
    return (1, 2) if chroma else (3, 4)


def vp9_margin(filt):
    return (0, 1) if filt == 3 else (3, 4)


def _pack(sizes, width):
    """shelves: boxes left to right, a new shelf when the row is full; returns the (y, x) of each and the total height"""
    y = x = shelf = 0
    out = []
    for hh, ww in sizes:
        assert ww <= width
        if x + ww > width:
            y, x, shelf = y + shelf, 0, 0
        out.append((y, x))
        x, shelf = x + ww, max(shelf, hh)
    return out, y + shelf


class Batch:
    """A laid-out list.  All geometry is in samples (rows, columns) of a plane `sstride` / `dstride` samples wide:
    spos[i]  the block's first sample in the source plane
    foot[i]  (y0, y1, x0, x1), end-exclusive: the reference's footprint
    sslot[i] the private rectangle around it (footprint + slack)
    dpos[i], dslot[i] the same for the destination; flat (put_hevc_*): dpos[i] is an int16 offset, dslot[i] = (o0, o1)
    s2pos[i] int16 offset of the other list's block"""

    def __init__(self, cells, margin, sstride, dstride, flat=False, smodulus=4, dmodulus=4, dmax=64):
        """smodulus / dmodulus: what c.smod / c.dmod are residues of (tests/h264_mc_matrix.py: 16); dmax: the largest block, the
        side of a destination slot's interior"""
        self.cells, self.margin, self.sstride, self.dstride, self.flat = cells, margin, sstride, dstride, flat
        b, a = margin
        sizes = [(c.h + b + a + 2 * SLACK_Y, c.w + b + a + 2 * SLACK_X + smodulus - 1) for c in cells]
        at, rows = _pack(sizes, sstride)
        self.srows = rows + 2                                   # a guard row above and below: the plane's own slack
        self.spos, self.foot, self.sslot = [], [], []
        for c, (y, x), (hh, ww) in zip(cells, at, sizes):
            y += 1
            py, px = y + SLACK_Y + b, x + SLACK_X + b
            px += (c.smod - (py * sstride + px)) % smodulus
            self.spos.append((py, px))
            self.foot.append((py - (b if c.my else 0), py + c.h + (a if c.my else 0), px - (b if c.mx else 0), px + c.w + (a if c.mx else 0)))
            self.sslot.append((y, y + hh, x, x + ww))
        self.dpos, self.dslot = [], []
        if flat:
            size = 64 * 64 + 2 * DSLACK + 3
            for i, c in enumerate(cells):
                o = i * size + DSLACK
                o += (c.dmod - o) % 4
                self.dpos.append(o)
                self.dslot.append((i * size, (i + 1) * size))
            self.dlen = len(cells) * size
        else:
            hh, ww = dmax + 2 * DSLACK, dmax + 2 * DSLACK + dmodulus - 1
            at, self.drows = _pack([(hh, ww)] * len(cells), dstride)
            for c, (y, x) in zip(cells, at):
                py, px = y + DSLACK, x + DSLACK
                px += (c.dmod - (py * dstride + px)) % dmodulus
                self.dpos.append((py, px))
                self.dslot.append((y, y + hh, x, x + ww))
        self.s2size = 64 * 64 + 8
        self.s2pos = [i * self.s2size + c.s2mod for i, c in enumerate(cells)]

    # ---- sample values ----
    def source(self, bd, seed):
        """random samples; every fifth slot is 0 / max stripes of noise, every fifth alternating 0 / max columns: both clips and
        the extremes of the 14-bit intermediates fire"""
        rng = np.random.default_rng(seed)
        maxv = (1 << bd) - 1
        src = rng.integers(0, maxv + 1, (self.srows, self.sstride)).astype(np.uint8 if bd == 8 else np.uint16)
        for i, (y0, y1, x0, x1) in enumerate(self.sslot):
            if i % 5 == 1:
                src[y0:y1, x0:x1] = rng.choice(np.array([0, maxv], src.dtype), (y1 - y0, x1 - x0))
            elif i % 5 == 3:
                src[y0:y1, x0:x1] = np.where((np.arange(x0, x1) + i // 5) & 1, maxv, 0).astype(src.dtype)[None, :]
        return src

    def footprints(self):
        m = np.zeros((self.srows, self.sstride), bool)
        for y0, y1, x0, x1 in self.foot:
            m[y0:y1, x0:x1] = True
        return m

    def poisoned(self, src, bd):
        """every sample outside the union of the footprints complemented (within the bit depth: at 8 bits, every byte)"""
        return np.where(self.footprints(), src, ((1 << bd) - 1) - src).astype(src.dtype)

    def destination(self, bd, seed):
        rng = np.random.default_rng(seed)
        if self.flat:
            return rng.integers(-30000, 30000, self.dlen).astype(np.int16)
        return rng.integers(0, 1 << bd, (self.drows, self.dstride)).astype(np.uint8 if bd == 8 else np.uint16)

    def src2(self, seed):
        rng = np.random.default_rng(seed)
        s2 = rng.integers(-8192, 16384, (len(self.cells), self.s2size)).astype(np.int16)
        s2[::5] = 16383
        s2[1::7] = -8192
        return s2.reshape(-1)

    def inside(self):
        """the destination samples that belong to a block"""
        if self.flat:
            m = np.zeros(self.dlen, bool)
            for c, o in zip(self.cells, self.dpos):
                m[o:o + 64 * c.h].reshape(c.h, 64)[:, :c.w] = True
            return m
        m = np.zeros((self.drows, self.dstride), bool)
        for c, (y, x) in zip(self.cells, self.dpos):
            m[y:y + c.h, x:x + c.w] = True
        return m

    # ---- byte offsets for the records ----
    def src_offset(self, i, ps):
        return (self.spos[i][0] * self.sstride + self.spos[i][1]) * ps

    def dst_offset(self, i, ps):
        return self.dpos[i] if self.flat else (self.dpos[i][0] * self.dstride + self.dpos[i][1]) * ps

    # ---- reporting ----
    def first_bad(self, got, want):
        """None, or the first mismatching cell as text: (w, h, mx, my, source mod 4, destination mod 4) and where in its slot"""
        bad = np.argwhere(got != want)
        if not len(bad):
            return None
        p = tuple(int(v) for v in bad[0])
        for i, (c, s) in enumerate(zip(self.cells, self.dslot)):
            if (s[0] <= p[0] < s[1]) if self.flat else (s[0] <= p[0] < s[1] and s[2] <= p[1] < s[3]):
                if self.flat:
                    rel = divmod(p[0] - self.dpos[i], 64)
                else:
                    rel = (p[0] - self.dpos[i][0], p[1] - self.dpos[i][1])
                return "%d mismatches; first in block %d (w %d, h %d, mx %d, my %d, src mod 4 %d, dst mod 4 %d)%s at row %d column %d of the block: " \
                       "got %d, want %d" % (len(bad), i, c.w, c.h, c.mx, c.my, c.smod, c.dmod, " avg" if c.avg else "", rel[0], rel[1],
                                            int(got[p]), int(want[p]))
        return "%d mismatches; first at %s, outside every slot" % (len(bad), p)


def lay_out_hevc(chroma, mode, sstride, dstride):
    return Batch(hevc_cells(chroma, mode), hevc_margin(chroma), sstride, dstride, flat=mode == 0)


def lay_out_vp9(filt, sstride, dstride):
    return Batch(vp9_cells(filt), vp9_margin(filt), sstride, dstride)


def _at(a, byte_off, typ=ffi.u8p):
    return C.cast(a.ctypes.data + int(byte_off), typ)


def hevc_want(b, chroma, mode, bd, src, dst0, s2):
    """the oracle over the whole list (mode 0 put, 1 uni, 2 uni_w, 3 bi, 4 bi_w)"""
    O = ffi.oracle()
    ps = src.itemsize
    want = dst0.copy()
    for i, c in enumerate(b.cells):
        sp = _at(src, b.src_offset(i, ps))
        if mode == 0:
            O.ffo_hevc_mc_bd(bd, chroma, 0, want.ctypes.data + 2 * b.dpos[i], 0, sp, b.sstride * ps, c.h, c.mx, c.my, c.w)
        elif mode == 1:
            O.ffo_hevc_mc_bd(bd, chroma, 1, want.ctypes.data + b.dst_offset(i, ps), b.dstride * ps, sp, b.sstride * ps, c.h, c.mx, c.my, c.w)
        else:
            d, wx0, wx1, ox = c.wt
            O.ffo_hevc_mc_w_bd(bd, chroma, mode, _at(want, b.dst_offset(i, ps)), b.dstride * ps, sp, b.sstride * ps,
                               _at(s2, 2 * b.s2pos[i], ffi.i16p), c.h, d, wx0, wx1, ox, c.mx, c.my, c.w)
    return want


def vp9_want(b, bd, src, dst0):
    O = ffi.oracle()
    ps = src.itemsize
    want = dst0.copy()
    for i, c in enumerate(b.cells):
        O.ffo_vp9_mc_bd(bd, c.filt, c.avg, _at(want, b.dst_offset(i, ps)), b.dstride * ps, _at(src, b.src_offset(i, ps)), b.sstride * ps,
                        c.w, c.h, c.mx, c.my)
    return want
