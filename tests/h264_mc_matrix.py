"""The cells of H.264's block motion-compensation kernels (h264.qpel_batch, h264.chroma_mc_batch and their _hbd faces) as
deterministic block lists, shared by tests/test_h264_mc_matrix_cpu.py and tests/test_gpu_h264_mc_matrix.py.  Nothing is random but
the sample values.

A *cell* is what the kernels branch on.
  luma    size x mcxy x put / avg x source address modulo 16 x destination address modulo 4 (luma_cells(): the cross product, 6144
          records laid out so that neighbours in list order differ in size and alignment: a group of four consecutive records there
          never passes the tile test of k_h264_qpel_m / _mp / _t), then the *group* family: runs of four consecutive 16 x 16 records
          "tiled"     all four dword-aligned at one dst % 16 of {0, 4, 8, 12}, put and avg mixed inside the group
          "offdword"  the same with one member at dst % 4 != 0: the tile test fails because of an address
          "small"     the same with one member 8 x 8
          and one last record, so that the list is no multiple of four.
  chroma  width x height x class {x = y = 0, only x, only y, both} x source address modulo 4 x destination address modulo 4 x
          put / avg, then every (x, y) of every width at one height (chroma_cells()).
  edges   FFHIP_MC_EMU records: the cross product of two ladders of block origins round a small picture (luma 48 x 32, chroma
          24 x 16) that sits in a larger allocation, for every size and mcxy (chroma: width and class), with unflagged interior
          records mixed in (luma_edge_cells(), chroma_edge_cells()).

Layout is tests/mc_matrix.py's Batch: a private source slot per block — the footprint's bounding box, SLACK_Y rows above and below
and SLACK_X samples left and right, which the aligned 16-byte chunk loads of the matrix-core kernels stay inside — and a private
destination slot with DSLACK samples all round; tests compare the WHOLE destination buffer.  One stride serves both planes, as
qpel_mc_func has it.  What a position really reads inside its bounding box (H + V: a cross, not a rectangle) is found by probing
the oracle (luma_mask(), chroma_mask()); poisoned() complements everything else.

Sample content goes by slot, four classes in turn (content_class()): uniform noise, binary noise of 0 and the maximum, flat 0, flat
maximum.  Binary noise drives the unclipped 6-tap sums to their extremes (-2550, 10710) and both clips of every plane."""
import ctypes as C
import functools
from collections import namedtuple

import numpy as np

import ffi
import mc_matrix as M
from ffi import u8p

SIZES = [16, 8, 4]
CONTENT = ["noise", "binary", "zero", "max"]
CHROMA_WIDTHS = [8, 4, 2]
CHROMA_HEIGHTS = [2, 4, 8, 16]
N_CROSS = 3 * 16 * 2 * 16 * 4          # 6144
N_GROUPS = 2563                        # 10252 records: with the last one the list has 16397, 13 over a multiple of 16
VARIANTS = ["tiled", "tiled", "offdword", "small"]
MC_EMU = 1                             # FFHIP_MC_EMU (include/ffhip.h)
LUMA_PIC, CHROMA_PIC = (48, 32), (24, 16)
PIC_AT = (8, 37)                       # row and column of the picture's sample (0, 0) in its allocation: no aligned origin

#: w, h: the block; mx, my: quarter (chroma: eighth) sample fractions; mcxy = mx + 4 * my (luma); smod / dmod: the addresses modulo 16
#: (chroma: modulo 4); fam: the family; flag, sx, sy: FFHIP_MC_EMU and the block's origin in the picture; rung: the ladders' names;
#: s2mod: unused here (mc_matrix.Batch lays out HEVC's second source by it)
Cell = namedtuple("Cell", "w h mx my smod dmod avg mcxy fam flag sx sy rung s2mod")


def _luma(size, mcxy, smod, dmod, avg, fam, flag=0, sx=0, sy=0, rung=None):
    return Cell(size, size, mcxy & 3, mcxy >> 2, smod, dmod, avg, mcxy, fam, flag, sx, sy, rung, 0)


def _chroma(w, h, x, y, smod, dmod, avg, fam, flag=0, sx=0, sy=0, rung=None):
    return Cell(w, h, x, y, smod, dmod, avg, 0, fam, flag, sx, sy, rung, 0)


def content_class(i):
    """the class of slot i: the four in turn, the turn shifted by one every four slots (so that a member's position in its group
    of four does not fix its class)"""
    return CONTENT[(i + i // 4) % 4]


def luma_cells():
    cells = []
    for i in range(N_CROSS):
        a, b, c, avg, mc = i % 3, (i // 3) % 4, (i // 12) % 16, (i // 192) % 2, i // 384
        d4, s16 = (a + b) % 4, (c + 5 * (a + 3 * b)) % 16          # one-to-one in (b, c) for every a; both move with every record
        cells.append(_luma(SIZES[a], mc, s16, d4 + 4 * ((i // 5) % 4), avg, "cross"))
    for g in range(N_GROUPS):
        variant, d16 = VARIANTS[(g // 16) % 4], 4 * (g % 4)
        mixed = 1 + (g // 4) % 14                                  # bit k: member k averages; never all four alike
        odd = (g // 4) % 4                                         # the member that differs, where the variant has one
        for k in range(4):
            size, dmod = 16, d16
            if variant == "offdword" and k == odd:
                dmod = d16 + 1 + (g // 16) % 3
            if variant == "small" and k == odd:
                size = 8
            cells.append(_luma(size, (g // 4 + g // 64 + 5 * k) % 16, (g + 5 * k) % 16, dmod, (mixed >> k) & 1, variant))
    cells.append(_luma(16, 10, 7, 8, 0, "last"))
    return cells


def groups(cells):
    """the runs of four consecutive records a wave of k_h264_qpel_m / _mp / _t takes together: (first index, the four cells)"""
    return [(i, cells[i:i + 4]) for i in range(0, len(cells) - 3, 4)]


def tile_candidate(four):
    """the kernels' tile test, on cells: four 16 x 16 records with dword-aligned destinations"""
    return len(four) == 4 and all(c.w == 16 and c.dmod % 4 == 0 for c in four)


def chroma_cells():
    cells = []
    k = {cls: 0 for cls in M.CLASSES}
    for wi, w in enumerate(CHROMA_WIDTHS):
        for hi, h in enumerate(CHROMA_HEIGHTS):
            for ci, cls in enumerate(M.CLASSES):
                for smod in range(4):
                    for dmod in range(4):
                        for avg in (0, 1):
                            x, y = M._fractions(cls, k[cls], 8)
                            k[cls] += 1
                            cells.append(_chroma(w, h, x, y, smod, dmod, avg, "cross"))
    for wi, w in enumerate(CHROMA_WIDTHS):
        for y in range(8):
            for x in range(8):
                i = len(cells)
                cells.append(_chroma(w, 4, x, y, i % 4, (i + i // 4) % 4, (i + y) & 1, "fractions"))
    for j in range(5):                                             # the list is no multiple of a workgroup's 16 blocks
        cells.append(_chroma(8, 8, 3 + j, 5 - j, j % 4, (j + 1) % 4, j & 1, "last"))
    # neighbours in list order differ in shape: a fixed stride through the list (a prime that does not divide its length)
    n = len(cells)
    assert n % 131
    return [cells[(131 * i) % n] for i in range(n)]


def ladder(length, lo, hi):
    """block origins on one axis of a picture `length` samples long, for a footprint that reaches from origin - lo to origin + hi:
    (name, origin)"""
    f = lo + hi + 1
    out = [("far before", -hi - f - 1), ("far after", length + f + lo),
           ("touches before", -hi), ("touches after", length - 1 + lo)]
    out += [("straddles before by %d" % k, lo - k) for k in (1, 2, 3)]
    out += [("straddles after by %d" % k, length - 1 + k - hi) for k in (1, 2, 3)]
    out += [("starts at 0", lo), ("ends at the last", length - 1 - hi), ("interior", lo + (length - f) // 2), ("-3000", -3000), ("+3000", 3000)]
    return out


LADDER_NAMES = [n for n, _ in ladder(48, 2, 18)]


def luma_edge_cells():
    """every size x mcxy x (rung of x) x (rung of y), put and avg alternating, flagged; after every fourth an unflagged record whose
    21 x 21 window lies inside the picture"""
    pw, ph = LUMA_PIC
    cells = []
    j = 0
    for size in SIZES:
        for mc in range(16):
            for nx, ox in ladder(pw, 2, size + 2):
                for ny, oy in ladder(ph, 2, size + 2):
                    j += 1
                    cells.append(_luma(size, mc, None, (j + j // 4) % 16, j & 1, "edge", MC_EMU, ox, oy, (nx, ny)))
                    if j % 4 == 0:
                        x, y = 2 + j // 4 % (pw - size - 4), 2 + j // 8 % (ph - size - 4)
                        cells.append(_luma(size, (mc + j // 4) % 16, None, (j // 4) % 16, (j >> 3) & 1, "interior", 0, x, y))
    return cells


def chroma_edge_cells():
    """every width x class x rung pair (heights in turn, the fractions of a class in turn), flagged, and unflagged interior ones"""
    pw, ph = CHROMA_PIC
    cells = []
    j = 0
    for wi, w in enumerate(CHROMA_WIDTHS):
        for ci, cls in enumerate(M.CLASSES):
            h = CHROMA_HEIGHTS[(wi + ci) % 4]
            for nx, ox in ladder(pw, 0, w - 1 + (ci & 1)):
                for ny, oy in ladder(ph, 0, h - 1 + (ci >> 1)):
                    j += 1
                    x, y = M._fractions(cls, j, 8)
                    cells.append(_chroma(w, h, x, y, None, (j + j // 4) % 4, j & 1, "edge", MC_EMU, ox, oy, (nx, ny)))
                    if j % 4 == 0:
                        px, py = j // 4 % (pw - w - 1), j // 8 % max(1, ph - h - 1)
                        cells.append(_chroma(w, min(h, 8), x, y, None, (j // 4) % 4, (j >> 3) & 1, "interior", 0, px, py))
    return cells


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle, and what it reads
# ---------------------------------------------------------------------------------------------------------------------------
def _oracle():
    O = ffi.oracle()
    O.ffo_h264_qpel_bd.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, u8p, u8p, C.c_ssize_t]
    O.ffo_h264_qpel_bd.restype = None
    O.ffo_h264_chroma_mc_bd.argtypes = [C.c_int, C.c_int, C.c_int, u8p, u8p, C.c_ssize_t, C.c_int, C.c_int, C.c_int]
    O.ffo_h264_chroma_mc_bd.restype = None
    return O


def _at(a, byte_off):
    return C.cast(a.ctypes.data + int(byte_off), u8p)


def oracle_block(O, chroma, bd, c, dst, dst_off, src, src_off, stride_bytes):
    """one record: the 8-bit functions at 8 bits, the _bd forms above"""
    if chroma:
        if bd == 8:
            O.ffo_h264_chroma_mc(c.avg, c.w, _at(dst, dst_off), _at(src, src_off), stride_bytes, c.h, c.mx, c.my)
        else:
            O.ffo_h264_chroma_mc_bd(bd, c.avg, c.w, _at(dst, dst_off), _at(src, src_off), stride_bytes, c.h, c.mx, c.my)
    elif bd == 8:
        O.ffo_h264_qpel(c.avg, SIZES.index(c.w), c.mcxy, _at(dst, dst_off), _at(src, src_off), stride_bytes)
    else:
        O.ffo_h264_qpel_bd(bd, c.avg, SIZES.index(c.w), c.mcxy, _at(dst, dst_off), _at(src, src_off), stride_bytes)


PROBE = 21          # the window probed: 21 x 21 samples from two above and left of the block (chroma: from the block's origin)
PROBE_BD = 14       # a corner of the centre position's window weighs 1 / 1024 in ONE output sample.  At 8 bits its complement moves
#                     that sample only when the sum happens to stand within 255 of a rounding step; at 14 bits, with the base samples
#                     in 4000 .. 5999, a complement is a step of more than 6000: every non-zero weight moves its output, none clips


def probe(chroma, c, org, bd=PROBE_BD, trials=2):
    """the samples of the PROBE x PROBE window (block origin at `org` in it) whose complement changes the oracle's output for cell c"""
    O = _oracle()
    stride, y0, x0 = 64, 16, 16
    maxv = (1 << bd) - 1
    rng = np.random.default_rng(1000 * c.w + 100 * c.h + 10 * c.mx + c.my + (5000 if chroma else 0))
    dt = np.uint8 if bd == 8 else np.uint16
    seen = np.zeros((PROBE, PROBE), bool)
    base, ref, out = np.zeros((64, stride), dt), np.zeros((16, stride), dt), np.zeros((16, stride), dt)
    ps = base.itemsize
    flat = base.reshape(-1)
    c = c._replace(avg=0)
    for t in range(trials):
        base[:] = rng.integers(0, maxv + 1, base.shape) if bd == 8 else rng.integers(4000, 6000, base.shape)
        oracle_block(O, chroma, bd, c, ref, 0, base, ((y0 + org) * stride + x0 + org) * ps, stride * ps)
        for r, q in np.argwhere(~seen):
            at = (y0 + r) * stride + x0 + q
            flat[at] = maxv - flat[at]
            oracle_block(O, chroma, bd, c, out, 0, base, ((y0 + org) * stride + x0 + org) * ps, stride * ps)
            flat[at] = maxv - flat[at]
            if not np.array_equal(out, ref):
                seen[r, q] = True
    return seen


@functools.lru_cache(maxsize=None)
def luma_mask(size, mcxy):
    """bool [21, 21]: what put_h264_qpel<size>_mc<mcxy> reads; [2, 2] is the block's first sample"""
    return probe(0, _luma(size, mcxy, 0, 0, 0, "probe"), 2)


@functools.lru_cache(maxsize=None)
def chroma_mask(w, h, x, y):
    """bool [21, 21] for one class (x and y matter only as zero or not): [0, 0] is the block's first sample"""
    return probe(1, _chroma(w, h, 4 if x else 0, 4 if y else 0, 0, 0, 0, "probe"), 0)


def luma_planes(mcxy):
    """which of F, H, V, J a position combines (h264qpel_template.c:313-459), for the shape checks of the probed masks"""
    mx, my = mcxy & 3, mcxy >> 2
    j = (mx == 2 and my != 0) or (my == 2 and mx != 0)
    v = (mx != 2 and my != 0) or mcxy == 8
    h = (my != 2 and mx != 0) or mcxy == 2
    f = mcxy in (0, 1, 3, 4, 12)
    return f, h, v, j


# ---------------------------------------------------------------------------------------------------------------------------
# layout
# ---------------------------------------------------------------------------------------------------------------------------
class H264Batch(M.Batch):
    """mc_matrix.Batch with one stride for both planes, H.264's footprints (probed masks inside the bounding boxes), the four
    content classes and a first_bad() that names an H.264 cell"""

    def __init__(self, cells, chroma, stride):
        self.chroma = chroma
        mod = 4 if chroma else 16
        laid = [c if c.smod is not None else c._replace(smod=0) for c in cells]
        M.Batch.__init__(self, laid, (0, 1) if chroma else (2, 3), stride, stride, smodulus=mod, dmodulus=mod, dmax=16)
        self.cells = cells
        self.stride = stride
        self.modulus = mod

    def mask(self, c):
        return chroma_mask(c.w, c.h, bool(c.mx), bool(c.my)) if self.chroma else luma_mask(c.w, c.mcxy)

    def source(self, bd, seed):
        rng = np.random.default_rng(seed)
        maxv = (1 << bd) - 1
        dt = np.uint8 if bd == 8 else np.uint16
        src = rng.integers(0, maxv + 1, (self.srows, self.sstride)).astype(dt)
        for i, (y0, y1, x0, x1) in enumerate(self.sslot):
            k = content_class(i)
            if k == "binary":
                src[y0:y1, x0:x1] = rng.choice(np.array([0, maxv], dt), (y1 - y0, x1 - x0))
            elif k != "noise":
                src[y0:y1, x0:x1] = maxv if k == "max" else 0
        return src

    def footprints(self):
        m = np.zeros((self.srows, self.sstride), bool)
        b = self.margin[0]
        for c, (py, px), (y0, y1, x0, x1) in zip(self.cells, self.spos, self.foot):
            k = self.mask(c)
            hh, ww = y1 - (py - b), x1 - (px - b)                   # the bounding box holds the whole mask
            assert not k[hh:].any() and not k[:, ww:].any()
            m[py - b:y1, px - b:x1] |= k[:hh, :ww]
        return m

    def records(self, ps):
        from ffmpeg_amd import h264
        rec = np.zeros(len(self.cells), h264.CHROMA_DTYPE if self.chroma else h264.QPEL_DTYPE)
        for i, c in enumerate(self.cells):
            rec[i]["dst_offset"], rec[i]["src_offset"], rec[i]["avg"] = self.dst_offset(i, ps), self.src_offset(i, ps), c.avg
            rec[i]["flags"], rec[i]["src_x"], rec[i]["src_y"] = c.flag, c.sx if c.flag else 0, c.sy if c.flag else 0
            if self.chroma:
                rec[i]["w_idx"], rec[i]["h"], rec[i]["x"], rec[i]["y"] = CHROMA_WIDTHS.index(c.w), c.h, c.mx, c.my
            else:
                rec[i]["mcxy"], rec[i]["size_idx"] = c.mcxy, SIZES.index(c.w)
        return rec

    def want(self, bd, src, dst0, first=0, n=None):
        """the oracle over records first .. first + n - 1"""
        O = _oracle()
        ps = src.itemsize
        out = dst0.copy()
        for i in range(first, len(self.cells) if n is None else first + n):
            oracle_block(O, self.chroma, bd, self.cells[i], out, self.dst_offset(i, ps), src, self.src_offset(i, ps), self.stride * ps)
        return out

    def inside(self, first=0, n=None):
        m = np.zeros((self.drows, self.dstride), bool)
        for i in range(first, len(self.cells) if n is None else first + n):
            (y, x), c = self.dpos[i], self.cells[i]
            m[y:y + c.h, x:x + c.w] = True
        return m

    def describe(self, i, ps=1):
        c = self.cells[i]
        shape = "w %d, h %d, x %d, y %d" % (c.w, c.h, c.mx, c.my) if self.chroma else "size %d, mcxy %d" % (c.w, c.mcxy)
        text = "block %d (%s, %s, %s, src mod %d %d, dst mod 4 %d, position %d in its group of four" % (
            i, c.fam, shape, "avg" if c.avg else "put", self.modulus, self.src_offset(i, ps) // ps % self.modulus, self.dst_offset(i, ps) // ps % 4, i % 4)
        if c.flag:
            text += ", FFHIP_MC_EMU at (%d, %d): x %s, y %s" % (c.sx, c.sy, c.rung[0], c.rung[1])
        return text + ")"

    def first_bad(self, got, want):
        """None, or the first mismatching cell as text: size (chroma: width and height), mcxy (chroma: x, y), put / avg, source
        address modulo 16 (chroma: 4), destination address modulo 4, the record's position in its group of four, and the row and
        column in the block"""
        bad = np.argwhere(got != want)
        if not len(bad):
            return None
        p = tuple(int(v) for v in bad[0])
        for i, s in enumerate(self.dslot):
            if s[0] <= p[0] < s[1] and s[2] <= p[1] < s[3]:
                return "%d mismatches; first in %s at row %d column %d of the block: got %d, want %d" % (
                    len(bad), self.describe(i, got.itemsize), p[0] - self.dpos[i][0], p[1] - self.dpos[i][1], int(got[p]), int(want[p]))
        return "%d mismatches; first at %s, outside every slot" % (len(bad), p)


class EdgeBatch(H264Batch):
    """H264Batch's destination slots; the source is ONE small picture inside a larger allocation whose surroundings are filled
    differently.  A flagged record's src_offset is the picture's sample (0, 0), an unflagged one's its block inside the picture."""

    def __init__(self, cells, chroma, stride):
        H264Batch.__init__(self, cells, chroma, stride)
        self.pic = CHROMA_PIC if chroma else LUMA_PIC
        self.srows = self.pic[1] + 2 * PIC_AT[0]
        assert PIC_AT[1] + self.pic[0] + 64 <= stride

    def picture(self):
        """bool mask of the picture in its allocation"""
        m = np.zeros((self.srows, self.stride), bool)
        m[PIC_AT[0]:PIC_AT[0] + self.pic[1], PIC_AT[1]:PIC_AT[1] + self.pic[0]] = True
        return m

    def source(self, bd, seed):
        """the picture: noise, its rim binary noise, two corners flat; the surroundings: a ramp no picture sample continues"""
        rng = np.random.default_rng(seed)
        maxv = (1 << bd) - 1
        dt = np.uint8 if bd == 8 else np.uint16
        pw, ph = self.pic
        pic = rng.integers(0, maxv + 1, (ph, pw)).astype(dt)
        rim = rng.choice(np.array([0, maxv], dt), (ph, pw))
        edge = np.ones((ph, pw), bool)
        edge[3:-3, 3:-3] = False
        pic[edge] = rim[edge]
        pic[0, 0], pic[-1, -1] = maxv, 0
        src = ((np.arange(self.srows)[:, None] * 7 + np.arange(self.stride)[None, :] * 3) % (maxv + 1)).astype(dt)
        src[PIC_AT[0]:PIC_AT[0] + ph, PIC_AT[1]:PIC_AT[1] + pw] = pic
        return src

    def poisoned(self, src, bd):
        """everything outside the picture complemented"""
        return np.where(self.picture(), src, ((1 << bd) - 1) - src).astype(src.dtype)

    def src_offset(self, i, ps):
        c = self.cells[i]
        org = PIC_AT[0] * self.stride + PIC_AT[1]
        return (org if c.flag else org + c.sy * self.stride + c.sx) * ps

    def gather(self, src, c):
        """the window the decoder's emulated_edge_mc() would leave for cell c: sample (x, y) of the picture at row clamp(y, 0,
        h - 1), column clamp(x, 0, w - 1) (include/ffhip.h), PROBE x PROBE from the margin before the block's origin"""
        pw, ph = self.pic
        b = self.margin[0]
        rows = np.clip(np.arange(c.sy - b, c.sy - b + PROBE), 0, ph - 1) + PIC_AT[0]
        cols = np.clip(np.arange(c.sx - b, c.sx - b + PROBE), 0, pw - 1) + PIC_AT[1]
        return src[np.ix_(rows, cols)]

    def want(self, bd, src, dst0, first=0, n=None):
        O = _oracle()
        ps = src.itemsize
        out = dst0.copy()
        b = self.margin[0]
        buf = np.zeros((PROBE, self.stride), src.dtype)
        for i in range(first, len(self.cells) if n is None else first + n):
            c = self.cells[i]
            if c.flag:
                buf[:, :PROBE] = self.gather(src, c)
                oracle_block(O, self.chroma, bd, c, out, self.dst_offset(i, ps), buf, (b * self.stride + b) * ps, self.stride * ps)
            else:
                oracle_block(O, self.chroma, bd, c, out, self.dst_offset(i, ps), src, self.src_offset(i, ps), self.stride * ps)
        return out


@functools.lru_cache(maxsize=None)
def _cells(kind):
    return {"luma": luma_cells, "chroma": chroma_cells, "luma_edge": luma_edge_cells, "chroma_edge": chroma_edge_cells}[kind]()


def lay_out(kind, stride):
    chroma = kind.startswith("chroma")
    return (EdgeBatch if kind.endswith("edge") else H264Batch)(_cells(kind), chroma, stride)
