"""Pictures for the H.264 whole-picture residual face (ffhip_h264_residual_pictures_dev / _host) and its model.

The model is the decoder's order through the oracle: macroblock by macroblock ffo_h264_idct_mb_bd (which 0: idct_add16, which 1:
idct8_add4), ffo_h264_chroma_dc_dequant_bd and ffo_h264_idct_add8_bd on a dense copy of sl->mb and the nnzc caches, both built from
the face's bits alone: a block whose bit is clear is zero in the copy whatever `coeffs` holds there (the generator leaves noise in
every uncoded block, so a face that read one would differ), and a count is the number of non-zero coefficients of the block, which
is what a decoder has.  The generator draws every block as one of: nothing but a DC (count 1, block[0] set: the *_dc_add branch of
idct_add16 / idct8_add4), one AC coefficient alone (count 1, block[0] clear: the transform), or several; chroma planes with and
without a coded DC, blocks with and without their bit under it.  coeff_offset is compacted per macroblock (0, 256 or 768
coefficients), the macroblocks lie in a shuffled order with gaps, and macroblocks that need nothing carry offsets that would be
malformed.

Values: at 8 bits any int16_t (so the int16_t truncation between the passes is reached), above |c| <= 2^(bit_depth + 6); the chroma DC
values a, b, c, d and qmul keep (|a| + |b| + |c| + |d|) * qmul below 2^31, as the reference multiplies signed ints.  special():
one macroblock at that bound and, at 8 bits, one whose dequantised DC is truncated to int16_t.
"""
import ctypes as C
import functools

import numpy as np

import ffi
from ffmpeg_amd import h264
from h264_intra_gen import SCAN8, scan8_chroma

POISON = 0xA7                    # stride padding and guard rows of the tests' buffers
MB, RES = h264.BS_MB_DTYPE, h264.RES_MB_DTYPE
X4 = [(i & 1) + 2 * ((i >> 2) & 1) for i in range(16)]
Y4 = [((i >> 1) & 1) + 2 * (i >> 3) for i in range(16)]


def _oracle():
    O = ffi.oracle()
    u8p, i16p, ip = ffi.u8p, ffi.i16p, C.POINTER(C.c_int)
    O.ffo_h264_idct_mb_bd.argtypes = [C.c_int, C.c_int, u8p, ip, i16p, C.c_ssize_t, u8p]
    O.ffo_h264_idct_add8_bd.argtypes = [C.c_int, C.c_int, C.POINTER(u8p), ip, i16p, C.c_ssize_t, u8p]
    O.ffo_h264_chroma_dc_dequant_bd.argtypes = [C.c_int, C.c_int, i16p, C.c_int]
    return O


def sample_dtype(bd):
    return np.uint16 if bd > 8 else np.uint8


def coef_dtype(bd):
    return np.int32 if bd > 8 else np.int16


def need_of(m, r, chroma):
    """rule 2"""
    if chroma and (int(r["chroma"]) | int(r["chroma_dc"])):
        return 768
    return 256 if int(m["nnz"]) else 0


class ResPicture:
    """one picture: mb (BS_MB_DTYPE), res (RES_MB_DTYPE), coeffs, ncoeffs, and `before`, the planes as the inter face left them"""

    def __init__(self, rng, mb_w, mb_h, bd=8, chroma=True, density=0.5, p_intra=0.12, p_t8=0.3, wild=0.3):
        self.mb_w, self.mb_h, self.bd, self.chroma = mb_w, mb_h, bd, chroma
        self.rng, self.wild = rng, wild
        n = mb_w * mb_h
        self.lim = 32767 if bd == 8 else 1 << (bd + 6)
        self.before = [rng.integers(0, 1 << bd, (16 * mb_h, 16 * mb_w)).astype(sample_dtype(bd))]
        if chroma:
            self.before += [rng.integers(0, 1 << bd, (8 * mb_h, 8 * mb_w)).astype(sample_dtype(bd)) for _ in range(2)]
        self.mb = np.zeros(n, MB)
        self.res = np.zeros(n, RES)
        self.mb["slice"] = rng.integers(0, 65536, n)              # rule 12: not looked at
        self.mb["qp"] = rng.integers(0, 256, n)
        self.mb["pad"] = rng.integers(0, 256, (n, 2))
        self.res["pad"] = rng.integers(0, 256, (n, 2))
        self.res["qmul"] = rng.integers(1, 1 << 17, (n, 2))
        self.blocks = [np.zeros(768, np.int64) for _ in range(n)]  # the coded content, sl->mb layout
        for m in range(n):
            intra, t8 = rng.random() < p_intra, rng.random() < p_t8
            self.mb["flags"][m] = intra | (t8 << 1) | (int(rng.integers(0, 64)) << 2)
            d = density if rng.random() < 0.8 else (0.0 if rng.random() < 0.5 else 1.0)
            if t8:
                for k in range(4):
                    if rng.random() < d:
                        self.set_luma8(m, k)
            else:
                for i in range(16):
                    if rng.random() < d:
                        self.set_luma4(m, i)
            if rng.random() < 0.6 and d > 0:
                for c in range(2):
                    self.set_chroma(m, c, dc=rng.random() < 0.6, bits=[j for j in range(4) if rng.random() < d])
        self.layout()

    # ---- content ----
    def _values(self, nco, kind=None):
        rng = self.rng
        v = np.zeros(nco, np.int64)
        kind = rng.choice(["dc", "ac1", "many"], p=[0.25, 0.15, 0.6]) if kind is None else kind
        big = rng.random() < self.wild
        lim = self.lim if big else 400 << max(self.bd - 8, 0)
        draw = lambda k: rng.integers(-lim, lim + 1, k)
        if kind == "dc":
            v[0] = draw(1)[0] or 77
        elif kind == "ac1":
            v[int(rng.integers(1, nco))] = draw(1)[0] or -55
        else:
            v[:] = draw(nco)
            v[rng.random(nco) < 0.5] = 0
            v[int(rng.integers(1, nco))] = v[int(rng.integers(1, nco))] or 9
        return v

    def set_luma4(self, m, i, values=None, kind=None):
        self.mb["nnz"][m] |= 1 << (X4[i] + 4 * Y4[i])
        self.blocks[m][16 * i:16 * i + 16] = self._values(16, kind) if values is None else values

    def set_luma8(self, m, k, values=None, kind=None):
        for i in range(4 * k, 4 * k + 4):                         # the FFHipH264BsMb contract: all four bits
            self.mb["nnz"][m] |= 1 << (X4[i] + 4 * Y4[i])
        self.blocks[m][64 * k:64 * k + 64] = self._values(64, kind) if values is None else values

    def set_chroma(self, m, c, dc, bits, qmul=None):
        rng, b = self.rng, self.blocks[m]
        for j in bits:
            self.res["chroma"][m] |= 1 << (4 * c + j)
            b[256 * (1 + c) + 16 * j:256 * (1 + c) + 16 * j + 16] = self._values(16)
        if dc:
            self.res["chroma_dc"][m] |= 1 << c
            lim = self.lim if rng.random() < self.wild else 300 << max(self.bd - 8, 0)
            dcs = rng.integers(-lim, lim + 1, 4)
            dcs[rng.random(4) < 0.2] = 0
            b[256 * (1 + c):256 * (2 + c):16][:4] = dcs
            top = ((1 << 31) - 1) // max(int(np.abs(dcs).sum()), 1)
            self.res["qmul"][m][c] = int(rng.integers(1, min(top, 1 << 17) + 1)) if qmul is None else qmul
        elif rng.random() < 0.5:                                  # a decoder leaves 0 there; the transform takes what it finds
            for j in bits:
                b[256 * (1 + c) + 16 * j] = 0

    # ---- coeffs and coeff_offset from the content ----
    def layout(self, shuffle=True):
        rng, n = self.rng, self.mb_w * self.mb_h
        need = [need_of(self.mb[m], self.res[m], self.chroma) for m in range(n)]
        order = rng.permutation(n) if shuffle else np.arange(n)
        at = 16 * int(rng.integers(0, 3))
        for m in order:
            if need[m]:
                self.res["coeff_offset"][m] = at
                at += need[m] + 16 * int(rng.integers(0, 2))
            else:                                                 # need 0: nothing happens whatever the offset says
                self.res["coeff_offset"][m] = rng.choice([-16, 7, 1 << 30, 0])
        # the macroblock that lies last ends with coeffs: the exact fit
        self.ncoeffs = max((int(self.res["coeff_offset"][m]) + need[m] for m in range(n) if need[m]), default=0)
        lim = 32767 if self.bd == 8 else 1 << (self.bd + 6)
        self.coeffs = rng.integers(-lim, lim + 1, max(self.ncoeffs, 16)).astype(coef_dtype(self.bd))   # noise under every uncoded block
        for m in range(n):
            if need[m]:
                o = int(self.res["coeff_offset"][m])
                coded = self.coded_mask(m)[:need[m]]
                self.coeffs[o:o + need[m]][coded] = self.blocks[m][:need[m]][coded]

    def coded_mask(self, m):
        """which of the 768 coefficients of macroblock m the rules read"""
        k = np.zeros(768, bool)
        nnz, t8 = int(self.mb["nnz"][m]), (int(self.mb["flags"][m]) >> 1) & 1
        for i in range(16):
            top = 4 * (i >> 2) if t8 else i
            if (nnz >> (X4[top] + 4 * Y4[top])) & 1:
                k[16 * i:16 * i + 16] = True
        if self.chroma:
            ch, cdc = int(self.res["chroma"][m]), int(self.res["chroma_dc"][m])
            for c in range(2):
                for j in range(4):
                    o = 256 * (1 + c) + 16 * j
                    if (ch >> (4 * c + j)) & 1:
                        k[o:o + 16] = True
                    elif (cdc >> c) & 1:
                        k[o] = True
        return k


def blank(mb_w, mb_h, bd=8, chroma=True, seed=1):
    """a picture without any residual, for hand-written cases: set_luma4 / set_luma8 / set_chroma, then layout()"""
    rng = np.random.default_rng(seed)
    pic = ResPicture(rng, mb_w, mb_h, bd, chroma, density=0.0, p_intra=0.0, p_t8=0.0, wild=0.0)
    pic.mb["flags"] = 0
    return pic


def special(pic):
    """macroblock 0: Cb at the multiplication's bound; macroblock 1 (8 bits): a dequantised Cr DC that int16_t truncates"""
    for m in range(min(2, pic.mb_w * pic.mb_h)):
        pic.mb["flags"][m] &= 0xFE
    lim = pic.lim
    pic.set_chroma(0, 0, dc=True, bits=[1])
    dcs = np.array([lim, -lim, lim // 2, -3])
    pic.blocks[0][256:512:16][:4] = dcs
    pic.res["qmul"][0][0] = ((1 << 31) - 1) // int(np.abs(dcs).sum())
    if pic.mb_w * pic.mb_h > 1:
        pic.set_chroma(1, 1, dc=True, bits=[2])
        pic.blocks[1][512:768:16][:4] = [30000, 0, -250, 0] if pic.bd == 8 else [3000, 1, 2, 3]
        pic.res["qmul"][1][1] = 4000
    pic.layout()
    return pic


def malformed(m, r, chroma, ncoeffs):
    """rule 3"""
    o = int(r["coeff_offset"])
    return o < 0 or o % 16 != 0 or o + need_of(m, r, chroma) > ncoeffs


def model(pic, has_chroma=None, lists=None):
    """(the planes after the residual, coverage): pic.before with the oracle's dispatchers run macroblock by macroblock; `lists`
    collects every such macroblock's dense sl->mb copy and nnzc cache as they are before the calls"""
    O = _oracle()
    bd, chroma = pic.bd, pic.chroma if has_chroma is None else has_chroma
    ps, cdt = (2 if bd > 8 else 1), coef_dtype(bd)
    want = [p.copy() for p in pic.before]
    sy = want[0].strides[0]
    sc = want[1].strides[0] if chroma else 0
    bo = np.zeros(48, np.int32)
    for i in range(16):
        bo[i] = 4 * Y4[i] * sy + 4 * X4[i] * ps
    for j in (1, 2):
        for k in range(4):
            bo[16 * j + k] = (k >> 1) * 4 * sc + (k & 1) * 4 * ps
    bop = bo.ctypes.data_as(C.POINTER(C.c_int))
    i16 = lambda a, at=0: C.cast(a.ctypes.data + at * a.itemsize, ffi.i16p)
    cover = {k: 0 for k in ("intra", "none", "malformed", "luma_only", "with_chroma", "t8", "blk4_dc", "blk4_ac1", "blk4_many", "blk8_dc",
                            "blk8_ac1", "blk8_many", "blk8_off", "cdc", "cdc_block_without_bit", "cdc_block_with_bit", "c_block", "dc_bound",
                            "dc_trunc")}
    for m in range(pic.mb_w * pic.mb_h):
        M, R = pic.mb[m], pic.res[m]
        if int(M["flags"]) & 1:
            cover["intra"] += 1
            continue
        need = need_of(M, R, chroma)
        if not need:
            cover["none"] += 1
            continue
        if malformed(M, R, chroma, pic.ncoeffs):
            cover["malformed"] += 1
            continue
        cover["with_chroma" if need == 768 else "luma_only"] += 1
        o = int(R["coeff_offset"])
        t8, nnz = (int(M["flags"]) >> 1) & 1, int(M["nnz"])
        dense, nnzc = np.zeros(768, cdt), np.zeros(120, np.uint8)
        for i in range(16):
            top = 4 * (i >> 2) if t8 else i
            if not (nnz >> (X4[top] + 4 * Y4[top])) & 1:
                cover["blk8_off"] += t8 and i % 4 == 0 and nnz != 0
                continue
            dense[16 * i:16 * i + 16] = pic.coeffs[o + 16 * i:o + 16 * i + 16]
        for i in range(16):
            blk = dense[64 * (i >> 2):64 * (i >> 2) + 64] if t8 else dense[16 * i:16 * i + 16]
            top = 4 * (i >> 2) if t8 else i
            if (nnz >> (X4[top] + 4 * Y4[top])) & 1:
                cnt = max(1, int(np.count_nonzero(blk)))
                nnzc[SCAN8[i]] = min(cnt, 64)
                if not t8 or i % 4 == 0:
                    kind = "dc" if cnt == 1 and blk[0] else "ac1" if cnt == 1 else "many"
                    cover["blk%d_%s" % (8 if t8 else 4, kind)] += 1
        cover["t8"] += t8
        ch, cdc = (int(R["chroma"]), int(R["chroma_dc"])) if need == 768 else (0, 0)
        for c in range(2):
            base = 256 * (1 + c)
            for j in range(4):
                if (ch >> (4 * c + j)) & 1:
                    dense[base + 16 * j:base + 16 * j + 16] = pic.coeffs[o + base + 16 * j:o + base + 16 * j + 16]
                    nnzc[scan8_chroma(1 + c, j)] = max(1, int(np.count_nonzero(dense[base + 16 * j + 1:base + 16 * j + 16])))
                    cover["c_block"] += 1
                    cover["cdc_block_with_bit"] += (cdc >> c) & 1
                elif (cdc >> c) & 1:
                    dense[base + 16 * j] = pic.coeffs[o + base + 16 * j]
                    cover["cdc_block_without_bit"] += 1
        if lists is not None:                                     # what a caller of the per-call batch faces assembles
            lists.append(dict(m=m, t8=t8, need=need, dense=dense.copy(), nnzc=nnzc.copy(), cdc=cdc, qmul=[int(q) for q in R["qmul"]]))
        my, mx = divmod(m, pic.mb_w)
        O.ffo_h264_idct_mb_bd(bd, t8, C.cast(want[0].ctypes.data + my * 16 * sy + mx * 16 * ps, ffi.u8p), bop, i16(dense), sy, ffi.ptr(nnzc))
        if need != 768:
            continue
        for c in range(2):
            base = 256 * (1 + c)
            if (cdc >> c) & 1:
                cover["cdc"] += 1
                q = int(R["qmul"][c])
                dcs = dense[base:base + 64:16].astype(np.int64)
                s = int(np.abs(dcs).sum()) * q
                assert s < 1 << 31, "the generator broke the multiplication's bound"
                cover["dc_bound"] += s + int(np.abs(dcs).sum()) >= 1 << 31      # one more step of qmul would overflow
                h = np.array([dcs[0] + dcs[1] + dcs[2] + dcs[3], dcs[0] - dcs[1] + dcs[2] - dcs[3], dcs[0] + dcs[1] - dcs[2] - dcs[3],
                              dcs[0] - dcs[1] - dcs[2] + dcs[3]])
                cover["dc_trunc"] += bd == 8 and bool((np.abs((h * q) >> 7) > 32767).any())
                O.ffo_h264_chroma_dc_dequant_bd(bd, 0, i16(dense, base), q)
        dd = (ffi.u8p * 2)(*[C.cast(want[1 + c].ctypes.data + my * 8 * sc + mx * 8 * ps, ffi.u8p) for c in range(2)])
        O.ffo_h264_idct_add8_bd(bd, 0, dd, bop, i16(dense), sc, ffi.ptr(nnzc))
    return want, cover


SET = {  # name: (mb_w, mb_h, depth, chroma, pictures, special)
    "1x1": (1, 1, 8, True, 3, True),
    "3x2": (3, 2, 8, True, 3, True),
    "5x4_10": (5, 4, 10, True, 2, True),
    "11x9": (11, 9, 8, True, 1, False),
    "11x9_9": (11, 9, 9, True, 1, False),
    "11x9_10": (11, 9, 10, True, 1, True),
    "11x9_12": (11, 9, 12, True, 1, False),
    "11x9_14": (11, 9, 14, True, 1, True),
    "3x2_mono": (3, 2, 8, False, 2, False),
    "3x2_mono_10": (3, 2, 10, False, 1, False),
    "3x2_x17": (3, 2, 8, True, 17, False),
    "121x1": (121, 1, 8, True, 1, False),
    "1x70": (1, 70, 10, True, 1, False),
}
NAMES = list(SET)
CPU_NAMES = NAMES[:10]


@functools.lru_cache(maxsize=None)
def picture_set(name):
    """(pictures, models) of a set: computed once and shared, so nobody writes into them"""
    mb_w, mb_h, bd, chroma, n, sp = SET[name]
    rng = np.random.default_rng(9700 + NAMES.index(name))
    pics = []
    for k in range(n):
        p = ResPicture(rng, mb_w, mb_h, bd, chroma, density=(0.5, 0.15, 0.9)[k % 3], p_intra=0.0 if mb_w * mb_h == 1 and k == 0 else 0.12)
        pics.append(special(p) if sp and k == 0 else p)
    return pics, [model(p) for p in pics]
