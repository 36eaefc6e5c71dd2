"""Pictures and models for the _fmt faces of the H.264 whole-picture inter prediction and residual (ffhip_h264_inter_pictures_fmt_dev /
_host, ffhip_h264_residual_pictures_fmt_dev / _host) at chroma_format_idc 2 (4:2:2) and 3 (4:4:4).  The generators of
h264_inter_picture_gen.py and h264_res_picture_gen.py are extended, not edited: the same slices, partitions, vectors and block
contents, with the reference and destination planes sized by the format.

The models are written from the rules of include/ffhip.h (4b / 4c of the inter face, 14 / 15 of the residual face), not from the rules
headers, and their samples are the oracle's:
  inter, 4:2:2: Cb / Cr through ffo_h264_chroma_mc_bd on w/2 x h blocks, origin + (mvx >> 3, mvy >> 2), fractions (mvx & 7, (mvy << 1) & 7),
         chroma_dy not applied; 4:4:4: Cb / Cr through ffo_h264_qpel_bd with the luma vector; the weights through ffo_h264_weight_bd /
         ffo_h264_biweight_bd of the plane's width with the chroma values.
  residual, 4:2:2: ffo_h264_chroma_dc_dequant_bd(bd, 1, ...) and ffo_h264_idct_add8_bd(bd, 1, ...) (which finds the offsets and the
         counts of the lower four blocks at i + 4); 4:4:4: ffo_h264_idct_mb_bd once per plane."""
import ctypes as C
import functools

import numpy as np

import ffi
import h264_inter_picture_gen as GI
import h264_res_picture_gen as GR
from ffmpeg_amd import h264
from h264_intra_gen import SCAN8

POISON = GI.POISON
RESF = h264.RES_MB_FMT_DTYPE
X4, Y4 = GR.X4, GR.Y4


def chroma_shape(fmt, mb_w, mb_h):
    """(rows, columns) of a chroma plane"""
    return (16 * mb_h) >> (fmt == 1), (16 * mb_w) >> (fmt != 3)


# ================================================================================================================== inter
class InterPicture(GI.InterPicture):
    """GI.InterPicture whose references' Cb / Cr have the format's size"""

    def __init__(self, rng, mb_w, mb_h, fmt, bd=8, nrefs=3, **kw):
        dt, top = GI.sample_dtype(bd), 1 << bd
        refs = [[rng.integers(0, top, (16 * mb_h, 16 * mb_w)).astype(dt)] +
                [rng.integers(0, top, chroma_shape(fmt, mb_w, mb_h)).astype(dt) for _ in range(2)] for _ in range(nrefs)]
        super().__init__(rng, mb_w, mb_h, bd=bd, chroma=True, nrefs=nrefs, refs=refs, **kw)
        self.fmt = fmt


def inter_blank(mb_w, mb_h, fmt, bd=8, nrefs=2, b=True, seed=1):
    """GI.blank at a format: all-inter, 4x4 partitions from list 0, ref_idx 0, vector (0, 0), one slice without weights"""
    pic = InterPicture(np.random.default_rng(seed), mb_w, mb_h, fmt, bd, nrefs, nslices=1, p_intra=0.0, free=True, types="B" if b else "P",
                       weights="none")
    s = pic.slices[0]
    s["num_ref"] = [nrefs, nrefs if b else 0]
    s["ref"][:] = 250
    for l in range(2 if b else 1):
        s["ref"][l][:nrefs] = np.arange(nrefs)
    s["implicit_weight"] = 32
    pic.mvf["mv"] = 0
    pic.mvf["ref_idx"] = [0, -1]
    return pic


def inter_model(pic, fill=POISON, oracle=True):
    """(want planes, plans, cover) as GI.model gives them, at pic.fmt 2 or 3 (oracle=False lists the calls without making them: the
    planes are not valid then).  cover: mcxy (size, mcxy) on luma, mcxy444 the same on
    Cb / Cr, cfrac the chroma fraction pairs, modes, sides, far (a vector component beyond +-8000 on a used list), low422 (4:2:2 chroma
    blocks whose source rows lie at or below row 8 * mb_h, where a 4:2:0 clamp would show), calls for picture_records()"""
    O = GI._oracle()
    fmt, bd, W, H = pic.fmt, pic.bd, 16 * pic.mb_w, 16 * pic.mb_h
    assert fmt in (2, 3)
    dt = GI.sample_dtype(bd)
    fillv = np.frombuffer(bytes([fill]) * 2, dt)[0]
    want = [np.full((H, W), fillv, dt)] + [np.full(chroma_shape(fmt, pic.mb_w, pic.mb_h), fillv, dt) for _ in range(2)]
    plans = np.zeros((pic.h4, pic.w4), GI.PLAN)
    cover = {"mcxy": set(), "mcxy444": set(), "cfrac": set(), "modes": set(), "parts": set(), "sides": set(), "far": 0, "low422": 0, "calls": []}
    calls = cover["calls"]
    PITCH = GI.PITCH
    stride = PITCH * np.dtype(dt).itemsize
    for i, parts in enumerate(pic.parts):
        my, mx = divmod(i, pic.mb_w)
        for by in range(4):
            for bx in range(4):
                plans[my * 4 + by, mx * 4 + bx] = GI.decide(pic, pic.mb[i], pic.mvf[my * 4 + by, mx * 4 + bx])      # rules 1, 2, 5 to 8
        if parts is None:
            continue
        for x, y, w, h, name in parts:
            f = pic.mvf[my * 4 + y // 4, mx * 4 + x // 4]
            p = plans[my * 4 + y // 4, mx * 4 + x // 4]
            mode = int(p["mode"])
            if mode == h264.INTER_SKIP:
                continue
            cover["modes"].add(mode)
            cover["parts"].add(name)
            bi = mode >= h264.INTER_BI_AVG
            lists = [0, 1] if bi else [int(p["list"])]
            px, py = mx * 16 + x, my * 16 + y
            for pl in range(3):
                as_luma = pl == 0 or fmt == 3                      # rule 3, and rule 4c on Cb / Cr
                pw, phh, ox, oy = (w, h, px, py) if as_luma else (w // 2, h, px // 2, py)          # rule 4b: 2 wide x 4 tall per 4x4 block
                dst, tmp = np.zeros((16, PITCH), dt), np.zeros((16, PITCH), dt)
                for n, L in enumerate(lists):
                    slot = int(p["slot"][n])
                    ref = pic.refs[slot][pl]
                    mvx, mvy = int(f["mv"][L][0]), int(f["mv"][L][1])
                    tgt, avg = (dst, 0) if n == 0 else (tmp, 0) if mode == h264.INTER_BI_W else (dst, 1)
                    stage = 2 if avg else int(tgt is tmp)
                    if as_luma:
                        sq = min(w, h)
                        mcxy = (mvx & 3) + ((mvy & 3) << 2)
                        cover["mcxy" if pl == 0 else "mcxy444"].add((sq, mcxy))
                        sx, sy = px + (mvx >> 2), py + (mvy >> 2)
                        if pl == 0:
                            cover["far"] += max(abs(mvx), abs(mvy)) > 8000
                            for side, out in (("left", sx - 2 < 0), ("top", sy - 2 < 0), ("right", sx + w + 3 > W), ("bottom", sy + h + 3 > H)):
                                if out:
                                    cover["sides"].add(side)
                        for qy in range(0, h, sq):
                            for qx in range(0, w, sq):
                                src = GI._window(ref, sx + qx - 2, sy + qy - 2, sq + 5, sq + 5) if oracle else dst
                                oracle and O.ffo_h264_qpel_bd(bd, avg, {16: 0, 8: 1, 4: 2}[sq], mcxy, GI._at(tgt, qy, qx), GI._at(src, 2, 2), stride)
                                calls.append(("mc", pl, stage, px + qx, py + qy, sq, sq, mcxy & 3, mcxy >> 2, slot, sx + qx, sy + qy, True))
                    else:
                        fx, fy = mvx & 7, (mvy << 1) & 7           # chroma_dy is 4:2:0's alone
                        sx, sy = ox + (mvx >> 3), oy + (mvy >> 2)
                        cover["cfrac"].add((fx, fy))
                        cover["low422"] += 8 * pic.mb_h <= sy < 16 * pic.mb_h - phh
                        src = GI._window(ref, sx, sy, pw + 1, phh + 1) if oracle else dst
                        oracle and O.ffo_h264_chroma_mc_bd(bd, avg, pw, GI._at(tgt, 0, 0), GI._at(src, 0, 0), stride, phh, fx, fy)
                        calls.append(("mc", pl, stage, ox, oy, pw, phh, fx, fy, slot, sx, sy, False))
                ld = int(p["luma_log2_denom"] if pl == 0 else p["chroma_log2_denom"])
                wt = p["luma_weight"] if pl == 0 else p["chroma_weight"][pl - 1]
                off = int(p["luma_offset"] if pl == 0 else p["chroma_offset"][pl - 1])
                if mode == h264.INTER_BI_W:
                    oracle and O.ffo_h264_biweight_bd(bd, pw, GI._at(dst, 0, 0), GI._at(tmp, 0, 0), stride, phh, ld, int(wt[0]), int(wt[1]), off)
                    calls.append(("w", pl, 1, ox, oy, pw, phh, ld, int(wt[0]), int(wt[1]), off))
                elif mode == h264.INTER_UNI_W and (pl == 0 or p["chroma_weighted"]):
                    oracle and O.ffo_h264_weight_bd(bd, pw, GI._at(dst, 0, 0), stride, phh, ld, int(wt[0]), off)
                    calls.append(("w", pl, 0, ox, oy, pw, phh, ld, int(wt[0]), 0, off))
                want[pl][oy:oy + phh, ox:ox + pw] = dst[:phh, :pw]
    return want, plans, cover


def picture_records(pic, calls, strides, ref_bytes):
    """inter_model()'s calls as the records of the picture object (h264.Picture made with chroma_format 2 or 3), in decoder order: as
    GI.picture_records, with mc_chroma blocks of up to 16 rows at 4:2:2 and mc_luma_plane / weight on plane 1 / 2 at 4:4:4"""
    ps = np.dtype(GI.sample_dtype(pic.bd)).itemsize
    out = []
    for c in calls:
        pl = c[1]
        if c[0] == "w":
            _, _, bi, x, y, w, h, ld, wd, ws, off = c
            r = np.zeros(1, h264.WEIGHT_DTYPE)
            r["dst_offset"] = r["src_offset"] = y * strides[pl] + x * ps
            r["w_idx"], r["height"], r["log2_denom"], r["bi"] = {16: 0, 8: 1, 4: 2, 2: 3}[w], h, ld, bi
            r["weightd"], r["weights"], r["offset"] = wd, ws, off
            out.append(("weight", (pl,), r))
            continue
        _, _, stage, x, y, w, h, fx, fy, slot, sx, sy, as_luma = c
        r = np.zeros(1, h264.QPEL_DTYPE if as_luma else h264.CHROMA_DTYPE)
        r["dst_offset"], r["src_offset"] = y * strides[pl] + x * ps, slot * ref_bytes[pl]
        r["flags"], r["src_x"], r["src_y"], r["avg"] = h264.MC_EMU, sx, sy, int(stage == h264.MC_AVG)
        if as_luma:
            r["mcxy"], r["size_idx"] = fx + 4 * fy, {16: 0, 8: 1, 4: 2}[w]
            out.append(("mc_luma", (stage,), r) if pl == 0 else ("mc_luma_plane", (pl, stage), r))
        else:
            r["w_idx"], r["h"], r["x"], r["y"] = {8: 0, 4: 1, 2: 2}[w], h, fx, fy
            out.append(("mc_chroma", (pl, stage), r))
    return out


#: name -> (seed, format, [InterPicture arguments per picture])
INTER_SET = {}
for _fmt in (2, 3):
    for _bd in (8, 10):
        _s = "%d_%d" % (_fmt, _bd)
        INTER_SET["1x1_" + _s] = (9801 + 10 * _fmt + _bd, _fmt, [dict(mb_w=1, mb_h=1, bd=_bd, nslices=1, p_intra=0.0, types="B")] * 3)
        INTER_SET["3x2_" + _s] = (9802 + 10 * _fmt + _bd, _fmt, [dict(mb_w=3, mb_h=2, bd=_bd)] * 3)
        INTER_SET["5x4_free_" + _s] = (9803 + 10 * _fmt + _bd, _fmt, [dict(mb_w=5, mb_h=4, bd=_bd, nslices=3, free=True, types="B")])
        INTER_SET["11x9_" + _s] = (9804 + 10 * _fmt + _bd, _fmt, [dict(mb_w=11, mb_h=9, bd=_bd, nslices=4, nrefs=5)])
    INTER_SET["3x2_x17_%d" % _fmt] = (9805 + _fmt, _fmt, [dict(mb_w=3, mb_h=2, nslices=2)] * (h264.INTER_PICS_PER_LAUNCH + 1))
INTER_NAMES = list(INTER_SET)
INTER_CPU_NAMES = [n for n in INTER_NAMES if "x17" not in n]


@functools.lru_cache(None)
def inter_set(name):
    """(pictures, [inter_model(picture)]) of a set, made once and shared: do not write to them"""
    seed, fmt, args = INTER_SET[name]
    rng = np.random.default_rng(seed)
    pics = [InterPicture(rng, fmt=fmt, **a) for a in args]
    return pics, [inter_model(p) for p in pics]


# =============================================================================================================== residual
def nnz_of_blocks(blocks):
    """the bits of a set of luma-order 4x4 blocks in FFHipH264BsMb.nnz's layout"""
    return sum(1 << (X4[i] + 4 * Y4[i]) for i in blocks)


class ResPicture(GR.ResPicture):
    """GR.ResPicture at a format.  res is a RES_MB_FMT_DTYPE view of the same records (chroma_lo422, nnz444).  4:2:2: chroma planes of
    eight blocks; 4:4:4: Cb / Cr drawn as luma planes with bits of their own."""

    def __init__(self, rng, mb_w, mb_h, fmt, bd=8, chroma=True, density=0.5, p_intra=0.12, p_t8=0.3, wild=0.3):
        self.fmt = fmt
        super().__init__(rng, mb_w, mb_h, bd, chroma=False, density=density, p_intra=p_intra, p_t8=p_t8, wild=wild)     # the luma plane
        self.chroma = chroma
        n = mb_w * mb_h
        self.resf = self.res.view(RESF)
        if chroma:
            self.before += [rng.integers(0, 1 << bd, chroma_shape(fmt, mb_w, mb_h)).astype(GR.sample_dtype(bd)) for _ in range(2)]
        self.resf["pad"] = rng.integers(0, 256, n)
        self.res["chroma"] = self.res["chroma_dc"] = 0            # the base class drew 4:2:0 chroma: dropped
        for b in self.blocks:
            b[256:] = 0
        if fmt == 3:
            self.res["chroma"], self.res["chroma_dc"] = rng.integers(0, 256, n), rng.integers(0, 256, n)       # not read
            self.resf["chroma_lo422"] = rng.integers(0, 256, n)
            self.resf["nnz444"] = 0
        else:
            self.resf["chroma_lo422"] = 0
        for m in range(n):
            d = density if rng.random() < 0.8 else (0.0 if rng.random() < 0.5 else 1.0)
            if not chroma or rng.random() >= 0.6 or d == 0:
                continue
            for c in range(2):
                if fmt == 3:
                    if (int(self.mb["flags"][m]) >> 1) & 1:
                        self.set_plane8(m, 1 + c, [k for k in range(4) if rng.random() < d])
                    else:
                        self.set_plane4(m, 1 + c, [i for i in range(16) if rng.random() < d])
                else:
                    self.set_chroma422(m, c, dc=rng.random() < 0.6, bits=[j for j in range(8) if rng.random() < d])
        if fmt == 3:
            self.resf["nnz444"] |= rng.integers(0, 1 << 16, (n, 2)).astype(np.uint32) << 16                     # the high halves are not read
        self.layout()

    # ---- content ----
    def set_plane4(self, m, pl, blocks):
        for i in blocks:
            self.resf["nnz444"][m][pl - 1] |= 1 << (X4[i] + 4 * Y4[i])
            self.blocks[m][256 * pl + 16 * i:256 * pl + 16 * i + 16] = self._values(16)

    def set_plane8(self, m, pl, blocks8):
        for k in blocks8:
            self.resf["nnz444"][m][pl - 1] |= nnz_of_blocks(range(4 * k, 4 * k + 4))
            self.blocks[m][256 * pl + 64 * k:256 * pl + 64 * k + 64] = self._values(64)

    def set_chroma422(self, m, c, dc, bits, qmul=None, dcs=None):
        rng, b = self.rng, self.blocks[m]
        base = 256 * (1 + c)
        for j in bits:
            if j < 4:
                self.res["chroma"][m] |= 1 << (4 * c + j)
            else:
                self.resf["chroma_lo422"][m] |= 1 << (4 * c + j - 4)
            b[base + 16 * j:base + 16 * j + 16] = self._values(16)
        if dc:
            self.res["chroma_dc"][m] |= 1 << c
            if dcs is None:
                lim = self.lim if rng.random() < self.wild else 300 << max(self.bd - 8, 0)
                dcs = rng.integers(-lim, lim + 1, 8)
                dcs[rng.random(8) < 0.2] = 0
            b[base:base + 128:16] = dcs
            top = ((1 << 31) - 1 - 128) // max(int(np.abs(dcs).sum()), 1)      # the reference adds 128 to the product
            self.res["qmul"][m][c] = int(rng.integers(1, min(top, 1 << 17) + 1)) if qmul is None else qmul
        elif rng.random() < 0.5:
            for j in bits:
                b[base + 16 * j] = 0

    # ---- what the rules read ----
    def need(self, m):
        return need_of(self.fmt, self.mb[m], self.resf[m], self.chroma)

    def layout(self, shuffle=True):
        if not hasattr(self, "resf"):                              # the base class's constructor: laid out again at the end of ours
            return
        rng, n = self.rng, self.mb_w * self.mb_h
        need = [self.need(m) for m in range(n)]
        order = rng.permutation(n) if shuffle else np.arange(n)
        at = 16 * int(rng.integers(0, 3))
        for m in order:
            if need[m]:
                self.res["coeff_offset"][m] = at
                at += need[m] + 16 * int(rng.integers(0, 2))
            else:
                self.res["coeff_offset"][m] = rng.choice([-16, 7, 1 << 30, 0])
        self.ncoeffs = max((int(self.res["coeff_offset"][m]) + need[m] for m in range(n) if need[m]), default=0)
        self.coeffs = rng.integers(-self.lim, self.lim + 1, max(self.ncoeffs, 16)).astype(GR.coef_dtype(self.bd))
        for m in range(n):
            if need[m]:
                o = int(self.res["coeff_offset"][m])
                coded = self.coded_mask(m)[:need[m]]
                self.coeffs[o:o + need[m]][coded] = self.blocks[m][:need[m]][coded]

    def plane_bits(self, m, pl):
        return int(self.mb["nnz"][m]) if pl == 0 else int(self.resf["nnz444"][m][pl - 1]) & 0xFFFF

    def chroma_bit(self, m, c, j):
        return (int(self.res["chroma"][m]) >> (4 * c + j)) & 1 if j < 4 else (int(self.resf["chroma_lo422"][m]) >> (4 * c + j - 4)) & 1

    def coded_mask(self, m):
        k = np.zeros(768, bool)
        t8 = (int(self.mb["flags"][m]) >> 1) & 1
        for pl in range(3 if self.fmt == 3 and self.chroma else 1):
            nnz = self.plane_bits(m, pl)
            for i in range(16):
                top = 4 * (i >> 2) if t8 else i
                if (nnz >> (X4[top] + 4 * Y4[top])) & 1:
                    k[256 * pl + 16 * i:256 * pl + 16 * i + 16] = True
        if self.chroma and self.fmt == 2:
            cdc = int(self.res["chroma_dc"][m])
            for c in range(2):
                for j in range(8):
                    o = 256 * (1 + c) + 16 * j
                    if self.chroma_bit(m, c, j):
                        k[o:o + 16] = True
                    elif (cdc >> c) & 1:
                        k[o] = True
        return k


def need_of(fmt, m, r, chroma):
    """rule 2 by format (rules 14 and 15); r: a RES_MB_FMT_DTYPE record"""
    if fmt == 3:
        c = chroma and (int(r["nnz444"][0]) | int(r["nnz444"][1])) & 0xFFFF
    else:
        c = chroma and (int(r["chroma"]) | int(r["chroma_dc"]) | (int(r["chroma_lo422"]) if fmt == 2 else 0))
    return 768 if c else 256 if int(m["nnz"]) else 0


def res_blank(mb_w, mb_h, fmt, bd=8, chroma=True, seed=1):
    """a picture without any residual, for hand-written cases: set_luma4 / set_luma8 / set_chroma422 / set_plane4 / set_plane8, then
    layout()"""
    pic = ResPicture(np.random.default_rng(seed), mb_w, mb_h, fmt, bd, chroma, density=0.0, p_intra=0.0, p_t8=0.0, wild=0.0)
    pic.mb["flags"] = pic.mb["nnz"] = 0
    pic.res["chroma"] = pic.res["chroma_dc"] = 0
    pic.resf["chroma_lo422"] = 0
    pic.resf["nnz444"] = 0
    for b in pic.blocks:
        b[:] = 0
    return pic


def res_special(pic):
    """4:2:2: macroblock 0: Cb's eight DCs at the multiplication's bound; macroblock 1 (8 bits): a dequantised Cr DC that int16_t truncates"""
    if pic.fmt != 2:
        return pic
    for m in range(min(2, pic.mb_w * pic.mb_h)):
        pic.mb["flags"][m] &= 0xFE
    lim = pic.lim
    dcs = np.array([lim, -lim, lim // 2, -3, lim, 7, -lim // 3, 0])
    pic.set_chroma422(0, 0, dc=True, bits=[1, 6], dcs=dcs, qmul=((1 << 31) - 1 - 128) // int(np.abs(dcs).sum()))
    if pic.mb_w * pic.mb_h > 1:
        pic.set_chroma422(1, 1, dc=True, bits=[2, 5], dcs=np.array([30000, 0, -250, 0, 5, 0, 0, 1] if pic.bd == 8 else [3000, 1, 2, 3, 4, 5, 6, 7]),
                          qmul=4000)
    pic.layout()
    return pic


def res_model(pic, lists=None):
    """(the planes after the residual, coverage): pic.before with the oracle's dispatchers run macroblock by macroblock; `lists`
    collects what a caller of the per-call batch faces assembles for every such macroblock: per plane that takes the luma path the
    256 dense coefficients and the 40-byte cache, at 4:2:2 the 768-coefficient image and the 120-byte cache as they are before the calls"""
    O = GR._oracle()
    fmt, bd, chroma = pic.fmt, pic.bd, pic.chroma
    assert fmt in (2, 3)
    ps, cdt = (2 if bd > 8 else 1), GR.coef_dtype(bd)
    want = [p.copy() for p in pic.before]
    strides = [w.strides[0] for w in want]
    sc = strides[1] if chroma else 0
    bo = np.zeros(48, np.int32)
    for i in range(16):
        bo[i] = 4 * Y4[i] * strides[0] + 4 * X4[i] * ps
    for j in (1, 2):
        for k in range(4):
            bo[16 * j + k] = (k >> 1) * 4 * sc + (k & 1) * 4 * ps
            bo[16 * j + 8 + k] = (2 + (k >> 1)) * 4 * sc + (k & 1) * 4 * ps     # ff_h264_idct_add8_422: the lower four at i + 4
    bop = bo.ctypes.data_as(C.POINTER(C.c_int))
    i16 = lambda a, at=0: C.cast(a.ctypes.data + at * a.itemsize, ffi.i16p)
    cover = {k: 0 for k in ("intra", "none", "malformed", "luma_only", "with_chroma", "t8", "cdc", "dc_up_with", "dc_up_without", "dc_lo_with",
                            "dc_lo_without", "c_up", "c_lo", "dc_bound", "dc_trunc", "t8_planes_differ", "plane4", "plane8", "clip_lo", "clip_hi")}
    for m in range(pic.mb_w * pic.mb_h):
        M, R = pic.mb[m], pic.resf[m]
        if int(M["flags"]) & 1:
            cover["intra"] += 1
            continue
        need = need_of(fmt, M, R, chroma)
        if not need:
            cover["none"] += 1
            continue
        o = int(R["coeff_offset"])
        if o < 0 or o % 16 or o + need > pic.ncoeffs:              # rule 3
            cover["malformed"] += 1
            continue
        cover["with_chroma" if need == 768 else "luma_only"] += 1
        t8 = (int(M["flags"]) >> 1) & 1
        cover["t8"] += t8
        my, mx = divmod(m, pic.mb_w)
        dense = np.zeros(768, cdt)
        planes = 3 if fmt == 3 and need == 768 else 1
        entry = dict(m=m, t8=t8, need=need, planes=[], cdc=int(R["chroma_dc"]), qmul=[int(q) for q in R["qmul"]])
        if lists is not None:
            lists.append(entry)
        if fmt == 3 and need == 768 and t8:
            cover["t8_planes_differ"] += len({pic.plane_bits(m, p) for p in range(3)}) == 3
        for pl in range(planes):                                   # rules 4, 5, 9; rule 15 per plane
            nnz, nnzc = pic.plane_bits(m, pl), np.zeros(120, np.uint8)
            for i in range(16):
                top = 4 * (i >> 2) if t8 else i
                if (nnz >> (X4[top] + 4 * Y4[top])) & 1:
                    dense[256 * pl + 16 * i:256 * pl + 16 * i + 16] = pic.coeffs[o + 256 * pl + 16 * i:o + 256 * pl + 16 * i + 16]
            for i in range(16):
                top = 4 * (i >> 2) if t8 else i
                if (nnz >> (X4[top] + 4 * Y4[top])) & 1:
                    blk = dense[256 * pl + 64 * (i >> 2):256 * pl + 64 * (i >> 2) + 64] if t8 else dense[256 * pl + 16 * i:256 * pl + 16 * i + 16]
                    nnzc[SCAN8[i]] = min(max(1, int(np.count_nonzero(blk))), 64)
                    cover["plane8" if t8 else "plane4"] += pl > 0 and (not t8 or i % 4 == 0)
            s = strides[pl]
            bol = np.array([4 * Y4[i] * s + 4 * X4[i] * ps for i in range(16)], np.int32)
            entry["planes"].append((dense[256 * pl:256 * pl + 256].copy(), nnzc[:40].copy()))
            O.ffo_h264_idct_mb_bd(bd, t8, C.cast(want[pl].ctypes.data + my * 16 * s + mx * 16 * ps, ffi.u8p), bol.ctypes.data_as(C.POINTER(C.c_int)),
                                  i16(dense, 256 * pl), s, ffi.ptr(nnzc))
        if fmt == 3 or need != 768:
            continue
        nnzc = np.zeros(120, np.uint8)
        cdc = int(R["chroma_dc"])
        for c in range(2):                                         # rule 14
            base = 256 * (1 + c)
            for j in range(8):
                at = SCAN8[j if j < 4 else j + 4] + 40 * (1 + c)   # scan8[16 * (1 + c) + j], the lower four at + 4
                half = "up" if j < 4 else "lo"
                if pic.chroma_bit(m, c, j):
                    dense[base + 16 * j:base + 16 * j + 16] = pic.coeffs[o + base + 16 * j:o + base + 16 * j + 16]
                    nnzc[at] = max(1, int(np.count_nonzero(dense[base + 16 * j + 1:base + 16 * j + 16])))
                    cover["c_" + half] += 1
                    cover["dc_%s_with" % half] += (cdc >> c) & 1
                elif (cdc >> c) & 1:
                    dense[base + 16 * j] = pic.coeffs[o + base + 16 * j]
                    cover["dc_%s_without" % half] += 1
            if (cdc >> c) & 1:
                cover["cdc"] += 1
                q = int(R["qmul"][c])
                dcs = dense[base:base + 128:16].astype(np.int64)
                tot = int(np.abs(dcs).sum())
                assert tot * q + 128 < 1 << 31, "the generator broke the multiplication's bound"
                cover["dc_bound"] += (tot + 0) * (q + 1) + 128 >= 1 << 31
                a, b = dcs[0::2] + dcs[1::2], dcs[0::2] - dcs[1::2]
                outs = []
                for t in (a, b):
                    z0, z1, z2, z3 = t[0] + t[2], t[0] - t[2], t[1] - t[3], t[1] + t[3]
                    outs += [z0 + z3, z1 + z2, z1 - z2, z0 - z3]
                cover["dc_trunc"] += bd == 8 and any(abs((int(v) * q + 128) >> 8) > 32767 for v in outs)
                O.ffo_h264_chroma_dc_dequant_bd(bd, 1, i16(dense, base), q)
        entry["chroma"] = (dense.copy(), nnzc.copy())               # after the DC transform: what idct_add8_422 is handed
        dd = (ffi.u8p * 2)(*[C.cast(want[1 + c].ctypes.data + my * 16 * sc + mx * 8 * ps, ffi.u8p) for c in range(2)])
        O.ffo_h264_idct_add8_bd(bd, 1, dd, bop, i16(dense), sc, ffi.ptr(nnzc))
    top = (1 << bd) - 1
    for w, b in zip(want, pic.before):
        cover["clip_lo"] += int(((w == 0) & (b != 0)).sum())
        cover["clip_hi"] += int(((w == top) & (b != top)).sum())
    return want, cover


#: name: (mb_w, mb_h, format, depth, pictures, special)
RES_SET = {}
for _fmt in (2, 3):
    for _bd in (8, 10):
        _s = "%d_%d" % (_fmt, _bd)
        RES_SET["1x1_" + _s] = (1, 1, _fmt, _bd, 3, True)
        RES_SET["3x2_" + _s] = (3, 2, _fmt, _bd, 3, True)
        RES_SET["5x4_" + _s] = (5, 4, _fmt, _bd, 1, False)
        RES_SET["11x9_" + _s] = (11, 9, _fmt, _bd, 1, True)
    for _bd in (9, 12, 14):
        RES_SET["5x4_%d_%d" % (_fmt, _bd)] = (5, 4, _fmt, _bd, 1, True)
    RES_SET["3x2_x17_%d" % _fmt] = (3, 2, _fmt, 8, h264.RES_PICS_PER_LAUNCH + 1, False)
    RES_SET["121x1_%d" % _fmt] = (121, 1, _fmt, 8, 1, False)
    RES_SET["1x70_%d" % _fmt] = (1, 70, _fmt, 10, 1, False)
RES_NAMES = list(RES_SET)
RES_CPU_NAMES = [n for n in RES_NAMES if not n.startswith(("3x2_x17", "121x1", "1x70"))]


@functools.lru_cache(None)
def res_set(name):
    """(pictures, models) of a set: computed once and shared, so nobody writes into them"""
    mb_w, mb_h, fmt, bd, n, sp = RES_SET[name]
    rng = np.random.default_rng(9900 + RES_NAMES.index(name))
    pics = []
    for k in range(n):
        p = ResPicture(rng, mb_w, mb_h, fmt, bd, density=(0.5, 0.15, 0.9)[k % 3], p_intra=0.0 if mb_w * mb_h == 1 and k == 0 else 0.12)
        pics.append(res_special(p) if sp and k == 0 else p)
    return pics, [res_model(p) for p in pics]
