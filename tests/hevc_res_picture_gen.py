"""Synthetic transform units for the residual picture face (ffhip_hevc_residual_pictures_dev), its sequential model, and an independent
restatement of H.265 8.6.2 / 8.6.4.2 / 8.6.6 / 8.6.8.

The generator builds what a decoder holds after entropy decoding: per picture and plane, TUs of every size with a realistic kind mix
(DCT, DC-only, the 4x4 luma DST, transform skip with rotation and RDPCM in both directions, transquant bypass with RDPCM, cbf-0
records) and, on 4:4:4, chroma records that use cross-component prediction from their co-located luma record.  DCT coefficients
follow a real scan: a scan order (diagonal, horizontal or vertical over 4x4 sub-blocks, H.265 6.5.3 to 6.5.5) and a last significant
position are drawn, only positions before it in scan order are filled, and col_limit is what cabac.c derives from that position.
Coefficients are packed back to back; residual slots are shuffled, with gaps between them, so that record order and layout differ.

The model runs the oracle's per-call functions record by record (ffo_hevc_idct_bd, _idct_dc_bd, _transform_4x4_luma_bd,
_dequant_bd, ffo_hevc_transform_rdpcm) with numpy rotation and cross-component.  The restatement shares nothing with it but the
standard's matrices: the transforms are matrix products with the int16 clip between the stages."""
import ctypes as C
import functools

import numpy as np

import ffi

DCT, DC, DST, SKIP, BYPASS, ZERO = 0, 1, 2, 3, 4, 5
ROTATE, RDPCM_H, RDPCM_V, CROSS = 0x08, 0x10, 0x20, 0x40
SCALES = (0, 1, -1, 2, -2, 4, -4, 8, -8)

RES_TU_DTYPE = np.dtype([("coeff_offset", np.int32), ("res_offset", np.int32), ("luma", np.int32), ("log2_size", np.uint8),
                         ("kind_flags", np.uint8), ("res_scale_val", np.int8), ("col_limit", np.uint8)])


def _oracle():
    L = ffi.oracle()
    assert L is not None, "the oracle library is not built"
    return L


# ---------------------------------------------------------------------------------------------------------------- scans and col_limit
def _scan4(kind):
    """the 4x4 scan (x, y) of scanIdx 0 diagonal (6.5.3), 1 horizontal (6.5.4), 2 vertical (6.5.5)"""
    return _scan(4, kind)


def _scan(n, kind):
    if kind == 1:
        return [(x, y) for y in range(n) for x in range(n)]
    if kind == 2:
        return [(x, y) for x in range(n) for y in range(n)]
    out = []
    for s in range(2 * n - 1):           # up-right diagonal: each anti-diagonal from bottom-left to top-right
        for y in range(n - 1, -1, -1):
            x = s - y
            if 0 <= x < n:
                out.append((x, y))
    return out


@functools.lru_cache(maxsize=None)
def scan_order(log2, kind):
    """the positions of an N x N block in scan order: sub-blocks in the scan's order, positions inside each in the same scan"""
    n = 1 << log2
    sub = _scan(n >> 2, kind)
    inner = _scan4(kind)
    return [(4 * sx + x, 4 * sy + y) for sx, sy in sub for x, y in inner]


def col_limit_of(last_x, last_y):
    """cabac.c (ff_hevc_hls_residual_coding) for a transform that is not the 4x4 DST; max_xy == 0 is idct_dc"""
    max_xy = max(last_x, last_y)
    col_limit = last_x + last_y + 4
    if max_xy < 4:
        col_limit = min(4, col_limit)
    elif max_xy < 8:
        col_limit = min(8, col_limit)
    elif max_xy < 12:
        col_limit = min(24, col_limit)
    return col_limit


def _coeff_values(rng, k, big):
    v = rng.integers(-64, 65, k)
    if big:
        v = np.where(rng.random(k) < 0.2, rng.integers(-32768, 32768, k), v * rng.integers(1, 400))
    return np.clip(v, -32768, 32767).astype(np.int16)


def dct_block(rng, log2, big=False):
    """(coefficients N*N int16, col_limit) consistent with a scan and a last significant position past DC"""
    n = 1 << log2
    kind = int(rng.integers(0, 3)) if log2 <= 3 else 0
    order = scan_order(log2, kind)
    while True:
        last = int(rng.integers(1, min(len(order), max(2, int(len(order) * rng.choice([0.05, 0.2, 0.6, 1.0]))))))
        lx, ly = order[last]
        if max(lx, ly) > 0:
            break
    c = np.zeros((n, n), np.int16)
    pos = order[:last + 1]
    vals = _coeff_values(rng, len(pos), big)
    keep = rng.random(len(pos)) < 0.5
    keep[-1] = True
    for (x, y), v, kk in zip(pos, vals, keep):
        if kk:
            c[y, x] = v if v != 0 or (x, y) != (lx, ly) else 1
    if c[ly, lx] == 0:
        c[ly, lx] = 1
    return c.reshape(-1), col_limit_of(lx, ly)


# ---------------------------------------------------------------------------------------------------------------------- generator
class ResPlane:
    """One plane of one picture: coeffs (int16), nres, tus (RES_TU_DTYPE grouped by size), size_start (5 ints)"""

    def __init__(self, coeffs, nres, tus, size_start):
        self.coeffs, self.nres, self.tus, self.size_start = coeffs, nres, tus, list(size_start)


def _record(rng, log2, kind, flags=0, col_limit=0, big=False, luma=0, scale=0):
    """(coefficients, record fields) of one TU"""
    n = 1 << log2
    if kind == DCT:
        c, col_limit = dct_block(rng, log2, big)
    elif kind == DC:
        c = np.zeros(n * n, np.int16)
        c[0] = _coeff_values(rng, 1, big)[0]
    elif kind == ZERO:
        c = np.zeros(n * n, np.int16)
    else:
        c = _coeff_values(rng, n * n, big)
        c[rng.random(n * n) < 0.5] = 0
    return c, dict(log2_size=log2, kind_flags=kind | flags, col_limit=col_limit, luma=luma, res_scale_val=scale)


def random_kind(rng, log2, plane):
    """a realistic mix: mostly DCT / DC, 4x4 luma DST, transform skip (rotation, RDPCM) and bypass (RDPCM) at a few percent"""
    u = rng.random()
    if log2 == 2 and plane == 0 and u < 0.25:
        return DST, 0
    if u < 0.55:
        return DCT, 0
    if u < 0.75:
        return DC, 0
    if u < 0.85:
        f = 0
        if log2 == 2 and rng.random() < 0.4:
            f |= ROTATE
        r = rng.random()
        f |= RDPCM_H if r < 0.3 else RDPCM_V if r < 0.6 else 0
        return SKIP, f
    if u < 0.93:
        f = ROTATE if log2 == 2 and rng.random() < 0.3 else 0
        r = rng.random()
        f |= RDPCM_H if r < 0.3 else RDPCM_V if r < 0.6 else 0
        return BYPASS, f
    return ZERO, 0


def build_planes(rng, counts, cfi, p_cross=0.5, big=False, kinds=None, gap=16):
    """one picture.  counts[p][s]: records of size 2 + s in plane p.  kinds(rng, log2, plane) -> (kind, flags) overrides the mix.
    On 4:4:4 the chroma planes get the luma plane's counts and a share p_cross of their records use cross-component prediction from
    the luma record of the same index."""
    nplanes = 3 if cfi else 1
    if cfi == 3:
        counts = [counts[0]] * 3
    planes = []
    for p in range(nplanes):
        cs, recs = [], []
        for s in range(4):
            log2 = s + 2
            for j in range(counts[p][s]):
                kind, flags = (kinds or random_kind)(rng, log2, p)
                if p == 0 and kind in (DST,) and log2 != 2:
                    kind = DCT
                scale, luma = 0, 0
                if cfi == 3 and p > 0 and rng.random() < p_cross:
                    flags |= CROSS
                    scale = int(rng.choice(SCALES))
                    luma = sum(counts[0][:s]) + j
                if kind == DST and (p != 0 or log2 != 2):
                    kind = DCT
                c, f = _record(rng, log2, kind, flags, big=big, luma=luma, scale=scale)
                cs.append(c)
                recs.append(f)
        tus = np.zeros(len(recs), RES_TU_DTYPE)
        off = 0
        for k, (c, f) in enumerate(zip(cs, recs)):
            tus[k]["coeff_offset"] = off
            off += c.size
            for key, v in f.items():
                tus[k][key] = v
        coeffs = np.concatenate(cs) if cs else np.zeros(16, np.int16)
        # residual slots in a shuffled order with gaps: sizes are multiples of 16 elements
        order = rng.permutation(len(recs))
        roff = 0
        for k in order:
            roff += gap * int(rng.integers(0, 3))
            tus[k]["res_offset"] = roff
            roff += 1 << (2 * int(tus[k]["log2_size"]))
        ss = [0]
        for s in range(4):
            ss.append(ss[-1] + counts[p][s])
        planes.append(ResPlane(coeffs, roff + gap, tus, ss))
    return planes


def planes_for_blocks(rng, blocks, nres, cfi, intra, p_cross=0.5):
    """records for transform blocks that already have residual slots, as the inter and intra picture faces' TU records give them:
    blocks[p] = [(x, y, log2, res_offset)], nres[p] the length of plane p's res buffer.  Kinds follow the mix; the 4x4 DST and
    rotation only in intra luma / intra CUs, as cabac.c applies them.  On 4:4:4 a share p_cross of the chroma records use
    cross-component prediction from the luma record at the same position and size."""
    planes, luma_at = [], {}
    for p, bl in enumerate(blocks):
        order = sorted(range(len(bl)), key=lambda k: bl[k][2])      # grouped by size, ascending
        cs, recs = [], []
        for rank, k in enumerate(order):
            x, y, log2, ro = bl[k]
            kind, flags = random_kind(rng, log2, p)
            if kind == DST and not intra:
                kind = DCT
            if not intra:
                flags &= ~ROTATE
            scale, luma = 0, 0
            if cfi == 3 and p > 0 and (x, y, log2) in luma_at and rng.random() < p_cross:
                flags |= CROSS
                scale, luma = int(rng.choice(SCALES)), luma_at[(x, y, log2)]
            if p == 0:
                luma_at[(x, y, log2)] = rank
            c, f = _record(rng, log2, kind, flags, luma=luma, scale=scale)
            f["res_offset"] = ro
            cs.append(c)
            recs.append(f)
        tus = np.zeros(len(recs), RES_TU_DTYPE)
        off = 0
        for k, (c, f) in enumerate(zip(cs, recs)):
            tus[k]["coeff_offset"] = off
            off += c.size
            for key, v in f.items():
                tus[k][key] = v
        ss = [0]
        for s in range(4):
            ss.append(ss[-1] + sum(1 for b in bl if b[2] == s + 2))
        planes.append(ResPlane(np.concatenate(cs) if cs else np.zeros(16, np.int16), nres[p], tus, ss))
    return planes


# -------------------------------------------------------------------------------------------------------------------------- model
def _i16p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int16))


def record_ok(planes, p, k, cfi):
    """the face's well-formedness rule (include/ffhip.h) for record k of plane p"""
    D = planes[p]
    t = D.tus[k]
    log2 = int(t["log2_size"])
    s = next((s for s in range(4) if D.size_start[s] <= k < D.size_start[s + 1]), None)
    kf = int(t["kind_flags"])
    kind = kf & 7
    if s is None or log2 != s + 2 or kind > ZERO or kf & 0x80:
        return False
    skipish = kind in (SKIP, BYPASS)
    if kind == DST and log2 != 2:
        return False
    if kf & ROTATE and (log2 != 2 or not skipish):
        return False
    if kf & (RDPCM_H | RDPCM_V) and (not skipish or (kf & (RDPCM_H | RDPCM_V)) == (RDPCM_H | RDPCM_V)):
        return False
    nn = 1 << (2 * log2)
    co, ro = int(t["coeff_offset"]), int(t["res_offset"])
    if co % 16 or ro % 16 or co < 0 or ro < 0 or co + nn > D.coeffs.size or ro + nn > D.nres:
        return False
    if kf & CROSS:
        if cfi != 3 or p == 0 or int(t["res_scale_val"]) not in SCALES:
            return False
        li = int(t["luma"])
        Y = planes[0]
        if not (Y.size_start[s] <= li < Y.size_start[s + 1]):
            return False
        if int(Y.tus[li]["kind_flags"]) & CROSS or not record_ok(planes, 0, li, cfi):
            return False
    return True


def unit_residual(D, k, bd, L=None):
    """record k of plane D without cross-component: rotate -> the kind's call -> RDPCM, through the oracle"""
    L = L or _oracle()
    t = D.tus[k]
    log2, kf = int(t["log2_size"]), int(t["kind_flags"])
    n = 1 << log2
    kind = kf & 7
    if kind == ZERO:
        return np.zeros(n * n, np.int16)
    c = D.coeffs[int(t["coeff_offset"]):int(t["coeff_offset"]) + n * n].copy()
    if kf & ROTATE:
        c = c[::-1].copy()
    if kind == DCT:
        L.ffo_hevc_idct_bd(C.c_int(bd), C.c_int(log2), _i16p(c), C.c_int(int(t["col_limit"])))
    elif kind == DC:
        L.ffo_hevc_idct_dc_bd(C.c_int(bd), C.c_int(log2), _i16p(c))
    elif kind == DST:
        L.ffo_hevc_transform_4x4_luma_bd(C.c_int(bd), _i16p(c))
    elif kind == SKIP:
        L.ffo_hevc_dequant_bd(C.c_int(bd), _i16p(c), C.c_int(log2))
    if kf & RDPCM_H:
        L.ffo_hevc_transform_rdpcm(_i16p(c), C.c_int(log2), C.c_int(0))
    elif kf & RDPCM_V:
        L.ffo_hevc_transform_rdpcm(_i16p(c), C.c_int(log2), C.c_int(1))
    return c


def model(planes, bd, cfi, fill=None):
    """per plane the res buffer (int16, nres elements) after the face: every well-formed record's residual; elsewhere `fill`"""
    L = _oracle()
    out = []
    for p, D in enumerate(planes):
        r = np.full(D.nres, 0 if fill is None else fill, np.int16)
        for k in range(len(D.tus)):
            if not record_ok(planes, p, k, cfi):
                continue
            t = D.tus[k]
            v = unit_residual(D, k, bd, L)
            if int(t["kind_flags"]) & CROSS:
                ry = unit_residual(planes[0], int(t["luma"]), bd, L).astype(np.int32)
                v = (v.astype(np.int32) + ((int(t["res_scale_val"]) * ry) >> 3)).astype(np.int16)
            ro = int(t["res_offset"])
            r[ro:ro + v.size] = v
        out.append(r)
    return out


# ------------------------------------------------------------------------------------------------------------------- restatement
_G = [64, 90, 90, 90, 89, 88, 87, 85, 83, 82, 80, 78, 75, 73, 70, 67, 64, 61, 57, 54, 50, 46, 43, 38, 36, 31, 25, 22, 18, 13, 9, 4]


def transmatrix(n):
    """H.265 8.6.4.2 transMatrix of size n: row k is basis function k (eq. 8-316 and the 32x32 matrix's columns)"""
    t = np.zeros((32, 32), np.int64)
    for k in range(32):
        for i in range(32):
            m = ((2 * i + 1) * k) % 128
            if k == 0:
                v = 64
            elif m < 32:
                v = _G[m]
            elif m in (32, 96):
                v = 0
            elif m < 64:
                v = -_G[64 - m]
            elif m < 96:
                v = -_G[m - 64]
            else:
                v = _G[128 - m]
            t[k, i] = v
    return t[::32 // n, :n]


DST_MATRIX = np.array([[29, 55, 74, 84], [74, 74, 0, -74], [84, -29, -74, 55], [55, -84, 74, -29]], np.int64)


def _wrap16(a):
    return ((np.asarray(a, np.int64) + 32768) % 65536 - 32768).astype(np.int64)


def restate_transform(c, m, bd):
    """8.6.4.2: the vertical stage, Clip3(coeffMin, coeffMax, (e + 64) >> 7), then the horizontal stage >> (20 - bitDepth); m[k][i]:
    basis function k at position i"""
    e = m.T @ c                                  # column j: y[i] = sum_k m[k][i] c[k][j]
    g = np.clip((e + 64) >> 7, -32768, 32767)
    r = g @ m                                    # row i: sum_k g[i][k] m[k][j]
    bds = 20 - bd
    return np.clip((r + (1 << (bds - 1))) >> bds, -32768, 32767)


def restate_unit(t, coeffs, bd):
    log2, kf = int(t["log2_size"]), int(t["kind_flags"])
    n = 1 << log2
    kind = kf & 7
    if kind == ZERO:
        return np.zeros((n, n), np.int64)
    c = coeffs[int(t["coeff_offset"]):int(t["coeff_offset"]) + n * n].astype(np.int64)
    if kf & ROTATE:                               # 7.3.8.11's rotation: x[n - 1 - i] for i in scan of the 4x4 block
        c = c[::-1]
    c = c.reshape(n, n)
    if kind in (DCT, DC):
        r = restate_transform(c, transmatrix(n), bd)
    elif kind == DST:
        r = restate_transform(c, DST_MATRIX, bd)
    elif kind == SKIP:                            # 8.6.4.2 transform skip: (c << tsShift) then the bdShift rounding, int16 storage
        ts, bds = 5 + log2, 20 - bd
        r = _wrap16(((c << ts) + (1 << (bds - 1))) >> bds)
    else:
        r = c
    if kf & RDPCM_H:                              # 8.6.8: accumulate along the rows, int16 storage
        r = _wrap16(np.cumsum(r, axis=1))
    elif kf & RDPCM_V:
        r = _wrap16(np.cumsum(r, axis=0))
    return r


def restate(planes, bd, cfi):
    """the final residual of every record of every plane, {(p, k): N x N int64}, by the standard (no col_limit shortcut)"""
    out = {}
    for p, D in enumerate(planes):
        for k in range(len(D.tus)):
            t = D.tus[k]
            r = restate_unit(t, D.coeffs, bd)
            if int(t["kind_flags"]) & CROSS:      # 8.6.6: r += (ResScaleVal * rY) >> 3
                ry = restate_unit(planes[0].tus[int(t["luma"])], planes[0].coeffs, bd)
                r = _wrap16(r + ((int(t["res_scale_val"]) * ry) >> 3))
            out[(p, k)] = r
    return out
