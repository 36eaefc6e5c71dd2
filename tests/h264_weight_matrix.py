"""The cell matrix of H.264's explicit weighting at any depth: the cells of test_gpu_mc_matrix.h264_weight_cells() (every w_idx x height
x log2_denom x {weight, biweight}, weights at -128, -1, 0, 1, 127, offsets at -128, 0, 127) laid out as that module's 8-bit test lays
them out, 16 x 16 slots with 4 samples of slack, on samples of `bd` bits, with the oracle's output (ffo_h264_weight_bd /
ffo_h264_biweight_bd).  tests/test_h264_weight_matrix_cpu.py checks that the case is not vacuous, tests/test_gpu_h264_hbd.py runs it
through ffhip_h264_weight_batch_dev_hbd.  A case is read-only; the last one made is kept."""
import ctypes as C
import functools

import numpy as np

import ffi
from ffi import u8p

DEPTHS = [8, 9, 10, 12, 14]
S, STRIDE = 4, 1083                     # slack round a 16 x 16 slot; one stride for both planes, in samples, odd
SW, SH = 16 + 2 * S + 3, 16 + 2 * S     # a slot: three more columns for the address residues
PER_ROW = STRIDE // SW


class Case:
    pass


@functools.lru_cache(maxsize=1)
def case(bd):
    from test_gpu_h264 import WEIGHT_DT
    from test_gpu_mc_matrix import h264_weight_cells
    c = Case()
    c.cells = cells = h264_weight_cells()
    c.bd, c.px = bd, 2 if bd > 8 else 1
    n, px, maxv = len(cells), c.px, (1 << bd) - 1
    dt = np.uint16 if bd > 8 else np.uint8
    rows = (n + PER_ROW - 1) // PER_ROW * SH
    rng = np.random.default_rng(130 + bd)
    dst0 = rng.integers(0, maxv + 1, (rows, STRIDE)).astype(dt)
    src = rng.integers(0, maxv + 1, (rows, STRIDE)).astype(dt)
    rec = np.zeros(n, WEIGHT_DT)
    c.geo = []
    for i, (w_idx, h, ld, bi, wd, ws, o) in enumerate(cells):
        y, x = (i // PER_ROW) * SH, (i % PER_ROW) * SW
        if i % 7 == 1:                                           # bands at the ends of the range: both clips, on both operands
            dst0[y:y + SH, x:x + SW] = rng.choice(np.array([0, maxv], dt), (SH, SW))
        elif i % 7 == 3:
            src[y:y + SH, x:x + SW] = rng.choice(np.array([0, maxv], dt), (SH, SW))
        elif i % 7 == 5:
            dst0[y:y + SH, x:x + SW] = maxv * (i // 7 & 1)
            src[y:y + SH, x:x + SW] = maxv * (i // 14 & 1)
        py = y + S
        qx0 = py * STRIDE + x + S
        pxl = x + S + (i + i // 6 - qx0) % 4                     # destination sample index modulo 4 in turn, for either kind
        qxl = x + S + (i // 4 - qx0) % 4                         # and the source's, independently
        c.geo.append((py, pxl))
        rec[i] = ((py * STRIDE + pxl) * px, (py * STRIDE + qxl) * px, w_idx, h, ld, bi, wd, ws, o, 0)
    want = dst0.copy()
    O = ffi.oracle()
    O.ffo_h264_weight_bd.argtypes = [C.c_int, C.c_int, u8p, C.c_ssize_t, C.c_int, C.c_int, C.c_int, C.c_int]
    O.ffo_h264_biweight_bd.argtypes = [C.c_int, C.c_int, u8p, u8p, C.c_ssize_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    c.inside = ins = np.zeros(dst0.shape, bool)
    for r, (py, pxl) in zip(rec, c.geo):
        w = 16 >> int(r["w_idx"])
        ins[py:py + int(r["height"]), pxl:pxl + w] = True
        pd = C.cast(want.ctypes.data + int(r["dst_offset"]), u8p)
        if r["bi"]:
            O.ffo_h264_biweight_bd(bd, w, pd, C.cast(src.ctypes.data + int(r["src_offset"]), u8p), STRIDE * px, int(r["height"]),
                                   int(r["log2_denom"]), int(r["weightd"]), int(r["weights"]), int(r["offset"]))
        else:
            O.ffo_h264_weight_bd(bd, w, pd, STRIDE * px, int(r["height"]), int(r["log2_denom"]), int(r["weightd"]), int(r["offset"]))
    c.dst0, c.src, c.want, c.rec = dst0, src, want, rec
    for a in (dst0, src, want, rec, ins):
        a.setflags(write=False)
    return c


def first_bad(c, got):
    """None, or the first wrong sample of the whole destination buffer with the cell of the slot it lies in"""
    bad = np.argwhere(got != c.want)
    if not len(bad):
        return None
    y, x = (int(v) for v in bad[0])
    i = (y // SH) * PER_ROW + x // SW
    if i >= len(c.cells):
        return "%d bits: %d mismatches; first at row %d column %d, past the last slot" % (c.bd, len(bad), y, x)
    return "%d bits: %d mismatches; first in block %d (w_idx, height, log2_denom, bi, weightd, weights, offset) = %s, dst mod 4 %d, at row %d " \
           "column %d: got %d, want %d" % (c.bd, len(bad), i, c.cells[i], int(c.rec[i]["dst_offset"]) // c.px % 4, y - c.geo[i][0], x - c.geo[i][1],
                                           got[y, x], c.want[y, x])
