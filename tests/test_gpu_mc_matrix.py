"""GPU tier of the motion-compensation matrix: hevc.mc_batch, hevc.mc_w_batch and vp9.mc_batch over the cell lists of
tests/mc_matrix.py — every block shape, interpolation class, fraction and address alignment — byte for byte against the oracle,
over the WHOLE destination buffer (a store that leaves its block is a mismatch), and once more on a source whose samples outside
the footprints are complemented.  A failure names the first wrong cell (w, h, mx, my, source mod 4, destination mod 4).
The last test is the same matrix for H.264's explicit weighting (h264.weight_batch).

The oracle's output for one (list, strides, depth) is computed once and shared by the kernel variants that run on it."""
import ctypes as C
import functools

import numpy as np
import pytest

import ffi
import mc_matrix as M
from ffi import u8p

pytestmark = pytest.mark.gpu

SSTRIDE = {"s16": 1024, "sodd": 1021}     # samples; at 8 bits a multiple of 16 lets the launchers hand 16 x 16 blocks to the matrix cores
DSTRIDE = {"d4": 1200, "dodd": 1203}      # whole dwords: packed stores where the address allows; odd: per-sample stores


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _back(t, like):
    return t.cpu().numpy().view(like.dtype).reshape(like.shape)


class _Case:
    """one list laid out, its sample planes, records and the oracle's output (read-only: shared between tests)"""


@functools.lru_cache(maxsize=2)
def _hevc_case(chroma, mode, bd, ss, sd):
    from ffmpeg_amd import hevc
    c = _Case()
    c.b = b = M.lay_out_hevc(chroma, mode, ss, sd)
    seed = 100 * bd + 10 * chroma + mode
    c.src, c.dst0, c.s2 = b.source(bd, seed), b.destination(bd, seed + 1), b.src2(seed + 2)
    c.want = M.hevc_want(b, chroma, mode, bd, c.src, c.dst0, c.s2)
    ps = c.src.itemsize
    n = len(b.cells)
    rec = np.zeros(n, hevc.MC_DTYPE if mode < 2 else hevc.MCW_DTYPE)
    for i, k in enumerate(b.cells):
        rec[i]["dst_offset"], rec[i]["src_offset"] = b.dst_offset(i, ps), b.src_offset(i, ps)
        rec[i]["width"], rec[i]["height"], rec[i]["mx"], rec[i]["my"] = k.w, k.h, k.mx, k.my
        if mode >= 2:
            rec[i]["src2_offset"] = b.s2pos[i]
            rec[i]["denom"], rec[i]["wx0"], rec[i]["wx1"], rec[i]["ox"] = k.wt
    c.rec = rec.view(np.uint8).reshape(n, rec.itemsize).copy()
    for a in (c.src, c.dst0, c.s2, c.want, c.rec):
        a.setflags(write=False)
    # not vacuous: the oracle changed most samples of the blocks and nothing else; the clips and the 14-bit extremes fire
    ins = b.inside()
    assert (c.want[ins] != c.dst0[ins]).mean() > .5
    assert np.array_equal(c.want[~ins], c.dst0[~ins])
    maxv = (1 << bd) - 1
    if mode == 0:
        assert c.want[ins].max() > maxv << (14 - bd) and c.want[ins].min() < 0
    else:
        assert (c.want[ins] == 0).any() and (c.want[ins] == maxv).any()
    return c


def _hevc_run(c, chroma, mode, bd, src):
    from ffmpeg_amd import hevc
    torch = _torch()
    b, ps, n = c.b, c.src.itemsize, len(c.b.cells)
    d_dst, d_src, d_rec = _dev(torch, c.dst0), _dev(torch, src), torch.from_numpy(c.rec.copy()).cuda()
    if mode < 2:
        hevc.mc_batch(chroma, mode, d_dst, b.dstride * ps, d_src, b.sstride * ps, d_rec, n, bit_depth=bd)
    else:
        hevc.mc_w_batch(chroma, mode, d_dst, b.dstride * ps, d_src, b.sstride * ps, _dev(torch, c.s2) if mode != 2 else None, d_rec, n, bit_depth=bd)
    torch.cuda.synchronize()
    return _back(d_dst, c.dst0)


HEVC8 = [(0, ss, sd) for ss in ("s16", "sodd") for sd in ("d4", "dodd")] + [(1, "sodd", sd) for sd in ("d4", "dodd")]


@pytest.mark.parametrize("old", ["default", "1"])
@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("chroma,ss,sd", HEVC8)
def test_hevc_matrix(chroma, ss, sd, mode, old, monkeypatch):
    """put (0), uni (1), uni_w (2), bi (3), bi_w (4) at 8 bits.  Luma with a source stride of whole 16 bytes (and, but for put, a
    destination stride of whole dwords) splits between k_hevc_qpel_m and k_hevc_mc<.., SKIP16>: the 16 x 16 records lie scattered
    in a batch that is no multiple of 64.  old = 1: the sample-per-lane kernel (FFHIP_HEVC_MC_OLD, the measure build)"""
    if old != "default":
        monkeypatch.setenv("FFHIP_HEVC_MC_OLD", old)
    c = _hevc_case(chroma, mode, 8, SSTRIDE[ss], DSTRIDE[sd])
    bad = c.b.first_bad(_hevc_run(c, chroma, mode, 8, c.src), c.want)
    assert bad is None, bad


@pytest.mark.parametrize("bd", [10, 12])
@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("chroma", [0, 1])
def test_hevc_matrix_hbd(chroma, mode, bd):
    """the same lists on 16-bit samples: offsets and strides in bytes (the address residues are those of the samples, doubled)"""
    c = _hevc_case(chroma, mode, bd, SSTRIDE["sodd"], DSTRIDE["dodd"])
    bad = c.b.first_bad(_hevc_run(c, chroma, mode, bd, c.src), c.want)
    assert bad is None, bad


@functools.lru_cache(maxsize=2)
def _vp9_case(filt, bd, ss, sd):
    from ffmpeg_amd import vp9
    c = _Case()
    c.b = b = M.lay_out_vp9(filt, ss, sd)
    seed = 100 * bd + 50 + filt
    c.src, c.dst0 = b.source(bd, seed), b.destination(bd, seed + 1)
    c.want = M.vp9_want(b, bd, c.src, c.dst0)
    ps = c.src.itemsize
    rec = np.array([(b.dst_offset(i, ps), b.src_offset(i, ps), k.w, k.h, k.filt, k.mx, k.my, k.avg, (0, 0)) for i, k in enumerate(b.cells)],
                   vp9.MC_DTYPE)
    c.rec = rec.view(np.uint8).reshape(len(rec), 16).copy()
    for a in (c.src, c.dst0, c.want, c.rec):
        a.setflags(write=False)
    ins = b.inside()
    assert (c.want[ins] != c.dst0[ins]).mean() > .5
    assert np.array_equal(c.want[~ins], c.dst0[~ins])
    assert (c.want[ins] == 0).any() and (c.want[ins] == (1 << bd) - 1).any()
    return c


def _vp9_run(c, bd, src):
    from ffmpeg_amd import vp9
    torch = _torch()
    b, ps = c.b, c.src.itemsize
    d_dst = _dev(torch, c.dst0)
    vp9.mc_batch(d_dst, b.dstride * ps, _dev(torch, src), b.sstride * ps, torch.from_numpy(c.rec.copy()).cuda(), len(b.cells), bit_depth=bd)
    torch.cuda.synchronize()
    return _back(d_dst, c.dst0)


@pytest.mark.parametrize("m", ["default", "0"])
@pytest.mark.parametrize("sd", ["d4", "dodd"])
@pytest.mark.parametrize("ss", ["s16", "sodd"])
@pytest.mark.parametrize("filt", [0, 1, 2, 3])
def test_vp9_matrix(filt, ss, sd, m, monkeypatch):
    """smooth, regular, sharp, bilinear at 8 bits; s16 with d4 splits between k_vp9_mc_m and k_vp9_mc<SKIP16>; m = 0: without the
    matrix-core kernel (FFHIP_VP9_MC_M, the measure build)"""
    if m != "default":
        monkeypatch.setenv("FFHIP_VP9_MC_M", m)
    c = _vp9_case(filt, 8, SSTRIDE[ss], DSTRIDE[sd])
    bad = c.b.first_bad(_vp9_run(c, 8, c.src), c.want)
    assert bad is None, bad


@pytest.mark.parametrize("bd", [10, 12])
@pytest.mark.parametrize("filt", [0, 1, 2, 3])
def test_vp9_matrix_hbd(filt, bd):
    c = _vp9_case(filt, bd, SSTRIDE["sodd"], DSTRIDE["dodd"])
    bad = c.b.first_bad(_vp9_run(c, bd, c.src), c.want)
    assert bad is None, bad


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("chroma,mode", [(0, 1), (1, 4)])
def test_hevc_poison(chroma, mode, bd):
    """luma uni (at 8 bits: both the matrix-core kernel and k_hevc_mc<.., SKIP16>) and chroma bi_w: nothing outside a block's
    footprint reaches its samples.  The kernels' documented over-reads (whole dwords, aligned 16-byte chunks) land in the slack."""
    ss, sd = (SSTRIDE["s16"], DSTRIDE["d4"]) if bd == 8 and not chroma else (SSTRIDE["sodd"], DSTRIDE["dodd"])
    c = _hevc_case(chroma, mode, bd, ss, sd)
    poisoned = c.b.poisoned(c.src, bd)
    assert (poisoned != c.src).mean() > .3
    first, second = _hevc_run(c, chroma, mode, bd, c.src), _hevc_run(c, chroma, mode, bd, poisoned)
    bad = c.b.first_bad(first, c.want)
    assert bad is None, bad
    bad = c.b.first_bad(second, first)
    assert bad is None, "poisoned source: " + bad


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("filt", [1, 3])
def test_vp9_poison(filt, bd):
    """regular (put and avg blocks; at 8 bits both k_vp9_mc_m and k_vp9_mc<SKIP16>) and bilinear"""
    ss, sd = (SSTRIDE["s16"], DSTRIDE["d4"]) if bd == 8 else (SSTRIDE["sodd"], DSTRIDE["dodd"])
    c = _vp9_case(filt, bd, ss, sd)
    assert sum(k.avg for k in c.b.cells) > 500
    poisoned = c.b.poisoned(c.src, bd)
    assert (poisoned != c.src).mean() > .3
    first, second = _vp9_run(c, bd, c.src), _vp9_run(c, bd, poisoned)
    bad = c.b.first_bad(first, c.want)
    assert bad is None, bad
    bad = c.b.first_bad(second, first)
    assert bad is None, "poisoned source: " + bad


# ---------------------------------------------------------------------------------------------------------------------------
# H.264 explicit weighting: weight_h264_pixels / biweight_h264_pixels through h264.weight_batch
# ---------------------------------------------------------------------------------------------------------------------------
def h264_weight_cells():
    """(w_idx, height, log2_denom, bi, weightd, weights, offset): every w_idx x height x log2_denom x {weight, biweight} with the
    weights at -128, -1, 0, 1, 127 (biweight: every pair), the offsets at -128, 0, 127, and one random draw each"""
    rng = np.random.default_rng(12)
    ladder, offs = [-128, -1, 0, 1, 127], [-128, 0, 127]
    cells = []
    for w_idx in range(4):
        for h in (2, 4, 8, 16):
            for ld in range(8):
                for wd in ladder:
                    for o in offs:
                        cells.append((w_idx, h, ld, 0, wd, 0, o))
                        for ws in ladder:
                            cells.append((w_idx, h, ld, 1, wd, ws, o))
                for bi in (0, 1):
                    cells.append((w_idx, h, ld, bi) + tuple(int(v) for v in rng.integers(-128, 128, 3)))
    return cells


def test_h264_weight_matrix():
    from ffmpeg_amd import h264
    from test_gpu_h264 import WEIGHT_DT
    torch = _torch()
    cells = h264_weight_cells()
    n = len(cells)
    assert n == 4 * 4 * 8 * (15 + 75 + 2)
    S, stride = 4, 1083                                          # slack round a 16 x 16 slot; one stride for both planes, odd
    sw, sh = 16 + 2 * S + 3, 16 + 2 * S
    per_row = stride // sw
    rows = (n + per_row - 1) // per_row * sh
    rng = np.random.default_rng(13)
    dst0 = rng.integers(0, 256, (rows, stride), dtype=np.uint8)
    src = rng.integers(0, 256, (rows, stride), dtype=np.uint8)
    rec = np.zeros(n, WEIGHT_DT)
    geo = []
    for i, (w_idx, h, ld, bi, wd, ws, o) in enumerate(cells):
        y, x = (i // per_row) * sh, (i % per_row) * sw
        if i % 7 == 1:                                           # bands at the ends of the range: both clips, on both operands
            dst0[y:y + sh, x:x + sw] = rng.choice(np.array([0, 255], np.uint8), (sh, sw))
        elif i % 7 == 3:
            src[y:y + sh, x:x + sw] = rng.choice(np.array([0, 255], np.uint8), (sh, sw))
        elif i % 7 == 5:
            dst0[y:y + sh, x:x + sw] = 255 * (i // 7 & 1)
            src[y:y + sh, x:x + sw] = 255 * (i // 14 & 1)
        py = y + S
        px = x + S + (i + i // 6 - (py * stride + x + S)) % 4    # destination address modulo 4 in turn, for either kind
        qx = x + S + (i // 4 - (py * stride + x + S)) % 4        # and the source's, independently
        geo.append((py, px))
        rec[i] = (py * stride + px, py * stride + qx, w_idx, h, ld, bi, wd, ws, o, 0)
    for w_idx in range(4):
        for bi in (0, 1):
            assert {(int(r["dst_offset"]) % 4) for r in rec[(rec["w_idx"] == w_idx) & (rec["bi"] == bi)]} == {0, 1, 2, 3}
    want = dst0.copy()
    O = ffi.oracle()
    ins = np.zeros(dst0.shape, bool)
    for r, (py, px) in zip(rec, geo):
        w = 16 >> int(r["w_idx"])
        ins[py:py + int(r["height"]), px:px + w] = True
        pd = C.cast(want.ctypes.data + int(r["dst_offset"]), u8p)
        if r["bi"]:
            O.ffo_h264_biweight(w, pd, C.cast(src.ctypes.data + int(r["src_offset"]), u8p), stride, int(r["height"]), int(r["log2_denom"]),
                                int(r["weightd"]), int(r["weights"]), int(r["offset"]))
        else:
            O.ffo_h264_weight(w, pd, stride, int(r["height"]), int(r["log2_denom"]), int(r["weightd"]), int(r["offset"]))
    assert (want[ins] != dst0[ins]).mean() > .5
    assert np.array_equal(want[~ins], dst0[~ins])
    assert (want[ins] == 0).any() and (want[ins] == 255).any()
    d_dst = torch.from_numpy(dst0.copy()).cuda()
    h264.weight_batch(d_dst, torch.from_numpy(src).cuda(), stride, torch.from_numpy(rec.view(np.uint8).reshape(n, 20).copy()).cuda(), n)
    torch.cuda.synchronize()
    got = d_dst.cpu().numpy()
    bad = np.argwhere(got != want)
    if len(bad):
        y, x = (int(v) for v in bad[0])
        i = (y // sh) * per_row + x // sw
        assert False, "%d mismatches; first in block %d (w_idx, height, log2_denom, bi, weightd, weights, offset) = %s, dst mod 4 %d, at row %d " \
                      "column %d: got %d, want %d" % (len(bad), i, cells[i], int(rec[i]["dst_offset"]) % 4, y - geo[i][0], x - geo[i][1],
                                                      got[y, x], want[y, x])
