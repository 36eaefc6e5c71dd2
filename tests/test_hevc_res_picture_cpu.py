"""CPU tier of the HEVC residual picture face (ffhip_hevc_residual_pictures_dev): the record ABI, the argument refusals (the overlap
refusals included), the refusal of a box without a device, the invariants of the synthetic generator, and the sequential model (the
oracle's per-call transforms in the reference's order) against an independent restatement of H.265 8.6.2 / 8.6.4.2 / 8.6.6 / 8.6.8."""
import ctypes as C

import numpy as np
import pytest

import hevc_res_picture_gen as G
from ffmpeg_amd import _lib, hevc


def test_record_sizes_match_the_c_structs():
    assert _lib.lib().ffhip_hevc_res_tu_record_size() == hevc.RES_TU_DTYPE.itemsize == G.RES_TU_DTYPE.itemsize == 16
    assert hevc.RES_TU_DTYPE == G.RES_TU_DTYPE
    assert C.sizeof(hevc.ResPlane) == 56 and C.sizeof(hevc.ResPic) == 3 * 56
    assert (hevc.RES_DCT, hevc.RES_DC, hevc.RES_DST, hevc.RES_SKIP, hevc.RES_BYPASS, hevc.RES_ZERO) == (0, 1, 2, 3, 4, 5)
    assert (hevc.RES_ROTATE, hevc.RES_RDPCM_H, hevc.RES_RDPCM_V, hevc.RES_CROSS) == (G.ROTATE, G.RDPCM_H, G.RDPCM_V, G.CROSS)


_BUFS = []


def _buf(nbytes):
    b = (C.c_uint64 * ((nbytes + 7) // 8 + 2))()
    _BUFS.append(b)
    return (C.addressof(b) + 15) & ~15


def _pics(n=1, ntus=4, ncoeffs=4096, nres=4096):
    """n pictures whose planes are distinct host buffers (only the face's host checks look at them)"""
    pics = (hevc.ResPic * n)()
    for i in range(n):
        for p in range(3):
            pl = pics[i].plane[p]
            pl.coeffs, pl.ncoeffs = _buf(2 * ncoeffs), ncoeffs
            pl.res, pl.nres = _buf(2 * nres), nres
            pl.tus = _buf(16 * ntus)
            for s, v in enumerate((0, ntus, ntus, ntus, ntus)):
                pl.size_start[s] = v
    return pics


def test_invalid_arguments():
    """FFHIP_EINVAL comes before the device check: these hold on any machine"""
    f = _lib.lib().ffhip_hevc_residual_pictures_dev
    E = _lib.EINVAL
    v = lambda pics: C.cast(pics, C.c_void_p)
    ok = v(_pics())
    assert f(9, 1, 1, ok, None) == E          # depth
    assert f(8, 4, 1, ok, None) == E          # chroma format
    assert f(8, -1, 1, ok, None) == E
    assert f(8, 1, 0, ok, None) == E          # npics
    assert f(8, 1, -1, ok, None) == E
    assert f(8, 1, 1, None, None) == E
    for field in ("coeffs", "res", "tus"):     # NULL or misaligned pointers of a used plane
        for val in (None, "mis"):
            pics = _pics()
            setattr(pics[0].plane[1], field, getattr(pics[0].plane[1], field) + 2 if val else None)
            assert f(8, 1, 1, v(pics), None) == E, (field, val)
    for field in ("ncoeffs", "nres"):          # negative lengths
        pics = _pics()
        setattr(pics[0].plane[0], field, -16)
        assert f(8, 1, 1, v(pics), None) == E, field
    pics = _pics()                              # size_start not starting at 0
    pics[0].plane[2].size_start[0] = 1
    assert f(8, 1, 1, v(pics), None) == E
    pics = _pics()                              # decreasing
    pics[0].plane[0].size_start[2] = 1
    assert f(8, 1, 1, v(pics), None) == E


def test_overlap_refusals():
    f = _lib.lib().ffhip_hevc_residual_pictures_dev
    E = _lib.EINVAL
    v = lambda pics: C.cast(pics, C.c_void_p)
    pics = _pics(2)                             # res over its own plane's coeffs
    pics[0].plane[0].res = pics[0].plane[0].coeffs
    assert f(8, 1, 2, v(pics), None) == E
    pics = _pics(2)                             # res over another picture's coeffs, partly
    pics[1].plane[2].res = pics[0].plane[1].coeffs + 2 * 4000
    assert f(8, 1, 2, v(pics), None) == E
    pics = _pics(2)                             # res over another plane's res
    pics[0].plane[2].res = pics[0].plane[1].res + 2 * 16
    assert f(8, 1, 2, v(pics), None) == E
    pics = _pics(2)                             # res over another picture's res
    pics[1].plane[0].res = pics[0].plane[0].res
    assert f(8, 1, 2, v(pics), None) == E
    pics = _pics(2)                             # shared coeffs are read only: allowed (ENOSYS here, not EINVAL)
    pics[1].plane[0].coeffs = pics[0].plane[0].coeffs
    assert f(8, 1, 2, v(pics), None) != E
    pics = _pics(1)                             # chroma format 0: planes 1 and 2 are not looked at
    pics[0].plane[1].res = pics[0].plane[0].res
    pics[0].plane[2].coeffs = None
    assert f(8, 0, 1, v(pics), None) != E
    pics = _pics(1)                             # a plane without records is not looked at
    for s in range(5):
        pics[0].plane[2].size_start[s] = 0
    pics[0].plane[2].res = pics[0].plane[0].res
    assert f(8, 1, 1, v(pics), None) != E


def test_no_device_is_enosys():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    pics = _pics(17)
    for cfi in range(4):
        for bd in (8, 10, 12):
            assert _lib.lib().ffhip_hevc_residual_pictures_dev(bd, cfi, 17, C.cast(pics, C.c_void_p), None) == _lib.ENOSYS


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("log2", [2, 3, 4, 5])
def test_scans_cover_the_block(kind, log2):
    order = G.scan_order(log2, kind)
    n = 1 << log2
    assert sorted(order) == [(x, y) for x in range(n) for y in range(n)]
    assert order[0] == (0, 0)
    # inside every 4x4 sub-block the scan is that of the 4x4 block
    assert [(x % 4, y % 4) for x, y in order[:16]] == G._scan4(kind)


def test_col_limit_matches_cabac():
    assert G.col_limit_of(1, 0) == 4 and G.col_limit_of(3, 3) == 4 and G.col_limit_of(0, 2) == 4
    assert G.col_limit_of(4, 0) == 8 and G.col_limit_of(7, 7) == 8
    assert G.col_limit_of(8, 0) == 12 and G.col_limit_of(11, 11) == 24
    assert G.col_limit_of(12, 0) == 16 and G.col_limit_of(31, 31) == 66


def test_generator_invariants():
    rng = np.random.default_rng(3)
    for cfi in range(4):
        planes = G.build_planes(rng, [[60, 30, 12, 4], [20, 10, 4, 2], [20, 10, 4, 2]], cfi)
        assert len(planes) == (3 if cfi else 1)
        kinds = set()
        for p, D in enumerate(planes):
            assert D.size_start[0] == 0 and all(a <= b for a, b in zip(D.size_start, D.size_start[1:]))
            assert D.size_start[4] == len(D.tus)
            spans = []
            for k, t in enumerate(D.tus):
                assert G.record_ok(planes, p, k, cfi)
                n = 1 << int(t["log2_size"])
                assert int(t["log2_size"]) == next(s for s in range(4) if D.size_start[s] <= k < D.size_start[s + 1]) + 2
                kf = int(t["kind_flags"])
                kinds.add(kf & 7)
                spans.append((int(t["res_offset"]), int(t["res_offset"]) + n * n))
                if kf & 7 == G.DCT:
                    c = D.coeffs[int(t["coeff_offset"]):int(t["coeff_offset"]) + n * n].reshape(n, n)
                    ys, xs = np.nonzero(c)
                    assert len(xs) and (xs.max() > 0 or ys.max() > 0)
                    assert int(t["col_limit"]) >= 4
                if kf & G.CROSS:
                    assert cfi == 3 and p > 0
                    lt = planes[0].tus[int(t["luma"])]
                    assert lt["log2_size"] == t["log2_size"]
            spans.sort()
            assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "res slots are disjoint"
        assert {G.DCT, G.DC, G.SKIP, G.BYPASS} <= kinds
    # the 4x4 DST, rotation, both RDPCM directions and cross-component all occur
    planes = G.build_planes(np.random.default_rng(5), [[200, 0, 0, 0]] * 3, 3)
    flags = [int(t["kind_flags"]) for D in planes for t in D.tus]
    assert any(f & 7 == G.DST for f in flags) and any(f & G.ROTATE for f in flags)
    assert any(f & G.RDPCM_H for f in flags) and any(f & G.RDPCM_V for f in flags) and any(f & G.CROSS for f in flags)
    assert any(f & G.CROSS and f & 7 == G.ZERO for f in flags)


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("cfi", [0, 1, 2, 3])
def test_model_matches_the_restatement(bd, cfi):
    rng = np.random.default_rng(100 * bd + cfi)
    for big in (False, True):
        planes = G.build_planes(rng, [[60, 24, 8, 3], [16, 8, 3, 1], [16, 8, 3, 1]], cfi, big=big)
        out = G.model(planes, bd, cfi, fill=0x5A5A)
        ref = G.restate(planes, bd, cfi)
        for (p, k), r in ref.items():
            t = planes[p].tus[k]
            n = 1 << int(t["log2_size"])
            ro = int(t["res_offset"])
            assert np.array_equal(out[p][ro:ro + n * n].astype(np.int64), r.reshape(-1)), (p, k, int(t["kind_flags"]))


def test_model_every_kind_and_flag_at_every_depth():
    """each kind alone at each size, rotation and RDPCM on skip and bypass, cross-component with every scale, against the restatement"""
    rng = np.random.default_rng(9)
    combos = [(G.DCT, 0), (G.DC, 0), (G.SKIP, 0), (G.SKIP, G.RDPCM_H), (G.SKIP, G.RDPCM_V), (G.BYPASS, 0), (G.BYPASS, G.RDPCM_H),
              (G.BYPASS, G.RDPCM_V), (G.ZERO, 0)]
    for bd in (8, 10, 12):
        for kind, fl in combos + [(G.DST, 0), (G.SKIP, G.ROTATE), (G.SKIP, G.ROTATE | G.RDPCM_V), (G.BYPASS, G.ROTATE | G.RDPCM_H)]:
            sizes = [2] if kind == G.DST or fl & G.ROTATE else [2, 3, 4, 5]
            counts = [[6 if s + 2 in sizes else 0 for s in range(4)]] * 3
            planes = G.build_planes(rng, counts, 3, p_cross=1.0, big=True, kinds=lambda r, l, p, k=kind, f=fl: (k, f) if p == 0 or k != G.DST
                                    else (G.DCT, 0))
            out = G.model(planes, bd, 3)
            for (p, k), r in G.restate(planes, bd, 3).items():
                t = planes[p].tus[k]
                ro, n = int(t["res_offset"]), 1 << int(t["log2_size"])
                assert np.array_equal(out[p][ro:ro + n * n].astype(np.int64), r.reshape(-1)), (bd, kind, fl, p, k)
