"""CPU tier of the VP9 inter frame face (ffhip_vp9_inter_frames_dev): the record ABI, the argument refusals, the refusal of a box without
a device, the invariants of the synthetic frame generator, ffhip_vp9_inter_block_preds against a restatement of vp9_mc_template.h,
and the sequential model (the oracle's MC on clamped windows) against the batch faces' route (the oracle's MC on references padded
with np.pad(mode="edge"))."""
import ctypes as C

import numpy as np
import pytest

import vp9_inter_frame_gen as G
from ffmpeg_amd import _lib, vp9


def test_record_sizes_match_the_c_structs():
    L = _lib.lib()
    assert L.ffhip_vp9_inter_pred_record_size() == vp9.INTER_PRED_DTYPE.itemsize == 20
    assert L.ffhip_vp9_inter_tu_record_size() == vp9.INTER_TU_DTYPE.itemsize == 12
    assert C.sizeof(vp9.InterPlane) == 40 and C.sizeof(vp9.InterRef) == 48 and C.sizeof(vp9.InterPic) == 3 * 40 + 24 + 3 * 48


_BUFS = []


def _buf(n=1 << 16):
    b = (C.c_uint64 * n)()
    _BUFS.append(b)
    return C.addressof(b)


def _pics(n=1, nrefs=2, stride=256):
    """n frames of 64 x 64 whose planes and references are distinct host buffers (only the face's host checks look at them)"""
    pics = (vp9.InterPic * n)()
    for i in range(n):
        for p in range(3):
            pics[i].plane[p] = vp9.InterPlane(_buf(), stride, _buf(16), _buf(16), _buf(16))
        pics[i].preds, pics[i].pred_sb_start = _buf(16), _buf(16)
        pics[i].nrefs = nrefs
        for r in range(nrefs):
            for p in range(3):
                pics[i].ref[r].base[p] = _buf()
                pics[i].ref[r].stride[p] = stride
    return pics


def test_invalid_arguments():
    """FFHIP_EINVAL comes before the device check: these hold on any machine"""
    f = _lib.lib().ffhip_vp9_inter_frames_dev
    E = _lib.EINVAL
    v = lambda pics: C.cast(pics, C.c_void_p)
    ok = v(_pics())
    assert f(9, 1, 1, 64, 64, 1, ok, None) == E                 # depth
    assert f(16, 1, 1, 64, 64, 1, ok, None) == E
    assert f(8, 2, 1, 64, 64, 1, ok, None) == E                 # subsampling
    assert f(8, 1, -1, 64, 64, 1, ok, None) == E
    assert f(8, 1, 1, 0, 64, 1, ok, None) == E                  # frame size
    assert f(8, 1, 1, 64, -8, 1, ok, None) == E
    assert f(8, 1, 1, 65536, 64, 1, ok, None) == E
    assert f(8, 1, 1, 64, 64, 0, ok, None) == E                 # npics
    assert f(8, 1, 1, 64, 64, -1, ok, None) == E
    assert f(8, 1, 1, 64, 64, 1, None, None) == E
    assert f(8, 1, 1, 64, 64, 1, v(_pics(stride=258)), None) == E    # stride not 4-byte aligned
    assert f(10, 1, 1, 64, 64, 1, v(_pics(stride=260)), None) == E   # nor 8-byte above 8 bits
    assert f(8, 1, 1, 300, 64, 1, v(_pics(stride=256)), None) == E   # stride below the decoded width (304)
    assert f(8, 1, 1, 250, 64, 1, v(_pics(stride=252)), None) == E   # 252 < 256: the decoded width, not the real one
    for field in ("base", "tus", "tu_sb_start", "coeffs"):           # NULL plane pointers
        pics = _pics()
        setattr(pics[0].plane[2], field, None)
        assert f(8, 1, 1, 64, 64, 1, v(pics), None) == E, field
    pics = _pics()
    pics[0].plane[1].base += 2                                       # misaligned plane
    assert f(8, 1, 1, 64, 64, 1, v(pics), None) == E
    for field in ("preds", "pred_sb_start"):
        pics = _pics()
        setattr(pics[0], field, None)
        assert f(8, 1, 1, 64, 64, 1, v(pics), None) == E, field
    for nrefs in (0, 4, -1):
        pics = _pics()
        pics[0].nrefs = nrefs
        assert f(8, 1, 1, 64, 64, 1, v(pics), None) == E, nrefs
    pics = _pics(nrefs=3)
    pics[0].ref[2].base[1] = None                                    # a NULL base among the first nrefs
    assert f(8, 1, 1, 64, 64, 1, v(pics), None) == E
    pics = _pics(nrefs=3)
    pics[0].ref[1].base[0] += 1                                      # an odd 16-bit reference
    assert f(10, 1, 1, 64, 64, 1, v(pics), None) == E
    pics = _pics(nrefs=3)
    pics[0].ref[1].stride[2] = 16                                    # a reference stride below the width
    assert f(8, 1, 1, 64, 64, 1, v(pics), None) == E
    # a reference plane that is a destination plane of the call: of the same frame, of another one, or overlapping one
    pics = _pics(n=3)
    pics[2].ref[1].base[0] = pics[2].plane[0].base
    assert f(8, 1, 1, 64, 64, 3, v(pics), None) == E
    pics = _pics(n=3)
    pics[0].ref[0].base[2] = pics[1].plane[1].base
    assert f(8, 1, 1, 64, 64, 3, v(pics), None) == E
    pics = _pics(n=2)
    pics[1].ref[1].base[1] = pics[0].plane[0].base + 256 * 40
    assert f(8, 1, 1, 64, 64, 2, v(pics), None) == E
    # a reference slot past nrefs is not looked at: a NULL there does not stop the checks, which go on to refuse the overlap
    pics = _pics(nrefs=1)
    pics[0].ref[1].base[0] = None
    pics[0].ref[0].base[0] = pics[0].plane[0].base + 256 * 63
    assert f(8, 1, 1, 64, 64, 1, v(pics), None) == E
    assert b"overlaps" in _lib.lib().ffhip_last_error()


@pytest.mark.skipif(_lib.lib().ffhip_device_count() > 0, reason="a HIP device is present: the refusal path is not reachable")
def test_no_device_refusals():
    L = _lib.lib()
    ok = C.cast(_pics(), C.c_void_p)
    assert L.ffhip_vp9_inter_frames_dev(8, 1, 1, 64, 64, 1, ok, None) == _lib.ENOSYS
    assert L.ffhip_vp9_inter_frames_dev(12, 0, 0, 61, 57, 1, ok, None) == _lib.ENOSYS
    assert L.ffhip_vp9_inter_frames_dev(10, 1, 0, 1, 1, 1, ok, None) == _lib.ENOSYS
    pics = _pics(nrefs=1)
    pics[0].ref[2].base[0] = None                                    # past nrefs
    assert L.ffhip_vp9_inter_frames_dev(8, 0, 1, 64, 64, 1, C.cast(pics, C.c_void_p), None) == _lib.ENOSYS


GEN_CASES = [(8, 1, 1, 203, 141), (10, 1, 0, 136, 64), (12, 0, 1, 77, 99), (8, 0, 0, 64, 64), (10, 1, 1, 257, 63)]


@pytest.mark.parametrize("bd,ss_h,ss_v,W,H", GEN_CASES)
def test_generator_invariants(bd, ss_h, ss_v, W, H):
    rng = np.random.default_rng(bd * 7 + ss_h * 3 + ss_v + W)
    fr = G.InterFrame(rng, W, H, bd, ss_h, ss_v)
    assert 1 <= fr.nrefs <= 3
    for ref in fr.refs:
        assert [r.shape for r in ref] == [(fr.rh[p], fr.rw[p]) for p in range(3)]
    assert [pl.shape for pl in fr.planes] == [(fr.dh[p], fr.dw[p]) for p in range(3)]
    for p in range(3):
        Cw, Ch = 64 >> fr.hs[p], 64 >> fr.vs[p]
        cover = np.zeros((fr.sb_h * Ch, fr.sb_w * Cw), np.int64)
        for rec in fr.preds:
            if (rec["flags"] >> 1) & 1 != int(p > 0):
                continue
            x, y, w, h = rec["x"], rec["y"], rec["w"], rec["h"]
            sy, sx = divmod(rec["sb"], fr.sb_w)
            assert w in (4, 8, 16, 32, 64) and h in (4, 8, 16, 32, 64) and 0 <= rec["filter"] <= 3 and rec["flags"] in (0, 1, 2, 3)
            assert sx * Cw <= x and x + w <= (sx + 1) * Cw and sy * Ch <= y and y + h <= (sy + 1) * Ch
            assert x < fr.dw[p] and y < fr.dh[p]                       # blocks start inside the decoded area
            assert rec["ref"][0] < fr.nrefs and (not rec["flags"] & 1 or rec["ref"][1] < fr.nrefs)
            cover[y:y + h, x:x + w] += 1
        assert (cover <= 1).all()                                      # disjoint
        for t in fr.tus[p]:
            N = 4 if t["tx"] == 4 else 4 << t["tx"]
            sy, sx = divmod(t["sb"], fr.sb_w)
            assert t["x"] % N == 0 and t["y"] % N == 0
            assert sx * Cw <= t["x"] and t["x"] + N <= (sx + 1) * Cw and sy * Ch <= t["y"] and t["y"] + N <= (sy + 1) * Ch
            assert t["x"] < fr.dw[p] and t["y"] < fr.dh[p]
            assert (cover[t["y"]:t["y"] + N, t["x"]:t["x"] + N] == 1).all()   # inside a predicted block
            assert t["coeff_offset"] + N * N <= len(fr.coeffs[p])
        arr, starts = fr.pack(fr.tus[p], vp9.INTER_TU_DTYPE, G.TU_FIELDS)
        assert starts[0] == 0 and starts[-1] == len(arr) and (np.diff(starts) >= 0).all()
    arr, starts = fr.pack(fr.preds, vp9.INTER_PRED_DTYPE, G.PRED_FIELDS)
    assert starts[-1] == len(fr.preds) == len(arr)


def test_generator_covers_what_it_promises():
    seen_bs, filters, edges, txs, comp, intra, overhang = set(), set(), set(), set(), 0, 0, 0
    for i, (bd, ss_h, ss_v, W, H) in enumerate(GEN_CASES):
        fr = G.InterFrame(np.random.default_rng(100 + i), W, H, bd, ss_h, ss_v, p_far=0.1)
        lo = G.InterFrame(np.random.default_rng(200 + i), W, H, bd, ss_h, ss_v, lossless=True)
        seen_bs |= {b[0] for b in fr.blocks}
        intra += sum(b[3] == "intra" for b in fr.blocks)
        for rec in fr.preds:
            filters.add(rec["filter"])
            comp += rec["flags"] & 1
            if not rec["flags"] & 2:
                overhang += rec["x"] + rec["w"] > fr.dw[0] or rec["y"] + rec["h"] > fr.dh[0]
                for r in range(1 + (rec["flags"] & 1)):
                    xi, yi, mx, my = G.rec_geometry(fr, rec, 0, r)
                    edges |= {d for d, c in (("left", xi - 3 < 0), ("right", xi + rec["w"] + 4 > fr.W), ("top", yi - 3 < 0),
                                             ("bottom", yi + rec["h"] + 4 > fr.H), ("far", abs(xi) > 4 * fr.W or abs(yi) > 4 * fr.H)) if c}
        for p in range(3):
            txs |= {t["tx"] for t in fr.tus[p] + lo.tus[p]}
    assert seen_bs == set(range(13))
    assert filters == {0, 1, 2, 3} and comp > 0 and intra > 0 and overhang > 0
    assert edges == {"left", "right", "top", "bottom", "far"}
    assert txs == {0, 1, 2, 3, 4}


# ---- ffhip_vp9_inter_block_preds against the restatement of vp9_mc_template.h ----
@pytest.mark.parametrize("ss_h,ss_v", [(1, 1), (1, 0), (0, 1), (0, 0)])
def test_block_preds_match_the_template(ss_h, ss_v):
    rng = np.random.default_rng(50 + 2 * ss_h + ss_v)
    n = 0
    for bs in range(13):
        for comp in (0, 1):
            for _ in range(12):
                mv = rng.integers(-600, 601, (4, 2, 2))
                mv[rng.random((4, 2, 2)) < 0.3] |= 1                   # odd
                mv[0, 0] = rng.choice([-32768, 32767, -1, 1, -7, 7]), rng.integers(-9, 10)
                ref = [int(rng.integers(0, 3)), int(rng.integers(0, 3))]
                row, col, filt = int(rng.integers(0, 200)), int(rng.integers(0, 300)), int(rng.integers(0, 4))
                got = vp9.inter_block_preds(bs, row, col, mv, comp, ref, filt, ss=(ss_h, ss_v))
                want = G.block_preds(bs, row, col, mv.tolist(), comp, ref, filt, ss_h, ss_v)
                assert len(got) == len(want), (bs, comp)
                for g, w in zip(got, want):
                    for f in G.PRED_FIELDS:
                        assert np.array_equal(np.asarray(g[f]), np.asarray(w[f])), (bs, comp, f, g[f], w[f])
                n += 1
    assert n == 13 * 2 * 12


def test_block_preds_refusals_and_rounding():
    L = _lib.lib()
    out = np.zeros(8, vp9.INTER_PRED_DTYPE)
    mv = np.zeros((4, 2, 2), np.int16)
    ref = np.zeros(2, np.uint8)
    f = lambda bs, row, col, filt, sh, sv: L.ffhip_vp9_inter_block_preds(out.ctypes.data, bs, row, col, mv.ctypes.data, 0, ref.ctypes.data,
                                                                         filt, sh, sv)
    for args in ((13, 0, 0, 0, 1, 1), (-1, 0, 0, 0, 1, 1), (0, -1, 0, 0, 1, 1), (0, 0, 8192, 0, 1, 1), (0, 0, 0, 4, 1, 1), (0, 0, 0, 0, 2, 1)):
        assert f(*args) == _lib.EINVAL, args
    assert L.ffhip_vp9_inter_block_preds(None, 0, 0, 0, mv.ctypes.data, 0, ref.ctypes.data, 0, 1, 1) == _lib.EINVAL
    assert [f(bs, 0, 0, 0, 1, 1) for bs in (0, 9, 10, 11, 12)] == [2, 2, 3, 3, 5]
    assert [f(bs, 0, 0, 0, 0, 0) for bs in (0, 9, 10, 11, 12)] == [2, 2, 4, 4, 8]
    # ROUNDED_DIV: half away from zero
    assert [G.rounded_div(a, 2) for a in (3, -3, 1, -1, 4, -4)] == [2, -2, 1, -1, 2, -2]
    assert [G.rounded_div(a, 4) for a in (6, -6, 5, -5, 2, -2, 1, -1)] == [2, -2, 1, -1, 1, -1, 0, 0]
    mv[:, 0] = [[-1, 3], [-2, 0], [0, 0], [0, 0]]
    rec = vp9.inter_block_preds(12, 1, 1, mv, 0, [0, 0], 0, ss=(1, 1))[-1]
    assert rec["flags"] == 2 and (rec["x"], rec["y"], rec["w"], rec["h"]) == (4, 4, 4, 4)
    assert rec["mv"][0].tolist() == [G.rounded_div(-3, 4), G.rounded_div(3, 4)] == [-1, 1]


# ---- the model: clamped windows against the batch faces' route ----
@pytest.mark.parametrize("bd", (8, 10, 12))
@pytest.mark.parametrize("ss_h,ss_v", [(1, 1), (1, 0), (0, 1), (0, 0)])
def test_model_matches_the_padded_route(bd, ss_h, ss_v):
    rng = np.random.default_rng(2000 + bd * 10 + 2 * ss_h + ss_v)
    for W, H, lossless in ((203, 141, False), (64, 72, True)):
        fr = G.InterFrame(rng, W, H, bd, ss_h, ss_v, p_far=0.0, p_edge=0.3, p_intra=0.05, lossless=lossless)
        a, b = G.model(fr), G.model(fr, route="pad")
        for p in range(3):
            assert np.array_equal(a[p], b[p]), p
        changed = sum(int((x != y).sum()) for x, y in zip(a, fr.planes))
        assert changed > 500


def test_model_leaves_uncovered_samples():
    rng = np.random.default_rng(77)
    fr = G.InterFrame(rng, 150, 100, 8, 1, 1, p_intra=0.5)
    out = G.model(fr)
    for p in range(3):
        cov = np.zeros(out[p].shape, bool)
        for rec in fr.preds:
            if (rec["flags"] >> 1) & 1 == int(p > 0):
                cov[rec["y"]:rec["y"] + rec["h"], rec["x"]:rec["x"] + rec["w"]] = True
        assert (~cov).any()
        assert np.array_equal(out[p][~cov], fr.planes[p][~cov])
