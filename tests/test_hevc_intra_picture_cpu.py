"""CPU tier of the HEVC intra picture wavefront (ffhip_hevc_intra_pictures_dev): the record ABI, the refusals of a box without a
device, the invariants of the synthetic picture generator, and properties of the sequential model that do not share its path."""
import ctypes as C

import numpy as np
import pytest

import hevc_intra_picture_gen as G
import hevc_pred_ref as R
from ffmpeg_amd import _lib, hevc


def test_tu_record_matches_the_c_struct():
    assert _lib.lib().ffhip_hevc_intra_tu_record_size() == hevc.INTRA_TU_DTYPE.itemsize == 16
    assert C.sizeof(hevc.IntraPlane) == 5 * 8 and C.sizeof(hevc.IntraPic) == 3 * 5 * 8


def _pics(n=1, **kw):
    buf = (C.c_uint64 * 64)()
    pics = (hevc.IntraPic * n)()
    for i in range(n):
        for p in range(3):
            pics[i].plane[p] = hevc.IntraPlane(C.addressof(buf), kw.get("stride", 256), C.addressof(buf), C.addressof(buf),
                                               C.addressof(buf))
    return pics


def test_invalid_arguments():
    """FFHIP_EINVAL comes before the device check: these hold on any machine"""
    f = _lib.lib().ffhip_hevc_intra_pictures_dev
    ok = C.cast(_pics(), C.c_void_p)
    assert f(9, 1, 64, 64, 5, 1, ok, None) == _lib.EINVAL               # depth
    assert f(8, 4, 64, 64, 5, 1, ok, None) == _lib.EINVAL               # chroma format
    assert f(8, 1, 64, 64, 3, 1, ok, None) == _lib.EINVAL               # CTB size
    assert f(8, 1, 64, 64, 7, 1, ok, None) == _lib.EINVAL
    assert f(8, 1, 60, 64, 5, 1, ok, None) == _lib.EINVAL               # picture size
    assert f(8, 1, 64, 0, 5, 1, ok, None) == _lib.EINVAL
    assert f(8, 1, 65536, 64, 5, 1, ok, None) == _lib.EINVAL
    assert f(8, 1, 64, 64, 5, 0, ok, None) == _lib.EINVAL               # npics
    assert f(8, 1, 64, 64, 5, 1, None, None) == _lib.EINVAL
    assert f(8, 1, 64, 64, 5, 1, C.cast(_pics(stride=258), C.c_void_p), None) == _lib.EINVAL   # stride not 4-byte aligned
    assert f(10, 1, 64, 64, 5, 1, C.cast(_pics(stride=260), C.c_void_p), None) == _lib.EINVAL  # nor 8-byte above 8 bits
    assert f(8, 1, 512, 64, 5, 1, C.cast(_pics(stride=256), C.c_void_p), None) == _lib.EINVAL  # stride below the width
    nul = _pics()
    nul[0].plane[2].res = None
    assert f(8, 1, 64, 64, 5, 1, C.cast(nul, C.c_void_p), None) == _lib.EINVAL
    assert f(8, 1, 64, 65528, 4, 1, ok, None) == _lib.EINVAL            # 3 x 4096 CTB rows: more than the progress pool holds


@pytest.mark.skipif(_lib.lib().ffhip_device_count() > 0, reason="a HIP device is present: the refusal path is not reachable")
def test_no_device_refusals():
    L = _lib.lib()
    ok = C.cast(_pics(), C.c_void_p)
    assert L.ffhip_hevc_intra_pictures_dev(8, 1, 64, 64, 5, 1, ok, None) == _lib.ENOSYS
    assert L.ffhip_hevc_intra_pictures_dev(12, 3, 64, 64, 6, 1, ok, None) == _lib.ENOSYS
    assert L.ffhip_hevc_intra_pictures_dev(8, 0, 64, 64, 4, 1, ok, None) == _lib.ENOSYS


GEN_CASES = [(8, 1, 4, (1, 1), 1, False, 1.0), (10, 2, 5, (2, 2), 3, True, 0.5), (12, 3, 6, (3, 1), 2, False, 0.6),
             (8, 0, 5, (1, 2), 4, True, 0.5), (8, 1, 5, (2, 1), 2, True, 0.4)]


@pytest.mark.parametrize("bd,cfi,log2_ctb,tiles,slices,cip,p_intra", GEN_CASES)
def test_generator_invariants(bd, cfi, log2_ctb, tiles, slices, cip, p_intra):
    rng = np.random.default_rng(bd * 7 + cfi)
    pic = G.Picture(rng, 200, 136, log2_ctb, bd, cfi, p_intra=p_intra, tiles=tiles, slices=slices, cip=cip)
    C_ = pic.C
    saw_later_inter = False
    for p in range(pic.nplanes):
        hs, vs = pic.hs[p], pic.vs[p]
        arr, starts = pic.pack(p, dtype=hevc.INTRA_TU_DTYPE)
        assert starts[0] == 0 and starts[-1] == len(arr) and (np.diff(starts) >= 0).all()
        recs = sorted(pic.recs[p], key=lambda r: r["ctb"])
        for a in range(pic.ctb_w * pic.ctb_h):
            rs = recs[starts[a]:starts[a + 1]]
            assert all(r["ctb"] == a for r in rs)                                  # contiguous, under its CTB
            assert [r["order"] for r in rs] == sorted(r["order"] for r in rs)       # in decoding order
            cy, cx = divmod(a, pic.ctb_w)
            for r in rs:
                N = 1 << r["log2_size"]
                assert cx * (C_ >> hs) <= r["x"] and r["x"] + N <= min((cx + 1) * (C_ >> hs), pic.W >> hs)
                assert cy * (C_ >> vs) <= r["y"] and r["y"] + N <= min((cy + 1) * (C_ >> vs), pic.H >> vs)
        for r in pic.recs[p]:
            N = 1 << r["log2_size"]
            luh, luv = (r["c_idx_unit"] >> 2) & 3, (r["c_idx_unit"] >> 4) & 3
            assert (2 * N) >> luh <= 16 and (2 * N) >> luv <= 16                     # unit bounds
            assert r["avail_left"] >> ((2 * N) >> luv) == 0 and r["avail_top"] >> ((2 * N) >> luh) == 0
            cur = pic.order[(r["y"] << vs) >> 2, (r["x"] << hs) >> 2]
            av = R.availability(N, r["avail_left"], r["avail_top"], r["flags"] & G.FLAG_CORNER, luh, luv)
            left, corner, top = R.split(av)
            pts = [(r["x"] - 1, r["y"] + i, a_) for i, a_ in enumerate(left)] + [(r["x"] - 1, r["y"] - 1, corner)] + \
                  [(r["x"] + i, r["y"] - 1, a_) for i, a_ in enumerate(top)]
            for x, y, a_ in pts:
                if not a_:
                    if 0 <= x < pic.W >> hs and 0 <= y < pic.H >> vs and pic.order[(y << vs) >> 2, (x << hs) >> 2] > cur and \
                            not pic.intra[(y << vs) >> 2, (x << hs) >> 2]:
                        saw_later_inter = True
                    continue
                assert 0 <= x < pic.W >> hs and 0 <= y < pic.H >> vs
                assert pic.order[(y << vs) >> 2, (x << hs) >> 2] < cur                 # never a sample decoded later
                if cip:
                    assert pic.intra[(y << vs) >> 2, (x << hs) >> 2]
    if p_intra < 1:
        assert saw_later_inter   # inter samples in the plane but later in z-order: the masks must exclude them


def _strip(pic, masks=True, res=True, modes=None):
    recs = []
    for p in range(pic.nplanes):
        rl = []
        for r in pic.recs[p]:
            r = dict(r)
            if masks:
                r["avail_left"] = r["avail_top"] = 0
                r["flags"] &= ~G.FLAG_CORNER
            if res:
                r["res_offset"] = -1
            if modes is not None:
                r["mode"] = modes
            rl.append(r)
        recs.append(rl)
    return recs


def _intra_mask(pic, p):
    m = np.zeros(pic.planes[p].shape, bool)
    for r in pic.recs[p]:
        N = 1 << r["log2_size"]
        m[r["y"]:r["y"] + N, r["x"]:r["x"] + N] = True
    return m


@pytest.mark.parametrize("bd,cfi", [(8, 1), (10, 2), (12, 3), (8, 0)])
def test_model_nothing_available_no_residual_is_mid_grey(bd, cfi):
    pic = G.Picture(np.random.default_rng(11 + cfi), 96, 64, 5, bd, cfi, p_intra=0.7)
    out = G.model(pic, _strip(pic))
    for p in range(pic.nplanes):
        m = _intra_mask(pic, p)
        assert m.any() and (out[p][m] == 1 << (bd - 1)).all()
        assert (out[p][~m] == pic.planes[p][~m]).all()


@pytest.mark.parametrize("bd,cfi", [(8, 1), (10, 3)])
def test_model_with_empty_masks_is_per_block_predict_raw(bd, cfi):
    pic = G.Picture(np.random.default_rng(21 + bd), 64, 48, 4, bd, cfi, strong=True)
    recs = _strip(pic, res=False)
    out = G.model(pic, recs)
    mx = (1 << bd) - 1
    for p in range(pic.nplanes):
        for r in recs[p]:
            N = 1 << r["log2_size"]
            line = np.arange(4 * N + 1) * 3 % (mx + 1)   # any line: nothing of it is available
            want = R.predict_raw(line, N, r["mode"], r["c_idx_unit"] & 3, bd, [False] * (4 * N + 1), strong=True,
                                 chroma444=cfi == 3)
            if r["res_offset"] >= 0:
                want = want + pic.res[p][r["res_offset"]:r["res_offset"] + N * N].reshape(N, N)
            assert (out[p][r["y"]:r["y"] + N, r["x"]:r["x"] + N] == np.clip(want, 0, mx)).all()


@pytest.mark.parametrize("bd,cfi", [(8, 1), (12, 2)])
def test_model_all_dc_on_constant_background_stays_constant(bd, cfi):
    """every intra block DC, no residual, inter CUs flat at mid-grey: whatever is available or substituted is mid-grey, and the
    garbage the intra areas start with is never read"""
    pic = G.Picture(np.random.default_rng(31 + bd), 128, 72, 5, bd, cfi, p_intra=0.6, tiles=(2, 1), slices=2)
    v = 1 << (bd - 1)
    for p in range(pic.nplanes):
        m = _intra_mask(pic, p)
        pic.planes[p][~m] = v
        assert (pic.planes[p][m] != v).any()
    out = G.model(pic, _strip(pic, masks=False, modes=1))
    for p in range(pic.nplanes):
        assert (out[p] == v).all()
