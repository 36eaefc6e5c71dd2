"""CPU tier of the HEVC inter picture face (ffhip_hevc_inter_pictures_dev): the record ABI, the argument refusals, the refusal of a box
without a device, the invariants of the synthetic picture generator, and the sequential model (the oracle's put_hevc_* in hevcdec.c's
order) against an independent numpy restatement of H.265 8.5.3.3.3 / 8.5.3.3.4.2 / 8.5.3.3.4.3."""
import ctypes as C

import numpy as np
import pytest

import hevc_inter_picture_gen as G
from ffmpeg_amd import _lib, hevc


def test_record_sizes_match_the_c_structs():
    L = _lib.lib()
    assert L.ffhip_hevc_inter_pu_record_size() == hevc.INTER_PU_DTYPE.itemsize == 20
    assert L.ffhip_hevc_inter_tu_record_size() == hevc.INTER_TU_DTYPE.itemsize == 12
    assert L.ffhip_hevc_inter_slice_record_size() == hevc.INTER_SLICE_DTYPE.itemsize == 424
    assert C.sizeof(hevc.InterPlane) == 40 and C.sizeof(hevc.InterRef) == 48 and C.sizeof(hevc.InterPic) == 3 * 40 + 32 + 16 * 48


_BUFS = []


def _buf(n=1 << 16):
    b = (C.c_uint64 * n)()
    _BUFS.append(b)
    return C.addressof(b)


def _pics(n=1, nrefs=2, stride=256, bd=8):
    """n pictures of 64 x 64 whose planes and references are distinct host buffers (only the face's host checks look at them)"""
    pics = (hevc.InterPic * n)()
    for i in range(n):
        for p in range(3):
            pics[i].plane[p] = hevc.InterPlane(_buf(), stride, _buf(16), _buf(16), _buf(16))
        pics[i].pus, pics[i].pu_ctb_start, pics[i].slices = _buf(16), _buf(16), _buf(128)
        pics[i].nslices, pics[i].nrefs = 1, nrefs
        for r in range(nrefs):
            for p in range(3):
                pics[i].ref[r].base[p] = _buf()
                pics[i].ref[r].stride[p] = stride
    return pics


def test_invalid_arguments():
    """FFHIP_EINVAL comes before the device check: these hold on any machine"""
    f = _lib.lib().ffhip_hevc_inter_pictures_dev
    E = _lib.EINVAL
    v = lambda pics: C.cast(pics, C.c_void_p)
    ok = v(_pics())
    assert f(9, 1, 64, 64, 5, 1, ok, None) == E               # depth
    assert f(8, 4, 64, 64, 5, 1, ok, None) == E               # chroma format
    assert f(8, -1, 64, 64, 5, 1, ok, None) == E
    assert f(8, 1, 64, 64, 3, 1, ok, None) == E               # CTB size
    assert f(8, 1, 64, 64, 7, 1, ok, None) == E
    assert f(8, 1, 60, 64, 5, 1, ok, None) == E               # picture size
    assert f(8, 1, 64, 0, 5, 1, ok, None) == E
    assert f(8, 1, 65536, 64, 5, 1, ok, None) == E
    assert f(8, 1, 64, 64, 5, 0, ok, None) == E               # npics
    assert f(8, 1, 64, 64, 5, -1, ok, None) == E
    assert f(8, 1, 64, 64, 5, 1, None, None) == E
    assert f(8, 1, 64, 64, 5, 1, v(_pics(stride=258)), None) == E   # stride not 4-byte aligned
    assert f(10, 1, 64, 64, 5, 1, v(_pics(stride=260)), None) == E  # nor 8-byte above 8 bits
    assert f(8, 1, 512, 64, 5, 1, v(_pics(stride=256)), None) == E  # stride below the width
    for field in ("base", "tus", "tu_ctb_start", "res"):            # NULL plane pointers
        pics = _pics()
        setattr(pics[0].plane[2], field, None)
        assert f(8, 1, 64, 64, 5, 1, v(pics), None) == E, field
    pics = _pics()
    pics[0].plane[1].base += 2                                      # misaligned plane
    assert f(8, 1, 64, 64, 5, 1, v(pics), None) == E
    for field in ("pus", "pu_ctb_start", "slices"):
        pics = _pics()
        setattr(pics[0], field, None)
        assert f(8, 1, 64, 64, 5, 1, v(pics), None) == E, field
    for nrefs in (-1, 17):
        pics = _pics()
        pics[0].nrefs = nrefs
        assert f(8, 1, 64, 64, 5, 1, v(pics), None) == E, nrefs
    pics = _pics()
    pics[0].nslices = -1
    assert f(8, 1, 64, 64, 5, 1, v(pics), None) == E
    pics = _pics(nrefs=3)
    pics[0].ref[2].base[1] = None                                   # a NULL base among the first nrefs
    assert f(8, 1, 64, 64, 5, 1, v(pics), None) == E
    pics = _pics(nrefs=3, bd=10)
    pics[0].ref[1].base[0] += 1                                     # an odd 16-bit reference
    assert f(10, 1, 64, 64, 5, 1, v(pics), None) == E
    pics = _pics(nrefs=3)
    pics[0].ref[1].stride[2] = 16                                   # a reference stride below the width
    assert f(8, 1, 64, 64, 5, 1, v(pics), None) == E
    # a reference plane that is a destination plane of the call: of the same picture, of another one, or overlapping one
    pics = _pics(n=3)
    pics[2].ref[1].base[0] = pics[2].plane[0].base
    assert f(8, 1, 64, 64, 5, 3, v(pics), None) == E
    pics = _pics(n=3)
    pics[0].ref[0].base[2] = pics[1].plane[1].base
    assert f(8, 1, 64, 64, 5, 3, v(pics), None) == E
    pics = _pics(n=2)
    pics[1].ref[1].base[1] = pics[0].plane[0].base + 256 * 40
    assert f(8, 1, 64, 64, 5, 2, v(pics), None) == E
    # a slot past nrefs is not looked at, nor is a chroma plane of a monochrome call: NULL pointers there do not stop the checks,
    # which go on to refuse the call for the overlap planted after them (never reaching the device)
    pics = _pics(nrefs=1)
    pics[0].ref[1].base[0] = None
    pics[0].plane[1].base = None
    pics[0].plane[2].res = None
    pics[0].ref[0].base[1] = None
    pics[0].ref[0].base[0] = pics[0].plane[0].base + 256 * 63
    assert f(8, 0, 64, 64, 5, 1, v(pics), None) == E
    assert b"overlaps" in _lib.lib().ffhip_last_error()


@pytest.mark.skipif(_lib.lib().ffhip_device_count() > 0, reason="a HIP device is present: the refusal path is not reachable")
def test_no_device_refusals():
    L = _lib.lib()
    ok = C.cast(_pics(), C.c_void_p)
    assert L.ffhip_hevc_inter_pictures_dev(8, 1, 64, 64, 5, 1, ok, None) == _lib.ENOSYS
    assert L.ffhip_hevc_inter_pictures_dev(12, 3, 64, 64, 6, 1, ok, None) == _lib.ENOSYS
    assert L.ffhip_hevc_inter_pictures_dev(10, 0, 64, 64, 4, 1, ok, None) == _lib.ENOSYS
    # a monochrome call with NULLs in the chroma planes and past nrefs passes the checks
    pics = _pics(nrefs=1)
    pics[0].ref[1].base[0] = None
    pics[0].plane[1].base = None
    pics[0].ref[0].base[1] = None
    assert L.ffhip_hevc_inter_pictures_dev(8, 0, 64, 64, 5, 1, C.cast(pics, C.c_void_p), None) == _lib.ENOSYS


GEN_CASES = [(8, 1, 4, 3), (10, 2, 5, 3), (12, 3, 6, 4), (8, 0, 5, 4), (8, 1, 6, 3), (10, 1, 6, 5)]


@pytest.mark.parametrize("bd,cfi,log2_ctb,min_cb", GEN_CASES)
def test_generator_invariants(bd, cfi, log2_ctb, min_cb):
    rng = np.random.default_rng(bd * 7 + cfi * 3 + log2_ctb)
    pic = G.InterPicture(rng, 264, 200, log2_ctb, bd, cfi, nrefs=5, nslices=3, min_cb=min_cb)
    C_ = pic.C
    cover = np.zeros((pic.H, pic.W), np.int64)
    for pu in pic.pus:
        x, y, w, h = pu["x"], pu["y"], pu["w"], pu["h"]
        cy, cx = divmod(pu["ctb"], pic.ctb_w)
        assert 4 <= w <= 64 and 4 <= h <= 64 and w % 4 == 0 and h % 4 == 0
        assert cx * C_ <= x and x + w <= min((cx + 1) * C_, pic.W) and cy * C_ <= y and y + h <= min((cy + 1) * C_, pic.H)
        assert pu["slice"] == pic.ctb_slice[pu["ctb"]]
        S = pic.slices[pu["slice"]]
        assert pu["flags"] in ((1,) if S["type"] == "P" else (1, 2, 3))
        assert not (pu["flags"] == 3 and w + h == 12)                          # no bi-prediction for 8x4 / 4x8
        for l in range(2):
            if pu["flags"] >> l & 1:
                assert pu["ref_idx"][l] < S["num_ref"][l] and S["ref"][l][pu["ref_idx"][l]] < pic.nrefs
        cover[y:y + h, x:x + w] += 1
    inter = np.repeat(np.repeat(pic.kind == 1, 4, 0), 4, 1)[:pic.H, :pic.W]
    assert (cover <= 1).all()                                                  # PUs are disjoint
    assert ((cover == 1) == inter).all()                                       # and tile the inter CUs exactly
    assert (pic.kind[:pic.H // 4, :pic.W // 4] == 2).any() and (pic.kind[:pic.H // 4, :pic.W // 4] == 3).any()
    for p in range(pic.nplanes):
        hs, vs = pic.hs[p], pic.vs[p]
        Cw, Ch = C_ >> hs, C_ >> vs
        for t in pic.tus[p]:
            N = 1 << t["log2_size"]
            cy, cx = divmod(t["ctb"], pic.ctb_w)
            assert 2 <= t["log2_size"] <= 5
            assert cx * Cw <= t["x"] and t["x"] + N <= min((cx + 1) * Cw, pic.W >> hs)
            assert cy * Ch <= t["y"] and t["y"] + N <= min((cy + 1) * Ch, pic.H >> vs)
            assert inter[t["y"] << vs, t["x"] << hs]                          # inside an inter CU
        arr, starts = pic.pack(pic.tus[p], hevc.INTER_TU_DTYPE, ("x", "y", "res_offset", "log2_size"))
        assert starts[0] == 0 and starts[-1] == len(arr) and (np.diff(starts) >= 0).all()
    arr, starts = pic.pack(pic.pus, hevc.INTER_PU_DTYPE, G.PU_FIELDS)
    assert starts[-1] == len(pic.pus)


def test_generator_covers_every_partition_mode_and_edge():
    seen, edges = set(), set()
    for i, (bd, cfi, log2_ctb, min_cb) in enumerate(GEN_CASES):
        pic = G.InterPicture(np.random.default_rng(100 + i), 264, 200, log2_ctb, bd, cfi, nrefs=3, min_cb=min_cb)
        seen |= {pu["part"] for pu in pic.pus}
        for pu in pic.pus:
            for l in range(2):
                if pu["flags"] >> l & 1:
                    bx, by, bw, bh, xi, yi, mx, my = G.pu_geometry(pic, pu, 0, l)
                    edges |= {d for d, c in (("left", xi - 3 < 0), ("right", xi + bw + 4 > pic.W), ("top", yi - 3 < 0),
                                             ("bottom", yi + bh + 4 > pic.H), ("far", abs(xi) > 4 * pic.W or abs(yi) > 4 * pic.H)) if c}
    assert seen == set(G.PART_MODES)
    assert edges == {"left", "right", "top", "bottom", "far"}


# ---- an independent restatement of the standard ----
LUMA_F = np.array([[0, 0, 0, 64, 0, 0, 0, 0], [-1, 4, -10, 58, 17, -5, 1, 0], [-1, 4, -11, 40, 40, -11, 4, -1], [0, 1, -5, 17, 58, -10, 4, -1]])
CHROMA_F = np.array([[0, 64, 0, 0], [-2, 58, 10, -2], [-4, 54, 16, -2], [-6, 46, 28, -4], [-4, 36, 36, -4], [-4, 28, 46, -6],
                     [-2, 16, 54, -4], [-2, 10, 58, -2]])


def spec_interp(ref, xint, yint, xfrac, yfrac, w, h, bd, chroma):
    """8.5.3.3.3.1 (luma) / 8.5.3.3.3.2 (chroma): the w x h array predSamplesLX at integer position (xint, yint) and phase
    (xfrac, yfrac), every reference coordinate Clip3(0, pic_size - 1, .)"""
    F, n, off = (CHROMA_F, 4, 1) if chroma else (LUMA_F, 8, 3)
    shift1, shift2, shift3 = min(4, bd - 8), 6, max(2, 14 - bd)
    H, W = ref.shape
    ys = np.arange(h)[:, None] + yint
    xs = np.arange(w)[None, :] + xint

    def at(yy, xx):
        return ref[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)].astype(np.int64)

    if xfrac == 0 and yfrac == 0:
        return at(ys, xs) << shift3
    if yfrac == 0:
        return sum(F[xfrac][i] * at(ys, xs + i - off) for i in range(n)) >> shift1
    if xfrac == 0:
        return sum(F[yfrac][i] * at(ys + i - off, xs) for i in range(n)) >> shift1
    # the horizontal samples of rows -off .. h + n - 1 - off, then the vertical filter over them
    hrow = lambda k: sum(F[xfrac][i] * at(ys + k - off, xs + i - off) for i in range(n)) >> shift1
    return sum(F[yfrac][k] * hrow(k) for k in range(n)) >> shift2


def spec_weighted(pred, bd, explicit=None):
    """8.5.3.3.4.2 default / 8.5.3.3.4.3 explicit weighted sample prediction.  pred: [L0] or [L0, L1] (predSamples); explicit:
    (log2_denom, [w0, w1], [o0, o1]) with the offsets as coded (scaled here by << (bd - 8))"""
    mx = (1 << bd) - 1
    shift1 = 14 - bd
    if explicit is None:
        if len(pred) == 1:
            return np.clip((pred[0] + (1 << (shift1 - 1))) >> shift1, 0, mx)
        shift2 = 15 - bd
        return np.clip((pred[0] + pred[1] + (1 << (shift2 - 1))) >> shift2, 0, mx)
    denom, w, o = explicit
    log2wd = denom + shift1
    o = [v << (bd - 8) for v in o]
    if len(pred) == 1:
        return np.clip(((pred[0] * w[0] + (1 << (log2wd - 1))) >> log2wd) + o[0], 0, mx)
    return np.clip((pred[0] * w[0] + pred[1] * w[1] + ((o[0] + o[1] + 1) << log2wd)) >> (log2wd + 1), 0, mx)


def spec_pu(pic, pu, p):
    S = pic.slices[pu["slice"]]
    preds, ws, os_ = [], [], []
    for l in range(2):
        if not pu["flags"] >> l & 1:
            continue
        ri = pu["ref_idx"][l]
        ref = pic.refs[S["ref"][l][ri]][p]
        mv = pu["mv"][l]
        hs, vs = pic.hs[p], pic.vs[p]
        x, y, w, h = pu["x"] >> hs, pu["y"] >> vs, pu["w"] >> hs, pu["h"] >> vs
        if p == 0:
            preds.append(spec_interp(ref, x + (mv[0] >> 2), y + (mv[1] >> 2), mv[0] & 3, mv[1] & 3, w, h, pic.bd, False))
            ws.append(S["luma_weight"][l][ri])
            os_.append(S["luma_offset"][l][ri])
        else:
            # 8.5.3.2.10 / 8.5.3.3.3.2: mvC in units of 1 / (4 << SubWidthC) ... expressed as eighths of a chroma sample
            sw, sh = 1 << hs, 1 << vs
            mvcx, mvcy = mv[0] * 2 // sw, mv[1] * 2 // sh
            preds.append(spec_interp(ref, x + (mvcx >> 3), y + (mvcy >> 3), mvcx & 7, mvcy & 7, w, h, pic.bd, True))
            ws.append(S["chroma_weight"][l][ri][p - 1])
            os_.append(S["chroma_offset"][l][ri][p - 1])
    explicit = (S["chroma_log2_denom"] if p else S["luma_log2_denom"], ws, os_) if S["weighted"] else None
    return spec_weighted(preds, pic.bd, explicit)


@pytest.mark.parametrize("bd", (8, 10, 12))
@pytest.mark.parametrize("cfi", (0, 1, 2, 3))
def test_model_matches_the_spec_restatement(bd, cfi):
    rng = np.random.default_rng(2000 + bd * 10 + cfi)
    n = 0
    for k in range(3):
        pic = G.InterPicture(rng, 136, 104, 5 + k % 2, bd, cfi, nrefs=int(rng.integers(1, 17)), nslices=3, p_inter=0.95, p_pcm=0.0,
                             p_far=0.1, min_cb=3 + k % 2)
        for pu in pic.pus:
            for p in range(pic.nplanes):
                got, want = G.predict_pu(pic, pu, p), spec_pu(pic, pu, p)
                assert np.array_equal(got, want), (bd, cfi, p, pu)
            n += 1
    assert n >= 100
