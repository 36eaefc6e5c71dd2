"""CPU tier of the HEVC in-loop filter picture face (ffhip_hevc_loop_filter_pictures_dev): the record ABI, the argument refusals, the
refusal of a box without a device, the invariants of the synthetic picture generator, and the sequential model (the oracle's
per-call deblocking and SAO functions in the reference's order) against an independent restatement of H.265 8.7.2.5 / 8.7.3."""
import ctypes as C

import numpy as np
import pytest

import hevc_lf_picture_gen as G
from ffmpeg_amd import _lib, hevc


def test_record_sizes_match_the_c_structs():
    assert _lib.lib().ffhip_hevc_lf_ctb_record_size() == hevc.LF_CTB_DTYPE.itemsize == 44
    assert C.sizeof(hevc.LfPlane) == 32 and C.sizeof(hevc.LfPic) == 3 * 32 + 5 * 8 + 8 + 8


_BUFS = []


def _buf(n=1 << 15):
    b = (C.c_uint64 * n)()
    _BUFS.append(b)
    return C.addressof(b)


def _pics(n=1, stride=256):
    """n pictures of 64 x 64 whose planes are distinct host buffers (only the face's host checks look at them)"""
    pics = (hevc.LfPic * n)()
    for i in range(n):
        for p in range(3):
            pics[i].plane[p] = hevc.LfPlane(_buf(), stride, _buf(), stride)
        pics[i].bs_ver, pics[i].bs_hor, pics[i].qp_y, pics[i].ctbs = _buf(64), _buf(64), _buf(64), _buf(64)
        pics[i].bs_stride, pics[i].cb_stride = 16, 8
    return pics


def test_invalid_arguments():
    """FFHIP_EINVAL comes before the device check: these hold on any machine"""
    f = _lib.lib().ffhip_hevc_loop_filter_pictures_dev
    E = _lib.EINVAL
    v = lambda pics: C.cast(pics, C.c_void_p)
    ok = v(_pics())
    assert f(9, 1, 64, 64, 5, 3, 1, ok, None) == E            # depth
    assert f(8, 4, 64, 64, 5, 3, 1, ok, None) == E            # chroma format
    assert f(8, -1, 64, 64, 5, 3, 1, ok, None) == E
    assert f(8, 1, 64, 64, 3, 3, 1, ok, None) == E            # CTB size
    assert f(8, 1, 64, 64, 7, 3, 1, ok, None) == E
    assert f(8, 1, 64, 64, 5, 2, 1, ok, None) == E            # min CB size
    assert f(8, 1, 64, 64, 5, 6, 1, ok, None) == E
    assert f(8, 1, 60, 64, 5, 3, 1, ok, None) == E            # picture size
    assert f(8, 1, 64, 0, 5, 3, 1, ok, None) == E
    assert f(8, 1, 65536, 64, 5, 3, 1, ok, None) == E
    assert f(8, 1, 64, 64, 5, 3, 0, ok, None) == E            # npics
    assert f(8, 1, 64, 64, 5, 3, -1, ok, None) == E
    assert f(8, 1, 64, 64, 5, 3, 1, None, None) == E
    for field in ("bs_ver", "bs_hor", "qp_y", "ctbs"):         # NULL maps
        pics = _pics()
        setattr(pics[0], field, None)
        assert f(8, 1, 64, 64, 5, 3, 1, v(pics), None) == E, field
    pics = _pics()
    pics[0].bs_stride = 15                                      # below width / 4
    assert f(8, 1, 64, 64, 5, 3, 1, v(pics), None) == E
    pics = _pics()
    pics[0].cb_stride = 7                                       # below the min-CB columns
    assert f(8, 1, 64, 64, 5, 3, 1, v(pics), None) == E
    for p, field, val in ((0, "src", None), (2, "dst", None), (1, "src_stride", 31), (0, "dst_stride", 63), (1, "dst_stride", 258)):
        pics = _pics()
        setattr(pics[0].plane[p], field, val)
        assert f(8, 1, 64, 64, 5, 3, 1, v(pics), None) == E, (p, field)
    pics = _pics()
    pics[0].plane[1].src += 2                                   # misaligned: four samples per access
    assert f(8, 1, 64, 64, 5, 3, 1, v(pics), None) == E
    pics = _pics()
    pics[0].plane[0].dst_stride = 130                           # 16-bit: a stride of 65 samples
    assert f(10, 1, 64, 64, 5, 3, 1, v(pics), None) == E
    # src and dst overlap: the same picture, and across pictures of one call
    pics = _pics()
    pics[0].plane[0].dst = pics[0].plane[0].src + 256 * 63
    assert f(8, 1, 64, 64, 5, 3, 1, v(pics), None) == E
    assert b"overlaps" in _lib.lib().ffhip_last_error()
    pics = _pics(2)
    pics[1].plane[2].src = pics[0].plane[1].dst + 16
    assert f(8, 1, 64, 64, 5, 3, 2, v(pics), None) == E
    # a monochrome call does not look at the chroma planes, so it goes on to refuse the overlap planted after them
    pics = _pics()
    pics[0].plane[1].src = None
    pics[0].plane[2].dst = None
    pics[0].plane[0].src = pics[0].plane[0].dst + 256 * 10
    assert f(8, 0, 64, 64, 5, 3, 1, v(pics), None) == E
    assert b"overlaps" in _lib.lib().ffhip_last_error()


@pytest.mark.skipif(_lib.lib().ffhip_device_count() > 0, reason="a HIP device is present: the refusal path is not reachable")
def test_no_device_refusals():
    L = _lib.lib()
    ok = C.cast(_pics(), C.c_void_p)
    assert L.ffhip_hevc_loop_filter_pictures_dev(8, 1, 64, 64, 5, 3, 1, ok, None) == _lib.ENOSYS
    assert L.ffhip_hevc_loop_filter_pictures_dev(12, 3, 64, 64, 6, 4, 1, ok, None) == _lib.ENOSYS
    assert L.ffhip_hevc_loop_filter_pictures_dev(10, 0, 64, 64, 4, 3, 1, ok, None) == _lib.ENOSYS
    pics = _pics()
    pics[0].bypass = None                                       # bypass is optional
    pics[0].plane[1].src = None                                 # monochrome: chroma planes unused
    assert L.ffhip_hevc_loop_filter_pictures_dev(8, 0, 64, 64, 5, 3, 1, C.cast(pics, C.c_void_p), None) == _lib.ENOSYS


@pytest.mark.parametrize("bd,cfi,log2_ctb", [(8, 1, 4), (10, 2, 5), (12, 3, 6), (8, 0, 5)])
def test_generator_invariants(bd, cfi, log2_ctb):
    """every edge kind, every SAO class, bypass CUs, partial CTBs and restore flags occur; the maps are in range"""
    rng = np.random.default_rng(100 + bd + cfi + log2_ctb)
    W, H = {4: (136, 88), 5: (200, 136), 6: (264, 200)}[log2_ctb]
    pics = [G.LfPicture(rng, W, H, log2_ctb, bd, cfi, tiles=(2, 2), nslices=4) for _ in range(6)]
    P = pics[0]
    assert W % P.C and H % P.C                                   # partial CTBs at the right and bottom
    bsv = np.concatenate([p.bs_ver.ravel() for p in pics])
    bsh = np.concatenate([p.bs_hor.ravel() for p in pics])
    assert {0, 1, 2} <= set(bsv.tolist()) and {0, 1, 2} <= set(bsh.tolist()) and bsv.max() <= 2 and bsh.max() <= 2
    assert all((p.bs_ver[:, 0] == 0).all() and (p.bs_hor[0, :] == 0).all() for p in pics)    # nothing on the picture border
    assert any(p.bypass.any() for p in pics)
    qp = np.concatenate([p.qp.ravel() for p in pics])
    assert qp.min() >= -6 * (bd - 8) and qp.max() <= 51
    kinds = {(c, r["sao_type"][c], r["sao_class"][c] if r["sao_type"][c] == 2 else 0) for p in pics for r in p.ctbs
             for c in range(p.nplanes)}
    for c in range(P.nplanes):
        assert (c, 0, 0) in kinds and (c, 1, 0) in kinds
        assert all((c, 2, k) in kinds for k in range(4)), c
    assert any(r["restore"] and (r["vert_edge"] or r["horiz_edge"] or r["diag_edge"]) for p in pics for r in p.ctbs)
    assert any(s["deblock_off"] for p in pics for s in p.slices) and any(not s["across"] for p in pics for s in p.slices)
    # a slice with deblocking disabled has bS 0 on every edge whose q0 lies in it
    for p in pics:
        for y in range(0, p.H, 4):
            for x in range(8, p.W, 8):
                if p.slices[p.slice_of[p.ctb_at(x, y)]]["deblock_off"]:
                    assert p.bs_ver[y >> 2, x >> 2] == 0


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("cfi", [0, 1, 2, 3])
def test_model_matches_the_spec_restatement(bd, cfi):
    """the model (the oracle's per-call filters in the reference's order, with the generator's restore flags) equals a per-sample
    restatement of the standard that takes neighbour availability from the slice and tile maps"""
    rng = np.random.default_rng(200 + bd * 10 + cfi)
    for log2_ctb, (W, H), tiles in ((4, (72, 56), (2, 2)), (5, (104, 72), (2, 1))):
        pic = G.LfPicture(rng, W, H, log2_ctb, bd, cfi, tiles=tiles, nslices=3, lf_across_tiles=bool(rng.integers(0, 2)))
        want = G.restate(pic)
        got = G.model(pic)
        for p in range(pic.nplanes):
            assert np.array_equal(got[p], want[p]), (log2_ctb, p, np.argwhere(got[p] != want[p])[:4].tolist())
        assert any((got[p] != pic.src[p]).any() for p in range(pic.nplanes))


def test_model_deblocking_only_and_sao_only():
    """the two stages alone also equal the restatement, and each changes the picture"""
    rng = np.random.default_rng(300)
    for kw in (dict(sao=False), dict(deblock=False)):
        pic = G.LfPicture(rng, 96, 64, 5, 10, 1, tiles=(2, 2), nslices=2, **kw)
        got, want = G.model(pic), G.restate(pic)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), kw
        assert any((a != s).any() for a, s in zip(got, pic.src)), kw
