"""CPU tier of VP9 inter frames from references of another size (ffhip_vp9_inter_frames_scaled_dev): the struct and record ABI, the
argument refusals (reference sizes, per-reference strides and overlap), the refusal without a device, ffhip_vp9_inter_block_preds_scaled
against a restatement of vp9_mc_template.h's SCALED instantiation, and the model of vp9_scaled_frame_gen.py (clamped windows, the
oracle's smc) against the route through edge-padded references, and against vp9_inter_frame_gen's model when nothing is scaled."""
import ctypes as C

import numpy as np
import pytest

import vp9_inter_frame_gen as G
import vp9_scaled_frame_gen as S
from ffmpeg_amd import _lib, vp9


def test_struct_sizes_and_record_fields():
    L = _lib.lib()
    assert L.ffhip_vp9_inter_pred_record_size() == vp9.INTER_PRED_DTYPE.itemsize == 20
    assert vp9.INTER_PRED_DTYPE.fields["box"][1] == 10 and vp9.INTER_PRED_DTYPE.fields["mv"][1] == 12
    assert C.sizeof(vp9.InterPicScaled) == C.sizeof(vp9.InterPic) + 24 == 312
    assert vp9.INTER_SCALED == S.SCALED == 4


_BUFS = []


def _buf(n=1 << 16):
    b = (C.c_uint64 * n)()
    _BUFS.append(b)
    return C.addressof(b)


def _pics(n=1, nrefs=2, stride=256, ref_size=(64, 64)):
    """n frames of 64 x 64 whose planes and references are distinct host buffers (only the face's host checks look at them)"""
    pics = (vp9.InterPicScaled * n)()
    for i in range(n):
        P = pics[i].pic
        for p in range(3):
            P.plane[p] = vp9.InterPlane(_buf(), stride, _buf(16), _buf(16), _buf(16))
        P.preds, P.pred_sb_start = _buf(16), _buf(16)
        P.nrefs = nrefs
        for r in range(nrefs):
            for p in range(3):
                P.ref[r].base[p] = _buf()
                P.ref[r].stride[p] = stride
            pics[i].ref_w[r], pics[i].ref_h[r] = ref_size
    return pics


def test_invalid_arguments():
    """FFHIP_EINVAL comes before the device check: these hold on any machine"""
    f = _lib.lib().ffhip_vp9_inter_frames_scaled_dev
    E = _lib.EINVAL
    v = lambda pics: C.cast(pics, C.c_void_p)
    ok = v(_pics())
    assert f(9, 1, 1, 64, 64, 1, ok, None) == E                  # depth, subsampling, size, npics as the unscaled face
    assert f(8, 2, 1, 64, 64, 1, ok, None) == E
    assert f(8, 1, 1, 0, 64, 1, ok, None) == E
    assert f(8, 1, 1, 64, 64, 0, ok, None) == E
    assert f(8, 1, 1, 64, 64, 1, None, None) == E
    for size in ((129, 64), (64, 129), (3, 64), (64, 3), (0, 64), (64, -1), (65536, 64)):   # outside 2x / 16x, or 1..65535
        pics = _pics(ref_size=(64, 64))
        pics[0].ref_w[1], pics[0].ref_h[1] = size
        assert f(8, 1, 1, 64, 64, 1, v(pics), None) == E, size
        assert b"reference 1" in _lib.lib().ffhip_last_error()
    pics = _pics(ref_size=(128, 128), stride=256)                    # a 2x reference needs a stride of its own width
    for r in range(2):
        for p in range(3):
            pics[0].pic.ref[r].stride[p] = 1024
    pics[0].pic.ref[1].stride[0] = 120                               # below 128
    assert f(8, 1, 1, 64, 64, 1, v(pics), None) == E
    pics[0].pic.ref[1].stride[0] = 128
    pics[0].pic.ref[1].stride[1] = 60                                # chroma: below (128 + 1) >> 1
    assert f(8, 1, 1, 64, 64, 1, v(pics), None) == E
    pics = _pics(n=2)                                                # overlap over the reference's own extent: 64 rows of the
    pics[1].ref_w[0], pics[1].ref_h[0] = 100, 100                    # frame's size miss the plane, 100 rows reach it
    for p in range(3):
        pics[1].pic.ref[0].stride[p] = 256
    pics[1].pic.ref[0].base[0] = pics[0].pic.plane[0].base - 256 * 80
    assert f(8, 1, 1, 64, 64, 2, v(pics), None) == E
    assert b"overlaps" in _lib.lib().ffhip_last_error()
    pics[1].ref_w[0], pics[1].ref_h[0] = 64, 64
    if _lib.lib().ffhip_device_count() == 0:
        assert f(8, 1, 1, 64, 64, 2, v(pics), None) == _lib.ENOSYS


@pytest.mark.skipif(_lib.lib().ffhip_device_count() > 0, reason="a HIP device is present: the refusal path is not reachable")
def test_no_device_refusals():
    L = _lib.lib()
    assert L.ffhip_vp9_inter_frames_scaled_dev(8, 1, 1, 64, 64, 1, C.cast(_pics(), C.c_void_p), None) == _lib.ENOSYS
    pics = _pics(ref_size=(32, 4), stride=256)                       # 2x up horizontally, 16x up vertically
    assert L.ffhip_vp9_inter_frames_scaled_dev(12, 0, 0, 64, 64, 1, C.cast(pics, C.c_void_p), None) == _lib.ENOSYS
    pics = _pics(nrefs=1)
    pics[0].ref_w[2] = 0                                             # past nrefs: not looked at
    assert L.ffhip_vp9_inter_frames_scaled_dev(10, 1, 0, 64, 64, 1, C.cast(pics, C.c_void_p), None) == _lib.ENOSYS


def test_ref_scale_matches_the_header_rule():
    assert S.ref_scale(64, 48, 128, 96) == ((32768, 32768), (32, 32))
    assert S.ref_scale(128, 96, 8, 6) == ((1024, 1024), (1, 1))
    assert S.ref_scale(100, 70, 150, 47) == (((150 << 14) // 100, (47 << 14) // 70), (24, 10))
    assert S.ref_scale(77, 53, 77, 53) == ((0, 0), (0, 0))


def test_block_preds_scaled_match_the_template():
    rng = np.random.default_rng(40)
    for bs in range(13):
        for ss in ((1, 1), (1, 0), (0, 1), (0, 0)):
            for comp in (0, 1):
                for _ in range(3):
                    mv = rng.integers(-3000, 3000, (4, 2, 2))
                    ref = [int(rng.integers(0, 3)), int(rng.integers(0, 3))]
                    filt, row, col = int(rng.integers(0, 4)), int(rng.integers(0, 500)), int(rng.integers(0, 500))
                    got = vp9.inter_block_preds_scaled(bs, row, col, mv, comp, ref, filt, ss)
                    want = S.block_preds_scaled(bs, row, col, mv.tolist(), comp, ref, filt, *ss)
                    assert len(got) == len(want), (bs, ss, comp)
                    for g, w in zip(got, want):
                        for f in S.PRED_FIELDS:
                            assert np.array_equal(np.asarray(g[f]), np.asarray(w[f])), (bs, ss, comp, f, g, w)
                        assert g["flags"] & vp9.INTER_SCALED
                        b0, b1 = int(g["box"][0]), int(g["box"][1])
                        assert (b0 & 15) + g["w"] <= 1 << (b1 & 15) and (b0 >> 4) + g["h"] <= 1 << (b1 >> 4)
    assert vp9.inter_block_preds_scaled(12, 0, 0, np.zeros((4, 2, 2)), 0, [0, 0], 0, (1, 1)).shape == (5,)
    with pytest.raises(Exception):
        vp9.inter_block_preds_scaled(13, 0, 0, np.zeros((4, 2, 2)), 0, [0, 0], 0)


@pytest.mark.parametrize("case", range(len(S.RATIOS)))
@pytest.mark.parametrize("bd,ss", [(8, (1, 1)), (10, (1, 0)), (12, (0, 1)), (8, (0, 0))], ids=["8-420", "10-422", "12-440", "8-444"])
def test_model_equals_the_padded_route(case, bd, ss):
    (W, H), sizes = S.RATIOS[case]
    rng = np.random.default_rng(4100 + case * 7 + bd + 2 * ss[0] + ss[1])
    fr = S.ScaledFrame(rng, W, H, bd, *ss, sizes, p_far=0.0, p_edge=0.2, p_comp=0.5)
    assert any(r["flags"] & S.SCALED for r in fr.preds)
    a, b = S.model(fr), S.model(fr, route="pad")
    for p in range(3):
        assert np.array_equal(a[p], b[p]), p


def test_generator_coverage():
    """every block size, compound blocks mixing a scaled and an unscaled reference, 64x64 blocks at 2x down, far MVs that hit the clip"""
    rng = np.random.default_rng(42)
    fr = S.ScaledFrame(rng, 96, 64, 8, 1, 1, [(144, 96), (96, 64)], p_comp=0.6, p_far=0.3, min_log2=2)
    bss = {b[0] for b in fr.blocks if b[3] == "inter"}
    assert {10, 11, 12} & bss
    mixed = [r for r in fr.preds if r["flags"] & 1 and r["flags"] & S.SCALED and fr.scaled(r["ref"][0]) != fr.scaled(r["ref"][1])]
    assert mixed
    big = S.ScaledFrame(np.random.default_rng(43), 64, 64, 8, 1, 1, [(128, 128)], p_intra=0, p_comp=0, min_log2=6)
    assert any(r["w"] == 64 and r["h"] == 64 for r in big.preds)
    assert any(abs(r["mv"][0][0]) > 1000 for r in fr.preds)


def test_unscaled_frames_match_the_inter_model():
    rng = np.random.default_rng(44)
    fr = S.ScaledFrame(rng, 99, 67, 10, 1, 1, [(99, 67), (99, 67)], p_far=0.2)
    assert not any(r["flags"] & S.SCALED for r in fr.preds)
    a, b = S.model(fr), G.model(fr)
    for p in range(3):
        assert np.array_equal(a[p], b[p]), p
