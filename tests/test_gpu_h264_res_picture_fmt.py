"""The _fmt face of the H.264 whole-picture residual on the GPU (ffhip_h264_residual_pictures_fmt_dev) at 4:2:2 and 4:4:4, byte for
byte against the host face and the model of h264_fmt_picture_gen.py: whole buffers with stride padding 0 and 8 samples and guard
rows, inputs unchanged; 17 pictures to a call, 121 x 1 and 1 x 70 macroblocks (8 macroblocks to a workgroup), 14 bits into both
clips; at 4:2:0 and monochrome against the existing face; against the per-call batch face; and chained behind the inter _fmt face on
one created stream with no synchronisation in between."""
import ctypes as C

import numpy as np
import pytest

import h264_fmt_picture_gen as F
import h264_res_picture_gen as GR
import test_gpu_h264_inter_picture as TGI
import test_gpu_h264_res_picture as TG
from ffmpeg_amd import _lib, h264

pytestmark = pytest.mark.gpu


def host_planes(pics, fmt):
    planes = [[b.copy() for b in p.before] for p in pics]
    args = [dict(dst=[a.ctypes.data for a in pl] + [None] * (3 - len(pl)), dst_stride=[a.strides[0] for a in pl] + [0] * (3 - len(pl)), mb=p.mb,
                 res=p.res, coeffs=p.coeffs, ncoeffs=p.ncoeffs) for p, pl in zip(pics, planes)]
    h264.residual_pictures_fmt_host(args, pics[0].mb_w, pics[0].mb_h, pics[0].bd, fmt)
    return planes


def run(pics, models, fmt, pad=0, what="", face=h264.residual_pictures_fmt, host=True):
    torch = TG._torch()
    if host:
        for k, (pl, (want, _)) in enumerate(zip(host_planes(pics, fmt), models)):
            assert all(np.array_equal(a, b) for a, b in zip(pl, want)), "%s picture %d: the host face differs from the model" % (what, k)
    up = [TG.upload(torch, p, m[0], pad) for p, m in zip(pics, models)]
    torch.cuda.synchronize()
    face([a for a, _ in up], pics[0].mb_w, pics[0].mb_h, pics[0].bd, fmt)
    assert _lib.lib().ffhip_stream_synchronize(None) == 0, _lib.lib().ffhip_last_error()
    torch.cuda.synchronize()
    TG.compare(up, what=what)
    return up


@pytest.mark.parametrize("fmt", [2, 3])
def test_picture_sets(fmt):
    """every set of the format, one call per set, tight rows and rows 8 samples wider: the device face, the host face and the model
    agree (5x4_*_14 reaches both clips: the CPU tier asserts it)"""
    for name in F.RES_NAMES:
        pics, models = F.res_set(name)
        if pics[0].fmt == fmt:
            for pad in (0, 8):
                run(pics, models, fmt, pad, name, host=pad == 0)


@pytest.mark.parametrize("name", ["3x2", "5x4_10", "3x2_mono"])
def test_at_420_and_monochrome_the_bytes_of_the_existing_face(name):
    pics, models = GR.picture_set(name)
    cfi = int(pics[0].chroma)
    a = run(pics, models, cfi, 4, name + " fmt", host=False)
    b = run(pics, models, cfi, 4, name + " existing", face=h264.residual_pictures, host=False)
    for (_, x), (_, y) in zip(a, b):
        for s, t in zip(x["bufs"], y["bufs"]):
            assert bool((s == t).all())


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("fmt", [2, 3])
def test_against_the_per_call_batch_face(fmt, bd):
    """the same content through ffhip_h264_idct_mb_batch_dev_hbd: which 0 / 1 per plane (luma, and Cb / Cr at 4:4:4) and which 4
    (idct_add8_422) on the dequantised image give the planes the face gives in one launch; both equal the model"""
    torch = TG._torch()
    L = _lib.lib()
    pic = F.ResPicture(np.random.default_rng(9950 + bd + fmt), 7, 5, fmt, bd, density=0.6, p_t8=0.5)
    lists = []
    want, cover = F.res_model(pic, lists=lists)
    assert cover["t8"] >= 3 and cover["luma_only"] >= 3 and cover["with_chroma"] >= 3
    arg, up = TG.upload(torch, pic, want, 0)
    planes = [TG._dev(torch, b) for b in pic.before]
    strides = [b.strides[0] for b in pic.before]
    ps, cdt = (2 if bd > 8 else 1), GR.coef_dtype(bd)
    typed = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    keep = []
    torch.cuda.synchronize()
    h264.residual_pictures_fmt([arg], pic.mb_w, pic.mb_h, bd, fmt)
    for pl in range(3 if fmt == 3 else 1):
        bo = np.zeros(48, np.int32)
        bo[:16] = [4 * F.Y4[i] * strides[pl] + 4 * F.X4[i] * ps for i in range(16)]
        for t8 in (0, 1):
            sel = [e for e in lists if e["t8"] == t8 and len(e["planes"]) > pl]
            if not sel:
                continue
            d = [typed(np.array([(e["m"] // pic.mb_w) * 16 * strides[pl] + (e["m"] % pic.mb_w) * 16 * ps for e in sel], np.int32)), typed(bo),
                 typed(np.array([e["planes"][pl][0] for e in sel], cdt)), typed(np.array([e["planes"][pl][1] for e in sel], np.uint8))]
            keep += d
            _lib.check(L.ffhip_h264_idct_mb_batch_dev_hbd(bd, t8, planes[pl].data_ptr(), None, strides[pl], d[0].data_ptr(), d[1].data_ptr(),
                                                          d[2].data_ptr(), d[3].data_ptr(), len(sel), None), "idct_mb")
    if fmt == 2:
        sel = [e for e in lists if "chroma" in e]
        bo = np.zeros(48, np.int32)
        for j in (1, 2):
            for k in range(4):
                bo[16 * j + k] = (k >> 1) * 4 * strides[1] + (k & 1) * 4 * ps
                bo[16 * j + 8 + k] = (2 + (k >> 1)) * 4 * strides[1] + (k & 1) * 4 * ps
        d = [typed(np.array([(e["m"] // pic.mb_w) * 16 * strides[1] + (e["m"] % pic.mb_w) * 8 * ps for e in sel], np.int32)), typed(bo),
             typed(np.array([e["chroma"][0] for e in sel], cdt)), typed(np.array([e["chroma"][1] for e in sel], np.uint8))]
        keep += d
        _lib.check(L.ffhip_h264_idct_mb_batch_dev_hbd(bd, 4, planes[1].data_ptr(), planes[2].data_ptr(), strides[1], d[0].data_ptr(), d[1].data_ptr(),
                                                      d[2].data_ptr(), d[3].data_ptr(), len(sel), None), "idct_add8_422")
    assert L.ffhip_stream_synchronize(None) == 0
    torch.cuda.synchronize()
    TG.compare([(arg, up)], what="face")
    for p, (t, w) in enumerate(zip(planes, want)):
        got = t.cpu().numpy().view(w.dtype).reshape(w.shape)
        assert np.array_equal(got, w), "plane %d: the per-call face differs from the model in %d samples" % (p, (got != w).sum())


@pytest.mark.parametrize("fmt,bd", [(2, 8), (3, 10)])
def test_inter_then_residual_on_one_created_stream(fmt, bd):
    """inter_fmt -> residual_fmt on a created stream with no synchronisation in between == the residual model run on the inter
    model's planes"""
    torch = TG._torch()
    L = _lib.lib()
    rng = np.random.default_rng(9960 + fmt)
    mb_w, mb_h, pad = 6, 5, 8
    ipic = F.InterPicture(rng, mb_w, mb_h, fmt, bd, nslices=2, nrefs=3, p_intra=0.15)
    pred = F.inter_model(ipic)[0]
    rpic = F.ResPicture(rng, mb_w, mb_h, fmt, bd)
    rpic.mb["flags"] = (rpic.mb["flags"] & 0xFE) | (ipic.mb["flags"] & 1)     # one macroblock array for both faces
    rpic.mb["slice"], rpic.mb["qp"] = ipic.mb["slice"], ipic.mb["qp"]
    rpic.before = pred
    rpic.layout()
    want = F.res_model(rpic)[0]
    iarg, iup = TGI.upload(torch, ipic, want, pad)               # the destination buffers: poisoned, expected to hold the chain's result
    mbs, res, co = TG._dev(torch, rpic.mb), TG._dev(torch, rpic.res), TG._dev(torch, rpic.coeffs)
    iarg["mb"] = mbs
    rarg = dict(dst=iarg["dst"], dst_stride=iarg["dst_stride"], mb=mbs, res=res, coeffs=co, ncoeffs=rpic.ncoeffs)
    st = C.c_void_p()
    assert L.ffhip_stream_create(C.byref(st)) == 0, L.ffhip_last_error()
    torch.cuda.synchronize()
    try:
        h264.inter_pictures_fmt([iarg], mb_w, mb_h, bd, fmt, stream=st.value)
        h264.residual_pictures_fmt([rarg], mb_w, mb_h, bd, fmt, stream=st.value)
        assert L.ffhip_stream_synchronize(st) == 0, L.ffhip_last_error()
    finally:
        torch.cuda.synchronize()
        assert L.ffhip_stream_destroy(st) == 0
    intra = np.repeat(np.repeat((ipic.mb["flags"] & 1).reshape(mb_h, mb_w) != 0, 16, 0), 16, 1)
    assert intra.any() and (want[0][~intra] != pred[0][~intra]).any()
    iup["keep"], iup["before"] = [], []                           # the inter inputs but mb: checked by the inter tests
    TGI.compare([(iarg, iup)], what="chain")
