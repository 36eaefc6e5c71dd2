"""H.264 residuals of whole pictures on the GPU (ffhip_h264_residual_pictures_dev), byte for byte against the host face and the model
of h264_res_picture_gen.py (the oracle's dispatchers in decoder order): whole destination buffers with their stride padding and a
guard row on either side, and the inputs, which must come back unchanged.  The picture sets of the CPU tier plus 17 pictures to a call
(two launches) and 121 x 1 / 1 x 70 macroblocks (8 macroblocks to a workgroup: a last workgroup with one and with six); then the same
content through the four per-call batch faces the face replaces, and the chain inter -> residual -> edge parameters -> deblock on
one stream against the oracle's serial sequence."""
import copy
import ctypes as C

import numpy as np
import pytest

import h264_res_picture_gen as G
from ffmpeg_amd import _lib, h264

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _poison(dtype):
    return np.frombuffer(bytes([G.POISON]) * 2, dtype)[0]


def padded(plane, pad):
    """the plane in rows `pad` samples wider with a guard row above and below, padding and guards poisoned"""
    a = np.full((plane.shape[0] + 2, plane.shape[1] + pad), _poison(plane.dtype), plane.dtype)
    a[1:-1, :plane.shape[1]] = plane
    return a


def upload(torch, pic, want, pad=0, npl=None):
    """(the face's dict, what compare() needs)"""
    npl = len(pic.before) if npl is None else npl
    bufs, exp, dst, strides = [], [], [], []
    for p in range(npl):
        b = padded(pic.before[p], pad)
        bufs.append(_dev(torch, b))
        exp.append(padded(want[p], pad))
        strides.append(b.strides[0])
        dst.append(bufs[-1].data_ptr() + strides[-1])
    ins = [_dev(torch, pic.mb), _dev(torch, pic.res), _dev(torch, pic.coeffs)]
    arg = dict(dst=dst + [None] * (3 - npl), dst_stride=strides + [0] * (3 - npl), mb=ins[0], res=ins[1], coeffs=ins[2], ncoeffs=pic.ncoeffs)
    return arg, dict(bufs=bufs, exp=exp, keep=ins, before=[t.clone() for t in ins])


def compare(up, view=lambda t: t, what=""):
    import torch
    for k, (_, u) in enumerate(up):
        for p, (t, e) in enumerate(zip(u["bufs"], u["exp"])):
            got = view(t).cpu().numpy().view(e.dtype).reshape(e.shape)
            bad = np.argwhere(got != e)
            assert not len(bad), "%s picture %d plane %d: %d samples differ, first at row %d column %d: got %d want %d" % (
                what, k, p, len(bad), bad[0][0] - 1, bad[0][1], got[tuple(bad[0])], e[tuple(bad[0])])
        for t, b in zip(u["keep"], u["before"]):
            assert torch.equal(t, b), "%s picture %d: an input was written" % (what, k)


def host_planes(pics, cfi):
    """the host face on tight copies of the planes"""
    planes = [[b.copy() for b in p.before] for p in pics]
    args = [dict(dst=[a.ctypes.data for a in pl] + [None] * (3 - len(pl)), dst_stride=[a.strides[0] for a in pl] + [0] * (3 - len(pl)), mb=p.mb,
                 res=p.res, coeffs=p.coeffs, ncoeffs=p.ncoeffs) for p, pl in zip(pics, planes)]
    h264.residual_pictures_host(args, pics[0].mb_w, pics[0].mb_h, pics[0].bd, cfi)
    return planes


def run(pics, models, pad=0, what="", cfi=None):
    torch = _torch()
    cfi = int(pics[0].chroma) if cfi is None else cfi
    for k, (pl, (want, _)) in enumerate(zip(host_planes(pics, cfi), models)):
        assert all(np.array_equal(a, b) for a, b in zip(pl, want)), "%s picture %d: the host face differs from the model" % (what, k)
    up = [upload(torch, p, m[0], pad) for p, m in zip(pics, models)]
    torch.cuda.synchronize()
    P0 = pics[0]
    h264.residual_pictures([a for a, _ in up], P0.mb_w, P0.mb_h, P0.bd, cfi)
    assert _lib.lib().ffhip_stream_synchronize(None) == 0, _lib.lib().ffhip_last_error()
    torch.cuda.synchronize()
    compare(up, what=what)


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("name", G.NAMES)
def test_picture_set(name, pad):
    """one call per set, with tight strides and with rows 8 samples wider: the device face, the host face and the model agree"""
    pics, models = G.picture_set(name)
    run(pics, models, pad, name)


def test_monochrome_through_chroma_format_idc_1_with_null_chroma():
    pics, models = G.picture_set("3x2_mono")
    run(pics, models, 4, "mono", cfi=1)


def test_the_reference_dispatchers_dc_forms_where_the_coefficient_type_wraps():
    """rule 9's exception at 8 bits, in every place a DC of 32736 .. 32767 can stand (tests/test_h264_res_picture_cpu.py has the
    same macroblock with the expected samples spelled out)"""
    pic = G.blank(2, 1, 8)
    dc = np.zeros(16, np.int64)
    for m, v in enumerate((32760, 32736)):
        dc[0] = v
        pic.set_luma4(m, 0, values=dc)
        ac = dc.copy()
        ac[5] = 1
        pic.set_luma4(m, 1, values=ac)
        pic.set_chroma(m, 0, dc=False, bits=[0])
        pic.blocks[m][256:272] = dc
        pic.set_chroma(m, 1, dc=True, bits=[2])
        pic.blocks[m][512:768:16][:4] = [v, 0, 0, 0]
        pic.res["qmul"][m][1] = 128
    pic.mb["flags"][1] = h264.BS_MB_T8X8
    pic.mb["nnz"][1] = 0
    big = np.zeros(64, np.int64)
    big[0] = 32767
    pic.set_luma8(1, 2, values=big)
    pic.layout()
    run([pic], [G.model(pic)], 4, "wrap")


# ------------------------------------------------------------------------------------ the adapter of tests/picture_faces.py
class Face:
    """the face alone, with the steps tests/picture_faces.py gives its adapters"""
    name, codec, pad = "h264_residual_pictures", "h264", 4

    def __init__(self, bd=8):
        self.bd = bd

    def build(self, seed):
        rng = np.random.default_rng(seed + self.bd)
        self.pics = [G.ResPicture(rng, 5, 4, self.bd) for _ in range(2)]
        self.models = [G.model(p) for p in self.pics]
        return self

    def fresh(self):
        return copy.copy(self)

    def upload(self, torch):
        self.up = [upload(torch, p, m[0], self.pad) for p, m in zip(self.pics, self.models)]

    def call(self, stream):
        h264.residual_pictures([a for a, _ in self.up], 5, 4, self.bd, 1, stream=stream)

    def inputs(self):
        return [t for _, u in self.up for t in u["keep"]]

    def outputs(self):
        return [t for _, u in self.up for t in u["bufs"]]

    def compare(self, view=lambda t: t):
        compare(self.up, view, self.name)


# ---------------------------------------------------------------------------------------------------- the four-launch chain
def batch_lists(pic, lists, strides):
    """what a caller of the per-call faces assembles on the host from the same content: per transform size an mb_offset list, the
    nnzc caches and dense coefficients; for chroma the 768-coefficient image, the 120-byte caches and the DC's block_offset / qmul"""
    ps = 2 if pic.bd > 8 else 1
    cdt = G.coef_dtype(pic.bd)
    bo = np.zeros(48, np.int32)
    for i in range(16):
        bo[i] = 4 * G.Y4[i] * strides[0] + 4 * G.X4[i] * ps
    for j in (1, 2):
        for k in range(4):
            bo[16 * j + k] = (k >> 1) * 4 * strides[1] + (k & 1) * 4 * ps
    out = dict(bo=bo)
    for t8 in (0, 1):
        sel = [e for e in lists if e["t8"] == t8]
        out["luma%d" % t8] = dict(
            mb_off=np.array([(e["m"] // pic.mb_w) * 16 * strides[0] + (e["m"] % pic.mb_w) * 16 * ps for e in sel], np.int32),
            blocks=np.array([e["dense"][:256] for e in sel], cdt).reshape(len(sel), 256),
            nnzc=np.array([e["nnzc"][:40] for e in sel], np.uint8).reshape(len(sel), 40))
    sel = [e for e in lists if e["need"] == 768]
    out["chroma"] = dict(
        mb_off=np.array([(e["m"] // pic.mb_w) * 8 * strides[1] + (e["m"] % pic.mb_w) * 8 * ps for e in sel], np.int32),
        blocks=np.array([e["dense"] for e in sel], cdt).reshape(len(sel), 768),
        nnzc=np.array([e["nnzc"] for e in sel], np.uint8).reshape(len(sel), 120),
        dc_off=np.array([k * 768 + 256 * (1 + c) for k, e in enumerate(sel) for c in range(2) if (e["cdc"] >> c) & 1], np.int32),
        dc_qmul=np.array([e["qmul"][c] for e in sel for c in range(2) if (e["cdc"] >> c) & 1], np.int32))
    return out


def launch_batch_chain(torch, bd, planes, strides, d, stream=None):
    """the four launches (idct_add16, idct8_add4, chroma_dc_dequant_idct, idct_add8) on device lists `d` of batch_lists()"""
    L = _lib.lib()
    st = h264._stream(stream)
    ok = lambda r: _lib.check(r, "a batch face")
    for t8 in (0, 1):
        l = d["luma%d" % t8]
        n = l["mb_off"].numel()
        if not n:
            continue
        if bd == 8:
            h264.idct_add_mb_batch(t8, planes[0], strides[0], l["mb_off"], d["bo"], l["blocks"], l["nnzc"], stream=stream)
        else:
            ok(L.ffhip_h264_idct_mb_batch_dev_hbd(bd, t8, planes[0].data_ptr(), None, strides[0], l["mb_off"].data_ptr(), d["bo"].data_ptr(),
                                                  l["blocks"].data_ptr(), l["nnzc"].data_ptr(), n, st))
    c = d["chroma"]
    n, ndc = c["mb_off"].numel(), c["dc_off"].numel()
    if ndc:
        if bd == 8:
            h264.chroma_dc_dequant_batch(c["blocks"], c["dc_off"], c["dc_qmul"], stream=stream)
        else:
            ok(L.ffhip_h264_dc_dequant_batch_dev_hbd(bd, 1, c["blocks"].data_ptr(), 0, None, 0, c["dc_off"].data_ptr(), c["dc_qmul"].data_ptr(), ndc, st))
    if n:
        if bd == 8:
            h264.idct_add8_batch(planes[1], planes[2], strides[1], c["mb_off"], d["bo"], c["blocks"], c["nnzc"], stream=stream)
        else:
            ok(L.ffhip_h264_idct_mb_batch_dev_hbd(bd, 3, planes[1].data_ptr(), planes[2].data_ptr(), strides[1], c["mb_off"].data_ptr(),
                                                  d["bo"].data_ptr(), c["blocks"].data_ptr(), c["nnzc"].data_ptr(), n, st))


def to_device(torch, lists):
    typed = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return {k: ({q: typed(a) for q, a in v.items()} if isinstance(v, dict) else typed(v)) for k, v in lists.items()}


@pytest.mark.parametrize("bd", [8, 10])
def test_against_the_four_launch_chain(bd):
    """the same content through ffhip_h264_idct_add_mb_batch_dev (which 0 and 1), ffhip_h264_chroma_dc_dequant_idct_batch_dev and
    ffhip_h264_idct_add8_batch_dev (their _hbd twins at 10 bits) gives the planes the face gives in one launch; both equal the model"""
    torch = _torch()
    rng = np.random.default_rng(9800 + bd)
    pic = G.ResPicture(rng, 7, 5, bd)
    lists = []
    want, cover = G.model(pic, lists=lists)
    assert cover["t8"] >= 3 and cover["luma_only"] >= 3 and cover["with_chroma"] >= 3 and cover["cdc"] >= 3
    arg, up = upload(torch, pic, want, 0)
    planes = [_dev(torch, b) for b in pic.before]
    strides = [b.strides[0] for b in pic.before]
    d = to_device(torch, batch_lists(pic, lists, strides))
    torch.cuda.synchronize()
    h264.residual_pictures([arg], pic.mb_w, pic.mb_h, bd, 1)
    launch_batch_chain(torch, bd, planes, strides, d)
    torch.cuda.synchronize()
    compare([(arg, up)], what="face")
    for p, (t, w) in enumerate(zip(planes, want)):
        got = t.cpu().numpy().view(w.dtype).reshape(w.shape)
        assert np.array_equal(got, w), "plane %d: the four-launch chain differs from the model in %d samples" % (p, (got != w).sum())


# -------------------------------------------------------------------------------------------------------------------- chain
class Chain:
    """ffhip_h264_inter_pictures_dev -> ffhip_h264_residual_pictures_dev -> ffhip_h264_edge_params_pictures_dev -> the deblock faces
    of luma, Cb and Cr, on one stream with no synchronisation in between and from one upload of mb / mvf: the planes equal the
    oracle's serial sequence (the inter model's prediction, this file's residual model on top of it, the oracle's frame filter on
    model A's tables of tests/h264_bs_picture_gen.py).  The steps tests/picture_faces.py gives its adapters."""
    codec, mb_w, mb_h = "h264", 6, 5

    def __init__(self, bd=8):
        self.bd = bd
        self.name = "h264_inter+residual+edge_params+deblock_%d" % bd

    def build(self, seed=9810):
        import ffi
        import h264_bs_picture_gen as B
        import h264_inter_picture_gen as I
        bd, mb_w, mb_h = self.bd, self.mb_w, self.mb_h
        rng = np.random.default_rng(seed + bd)
        dt, sh = G.sample_dtype(bd), bd - 8
        smooth = lambda h, w: (rng.integers(118, 138, (h, w)) << sh).astype(dt)    # flat enough for the filter to switch on
        shapes = ((16 * mb_h, 16 * mb_w), (8 * mb_h, 8 * mb_w), (8 * mb_h, 8 * mb_w))
        refs = [[smooth(*s) for s in shapes] for _ in range(3)]
        pic = self.pic = I.InterPicture(rng, mb_w, mb_h, bd, nslices=2, nrefs=3, p_intra=0.15, weights="none", refs=refs)
        n = mb_w * mb_h
        pic.mb["qp"] = rng.integers(26, 44, n) + 6 * sh
        # the residual of the inter macroblocks on the same macroblock array: its nnz bits are what the filter sees
        res = self.res = G.blank(mb_w, mb_h, bd, seed=seed)
        res.mb = pic.mb
        small = lambda k: rng.integers(-60, 60, k) << sh
        for m in np.nonzero((pic.mb["flags"] & 1) == 0)[0]:
            if rng.random() < 0.3:
                pic.mb["flags"][m] |= h264.BS_MB_T8X8
                for k in range(4):
                    if rng.random() < 0.5:
                        res.set_luma8(m, k, values=small(64))
            else:
                for i in range(16):
                    r = rng.random()
                    if r < 0.5:
                        v = small(16)
                        if r < 0.2:
                            v[1:] = 0
                        res.set_luma4(m, i, values=v)
            if rng.random() < 0.6:
                for c in range(2):
                    res.set_chroma(m, c, dc=rng.random() < 0.7, bits=[j for j in range(4) if rng.random() < 0.4])
        res.layout()
        # what the planes hold before: the intra macroblocks' samples stay
        self.before = [smooth(*s) for s in shapes]
        a, b = I.model(pic)[0], I.model(pic, fill=I.POISON ^ 0xFF)[0]
        res.before = [np.where(x == y, x, z) for x, y, z in zip(a, b, self.before)]
        want, cover = G.model(res)
        assert cover["with_chroma"] >= 5 and cover["t8"] >= 2 and cover["intra"] >= 1
        self.predicted = [w.copy() for w in want]
        bs = self.bs = B.blank(mb_w, mb_h, 0, 6 * sh)
        bs.mb, bs.mvf = pic.mb, pic.mvf
        bs.slices = np.zeros(pic.nslices, h264.BS_SLICE_DTYPE)
        bs.slices["ref"], bs.slices["num_ref"], bs.slices["flags"] = pic.slices["ref"], pic.slices["num_ref"], pic.is_b
        bs.nslices = pic.nslices
        self.tables = B.model_a(bs)
        O = ffi.oracle()
        O.ffo_h264_deblock_frame_bd.argtypes = [C.c_int, C.c_int, ffi.u8p, C.c_ssize_t, C.c_int, C.c_int, C.c_void_p]
        for p, t in enumerate(("luma", "cb", "cr")):
            e = C.c_void_p(np.ascontiguousarray(self.tables[t]).ctypes.data)
            at = C.cast(want[p].ctypes.data, ffi.u8p)
            if bd > 8:
                O.ffo_h264_deblock_frame_bd(bd, int(p > 0), at, want[p].strides[0], mb_w, mb_h, e)
            else:
                (O.ffo_h264_deblock_frame_chroma if p else O.ffo_h264_deblock_frame)(at, want[p].strides[0], mb_w, mb_h, e)
        self.want = want
        assert all((w != q).sum() > 50 for w, q in zip(want, self.predicted)), "the filter changed next to nothing"
        assert all((q != r).sum() > 50 for q, r in zip(self.predicted, res.before)), "the residual changed next to nothing"
        return self

    def fresh(self):
        return copy.copy(self)

    def upload(self, torch):
        pic, res = self.pic, self.res
        m = self.bs.maps()
        self.planes = [_dev(torch, b) for b in self.before]
        self.refs = [[_dev(torch, r[p]) for p in range(3)] for r in pic.refs]
        self.ins = dict(mb=_dev(torch, pic.mb), mvf=_dev(torch, pic.mvf), slices=_dev(torch, pic.slices), bs_slices=_dev(torch, self.bs.slices),
                        chroma_qp=_dev(torch, m["chroma_qp"]), res=_dev(torch, res.res), coeffs=_dev(torch, res.coeffs))
        n = self.mb_w * self.mb_h
        self.edges = [torch.full((n * per * 12,), 0xEE, dtype=torch.uint8, device="cuda") for per in (8, 4, 4)]

    def call(self, stream):
        pic, i, bd = self.pic, self.ins, self.bd
        strides = [b.strides[0] for b in self.before]
        h264.inter_pictures([dict(dst=self.planes, dst_stride=strides, mb=i["mb"], mvf=i["mvf"], slices=i["slices"], mvf_stride=pic.w4,
                                  nslices=pic.nslices, refs=[dict(base=r, stride=strides) for r in self.refs])], pic.mb_w, pic.mb_h, bd, 1, stream=stream)
        h264.residual_pictures([dict(dst=self.planes, dst_stride=strides, mb=i["mb"], res=i["res"], coeffs=i["coeffs"], ncoeffs=self.res.ncoeffs)],
                               pic.mb_w, pic.mb_h, bd, 1, stream=stream)
        h264.edge_params_pictures([dict(mb=i["mb"], mvf=i["mvf"], slices=i["bs_slices"], chroma_qp=i["chroma_qp"], luma=self.edges[0],
                                        cb=self.edges[1], cr=self.edges[2], mvf_stride=pic.w4, nslices=pic.nslices)], pic.mb_w, pic.mb_h, 0,
                                  6 * (bd - 8), stream=stream)
        for p, (pl, e) in enumerate(zip(self.planes, self.edges)):
            h, s = self.before[p].shape[0], strides[p]
            if bd > 8:
                h264.deblock_frames_hbd(bd, pl, h * s, 1, s, pic.mb_w, pic.mb_h, e, chroma=p > 0, stream=stream)
            else:
                (h264.deblock_frames_chroma if p else h264.deblock_frames)(pl, h * s, 1, s, pic.mb_w, pic.mb_h, e, stream=stream)

    def inputs(self):
        return list(self.ins.values()) + [t for r in self.refs for t in r]

    def outputs(self):
        return list(self.planes) + list(self.edges)

    def compare(self, view=lambda t: t):
        for t, e in zip(("luma", "cb", "cr"), self.edges):
            assert np.array_equal(view(e).cpu().numpy().view(h264.EDGE_DTYPE), self.tables[t]), "%s: the %s table differs from model A" % (self.name, t)
        for p, (pl, w) in enumerate(zip(self.planes, self.want)):
            got = view(pl).cpu().numpy().view(w.dtype).reshape(w.shape)
            assert np.array_equal(got, w), "%s: plane %d: %d samples differ from the oracle's serial sequence" % (self.name, p, (got != w).sum())


@pytest.mark.parametrize("bd", [8, 10])
def test_chained_from_the_prediction_into_the_filter_on_one_stream(bd):
    """Chain on the NULL stream (tests/test_gpu_h264_res_picture_streams.py runs it on a created one)"""
    torch = _torch()
    chain = Chain(bd).build()
    chain.upload(torch)
    torch.cuda.synchronize()
    chain.call(None)
    assert _lib.lib().ffhip_stream_synchronize(None) == 0, _lib.lib().ffhip_last_error()
    torch.cuda.synchronize()
    chain.compare()
