"""HEVC inter reconstruction of whole pictures on the GPU (ffhip_hevc_inter_pictures_dev), byte for byte against the sequential model
of hevc_inter_picture_gen.py (the oracle's put_hevc_* on clamped windows), stride padding included.  Every call is followed by
ffhip_stream_synchronize(None) == 0."""
import numpy as np
import pytest

import hevc_inter_picture_gen as G
from ffmpeg_amd import _lib, hevc

pytestmark = pytest.mark.gpu

SENT = 0x5A


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _dt(bd):
    return np.uint8 if bd == 8 else np.uint16


def _plane_bytes(a, bd, stride, fill=SENT):
    """a plane (int64 samples) as a (h, stride) byte image, the padding filled with `fill`"""
    h, w = a.shape
    ps = 1 if bd == 8 else 2
    host = np.full((h, stride), fill, np.uint8)
    host[:, :w * ps] = a.astype(_dt(bd)).view(np.uint8).reshape(h, w * ps)
    return host


def _stride(w, bd, extra):
    ps = 1 if bd == 8 else 2
    return (w * ps + 63) // 64 * 64 + extra


def upload_refs(torch, pic, extra=0):
    """the DPB on the device: per slot, per plane (tensor, stride)"""
    out = []
    for ref in pic.refs:
        planes = []
        for p in range(pic.nplanes):
            st = _stride(ref[p].shape[1], pic.bd, extra + 8 * p)
            planes.append((torch.from_numpy(_plane_bytes(ref[p], pic.bd, st, 0x33)).cuda(), st))
        out.append(planes)
    return out


def upload(torch, pic, extra=0, pus=None, tus=None, refs=None, planes=None):
    """(the face's tuple for this picture, the destination (host image, device tensor) per plane, tensors to keep alive)"""
    pus = pic.pus if pus is None else pus
    tus = pic.tus if tus is None else tus
    src = pic.planes if planes is None else planes
    keep, dst, pl = [], [], []
    for p in range(pic.nplanes):
        h, w = src[p].shape
        st = _stride(w, pic.bd, extra)
        host = _plane_bytes(src[p], pic.bd, st)
        d = torch.from_numpy(host.copy()).cuda()
        arr, starts = pic.pack(tus[p], hevc.INTER_TU_DTYPE, ("x", "y", "res_offset", "log2_size"))
        d_tus = torch.from_numpy(arr.view(np.uint8).copy() if len(arr) else np.zeros(16, np.uint8)).cuda()
        d_st = torch.from_numpy(starts).cuda()
        d_res = torch.from_numpy(pic.res[p].astype(np.int16)).cuda()
        keep += [d, d_tus, d_st, d_res]
        pl.append((d, st, d_tus, d_st, d_res))
        dst.append((host, d))
    arr, starts = pic.pack(pus, hevc.INTER_PU_DTYPE, G.PU_FIELDS)
    d_pus = torch.from_numpy(arr.view(np.uint8).copy() if len(arr) else np.zeros(20, np.uint8)).cuda()
    d_pst = torch.from_numpy(starts).cuda()
    d_sl = torch.from_numpy(pic.slice_table(hevc.INTER_SLICE_DTYPE).view(np.uint8).copy()).cuda()
    refs = upload_refs(torch, pic) if refs is None else refs
    keep += [d_pus, d_pst, d_sl, refs]
    return (pl, d_pus, d_pst, d_sl, refs), dst, keep


def compare(pic, dst, want):
    ps = 1 if pic.bd == 8 else 2
    for p, (host, d) in enumerate(dst):
        h, w = want[p].shape
        exp = host.copy()
        exp[:, :w * ps] = want[p].astype(_dt(pic.bd)).view(np.uint8).reshape(h, w * ps)
        got = d.cpu().numpy()
        bad = np.argwhere(got != exp)
        assert not len(bad), "plane %d: %d mismatches, first (row, byte) %s: got %s want %s" % (
            p, len(bad), bad[:3].tolist(), got[tuple(bad[0])], exp[tuple(bad[0])])


def run(pics, extra=0, pus=None, tus=None):
    """reconstruct the pictures (one geometry) in one call and compare every plane, padding included, with the model"""
    torch = _torch()
    P0 = pics[0]
    args, dsts, keep = [], [], []
    for i, pic in enumerate(pics):
        a, dst, k = upload(torch, pic, extra, pus[i] if pus else None, tus[i] if tus else None)
        args.append(a)
        dsts.append(dst)
        keep.append(k)
    hevc.inter_pictures(args, P0.W, P0.H, P0.log2_ctb, chroma_format_idc=P0.cfi, bit_depth=P0.bd)
    assert _lib.lib().ffhip_stream_synchronize(None) == 0, _lib.lib().ffhip_last_error()
    torch.cuda.synchronize()
    for pic, dst in zip(pics, dsts):
        compare(pic, dst, G.model(pic))


GRID = [(bd, cfi, log2_ctb) for bd in (8, 10, 12) for cfi in (0, 1, 2, 3) for log2_ctb in (4, 5, 6)]


@pytest.mark.parametrize("bd,cfi,log2_ctb", GRID)
def test_depth_format_ctb(bd, cfi, log2_ctb):
    rng = np.random.default_rng(3000 + bd * 100 + cfi * 10 + log2_ctb)
    W, H = {4: (88, 56), 5: (104, 72), 6: (200, 136)}[log2_ctb]    # not multiples of the CTB
    run([G.InterPicture(rng, W, H, log2_ctb, bd, cfi, nrefs=3, nslices=2, min_cb=3 + (log2_ctb == 6))])


SLICE_KINDS = [(["P"], False), (["P"], True), (["B"], False), (["B"], True), (["P", "B", "B", "P"], None)]


@pytest.mark.parametrize("types,weighted", SLICE_KINDS)
def test_slice_kinds(types, weighted):
    rng = np.random.default_rng(4000 + SLICE_KINDS.index((types, weighted)))
    for bd in (8, 10):
        run([G.InterPicture(rng, 160, 96, 5, bd, 1, nrefs=6, nslices=4, slice_types=types, weighted=weighted)])


def test_1080p():
    run([G.InterPicture(np.random.default_rng(5), 1920, 1080, 6, 8, 1, nrefs=4, nslices=3, p_inter=0.9, p_pcm=0.02)])


def test_sixteen_pictures_with_their_own_dpbs():
    rng = np.random.default_rng(6)
    run([G.InterPicture(rng, 96, 64, 5, 10, 1, nrefs=1 + i, nslices=1 + i % 3) for i in range(16)])


def test_seventeen_pictures_are_split():
    rng = np.random.default_rng(7)
    run([G.InterPicture(rng, 64, 48, 4, 8, 2, nrefs=1 + i % 16, nslices=2) for i in range(17)])


def test_stride_padding_survives():
    rng = np.random.default_rng(8)
    run([G.InterPicture(rng, 136, 88, 4, 8, 1)], extra=72)
    run([G.InterPicture(rng, 136, 88, 5, 12, 2)], extra=40)


def test_far_out_mvs():
    rng = np.random.default_rng(9)
    run([G.InterPicture(rng, 128, 96, 5, 8, 1, p_far=0.3, nrefs=2)])
    run([G.InterPicture(rng, 128, 96, 6, 10, 3, p_far=0.3, nrefs=2)])


def test_malformed_records_write_nothing():
    """each class of malformed record, inserted beside the real ones: the planes are those of the real records alone"""
    rng = np.random.default_rng(10)
    pic = G.InterPicture(rng, 200, 128, 5, 8, 1, nrefs=3, nslices=2, p_inter=0.6, p_pcm=0.2)
    ctb_of = lambda x, y: (y >> 5) * pic.ctb_w + (x >> 5)
    # a slice whose list 0 names a DPB slot past nrefs (the real PUs never use it)
    pic.slices.append(dict(pic.slices[0], ref=np.full((2, 16), pic.nrefs, np.int64), num_ref=[1, 1], weighted=0))
    hole = [(x, y) for y in range(0, pic.H, 8) for x in range(0, 184, 8) if (pic.kind[y >> 2, x >> 2:(x >> 2) + 2] != 1).all()]
    assert len(hole) >= 18
    bad = []
    for j, (x, y) in enumerate(hole[:18]):
        a = ctb_of(x, y)
        b = dict(x=x, y=y, w=8, h=8, flags=1, ref_idx=[0, 0], slice=int(pic.ctb_slice[a]), mv=[[5, -3], [-7, 2]], ctb=a, part="bad")
        kind = j % 9
        if kind == 0:
            b["w"] = 6                                          # not a multiple of 4
        elif kind == 1:
            b["h"] = 68                                         # out of range
        elif kind == 2:
            b["w"] = 0
        elif kind == 3:
            b["ctb"] = (a + 1) % (pic.ctb_w * pic.ctb_h)        # listed under another CTB
        elif kind == 4:
            b["flags"] = 0
        elif kind == 5:
            b["slice"] = len(pic.slices)                         # no such slice
        elif kind == 6:
            b["ref_idx"] = [pic.slices[b["slice"]]["num_ref"][0], 0]   # past the list
        elif kind == 7:
            b["slice"] = len(pic.slices) - 1                     # a DPB slot past nrefs
        else:
            b["x"], b["ctb"] = 196, ctb_of(196, y)               # inside its CTB, across the picture's right edge
        bad.append(b)
    tus = []
    for p in range(pic.nplanes):
        tl = list(pic.tus[p])
        for j, t in enumerate([t for t in tl if t["res_offset"] >= 0][:8]):
            b = dict(t)
            kind = j % 4
            if kind == 0:
                b["log2_size"] = 6
            elif kind == 1:
                b["log2_size"] = 1
            elif kind == 2:
                b["ctb"] = (t["ctb"] + 1) % (pic.ctb_w * pic.ctb_h)   # outside its CTB
            else:
                b["x"], b["y"], b["log2_size"] = (pic.W >> pic.hs[p]) - 4, 0, 3   # across the plane's right edge
                b["ctb"] = ctb_of(pic.W - 8, 0)
            tl.append(b)
        tus.append(tl)
    run([pic], pus=[pic.pus + bad], tus=[tus])


def test_chained_with_intra_pictures_on_one_stream():
    """a P picture with intra CUs: inter pictures, then intra pictures, on one stream, equal to the two models in that order"""
    import hevc_intra_picture_gen as IG
    torch = _torch()
    rng = np.random.default_rng(11)
    W, H, lc, bd, cfi = 192, 128, 5, 8, 1
    ip = IG.Picture(rng, W, H, lc, bd, cfi, p_intra=0.5)
    pic = G.InterPicture(rng, W, H, lc, bd, cfi, nrefs=3, nslices=1, slice_types=["P"], p_inter=1.0, p_pcm=0.0)
    # the inter PUs / TUs are 8 x 8 luma blocks where the intra generator left inter CUs
    pus, tus = [], [[] for _ in range(pic.nplanes)]
    res = [[] for _ in range(pic.nplanes)]
    nres = [0] * pic.nplanes
    for y in range(0, H, 8):
        for x in range(0, W, 8):
            if ip.intra[y >> 2, x >> 2]:
                continue
            a = (y >> lc) * pic.ctb_w + (x >> lc)
            pus.append(dict(x=x, y=y, w=8, h=8, flags=1, ref_idx=[int(rng.integers(0, pic.slices[0]["num_ref"][0])), 0], slice=0,
                            mv=[[int(v) for v in rng.integers(-80, 81, 2)], [0, 0]], ctb=a, part="2Nx2N"))
            for p in range(pic.nplanes):
                N = 8 >> (p > 0)
                res[p].append(rng.integers(-40, 41, N * N).astype(np.int16))
                tus[p].append(dict(x=x >> (p > 0), y=y >> (p > 0), res_offset=nres[p], log2_size=3 - (p > 0), ctb=a))
                nres[p] += N * N
    pic.pus, pic.tus = pus, tus
    pic.res = [np.concatenate(r) for r in res]
    start = [pl.copy() for pl in ip.planes]
    a, dst, keep = upload(torch, pic, planes=start)
    intra_args = []
    for p in range(ip.nplanes):
        arr, starts = ip.pack(p, dtype=hevc.INTRA_TU_DTYPE)
        d_tus = torch.from_numpy(arr.view(np.uint8).copy()).cuda()
        d_st = torch.from_numpy(starts).cuda()
        d_res = torch.from_numpy(ip.res[p].astype(np.int16)).cuda()
        keep += [d_tus, d_st, d_res]
        intra_args.append((dst[p][1], a[0][p][1], d_tus, d_st, d_res))
    hevc.inter_pictures([a], W, H, lc, chroma_format_idc=cfi, bit_depth=bd)
    hevc.intra_pictures([intra_args], W, H, lc, chroma_format_idc=cfi, bit_depth=bd)
    assert _lib.lib().ffhip_stream_synchronize(None) == 0, _lib.lib().ffhip_last_error()
    torch.cuda.synchronize()
    after_inter = G.model(pic, planes=start)
    ip.planes = after_inter
    compare(pic, dst, IG.model(ip))


@pytest.mark.parametrize("bd,cfi", [(8, 1), (10, 1), (8, 3), (12, 2)])
def test_same_planes_as_the_batch_faces(bd, cfi):
    """for MVs that keep every window inside an 80-sample edge-replicated border, the new face gives the planes of mc_batch /
    mc_w_batch + idct_batch (add only) on padded references"""
    import hevc_inter_batch_path as BP
    torch = _torch()
    rng = np.random.default_rng(5000 + bd * 10 + cfi)
    pic = G.InterPicture(rng, 256, 160, 6, bd, cfi, nrefs=4, nslices=3, p_far=0.0)
    a, dst, keep = upload(torch, pic)
    hevc.inter_pictures([a], pic.W, pic.H, pic.log2_ctb, chroma_format_idc=cfi, bit_depth=bd)
    strides = [pl[1] for pl in a[0]]
    other = [torch.from_numpy(host.copy()).cuda() for host, _ in dst]
    path = BP.BatchPath(torch, pic, strides)
    path.run(other)
    assert _lib.lib().ffhip_stream_synchronize(None) == 0, _lib.lib().ffhip_last_error()
    torch.cuda.synchronize()
    for p in range(pic.nplanes):
        assert torch.equal(dst[p][1], other[p]), "plane %d differs from the batch faces" % p
    compare(pic, dst, G.model(pic))
