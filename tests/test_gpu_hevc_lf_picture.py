"""HEVC in-loop filtering of whole pictures on the GPU (ffhip_hevc_loop_filter_pictures_dev), byte for byte against the sequential
model of hevc_lf_picture_gen.py (the oracle's per-call deblocking and SAO in the reference's order), the dst stride padding and
src included; against today's per-call path on the batch faces; and chained after the inter and intra picture faces.  Every call
is followed by ffhip_stream_synchronize(None) == 0."""
import numpy as np
import pytest

import hevc_lf_picture_gen as G
from ffmpeg_amd import _lib, hevc

pytestmark = pytest.mark.gpu

SENT = 0x5A


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _dt(bd):
    return np.uint8 if bd == 8 else np.uint16


def _plane_bytes(a, bd, stride, fill):
    h, w = a.shape
    ps = 1 if bd == 8 else 2
    host = np.full((h, stride), fill, np.uint8)
    host[:, :w * ps] = a.astype(_dt(bd)).view(np.uint8).reshape(h, w * ps)
    return host


def _stride(w, bd, extra):
    ps = 1 if bd == 8 else 2
    return (w * ps + 63) // 64 * 64 + extra


def upload_maps(torch, pic, bs=None, ctbs=None, pad=3):
    """the face's maps on the device, with strides wider than the picture"""
    bs_ver, bs_hor = (pic.bs_ver, pic.bs_hor) if bs is None else bs
    bw = bs_ver.shape[1] + pad
    bsv = np.zeros((bs_ver.shape[0], bw), np.uint8)
    bsh = np.zeros_like(bsv)
    bsv[:, :bs_ver.shape[1]], bsh[:, :bs_hor.shape[1]] = bs_ver, bs_hor
    cw = pic.nb_w + pad
    qp = np.zeros((pic.nb_h, cw), np.int8)
    qp[:, :pic.nb_w] = pic.qp
    byp = np.zeros((pic.nb_h, cw), np.uint8)
    byp[:, :pic.nb_w] = pic.bypass
    table = pic.ctb_table(hevc.LF_CTB_DTYPE) if ctbs is None else ctbs
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return dict(bs_ver=t(bsv), bs_hor=t(bsh), qp_y=t(qp), bypass=t(byp) if pic.bypass.any() else None,
                ctbs=t(table.view(np.uint8)), bs_stride=bw, cb_stride=cw, cb_qp_offset=pic.cb_qp_offset, cr_qp_offset=pic.cr_qp_offset)


def upload(torch, pic, extra=0, planes=None, **kw):
    """(the face's tuple, per plane (src tensor, src host image, dst tensor, dst host image), maps)"""
    src = pic.src if planes is None else planes
    pl, io = [], []
    for p in range(pic.nplanes):
        h, w = src[p].shape
        ss, ds = _stride(w, pic.bd, 32 + 8 * p), _stride(w, pic.bd, extra)
        sh = _plane_bytes(src[p], pic.bd, ss, 0x33)
        dh = np.full((h, ds), SENT, np.uint8)
        s, d = torch.from_numpy(sh.copy()).cuda(), torch.from_numpy(dh.copy()).cuda()
        pl.append((s, ss, d, ds))
        io.append((s, sh, d, dh))
    maps = upload_maps(torch, pic, **kw)
    return (pl, maps), io


def compare(pic, io, want):
    ps = 1 if pic.bd == 8 else 2
    for p, (s, sh, d, dh) in enumerate(io):
        assert np.array_equal(s.cpu().numpy(), sh), "plane %d: src was written" % p
        h, w = want[p].shape
        exp = dh.copy()
        exp[:, :w * ps] = want[p].astype(_dt(pic.bd)).view(np.uint8).reshape(h, w * ps)
        got = d.cpu().numpy()
        bad = np.argwhere(got != exp)
        assert not len(bad), "plane %d: %d mismatches, first (row, byte) %s: got %s want %s" % (
            p, len(bad), bad[:3].tolist(), got[tuple(bad[0])], exp[tuple(bad[0])])


def run(pics, extra=0):
    torch = _torch()
    P0 = pics[0]
    args, ios = [], []
    for pic in pics:
        a, io = upload(torch, pic, extra)
        args.append(a)
        ios.append(io)
    hevc.loop_filter_pictures(args, P0.W, P0.H, P0.log2_ctb, P0.lmc, chroma_format_idc=P0.cfi, bit_depth=P0.bd)
    assert _lib.lib().ffhip_stream_synchronize(None) == 0, _lib.lib().ffhip_last_error()
    torch.cuda.synchronize()
    for pic, io in zip(pics, ios):
        compare(pic, io, G.model(pic))


GRID = [(bd, cfi, log2_ctb) for bd in (8, 10, 12) for cfi in (0, 1, 2, 3) for log2_ctb in (4, 5, 6)]


@pytest.mark.parametrize("bd,cfi,log2_ctb", GRID)
def test_depth_format_ctb(bd, cfi, log2_ctb):
    rng = np.random.default_rng(7000 + bd * 100 + cfi * 10 + log2_ctb)
    W, H = {4: (88, 56), 5: (104, 72), 6: (208, 144)}[log2_ctb]    # not multiples of the CTB; multiples of a 16-sample min CB
    run([G.LfPicture(rng, W, H, log2_ctb, bd, cfi, tiles=(2, 2), nslices=3, log2_min_cb=3 + (log2_ctb == 6) * int(rng.integers(0, 2)))])


@pytest.mark.parametrize("kind", ["deblock", "sao"])
@pytest.mark.parametrize("bd", [8, 10])
def test_one_stage_alone(kind, bd):
    rng = np.random.default_rng(7500 + bd + (kind == "sao"))
    for cfi in (1, 3):
        run([G.LfPicture(rng, 168, 104, 5, bd, cfi, tiles=(2, 2), nslices=3, deblock=kind == "deblock", sao=kind == "sao")])


def test_1080p():
    run([G.LfPicture(np.random.default_rng(7600), 1920, 1080, 6, 8, 1, tiles=(3, 2), nslices=4)])


def test_sixteen_pictures():
    rng = np.random.default_rng(7601)
    run([G.LfPicture(rng, 96, 64, 5, 10, 1, nslices=1 + i % 3) for i in range(16)])


def test_seventeen_pictures_are_split():
    rng = np.random.default_rng(7602)
    run([G.LfPicture(rng, 64, 48, 4, 8, 2, nslices=2) for i in range(17)])


def test_stride_padding_survives_and_src_is_unchanged():
    rng = np.random.default_rng(7603)
    run([G.LfPicture(rng, 136, 88, 4, 8, 1)], extra=72)
    run([G.LfPicture(rng, 136, 88, 5, 12, 2)], extra=40)


def test_malformed_maps_give_the_defined_output():
    """bS 3..255 leave their segments unfiltered; out-of-range SAO types, classes and band positions leave the component deblocked;
    nothing outside the planes is written"""
    torch = _torch()
    rng = np.random.default_rng(7604)
    pic = G.LfPicture(rng, 136, 104, 5, 10, 1, tiles=(2, 2), nslices=3)
    bsv, bsh = pic.bs_ver.copy(), pic.bs_hor.copy()
    for m in (bsv, bsh):
        hit = rng.random(m.shape) < 0.2
        m[hit] = rng.integers(3, 256, int(hit.sum()))
    table = pic.ctb_table(hevc.LF_CTB_DTYPE)
    for i in range(len(table)):
        j = i % 4
        if j == 1:
            table[i]["sao_type"][i % 3] = 3 + i % 200
        elif j == 2:
            table[i]["sao_type"][i % 3], table[i]["sao_class"][i % 3] = 1, 32 + i % 100
        elif j == 3:
            table[i]["sao_type"][i % 3], table[i]["sao_class"][i % 3] = 2, 4 + i % 100
    a, io = upload(torch, pic, extra=24, bs=(bsv, bsh), ctbs=table)
    hevc.loop_filter_pictures([a], pic.W, pic.H, pic.log2_ctb, pic.lmc, chroma_format_idc=1, bit_depth=10)
    assert _lib.lib().ffhip_stream_synchronize(None) == 0, _lib.lib().ffhip_last_error()
    # the model of the same picture with those entries read as the face defines them
    pic.bs_ver = np.where(bsv > 2, 0, bsv).astype(np.uint8)
    pic.bs_hor = np.where(bsh > 2, 0, bsh).astype(np.uint8)
    for i, r in enumerate(pic.ctbs):
        r["sao_type"] = [int(t) if t <= 2 else 0 for t in table[i]["sao_type"]]
        r["sao_class"] = [int(c) for c in table[i]["sao_class"]]
    compare(pic, io, G.model(pic))


@pytest.mark.parametrize("bd,cfi", [(8, 1), (10, 1), (8, 3), (12, 2)])
def test_same_planes_as_the_per_call_path(bd, cfi):
    """the face equals today's per-call path: edge records -> loop_filter_batch x 2 -> copy -> sao_batch + sao_restore_batch ->
    the bypass copy-back"""
    import hevc_lf_batch_path as BP
    torch = _torch()
    rng = np.random.default_rng(7700 + bd * 10 + cfi)
    pic = G.LfPicture(rng, 200, 136, 6, bd, cfi, tiles=(2, 2), nslices=3)
    a, io = upload(torch, pic)
    hevc.loop_filter_pictures([a], pic.W, pic.H, pic.log2_ctb, pic.lmc, chroma_format_idc=cfi, bit_depth=bd)
    path = BP.BatchPath(torch, pic)
    work = path.upload(pic.src)
    path.run(work)
    assert _lib.lib().ffhip_stream_synchronize(None) == 0, _lib.lib().ffhip_last_error()
    torch.cuda.synchronize()
    other = path.planes(work)
    want = G.model(pic)
    for p in range(pic.nplanes):
        assert np.array_equal(other[p], want[p]), "plane %d: the per-call path differs from the model" % p
    compare(pic, io, want)


@pytest.mark.parametrize("bd", [8, 10])
def test_chained_after_inter_and_intra_pictures_on_one_stream(bd):
    """inter pictures -> intra pictures -> loop filter pictures on one stream, equal to the three models chained"""
    import hevc_inter_picture_gen as PG
    import hevc_intra_picture_gen as IG
    import test_gpu_hevc_inter_picture as TI
    torch = _torch()
    rng = np.random.default_rng(7800 + bd)
    W, H, lc, cfi = 192, 128, 5, 1
    ip = IG.Picture(rng, W, H, lc, bd, cfi, p_intra=0.5)
    pic = PG.InterPicture(rng, W, H, lc, bd, cfi, nrefs=3, nslices=1, slice_types=["P"], p_inter=1.0, p_pcm=0.0)
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
    a, dst, keep = TI.upload(torch, pic, planes=start)
    intra_args = []
    for p in range(ip.nplanes):
        arr, starts = ip.pack(p, dtype=hevc.INTRA_TU_DTYPE)
        d_tus = torch.from_numpy(arr.view(np.uint8).copy()).cuda()
        d_st = torch.from_numpy(starts).cuda()
        d_res = torch.from_numpy(ip.res[p].astype(np.int16)).cuda()
        keep += [d_tus, d_st, d_res]
        intra_args.append((dst[p][1], a[0][p][1], d_tus, d_st, d_res))
    lf = G.LfPicture(rng, W, H, lc, bd, cfi, tiles=(2, 1), nslices=2)
    maps = upload_maps(torch, lf)
    outs, lf_planes = [], []
    for p in range(lf.nplanes):
        h, w = lf.src[p].shape
        ds = _stride(w, bd, 16)
        dh = np.full((h, ds), SENT, np.uint8)
        d = torch.from_numpy(dh.copy()).cuda()
        outs.append((d, dh))
        lf_planes.append((dst[p][1], a[0][p][1], d, ds))
    hevc.inter_pictures([a], W, H, lc, chroma_format_idc=cfi, bit_depth=bd)
    hevc.intra_pictures([intra_args], W, H, lc, chroma_format_idc=cfi, bit_depth=bd)
    hevc.loop_filter_pictures([(lf_planes, maps)], W, H, lc, lf.lmc, chroma_format_idc=cfi, bit_depth=bd)
    assert _lib.lib().ffhip_stream_synchronize(None) == 0, _lib.lib().ffhip_last_error()
    torch.cuda.synchronize()
    ip.planes = PG.model(pic, planes=start)
    recon = IG.model(ip)
    want = G.model(lf, planes=recon)
    ps = 1 if bd == 8 else 2
    for p, (d, dh) in enumerate(outs):
        h, w = want[p].shape
        exp = dh.copy()
        exp[:, :w * ps] = want[p].astype(_dt(bd)).view(np.uint8).reshape(h, w * ps)
        assert np.array_equal(d.cpu().numpy(), exp), "plane %d differs from the chained models" % p
