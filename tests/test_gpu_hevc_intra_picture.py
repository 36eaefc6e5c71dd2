"""HEVC intra reconstruction of whole pictures on the GPU (ffhip_hevc_intra_pictures_dev), byte for byte against the sequential model
of hevc_intra_picture_gen.py.  Every case also checks that ffhip_stream_synchronize returns 0, so a lost row hand-off fails it."""
import numpy as np
import pytest

import hevc_intra_picture_gen as G
from ffmpeg_amd import _lib, hevc

pytestmark = pytest.mark.gpu

SENT = 0xA5


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def upload(torch, pics, extra=0, recs=None):
    """(the face's list of pictures, per plane (pic, p, host image, device plane, stride, h, w), tensors to keep alive)"""
    P0 = pics[0]
    ps = 1 if P0.bd == 8 else 2
    dt = np.uint8 if ps == 1 else np.uint16
    keep, args, hosts = [], [], []
    for i, pic in enumerate(pics):
        planes = []
        for p in range(pic.nplanes):
            h, w = pic.planes[p].shape
            stride = (w * ps + 63) // 64 * 64 + extra
            host = np.full((h, stride), SENT, np.uint8)
            host.view(np.uint8)[:, :w * ps] = pic.planes[p].astype(dt).view(np.uint8).reshape(h, w * ps)
            arr, starts = pic.pack(p, recs[i][p] if recs else None, dtype=hevc.INTRA_TU_DTYPE)
            d_plane = torch.from_numpy(host.copy()).cuda()
            d_tus = torch.from_numpy(arr.view(np.uint8).copy() if len(arr) else np.zeros(16, np.uint8)).cuda()
            d_st = torch.from_numpy(starts).cuda()
            d_res = torch.from_numpy(pic.res[p].astype(np.int16)).cuda()
            keep += [d_plane, d_tus, d_st, d_res]
            planes.append((d_plane, stride, d_tus, d_st, d_res))
            hosts.append((pic, p, host, d_plane, stride, h, w))
        args.append(planes)
    return args, hosts, keep


def compare(hosts, models=None):
    """every plane of upload()'s `hosts`, padding included, against the model (models: id(pic) -> planes; computed here when absent)"""
    models = {} if models is None else models
    for pic, p, host, d_plane, stride, h, w in hosts:
        ps = 1 if pic.bd == 8 else 2
        dt = np.uint8 if ps == 1 else np.uint16
        if id(pic) not in models:
            models[id(pic)] = G.model(pic)
        want = host.copy()
        want[:, :w * ps] = models[id(pic)][p].astype(dt).view(np.uint8).reshape(h, w * ps)
        got = d_plane.cpu().numpy()
        bad = np.argwhere(got != want)
        assert not len(bad), "plane %d: %d mismatches, first (row, byte) %s: got %s want %s" % (
            p, len(bad), bad[:3].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def run(pics, extra=0, recs=None, stream=None):
    """reconstruct the pictures (one geometry) in one call; compare every plane, padding included, with the model.
    extra: bytes of stride padding beyond the plane (a sentinel there must survive); recs: per picture, per plane record lists
    to send instead of the generator's (the model still uses the generator's)"""
    torch = _torch()
    P0 = pics[0]
    args, hosts, keep = upload(torch, pics, extra, recs)
    hevc.intra_pictures(args, P0.W, P0.H, P0.log2_ctb, chroma_format_idc=P0.cfi, bit_depth=P0.bd, stream=stream)
    assert _lib.lib().ffhip_stream_synchronize(stream) == 0, _lib.lib().ffhip_last_error()
    torch.cuda.synchronize()
    compare(hosts)


GRID = [(bd, cfi, log2_ctb) for bd in (8, 10, 12) for cfi in (0, 1, 2, 3) for log2_ctb in (4, 5, 6)]


@pytest.mark.parametrize("bd,cfi,log2_ctb", GRID)
def test_depth_format_ctb(bd, cfi, log2_ctb):
    rng = np.random.default_rng(1000 + bd * 100 + cfi * 10 + log2_ctb)
    W, H = {4: (88, 56), 5: (104, 72), 6: (200, 136)}[log2_ctb]    # not multiples of the CTB
    run([G.Picture(rng, W, H, log2_ctb, bd, cfi, p_intra=0.8)])


@pytest.mark.parametrize("bd", (8, 10))
def test_all_intra_1080p(bd):
    run([G.Picture(np.random.default_rng(bd), 1920, 1080, 6, bd, 1, p_intra=1.0)])


def test_half_inter_constrained_intra_pred():
    rng = np.random.default_rng(7)
    run([G.Picture(rng, 256, 192, 5, 8, 1, p_intra=0.5, cip=True)])
    run([G.Picture(rng, 256, 192, 4, 10, 2, p_intra=0.5, cip=True)])


def test_slices_and_tiles():
    rng = np.random.default_rng(8)
    run([G.Picture(rng, 320, 200, 5, 8, 1, p_intra=0.8, tiles=(3, 2), slices=5)])
    run([G.Picture(rng, 192, 136, 4, 12, 3, p_intra=0.9, tiles=(2, 3), slices=7, cip=True)])


def test_five_pictures_in_one_call():
    rng = np.random.default_rng(9)
    run([G.Picture(rng, 160, 96, 5, 10, 1, p_intra=p, tiles=(1 + i % 2, 1), slices=1 + i, cip=i % 2 == 1)
         for i, p in enumerate((1.0, 0.7, 0.5, 0.9, 0.3))])


def test_wide_strides_keep_their_padding():
    rng = np.random.default_rng(10)
    run([G.Picture(rng, 136, 88, 4, 8, 1)], extra=72)
    run([G.Picture(rng, 136, 88, 5, 12, 2)], extra=40)


def test_malformed_records_write_nothing():
    rng = np.random.default_rng(11)
    pic = G.Picture(rng, 192, 128, 5, 8, 1, p_intra=0.8)
    recs = []
    for p in range(pic.nplanes):
        rl = list(pic.recs[p])
        good = [r for r in rl if r["log2_size"] <= 3]
        for j, r in enumerate(good[:: max(1, len(good) // 6)][:6]):
            b = dict(r)
            kind = j % 6
            if kind == 0:
                b["mode"] = 35
            elif kind == 1:
                b["log2_size"] = 6
            elif kind == 2:
                b["log2_size"] = 1
            elif kind == 3:
                b["x"] = r["x"] + (32 >> (1 if p else 0))       # outside the CTB it is listed under
            elif kind == 4:
                b["c_idx_unit"] = (r["c_idx_unit"] & 3)             # 1-sample units: more than 16 per side at 16x16 and up
                b["log2_size"] = 4
            else:
                b["x"] = r["x"] + 2                                 # off the 4-sample grid
            b["res_offset"] = 0
            rl.insert(rl.index(r), b)                               # ahead of a real block of the same CTB
        recs.append(rl)
    run([pic], recs=[recs])
