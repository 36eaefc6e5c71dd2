"""HEVC deblocking boundary strengths of whole pictures on the GPU (ffhip_hevc_boundary_strengths_pictures_dev), byte for byte
against the device-free host face and model A of hevc_bs_picture_gen.py on the picture set of the CPU tier, guard bytes included;
and chained into ffhip_hevc_loop_filter_pictures_dev on one stream with no host synchronisation in between."""
import numpy as np
import pytest

import hevc_bs_picture_gen as G
from ffmpeg_amd import _lib, hevc

pytestmark = pytest.mark.gpu

GUARD = 0x5A


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def upload(torch, pic, pad=0):
    """(the face's dict of device tensors, the host dict of the same picture)"""
    m = pic.maps(pad=pad, guard=GUARD)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    d = dict(m)
    for k in ("mvf", "tu", "ctb_slice", "slices"):
        d[k] = t(m[k])
    d["ctb_tile"] = t(m["ctb_tile"]) if m["ctb_tile"] is not None else None
    d["_ver"], d["_hor"] = t(m["_ver"]), t(m["_hor"])
    row = pic.w4 + pad
    d["bs_ver"], d["bs_hor"] = d["_ver"][row:], d["_hor"][row:]           # behind the guard row
    d["_in"] = {k: d[k].clone() for k in ("mvf", "tu", "ctb_slice", "slices")}
    return d, m


def compare(pics, up):
    """the device maps of upload()'s (d, m) pairs against the host face and model A, guard bytes included; the inputs unchanged"""
    import torch
    P0 = pics[0]
    hevc.boundary_strengths_pictures_host([m for _, m in up], P0.W, P0.H, P0.log2_ctb)
    for k, (pic, (d, m)) in enumerate(zip(pics, up)):
        av, ah, _, _ = G.model_a_of(pic)
        for name, dev, host, want in (("bs_ver", d["_ver"], m["_ver"], av), ("bs_hor", d["_hor"], m["_hor"], ah)):
            exp = np.full_like(host, GUARD)
            exp[1:-1, :pic.w4] = want
            assert np.array_equal(host, exp), "picture %d %s: the host face differs from model A" % (k, name)
            got = dev.cpu().numpy().reshape(host.shape)
            bad = np.argwhere(got != exp)
            assert not len(bad), "picture %d %s: %d mismatches, first (row, col) %s: got %s want %s" % (
                k, name, len(bad), (bad[:3] - [1, 0]).tolist(), got[tuple(bad[0])], exp[tuple(bad[0])])
        for key, before in d["_in"].items():
            assert torch.equal(d[key], before), "picture %d: %s was written" % (k, key)


def run(pics, pad=0, stream=None):
    torch = _torch()
    P0 = pics[0]
    up = [upload(torch, p, pad) for p in pics]
    hevc.boundary_strengths_pictures([d for d, _ in up], P0.W, P0.H, P0.log2_ctb, stream=stream)
    assert _lib.lib().ffhip_stream_synchronize(stream) == 0, _lib.lib().ffhip_last_error()
    torch.cuda.synchronize()
    compare(pics, up)


@pytest.mark.parametrize("i", range(len(G.SET)))
def test_picture_set(i):
    """the CPU tier's set, one call per entry: 17 pictures in one call (two launches), three CTB sizes, strides wider than the
    picture (maps that are not dword aligned) and equal to it"""
    run(G.picture_set(i), pad=(0, 3, 5)[i % 3])


def test_2160p():
    run([G.BsPicture(np.random.default_rng(9300), 3840, 2160, 6, tiles=(3, 2), nslices=4)], pad=0)


def test_2160p_small_ctbs_unaligned_maps():
    run([G.BsPicture(np.random.default_rng(9301), 3840, 2160, 4, tiles=(2, 3), nslices=3)], pad=1)


def test_seventeen_pictures_are_split():
    rng = np.random.default_rng(9302)
    run([G.BsPicture(rng, 200, 136, 5, tiles=(2, 2), nslices=1 + k % 4) for k in range(17)], pad=2)


def test_malformed_maps_give_the_defined_output():
    """slice indices out of range, ref_idx out of range, pred_flag above 3: the device equals the host face and model A"""
    rng = np.random.default_rng(9303)
    pic = G.BsPicture(rng, 264, 200, 5, tiles=(2, 2), nslices=3)
    pic.ctb_slice[rng.random(pic.ctb_slice.shape) < 0.2] = 7
    hit = rng.random(pic.mvf.shape) < 0.1
    pic.mvf["ref_idx"][hit] = rng.integers(-128, 128, (int(hit.sum()), 2))
    hit = rng.random(pic.mvf.shape) < 0.05
    pic.mvf["pred_flag"][hit] = rng.integers(4, 256, int(hit.sum()))
    pic.slices[1]["num_ref"][0] = 17
    run([pic], pad=3)


class Chain:
    """_dev -> ffhip_hevc_loop_filter_pictures_dev with no synchronisation between them: the planes equal the planes filtered from
    model A's maps uploaded from the host.  upload / call(stream) / compare, inputs() / outputs() as tests/picture_faces.py has them."""
    name = "hevc_boundary_strengths+loop_filter"
    W, H, lc, bd, cfi = 264, 200, 5, 8, 1

    def upload(self, torch):
        import hevc_lf_picture_gen as LG
        import test_gpu_hevc_lf_picture as TL
        rng = np.random.default_rng(9304)
        self.bpic = G.BsPicture(rng, self.W, self.H, self.lc, tiles=(2, 2), nslices=3)
        self.lf = lf = LG.LfPicture(rng, self.W, self.H, self.lc, self.bd, self.cfi, tiles=(2, 2), nslices=3)
        self.av, self.ah, _, _ = av, ah, _, _ = G.model_a_of(self.bpic)
        assert {1, 2} <= set(av.ravel().tolist()) and {1, 2} <= set(ah.ravel().tolist())
        # a: the maps made on the device, into the tensors the filter reads
        (self.planes_a, self.maps_a), self.io_a = TL.upload(torch, lf, bs=(np.full_like(av, 0xEE), np.full_like(ah, 0xEE)))
        self.d, _ = upload(torch, self.bpic)
        self.d["bs_ver"], self.d["bs_hor"], self.d["bs_stride"] = self.maps_a["bs_ver"], self.maps_a["bs_hor"], self.maps_a["bs_stride"]
        # b: model A's maps uploaded from the host
        (self.planes_b, self.maps_b), self.io_b = TL.upload(torch, lf, bs=(av, ah))

    def call(self, stream):
        lf, kw = self.lf, dict(chroma_format_idc=self.cfi, bit_depth=self.bd, stream=stream)
        hevc.boundary_strengths_pictures([self.d], self.W, self.H, self.lc, stream=stream)
        hevc.loop_filter_pictures([(self.planes_a, self.maps_a)], self.W, self.H, self.lc, lf.lmc, **kw)
        hevc.loop_filter_pictures([(self.planes_b, self.maps_b)], self.W, self.H, self.lc, lf.lmc, **kw)

    def inputs(self):
        ins = [self.d[k] for k in ("mvf", "tu", "ctb_slice", "slices", "ctb_tile") if self.d[k] is not None]
        ins += [t for k, t in self.maps_a.items() if hasattr(t, "is_cuda") and k not in ("bs_ver", "bs_hor")]
        return ins + [t for t in self.maps_b.values() if hasattr(t, "is_cuda")] + [s for io in (self.io_a, self.io_b) for s, _, _, _ in io]

    def outputs(self):
        return [self.maps_a["bs_ver"], self.maps_a["bs_hor"]] + [d for io in (self.io_a, self.io_b) for _, _, d, _ in io]

    def compare(self, view=lambda t: t):
        import hevc_lf_picture_gen as LG
        import test_gpu_hevc_lf_picture as TL
        lf = self.lf
        lf.bs_ver, lf.bs_hor = self.av, self.ah
        want = LG.model(lf)
        TL.compare(lf, [(s, sh, view(d), dh) for s, sh, d, dh in self.io_b], want)
        TL.compare(lf, [(s, sh, view(d), dh) for s, sh, d, dh in self.io_a], want)
        assert any((w != s).any() for w, s in zip(want, lf.src))


def test_chained_into_the_loop_filter_on_one_stream():
    """Chain on the NULL stream (tests/test_gpu_picture_streams.py runs it on a created one)"""
    torch = _torch()
    chain = Chain()
    chain.upload(torch)
    torch.cuda.synchronize()
    chain.call(None)
    assert _lib.lib().ffhip_stream_synchronize(None) == 0, _lib.lib().ffhip_last_error()
    torch.cuda.synchronize()
    chain.compare()
