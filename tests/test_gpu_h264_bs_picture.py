"""H.264 deblocking edge parameters of whole pictures on the GPU (ffhip_h264_edge_params_pictures_dev), byte for byte against the
device-free host face and model A of h264_bs_picture_gen.py on the picture set of the CPU tier, guard records included; and chained
into ffhip_h264_deblock_frames_dev and ffhip_h264_deblock_frames_chroma_dev (10 bits: ffhip_h264_deblock_frames_dev_hbd) on one stream
with no host synchronisation in between, against the oracle's serial filter run on model A's tables."""
import copy
import ctypes as C

import numpy as np
import pytest

import ffi
import h264_bs_picture_gen as G
from ffmpeg_amd import _lib, h264

pytestmark = pytest.mark.gpu

TABLES = ("luma", "cb", "cr")
INPUTS = ("mb", "mvf", "slices", "chroma_qp")


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def upload(torch, pic, pad=0):
    """(the face's dict of device tensors, the host dict of the same picture): the tables sit behind one guard record"""
    m = pic.maps(pad=pad)
    d = dict(m)
    for k in INPUTS:
        d[k] = _dev(torch, m[k]) if m[k] is not None else None
    for k in TABLES:
        if k in m:
            d["_" + k] = _dev(torch, m["_" + k])
            d[k] = d["_" + k][12:]
    d["_in"] = {k: d[k].clone() for k in INPUTS if d[k] is not None}
    return d, m


def compare(pics, up, wants=None):
    """the device tables of upload()'s (d, m) pairs against the host face and model A, guard records included; the inputs unchanged"""
    import torch
    P0 = pics[0]
    h264.edge_params_pictures_host([m for _, m in up], P0.mb_w, P0.mb_h, P0.field, P0.bd_off)
    for k, (pic, (d, m)) in enumerate(zip(pics, up)):
        a = wants[k] if wants is not None else G.model_a_of(pic)
        assert ("cb" in a) == ("cb" in m)
        for t in TABLES:
            if t not in a:
                continue
            exp = np.zeros(len(a[t]) + 2, h264.EDGE_DTYPE)
            exp.view(np.uint8)[:] = G.GUARD
            exp[1:-1] = a[t]
            assert np.array_equal(m["_" + t], exp), "picture %d %s: the host face differs from model A" % (k, t)
            got = d["_" + t].cpu().numpy().view(h264.EDGE_DTYPE)
            bad = np.nonzero(got != exp)[0]
            assert not len(bad), "picture %d %s: %d records differ, first %s: got %s want %s" % (
                k, t, len(bad), (bad[:3] - 1).tolist(), got[bad[0]], exp[bad[0]])
        for key, before in d["_in"].items():
            assert torch.equal(d[key], before), "picture %d: %s was written" % (k, key)


def run(pics, pad=0, stream=None, wants=None):
    torch = _torch()
    P0 = pics[0]
    up = [upload(torch, p, pad) for p in pics]
    h264.edge_params_pictures([d for d, _ in up], P0.mb_w, P0.mb_h, P0.field, P0.bd_off, stream=stream)
    assert _lib.lib().ffhip_stream_synchronize(stream) == 0, _lib.lib().ffhip_last_error()
    torch.cuda.synchronize()
    compare(pics, up, wants)


@pytest.mark.parametrize("i", range(len(G.SET)))
def test_picture_set(i):
    """the CPU tier's set, one call per entry: 1 x 1, 5 x 3 and 9 x 7 macroblocks (tiles ragged on both axes), 17 pictures of 6 x 5 in one
    call (two launches), frame and field, with and without chroma tables, an mvf stride wider than the picture"""
    run(G.picture_set(i), pad=G.set_pad(i))


def test_120x68():
    run([G.BsPicture(np.random.default_rng(9420), 120, 68, 0, 0, 4)], pad=0)


def test_240x135_field_10_bits():
    run([G.BsPicture(np.random.default_rng(9421), 240, 135, 1, 12, 6)], pad=4)


@pytest.mark.parametrize("field", [0, 1])
def test_malformed_maps_give_the_defined_output(field):
    pic = G.malformed(np.random.default_rng(9410 + field), field=field)
    run([pic], pad=2, wants=[G.model_a(pic)])


class Face:
    """the face alone, with the steps tests/picture_faces.py gives its adapters: build / upload / call(stream) / inputs / outputs /
    compare(view)"""
    name, codec, pad = "h264_edge_params", "h264", 3

    def build(self, seed):
        self.pic = G.BsPicture(np.random.default_rng(seed), 9, 7, 0, 0, 4)
        self.want = G.model_a(self.pic)
        return self

    def fresh(self):
        return copy.copy(self)

    def upload(self, torch):
        self.d, self.m = upload(torch, self.pic, self.pad)

    def call(self, stream):
        p = self.pic
        h264.edge_params_pictures([self.d], p.mb_w, p.mb_h, p.field, p.bd_off, stream=stream)

    def inputs(self):
        return [self.d[k] for k in INPUTS]

    def outputs(self):
        return [self.d["_" + k] for k in TABLES]

    def compare(self, view=lambda t: t):
        d = dict(self.d)
        for k in TABLES:
            d["_" + k] = view(self.d["_" + k])
        compare([self.pic], [(d, self.m)], [self.want])


class Chain:
    """_dev -> ffhip_h264_deblock_frames_dev -> ffhip_h264_deblock_frames_chroma_dev (Cb, Cr) with no synchronisation between them
    (bit_depth 10: ffhip_h264_deblock_frames_dev_hbd three times): the planes equal the oracle's serial filter run on model A's
    tables.  upload / call(stream) / compare, inputs() / outputs() as tests/picture_faces.py has them."""
    mb_w, mb_h = 9, 7

    def __init__(self, bit_depth=8):
        self.bd = bit_depth
        self.name = "h264_edge_params+deblock_%d" % bit_depth

    def build(self, seed=9430):
        rng = np.random.default_rng(seed + self.bd)
        bd_off = 6 * (self.bd - 8)
        self.pic = G.BsPicture(rng, self.mb_w, self.mb_h, 0, bd_off, 3)
        self.pic.slices["idc"] = [0, 2, 0]
        self.want = G.model_a(self.pic)
        assert all((self.want[t]["alpha"] > 0).sum() > 20 for t in TABLES)
        dt, sh = (np.uint8, 0) if self.bd == 8 else (np.uint16, self.bd - 8)
        H, W = 16 * self.mb_h, 16 * self.mb_w
        self.src = [(rng.integers(122, 134, (h, w)) << sh).astype(dt) for h, w in ((H, W), (H // 2, W // 2), (H // 2, W // 2))]
        O = ffi.oracle()
        u8p = C.POINTER(C.c_uint8)
        O.ffo_h264_deblock_frame_bd.argtypes = [C.c_int, C.c_int, u8p, C.c_ssize_t, C.c_int, C.c_int, C.c_void_p]
        self.filtered = [s.copy() for s in self.src]
        for p, (pl, t) in enumerate(zip(self.filtered, TABLES)):
            e = C.c_void_p(np.ascontiguousarray(self.want[t]).ctypes.data)
            at = C.cast(pl.ctypes.data, u8p)
            if self.bd > 8:
                O.ffo_h264_deblock_frame_bd(self.bd, int(p > 0), at, pl.strides[0], self.mb_w, self.mb_h, e)
            elif p:
                O.ffo_h264_deblock_frame_chroma(at, pl.strides[0], self.mb_w, self.mb_h, e)
            else:
                O.ffo_h264_deblock_frame(at, pl.strides[0], self.mb_w, self.mb_h, e)
        return self

    def fresh(self):
        return copy.copy(self)

    def upload(self, torch):
        if not hasattr(self, "pic"):
            self.build()
        m = self.pic.maps()
        self.d = {k: _dev(torch, m[k]) for k in INPUTS}
        n = self.mb_w * self.mb_h
        for t, per in (("luma", 8), ("cb", 4), ("cr", 4)):       # tables of their own allocations: 16-byte aligned, as the 16-bit filter asks
            self.d[t] = torch.full((n * per * 12,), 0xEE, dtype=torch.uint8, device="cuda")
        self.d["mvf_stride"], self.d["nslices"] = m["mvf_stride"], m["nslices"]
        self.planes = [_dev(torch, s) for s in self.src]

    def call(self, stream):
        p = self.pic
        h264.edge_params_pictures([self.d], p.mb_w, p.mb_h, 0, p.bd_off, stream=stream)
        for i, (pl, t) in enumerate(zip(self.planes, TABLES)):
            h, stride = self.src[i].shape[0], self.src[i].strides[0]
            if self.bd > 8:
                h264.deblock_frames_hbd(self.bd, pl, h * stride, 1, stride, p.mb_w, p.mb_h, self.d[t], chroma=i > 0, stream=stream)
            elif i:
                h264.deblock_frames_chroma(pl, h * stride, 1, stride, p.mb_w, p.mb_h, self.d[t], stream=stream)
            else:
                h264.deblock_frames(pl, h * stride, 1, stride, p.mb_w, p.mb_h, self.d[t], stream=stream)

    def inputs(self):
        return [self.d[k] for k in INPUTS]

    def outputs(self):
        return [self.d[t] for t in TABLES] + list(self.planes)

    def compare(self, view=lambda t: t):
        for t in TABLES:
            got = view(self.d[t]).cpu().numpy().view(h264.EDGE_DTYPE)
            assert np.array_equal(got, self.want[t]), "%s: the %s table differs from model A" % (self.name, t)
        for i, (pl, want, src) in enumerate(zip(self.planes, self.filtered, self.src)):
            got = view(pl).cpu().numpy().view(src.dtype).reshape(src.shape)
            assert np.array_equal(got, want), "%s: plane %d: %d samples differ from the oracle" % (self.name, i, (got != want).sum())
            assert (want != src).sum() > 20, "%s: plane %d: the filter changed next to nothing" % (self.name, i)


@pytest.mark.parametrize("bit_depth", [8, 10])
def test_chained_into_the_deblock_faces_on_one_stream(bit_depth):
    """Chain on the NULL stream (tests/test_gpu_h264_bs_picture_streams.py runs it on a created one)"""
    torch = _torch()
    chain = Chain(bit_depth).build()
    chain.upload(torch)
    torch.cuda.synchronize()
    chain.call(None)
    assert _lib.lib().ffhip_stream_synchronize(None) == 0, _lib.lib().ffhip_last_error()
    torch.cuda.synchronize()
    chain.compare()
