"""The H.264 edge-parameter face with a chroma format (ffhip_h264_edge_params_pictures_fmt_dev) and the frame-order filter of whole
pictures (ffhip_h264_deblock_pictures_fmt_dev) on the GPU, at chroma_format_idc 0 .. 3:
 * the device tables byte for byte against the host face and model A of h264_bs_fmt_gen.py, guard records included, inputs unchanged;
 * edge parameters -> filter on one stream with no host synchronisation, against the oracle's serial filters run on model A's tables
   (at 4:2:0 against the existing frame faces as well);
 * the whole P / B chain inter -> residual -> edge parameters -> filter from one mb / mvf pair, against the host faces followed by the
   oracle's filters;
 * both on a created stream and behind a busy NULL stream with the staged runs of tests/picture_faces.py."""
import copy
import ctypes as C

import numpy as np
import pytest

import ffi
import h264_bs_fmt_gen as F
import h264_fmt_picture_gen as FP
import h264_inter_picture_gen as GI
import h264_res_picture_gen as GR
import picture_faces as PF
from ffmpeg_amd import _lib, h264

pytestmark = pytest.mark.gpu

TABLES = ("luma", "cb", "cr")
INPUTS = ("mb", "mvf", "slices", "chroma_qp")
E = h264.EDGE_DTYPE


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _oracle():
    O = ffi.oracle()
    O.ffo_h264_deblock_frame_bd.argtypes = [C.c_int, C.c_int, ffi.u8p, C.c_ssize_t, C.c_int, C.c_int, C.c_void_p]
    O.ffo_h264_deblock_frame_bd.restype = None
    O.ffo_h264_deblock_frame_c422_bd.argtypes = [C.c_int, ffi.u8p, C.c_ssize_t, C.c_int, C.c_int, C.c_void_p]
    O.ffo_h264_deblock_frame_c422_bd.restype = None
    return O


def oracle_filter(fmt, bd, planes, tables, mb_w, mb_h):
    """the oracle's serial frame filters, in place on the numpy planes: plane 0 and every plane of 4:4:4 by the luma filter, Cb / Cr of
    4:2:0 by the chroma one, of 4:2:2 by ffo_h264_deblock_frame_c422_bd"""
    O = _oracle()
    for p, (pl, t) in enumerate(zip(planes, TABLES)):
        if p and fmt == 0:
            break
        e = np.ascontiguousarray(tables[t])
        at, s, ev = C.cast(pl.ctypes.data, ffi.u8p), pl.strides[0], C.c_void_p(e.ctypes.data)
        if p and fmt == 2:
            O.ffo_h264_deblock_frame_c422_bd(bd, at, s, mb_w, mb_h, ev)
        elif bd > 8:
            O.ffo_h264_deblock_frame_bd(bd, int(p > 0 and fmt == 1), at, s, mb_w, mb_h, ev)
        elif p and fmt == 1:
            O.ffo_h264_deblock_frame_chroma(at, s, mb_w, mb_h, ev)
        else:
            O.ffo_h264_deblock_frame(at, s, mb_w, mb_h, ev)


# ------------------------------------------------------------------------------------------------ the tables: device == host == A
def upload(torch, pic, pad=0):
    """(the face's dict of device tensors, the host dict of the same picture): each table sits behind one guard record"""
    m = pic.maps(pad=pad)
    d = dict(m)
    for k in INPUTS:
        d[k] = _dev(torch, m[k])
    for k in TABLES:
        d["_" + k] = _dev(torch, m["_" + k])
        d[k] = d["_" + k][12:]
    d["_in"] = {k: d[k].clone() for k in INPUTS}
    return d, m


def compare(pics, up, wants=None, view=lambda t: t):
    """the device tables of upload()'s (d, m) pairs against the host face and model A, guard records included (format 0: cb / cr are
    guard bytes throughout); the inputs unchanged"""
    import torch
    P0 = pics[0]
    h264.edge_params_pictures_fmt_host([m for _, m in up], P0.mb_w, P0.mb_h, P0.field, P0.bd_off, P0.fmt)
    for k, (pic, (d, m)) in enumerate(zip(pics, up)):
        a = wants[k] if wants is not None else F.model_a_of(pic)
        for t in TABLES:
            exp = np.zeros(len(m["_" + t]), E)
            exp.view(np.uint8)[:] = F.GUARD
            if t in a:
                assert len(a[t]) == len(exp) - 2
                exp[1:-1] = a[t]
            assert np.array_equal(m["_" + t], exp), "picture %d %s: the host face differs from model A" % (k, t)
            got = view(d["_" + t]).cpu().numpy().view(E)
            bad = np.nonzero(got != exp)[0]
            assert not len(bad), "picture %d %s: %d records differ, first %s: got %s want %s" % (
                k, t, len(bad), (bad[:3] - 1).tolist(), got[bad[0]], exp[bad[0]])
        for key, before in d["_in"].items():
            assert torch.equal(d[key], before), "picture %d: %s was written" % (k, key)


def run(pics, pad=0, stream=None, wants=None):
    torch = _torch()
    P0 = pics[0]
    up = [upload(torch, p, pad) for p in pics]
    torch.cuda.synchronize()
    h264.edge_params_pictures_fmt([d for d, _ in up], P0.mb_w, P0.mb_h, P0.field, P0.bd_off, P0.fmt, stream=stream)
    assert _lib.lib().ffhip_stream_synchronize(stream) == 0, _lib.lib().ffhip_last_error()
    torch.cuda.synchronize()
    compare(pics, up, wants)


@pytest.mark.parametrize("i", range(len(F.SET)))
def test_picture_set(i):
    """the CPU tier's set, one call per entry and format: 1 x 1, 5 x 3 and 9 x 7 macroblocks (tiles ragged on both axes), 17 pictures of
    6 x 5 in one call (two launches), frame and field, qp_bd_offset 0 and 12, an mvf stride wider than the picture"""
    run(F.picture_set(i), pad=F.set_pad(i))


@pytest.mark.parametrize("fmt", [2, 3])
@pytest.mark.parametrize("field", [0, 1])
def test_malformed_maps_give_the_defined_output(fmt, field):
    pic = F.malformed(np.random.default_rng(9710 + field), fmt, field=field)
    run([pic], pad=2, wants=[F.model_a(pic)])


def test_formats_0_and_1_give_the_existing_face():
    """the same device tensors through ffhip_h264_edge_params_pictures_dev: equal bytes (format 0: with NULL chroma tables)"""
    torch = _torch()
    for fmt in (0, 1):
        pic = F.FmtPicture(np.random.default_rng(9720 + fmt), fmt, 9, 7, 0, 0, 3)
        (a, _), (b, _) = upload(torch, pic, 1), upload(torch, pic, 1)
        old = dict(b)
        if fmt == 0:
            old["chroma_qp"] = old["cb"] = old["cr"] = None
        torch.cuda.synchronize()
        h264.edge_params_pictures_fmt([a], 9, 7, 0, 0, fmt)
        h264.edge_params_pictures([old], 9, 7, 0, 0)
        assert _lib.lib().ffhip_stream_synchronize(None) == 0, _lib.lib().ffhip_last_error()
        torch.cuda.synchronize()
        for t in TABLES:
            assert torch.equal(a["_" + t], b["_" + t]), (fmt, t)


class Face:
    """the edge-parameter face alone at a format, with the steps tests/picture_faces.py gives its adapters"""
    codec, pad = "h264", 3

    def __init__(self, fmt):
        self.fmt = fmt
        self.name = "h264_edge_params_fmt%d" % fmt

    def build(self, seed):
        self.pic = F.FmtPicture(np.random.default_rng(seed + self.fmt), self.fmt, 9, 7, 0, 0, 4)
        self.want = F.model_a(self.pic)
        return self

    def fresh(self):
        return copy.copy(self)

    def upload(self, torch):
        self.d, self.m = upload(torch, self.pic, self.pad)

    def call(self, stream):
        p = self.pic
        h264.edge_params_pictures_fmt([self.d], p.mb_w, p.mb_h, p.field, p.bd_off, p.fmt, stream=stream)

    def inputs(self):
        return [self.d[k] for k in INPUTS]

    def outputs(self):
        return [self.d["_" + k] for k in TABLES]

    def compare(self, view=lambda t: t):
        compare([self.pic], [(self.d, self.m)], [self.want], view)


# --------------------------------------------------------------------------------------------------- edge parameters -> filter
def plane_shapes(fmt, mb_w, mb_h):
    return [(16 * mb_h, 16 * mb_w)] + ([FP.chroma_shape(fmt, mb_w, mb_h)] * 2 if fmt else [])


class Chain:
    """edge_params_pictures_fmt -> deblock_pictures_fmt on one stream with no synchronisation in between, npics pictures to a call: the
    tables equal model A's and the planes the oracle's serial filters run on model A's tables.  shift: the planes start that many
    bytes into their (256-byte aligned) tensors."""
    mb_w, mb_h = 9, 7

    def __init__(self, fmt, bd=8, npics=1, shift=0):
        self.fmt, self.bd, self.npics, self.shift = fmt, bd, npics, shift
        self.name = "h264_edge_params+deblock_fmt%d_%d_x%d" % (fmt, bd, npics)

    def build(self, seed=9730):
        fmt, bd, mb_w, mb_h = self.fmt, self.bd, self.mb_w, self.mb_h
        rng = np.random.default_rng(seed + 16 * fmt + bd)
        dt, sh = (np.uint8, 0) if bd == 8 else (np.uint16, bd - 8)
        self.pics, self.wants, self.src, self.filtered = [], [], [], []
        for _ in range(self.npics):
            pic = F.FmtPicture(rng, fmt, mb_w, mb_h, 0, 6 * sh, 3)
            pic.slices["idc"] = [0, 2, 0]
            want = F.model_a(pic)
            src = [(rng.integers(122, 134, s) << sh).astype(dt) for s in plane_shapes(fmt, mb_w, mb_h)]
            out = [s.copy() for s in src]
            oracle_filter(fmt, bd, out, want, mb_w, mb_h)
            assert all((o != s).sum() > 20 for o, s in zip(out, src)), "%s: the filter changed next to nothing" % self.name
            self.pics.append(pic), self.wants.append(want), self.src.append(src), self.filtered.append(out)
        return self

    def fresh(self):
        return copy.copy(self)

    def upload(self, torch):
        if not hasattr(self, "pics"):
            self.build()
        n = self.mb_w * self.mb_h
        self.d, self.planes, self.bufs = [], [], []
        for pic, src in zip(self.pics, self.src):
            m = pic.maps()
            d = {k: _dev(torch, m[k]) for k in INPUTS}
            for t, per in (("luma", 8), ("cb", F.PER[self.fmt]), ("cr", F.PER[self.fmt])):   # tensors of their own: 16-byte aligned
                d[t] = torch.full((n * per * 12,), 0xEE, dtype=torch.uint8, device="cuda")
            d["mvf_stride"], d["nslices"] = m["mvf_stride"], m["nslices"]
            self.d.append(d)
            bufs = [torch.cat([torch.full((self.shift,), 0x11, dtype=torch.uint8, device="cuda"), _dev(torch, s)]) for s in src]
            self.bufs.append(bufs)
            self.planes.append([b[self.shift:] for b in bufs])

    def strides(self):
        s = [a.strides[0] for a in self.src[0]]
        return s[0], (s[1] if len(s) > 1 else 0)

    def call(self, stream):
        p = self.pics[0]
        h264.edge_params_pictures_fmt(self.d, p.mb_w, p.mb_h, 0, p.bd_off, self.fmt, stream=stream)
        sy, sc = self.strides()
        lf = [dict(planes=pl, edges=[d[t] for t in TABLES[:len(pl)]]) for pl, d in zip(self.planes, self.d)]
        h264.deblock_pictures_fmt(lf, p.mb_w, p.mb_h, sy, sc, self.bd, self.fmt, stream=stream)

    def inputs(self):
        return [d[k] for d in self.d for k in INPUTS]

    def outputs(self):
        return [d[t] for d in self.d for t in TABLES] + [b for bufs in self.bufs for b in bufs]

    def compare(self, view=lambda t: t):
        for k, (d, want, bufs, filtered, src) in enumerate(zip(self.d, self.wants, self.bufs, self.filtered, self.src)):
            for t in TABLES:
                got = view(d[t]).cpu().numpy().view(E)
                if t in want:
                    assert np.array_equal(got, want[t]), "%s: picture %d: the %s table differs from model A" % (self.name, k, t)
                else:
                    assert (got.view(np.uint8) == 0xEE).all(), "%s: picture %d: %s written at format 0" % (self.name, k, t)
            for i, (b, w) in enumerate(zip(bufs, filtered)):
                raw = view(b).cpu().numpy()
                assert (raw[:self.shift] == 0x11).all()
                got = raw[self.shift:].view(w.dtype).reshape(w.shape)
                assert np.array_equal(got, w), "%s: picture %d plane %d: %d samples differ from the oracle" % (self.name, k, i, (got != w).sum())


def run_chain(chain):
    torch = _torch()
    chain.upload(torch)
    torch.cuda.synchronize()
    chain.call(None)
    assert _lib.lib().ffhip_stream_synchronize(None) == 0, _lib.lib().ffhip_last_error()
    torch.cuda.synchronize()
    chain.compare()
    return chain


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("fmt", range(4))
def test_chained_into_the_deblock_face_on_one_stream(fmt, bd):
    """on the NULL stream, one picture to a call (4:2:2: three); at 4:2:0 the existing frame faces give the same planes from the same
    device tables"""
    torch = _torch()
    ch = run_chain(Chain(fmt, bd, 3 if fmt == 2 else 1).build())
    if fmt != 1:
        return
    p, d = ch.pics[0], ch.d[0]
    planes = [_dev(torch, s) for s in ch.src[0]]
    torch.cuda.synchronize()
    for i, (pl, t) in enumerate(zip(planes, TABLES)):
        h, s = ch.src[0][i].shape[0], ch.src[0][i].strides[0]
        if bd > 8:
            h264.deblock_frames_hbd(bd, pl, h * s, 1, s, p.mb_w, p.mb_h, d[t], chroma=i > 0)
        elif i:
            h264.deblock_frames_chroma(pl, h * s, 1, s, p.mb_w, p.mb_h, d[t])
        else:
            h264.deblock_frames(pl, h * s, 1, s, p.mb_w, p.mb_h, d[t])
    assert _lib.lib().ffhip_stream_synchronize(None) == 0, _lib.lib().ffhip_last_error()
    torch.cuda.synchronize()
    for a, b in zip(planes, ch.planes[0]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("fmt", [1, 3])
def test_planes_that_are_only_4_byte_aligned(fmt):
    """8 bits: planes 4 bytes into their tensors take the launchers' plane-by-plane paths; the same bytes"""
    run_chain(Chain(fmt, 8, 2, shift=4).build())


# ----------------------------------------------------------------------------------------------------------- the whole chain
class WholeChain:
    """inter_pictures_fmt -> residual_pictures_fmt -> edge_params_pictures_fmt -> deblock_pictures_fmt on one stream from one upload of
    mb / mvf, at 5 x 3 macroblocks: the planes equal the host faces of the first three run in that order on host arrays, followed by
    the oracle's serial filters on the host face's tables.  The records are tests/h264_fmt_picture_gen.py's (formats 2 and 3) and
    the generators' it extends (0 and 1)."""
    codec, mb_w, mb_h = "h264", 5, 3

    def __init__(self, fmt, bd=8):
        self.fmt, self.bd = fmt, bd
        self.name = "h264_whole_chain_fmt%d_%d" % (fmt, bd)

    def build(self, seed=9740):
        fmt, bd, mb_w, mb_h = self.fmt, self.bd, self.mb_w, self.mb_h
        rng = np.random.default_rng(seed + 16 * fmt + bd)
        dt, sh = GI.sample_dtype(bd), bd - 8
        shapes = plane_shapes(fmt, mb_w, mb_h)
        smooth = lambda s: (rng.integers(118, 138, s) << sh).astype(dt)         # flat enough for the filter to switch on
        refs = [[smooth(s) for s in shapes] + [None] * (3 - len(shapes)) for _ in range(3)]
        kw = dict(nslices=2, nrefs=3, p_intra=0.15, weights="none")
        if fmt >= 2:
            ip = FP.InterPicture(rng, mb_w, mb_h, fmt, bd, **kw)
            rp = FP.ResPicture(rng, mb_w, mb_h, fmt, bd, density=0.3, wild=0.0)
        else:
            ip = GI.InterPicture(rng, mb_w, mb_h, bd, chroma=fmt == 1, refs=refs, **kw)
            rp = GR.ResPicture(rng, mb_w, mb_h, bd, chroma=fmt == 1, density=0.3, wild=0.0)
        ip.refs = refs
        rp.mb["flags"] = (rp.mb["flags"] & 0xFE) | (ip.mb["flags"] & 1)            # one macroblock array for every face
        rp.mb["slice"] = ip.mb["slice"]
        rp.mb["qp"] = rng.integers(28, 46, mb_w * mb_h) + 6 * sh
        rp.layout()
        self.ip, self.rp, self.mb = ip, rp, rp.mb
        self.before = [smooth(s) for s in shapes]
        self.bs_slices = np.zeros(ip.nslices, h264.BS_SLICE_DTYPE)
        self.bs_slices["ref"], self.bs_slices["num_ref"], self.bs_slices["flags"] = ip.slices["ref"], ip.slices["num_ref"], ip.is_b
        self.chroma_qp = np.stack([F.G.chroma_qp_table(2, 6 * sh), F.G.chroma_qp_table(-3, 6 * sh)])
        # ---- the expected planes: the host faces, then the oracle's filters
        n, npl = mb_w * mb_h, len(shapes)
        want = [b.copy() for b in self.before]
        pad3 = lambda l, fill: list(l) + [fill] * (3 - len(l))
        strides = pad3([w.strides[0] for w in want], 0)
        dst = pad3([w.ctypes.data for w in want], None)
        h264.inter_pictures_fmt_host([dict(dst=dst, dst_stride=strides, mb=self.mb, mvf=ip.mvf, slices=ip.slices, mvf_stride=ip.w4,
                                           nslices=ip.nslices, refs=[dict(base=r, stride=strides, chroma_dy=0) for r in refs])], mb_w, mb_h, bd, fmt)
        h264.residual_pictures_fmt_host([dict(dst=dst, dst_stride=strides, mb=self.mb, res=rp.res, coeffs=rp.coeffs, ncoeffs=rp.ncoeffs)],
                                        mb_w, mb_h, bd, fmt)
        self.predicted = [w.copy() for w in want]
        self.tables = {t: np.zeros(n * per, E) for t, per in (("luma", 8), ("cb", F.PER[fmt]), ("cr", F.PER[fmt]))}
        h264.edge_params_pictures_fmt_host([dict(mb=self.mb, mvf=ip.mvf, slices=self.bs_slices, chroma_qp=self.chroma_qp, mvf_stride=ip.w4,
                                                 nslices=ip.nslices, **self.tables)], mb_w, mb_h, 0, 6 * sh, fmt)
        oracle_filter(fmt, bd, want, self.tables, mb_w, mb_h)
        self.want = want
        assert all((w != q).sum() > 30 for w, q in zip(want, self.predicted)), "%s: the filter changed next to nothing" % self.name
        assert all((q != b).sum() > 30 for q, b in zip(self.predicted, self.before)), "%s: the prediction changed next to nothing" % self.name
        return self

    def fresh(self):
        return copy.copy(self)

    def upload(self, torch):
        ip, rp = self.ip, self.rp
        npl = len(self.before)
        self.planes = [_dev(torch, b) for b in self.before]
        self.refs = [[_dev(torch, r[p]) for p in range(npl)] for r in ip.refs]
        self.ins = dict(mb=_dev(torch, self.mb), mvf=_dev(torch, ip.mvf), slices=_dev(torch, ip.slices), bs_slices=_dev(torch, self.bs_slices),
                        chroma_qp=_dev(torch, self.chroma_qp), res=_dev(torch, rp.res), coeffs=_dev(torch, rp.coeffs))
        n = self.mb_w * self.mb_h
        self.edges = [torch.full((n * per * 12,), 0xEE, dtype=torch.uint8, device="cuda") for per in (8, F.PER[self.fmt], F.PER[self.fmt])]

    def call(self, stream):
        ip, i, bd, fmt, mb_w, mb_h = self.ip, self.ins, self.bd, self.fmt, self.mb_w, self.mb_h
        pad3 = lambda l, fill: list(l) + [fill] * (3 - len(l))
        strides = pad3([b.strides[0] for b in self.before], 0)
        dst = pad3(self.planes, None)
        h264.inter_pictures_fmt([dict(dst=dst, dst_stride=strides, mb=i["mb"], mvf=i["mvf"], slices=i["slices"], mvf_stride=ip.w4,
                                      nslices=ip.nslices, refs=[dict(base=pad3(r, None), stride=strides) for r in self.refs])], mb_w, mb_h, bd, fmt,
                                stream=stream)
        h264.residual_pictures_fmt([dict(dst=dst, dst_stride=strides, mb=i["mb"], res=i["res"], coeffs=i["coeffs"], ncoeffs=self.rp.ncoeffs)],
                                   mb_w, mb_h, bd, fmt, stream=stream)
        h264.edge_params_pictures_fmt([dict(mb=i["mb"], mvf=i["mvf"], slices=i["bs_slices"], chroma_qp=i["chroma_qp"], luma=self.edges[0],
                                            cb=self.edges[1], cr=self.edges[2], mvf_stride=ip.w4, nslices=ip.nslices)], mb_w, mb_h, 0, 6 * (bd - 8),
                                      fmt, stream=stream)
        h264.deblock_pictures_fmt([dict(planes=self.planes, edges=self.edges[:len(self.planes)])], mb_w, mb_h, strides[0], strides[1], bd, fmt,
                                  stream=stream)

    def inputs(self):
        return list(self.ins.values()) + [t for r in self.refs for t in r]

    def outputs(self):
        return list(self.planes) + list(self.edges)

    def compare(self, view=lambda t: t):
        for t, e in zip(TABLES, self.edges):
            got = view(e).cpu().numpy().view(E)
            if self.fmt or t == "luma":
                assert np.array_equal(got, self.tables[t]), "%s: the %s table differs from the host face's" % (self.name, t)
            else:
                assert (got.view(np.uint8) == 0xEE).all()
        for p, (pl, w) in enumerate(zip(self.planes, self.want)):
            got = view(pl).cpu().numpy().view(w.dtype).reshape(w.shape)
            assert np.array_equal(got, w), "%s: plane %d: %d samples differ from the host faces and the oracle's filters" % (
                self.name, p, (got != w).sum())


@pytest.mark.parametrize("fmt,bd", [(0, 8), (1, 8), (2, 8), (3, 8), (2, 10), (3, 10)])
def test_the_whole_chain_from_one_mb_mvf_pair(fmt, bd):
    run_chain(WholeChain(fmt, bd).build())


# --------------------------------------------------------------------------------------------------------------- streams
@pytest.fixture(scope="module")
def delay():
    return PF.Delay(_torch())


@pytest.fixture
def stream():
    L = _lib.lib()
    assert L.ffhip_set_device(0) == 0
    st = C.c_void_p()
    assert L.ffhip_stream_create(C.byref(st)) == 0, L.ffhip_last_error()
    yield st
    assert L.ffhip_stream_destroy(st) == 0


STAGED = {"face2": lambda: Face(2).build(9750), "face3": lambda: Face(3).build(9750), "chain2": lambda: Chain(2, 8, 3).build(),
          "chain3_10": lambda: Chain(3, 10, 1).build(), "chain1": lambda: Chain(1, 8, 1).build(), "whole2": lambda: WholeChain(2, 8).build()}


@pytest.mark.parametrize("what", list(STAGED))
@pytest.mark.parametrize("late", [False, True])
def test_on_a_created_stream_and_behind_a_busy_null_stream(what, late, stream, delay):
    """late False: on a created stream behind a delay, every tensor poisoned until the stream itself puts the real bytes in place; True:
    behind a busy NULL stream with every progress-pool slot dirtied by a decoy"""
    torch = _torch()
    f = STAGED[what]()
    view, ins, keep = PF.run_staged(torch, _lib.lib(), stream, [f], delay, late=late)
    PF.check_staged(torch, [f], view, ins)
