"""H.264 inter prediction of whole pictures on the GPU (ffhip_h264_inter_pictures_dev), byte for byte against the model of
h264_inter_picture_gen.py (the decoder-order calls of mc_part() through the oracle): whole destination buffers with their stride
padding and a guard row on either side, poisoned before the call, so that a sample no rule writes must keep the poison; the inputs
must come back unchanged.  The picture sets of the CPU tier (1 x 1, 3 x 2, 5 x 4 and 11 x 9 macroblocks, 1, 3 and 17 pictures to a
call, 8 and 10 bits, monochrome), then constructed pictures: every mcxy at 8x8 and 4x4 and every chroma fraction, vectors across
every side and corner and far outside, every way the lists combine, intra and malformed blocks, 14 bits into both clips, and the two
fields of a frame in one buffer."""
import copy

import numpy as np
import pytest

import h264_inter_picture_gen as G
from ffmpeg_amd import _lib, h264

pytestmark = pytest.mark.gpu

REF_PAD = 0x33


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _poison(dtype):
    return np.frombuffer(bytes([G.POISON]) * 2, dtype)[0]


def _padded(plane, pad, fill):
    """the plane in rows `pad` samples wider, the padding holding `fill` bytes"""
    a = np.full((plane.shape[0], plane.shape[1] + pad), np.frombuffer(bytes([fill]) * 2, plane.dtype)[0], plane.dtype)
    a[:, :plane.shape[1]] = plane
    return a


def upload(torch, pic, want, pad=0):
    """(the face's dict, what compare() needs): the references in tensors of their own, rows `pad` samples wider than the picture; the
    destination planes poisoned, with stride padding and a guard row above and below"""
    ps = np.dtype(G.sample_dtype(pic.bd)).itemsize
    npl = 3 if pic.chroma else 1
    refs, keep = [], []
    for r, dy in zip(pic.refs, pic.chroma_dy):
        t = [_dev(torch, _padded(r[p], pad, REF_PAD)) for p in range(npl)]
        keep += t
        refs.append(dict(base=t + [None] * (3 - npl), stride=[(r[p].shape[1] + pad) * ps for p in range(npl)] + [0] * (3 - npl), chroma_dy=dy))
    bufs, exp, dst, strides = [], [], [], []
    for p in range(npl):
        e = _padded(want[p], pad, G.POISON)
        guard = np.full_like(e[:1], _poison(e.dtype))
        e = np.concatenate([guard, e, guard])
        t = torch.full((e.size * ps,), G.POISON, dtype=torch.uint8, device="cuda")
        bufs.append(t)
        exp.append(e)
        strides.append(e.shape[1] * ps)
        dst.append(t.data_ptr() + strides[-1])
    ins = [_dev(torch, pic.mb), _dev(torch, pic.mvf), _dev(torch, pic.slices)]
    keep += ins
    arg = dict(dst=dst + [None] * (3 - npl), dst_stride=strides + [0] * (3 - npl), mb=ins[0], mvf=ins[1], slices=ins[2], mvf_stride=pic.w4,
               nslices=pic.nslices, refs=refs)
    return arg, dict(bufs=bufs, exp=exp, keep=keep, before=[t.clone() for t in keep])


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


def run(pics, models, pad=0, what="", cfi=None):
    torch = _torch()
    up = [upload(torch, p, m[0], pad) for p, m in zip(pics, models)]
    torch.cuda.synchronize()
    P0 = pics[0]
    h264.inter_pictures([a for a, _ in up], P0.mb_w, P0.mb_h, P0.bd, int(P0.chroma) if cfi is None else cfi)
    assert _lib.lib().ffhip_stream_synchronize(None) == 0, _lib.lib().ffhip_last_error()
    torch.cuda.synchronize()
    compare(up, what=what)


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("name", G.NAMES)
def test_picture_set(name, pad):
    """the CPU tier's sets, one call per set (17 pictures: two launches), with tight strides and with rows 8 samples wider"""
    pics, models = G.picture_set(name)
    run(pics, models, pad, name)


def test_monochrome_through_chroma_format_idc_1_with_null_chroma():
    pics, models = G.picture_set("3x2_mono")
    run(pics, models, 4, "mono", cfi=1)


def _edited(pic):
    """the model of a picture edited by hand"""
    return [pic], [G.model(pic)]


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("lists", ["l0", "l1", "bi"])
def test_every_mcxy_at_8x8_and_4x4_and_every_chroma_fraction(bd, lists):
    ri = {"l0": [1, -1], "l1": [-1, 0], "bi": [0, 1]}[lists]
    # 2 x 2 macroblocks of four 8x8 partitions: partition i at position mcxy i
    a = G.blank(2, 2, bd, nrefs=2, seed=9520 + bd)
    a.parts = [[(8 * (q & 1), 8 * (q >> 1), 8, 8, "8x8") for q in range(4)] for _ in range(4)]
    for i in range(16):
        my, mx, q = i >> 3, (i >> 2) & 1, i & 3
        blk = a.mvf[my * 4 + 2 * (q >> 1):my * 4 + 2 * (q >> 1) + 2, mx * 4 + 2 * (q & 1):mx * 4 + 2 * (q & 1) + 2]
        blk["ref_idx"] = ri
        blk["mv"] = [[(i & 3) + 4 * ((i * 7) % 5 - 2), (i >> 2) + 4 * ((i * 3) % 7 - 3)], [(i >> 2) - 8, (i & 3) + 12]]
    # 2 x 2 macroblocks of 4x4 blocks: block i with the eighth-sample fractions (i & 7, i >> 3), so every mcxy four times
    b = G.blank(2, 2, bd, nrefs=2, seed=9530 + bd)
    for i in range(64):
        b.mvf[i >> 3, i & 7]["ref_idx"] = ri
        b.mvf[i >> 3, i & 7]["mv"] = [[(i & 7) - 16, (i >> 3) + 8], [(i >> 3) + 24, (i & 7) - 8]]
    ma, mb_ = G.model(a), G.model(b)
    assert {m for s, m in ma[2]["mcxy"] if s == 8} == set(range(16)) == {m for s, m in mb_[2]["mcxy"] if s == 4}
    assert len(mb_[2]["cfrac"]) == 64
    run([a, b], [ma, mb_], 4, "mcxy " + lists)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("reach", [70, 2000, 32767])
def test_vectors_across_every_side_and_corner_and_far_outside(bd, reach):
    rng = np.random.default_rng(9540 + bd + reach)
    pic = G.InterPicture(rng, 3, 2, bd, nslices=2, free=True, types="B", p_intra=0.0)
    dirs = [(-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1)]
    for y in range(pic.h4):
        for x in range(pic.w4):
            for l in range(2):
                dx, dy = dirs[(x + 3 * y + 5 * l) % 8]
                pic.mvf[y, x]["mv"][l] = np.clip([dx * reach + rng.integers(-3, 4), dy * reach + rng.integers(-3, 4)], -32768, 32767)
    pics, models = _edited(pic)
    assert models[0][2]["sides"] == {"left", "top", "right", "bottom"}
    assert {int(pic.mvf["mv"].min()), int(pic.mvf["mv"].max())} == {-32768, 32767} or reach < 32767
    run(pics, models, 0, "reach %d" % reach)


def _weighted(bd, kind, seed):
    """a 3 x 2 picture of 4x4 blocks in one B slice: `kind` none, implicit, or (luma denominator, chroma denominator, offset)"""
    rng = np.random.default_rng(seed)
    pic = G.InterPicture(rng, 3, 2, bd, nslices=1, free=True, types="B", p_intra=0.0, weights="explicit" if isinstance(kind, tuple) else kind)
    s = pic.slices[0]
    if isinstance(kind, tuple):
        s["luma_log2_denom"], s["chroma_log2_denom"] = kind[:2]
        s["use_weight_chroma"] = kind[2] > 0
        s["luma_weight"][:, 0, 1] = s["chroma_weight"][:, 0, :, 1] = kind[2]         # list 0: the extreme; list 1: by ref_idx
        s["luma_weight"][:, 1, 1] = np.resize([kind[2], 0, kind[2] // 2], 32)
        s["chroma_weight"][:, 1, :, 1] = np.resize([kind[2], 0, kind[2] // 2], 32)[:, None]
    return pic


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("kind", ["none", "implicit", (0, 7, -128), (7, 0, 127), (0, 0, 127), (7, 7, -128)], ids=str)
def test_every_way_the_lists_combine(bd, kind):
    pic = _weighted(bd, kind, 9550 + bd)
    pics, models = _edited(pic)
    modes = models[0][2]["modes"]
    if kind == "none":
        assert modes == {h264.INTER_UNI, h264.INTER_BI_AVG} and set(np.unique(models[0][1]["list"])) == {0, 1}
    elif kind == "implicit":
        assert modes == {h264.INTER_UNI, h264.INTER_BI_AVG, h264.INTER_BI_W}
    else:
        assert modes == {h264.INTER_UNI_W, h264.INTER_BI_W}
        assert kind[2] in models[0][1]["luma_offset"] and 2 * kind[2] in models[0][1]["luma_offset"]
    run(pics, models, 4, str(kind))


def test_14_bits_reach_both_clips():
    pic = _weighted(14, (1, 1, 127), 9560)
    s = pic.slices[0]
    s["luma_weight"][..., 0] = np.where(np.arange(64).reshape(32, 2) & 1, 127, -128)
    s["chroma_weight"][..., 0] = np.where(np.arange(128).reshape(32, 2, 2) & 2, 127, -128)
    pics, models = _edited(pic)
    for p in range(3):
        assert (models[0][0][p] == 0).sum() > 20 and (models[0][0][p] == 16383).sum() > 20 and ((models[0][0][p] > 0) & (models[0][0][p] < 16383)).any()
    run(pics, models, 0, "14 bits")


@pytest.mark.parametrize("bd", [8, 10])
def test_intra_and_malformed_blocks_keep_the_poison(bd):
    rng = np.random.default_rng(9570 + bd)
    pic = G.InterPicture(rng, 4, 3, bd, nslices=1, free=True, types="B", p_intra=0.0, weights="explicit")
    bad = np.zeros(2, h264.INTER_SLICE_DTYPE)                     # slices 1 and 2 are slice 0 with one fault each
    bad[:] = pic.slices[0]
    bad[0]["chroma_log2_denom"] = 8
    bad[1]["use_weight"] = 3
    pic.slices = np.concatenate([pic.slices, bad])
    pic.nslices = 3
    pic.mb["flags"][[1, 6]] = h264.BS_MB_INTRA
    pic.mb["slice"][[2, 7, 9]] = [1, 2, 3]                        # bad denominator, bad use_weight, no such slice
    pic.free_parts()
    pic.slices[0]["ref"][1][0] = pic.nrefs                        # list 1's ref_idx 0 names a slot that is not there
    n1 = int(pic.slices[0]["num_ref"][0])
    for k, (y, x) in enumerate(zip(*np.nonzero(rng.random((pic.h4, pic.w4)) < 0.2))):
        pic.mvf[y, x]["ref_idx"] = [[-1, -1], [n1, -1], [0, 32], [127, 0], [-7, -128]][k % 5]
    pics, models = _edited(pic)
    skip = models[0][1]["mode"] == h264.INTER_SKIP
    assert skip[:4, 4:8].all() and skip[:4, 8:12].all() and skip[4:8, 12:16].all() and skip[8:12, 4:8].all()
    assert skip.sum() > 5 * 16 + 10 and (~skip).sum() >= 20
    assert (models[0][0][0] == _poison(models[0][0][0].dtype)).sum() >= 16 * skip.sum()
    run(pics, models, 4, "malformed")


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("parity", [0, 1])
def test_a_field_predicted_from_the_other_field_of_its_frame(bd, parity):
    """the destination field's rows interleave with the rows of reference slot 0, the other field of the same buffer (chroma_dy
    2 * (parity - other parity) = +-2); slots 1 and 2 are the fields of another frame"""
    torch = _torch()
    rng = np.random.default_rng(9580 + bd + parity)
    mb_w, mb_h, pad = 3, 2, 8
    dt, ps = G.sample_dtype(bd), 1 if bd == 8 else 2
    shapes = [(32 * mb_h, 16 * mb_w + pad), (16 * mb_h, 8 * mb_w + pad), (16 * mb_h, 8 * mb_w + pad)]
    cur = [rng.integers(0, 1 << bd, s).astype(dt) for s in shapes]
    other = [rng.integers(0, 1 << bd, s).astype(dt) for s in shapes]
    width = lambda a, p: a[:, :(16 if p == 0 else 8) * mb_w]
    field = lambda fr, par: [width(fr[p][par::2], p) for p in range(3)]
    refs = [field(cur, 1 - parity), field(other, parity), field(other, 1 - parity)]
    dys = [2 * (parity - (1 - parity)), 0, 2 * (parity - (1 - parity))]
    pic = G.InterPicture(rng, mb_w, mb_h, bd, nslices=2, nrefs=3, types="B", refs=refs, chroma_dy=dys)
    want, _, cover = G.model(pic)
    other_fill = G.model(pic, fill=G.POISON ^ 0xFF)[0]              # what differs between the two is what no rule writes
    exp = [c.copy() for c in cur]
    for p in range(3):
        rows = exp[p][parity::2]
        rows[:, :want[p].shape[1]] = np.where(want[p] != other_fill[p], rows[:, :want[p].shape[1]], want[p])
    d_cur, d_other = [_dev(torch, c) for c in cur], [_dev(torch, c) for c in other]
    strides = [s[1] * ps for s in shapes]
    fref = lambda d, par, dy: dict(base=[d[p].data_ptr() + par * strides[p] for p in range(3)], stride=[2 * s for s in strides], chroma_dy=dy)
    ins = [_dev(torch, pic.mb), _dev(torch, pic.mvf), _dev(torch, pic.slices)]
    arg = dict(dst=[d_cur[p].data_ptr() + parity * strides[p] for p in range(3)], dst_stride=[2 * s for s in strides], mb=ins[0], mvf=ins[1],
               slices=ins[2], mvf_stride=pic.w4, nslices=pic.nslices,
               refs=[fref(d_cur, 1 - parity, dys[0]), fref(d_other, parity, 0), fref(d_other, 1 - parity, dys[2])])
    torch.cuda.synchronize()
    h264.inter_pictures([arg], mb_w, mb_h, bd, 1)
    torch.cuda.synchronize()
    for p in range(3):
        got = d_cur[p].cpu().numpy().view(dt).reshape(shapes[p])
        bad = np.argwhere(got != exp[p])
        assert not len(bad), "plane %d: %d samples differ, first at %s" % (p, len(bad), bad[0].tolist())
        assert np.array_equal(d_other[p].cpu().numpy().view(dt).reshape(shapes[p]), other[p])
    assert (exp[0] != cur[0]).sum() > 1000 and any(y & 1 for _, y in cover["cfrac"])


# ------------------------------------------------------------------------------------ the adapter of tests/picture_faces.py
class Face:
    """the face alone, with the steps tests/picture_faces.py gives its adapters: build / upload / call(stream) / inputs / outputs /
    compare(view)"""
    name, codec, pad = "h264_inter_pictures", "h264", 4

    def __init__(self, bd=8):
        self.bd = bd

    def build(self, seed):
        rng = np.random.default_rng(seed + self.bd)
        self.pics = [G.InterPicture(rng, 5, 4, self.bd, nslices=3, nrefs=3) for _ in range(2)]
        self.models = [G.model(p) for p in self.pics]
        return self

    def fresh(self):
        return copy.copy(self)

    def upload(self, torch):
        self.up = [upload(torch, p, m[0], self.pad) for p, m in zip(self.pics, self.models)]

    def call(self, stream):
        h264.inter_pictures([a for a, _ in self.up], 5, 4, self.bd, 1, stream=stream)

    def inputs(self):
        return [t for _, u in self.up for t in u["keep"]]

    def outputs(self):
        return [t for _, u in self.up for t in u["bufs"]]

    def compare(self, view=lambda t: t):
        # the inputs are compared by the staged run against what it staged; here against what upload() put there
        compare(self.up, view, self.name)


# -------------------------------------------------------------------------------------------------------------------- chains
def _one_base(torch, pic, pad):
    """the references of a plane one behind the other in one tensor, rows as wide as the destination's: what the picture object
    takes (one base and one stride per plane).  (tensors, strides in bytes, bytes between two references)"""
    ps = np.dtype(G.sample_dtype(pic.bd)).itemsize
    tens, strides, step = [], [], []
    for p in range(3):
        rows = np.concatenate([_padded(r[p], pad, REF_PAD) for r in pic.refs])
        tens.append(_dev(torch, rows))
        strides.append(rows.shape[1] * ps)
        step.append(pic.refs[0][p].shape[0] * strides[-1])
    return tens, strides, step


@pytest.mark.parametrize("bd", [8, 10])
def test_against_the_picture_object(bd):
    """the same content recorded call by call into h264.Picture and flushed (put, put into the scratch plane, avg, weight / biweight:
    four passes) gives the planes the face gives in one launch; both equal the model"""
    torch = _torch()
    rng = np.random.default_rng(9600 + bd)
    pad = 8
    pic = G.InterPicture(rng, 5, 4, bd, nslices=3, nrefs=3)
    want, _, cover = G.model(pic)
    refs, strides, step = _one_base(torch, pic, pad)
    exp = [_padded(w, pad, G.POISON) for w in want]
    face = [torch.full((e.nbytes,), G.POISON, dtype=torch.uint8, device="cuda") for e in exp]
    flushed = [t.clone() for t in face]
    ins = [_dev(torch, pic.mb), _dev(torch, pic.mvf), _dev(torch, pic.slices)]
    arg = dict(dst=face, dst_stride=strides, mb=ins[0], mvf=ins[1], slices=ins[2], mvf_stride=pic.w4, nslices=pic.nslices,
               refs=[dict(base=[refs[p].data_ptr() + k * step[p] for p in range(3)], stride=strides) for k in range(pic.nrefs)])
    obj = h264.Picture(pic.mb_w, pic.mb_h, bit_depth=bd)
    G.record(obj, G.picture_records(pic, cover["calls"], strides, step))
    torch.cuda.synchronize()
    h264.inter_pictures([arg], pic.mb_w, pic.mb_h, bd, 1)
    obj.flush(flushed, strides, refs)
    torch.cuda.synchronize()
    obj.close()
    for p in range(3):
        a, b = (t.cpu().numpy().view(exp[p].dtype).reshape(exp[p].shape) for t in (face[p], flushed[p]))
        assert np.array_equal(a, exp[p]), "plane %d: the face differs from the model in %d samples" % (p, (a != exp[p]).sum())
        assert np.array_equal(b, exp[p]), "plane %d: the picture object differs from the model in %d samples" % (p, (b != exp[p]).sum())
    assert cover["modes"] == {1, 2, 3, 4} and len(cover["calls"]) > 300


class Chain:
    """face -> ffhip_h264_idct_add_mb_batch_dev (idct_add16 on the inter macroblocks' luma) -> ffhip_h264_edge_params_pictures_dev ->
    ffhip_h264_deblock_frames_dev / _chroma_dev, on one stream with no synchronisation in between and from one upload of mb / mvf:
    the planes equal the oracle's serial sequence (the model's prediction, ffo_h264_idct_add16 macroblock by macroblock, the
    oracle's frame filter on model A's tables of tests/h264_bs_picture_gen.py).  The steps tests/picture_faces.py gives its adapters."""
    name, codec, mb_w, mb_h = "h264_inter+idct+edge_params+deblock", "h264", 6, 5

    def build(self, seed=9610):
        import ctypes as C

        import ffi
        import h264_bs_picture_gen as B
        from h264_intra_gen import SCAN8
        rng = np.random.default_rng(seed)
        mb_w, mb_h = self.mb_w, self.mb_h
        smooth = lambda h, w: rng.integers(118, 138, (h, w)).astype(np.uint8)     # flat enough for the filter to switch on
        refs = [[smooth(16 * mb_h, 16 * mb_w), smooth(8 * mb_h, 8 * mb_w), smooth(8 * mb_h, 8 * mb_w)] for _ in range(3)]
        pic = self.pic = G.InterPicture(rng, mb_w, mb_h, 8, nslices=2, nrefs=3, p_intra=0.15, weights="none", refs=refs)
        n = mb_w * mb_h
        inter = np.nonzero((pic.mb["flags"] & 1) == 0)[0]
        # the residual of the inter macroblocks, and the non-zero bits the filter sees
        self.stride = stride = 16 * mb_w
        self.bo = np.array([(i & 1) * 4 + ((i >> 1) & 1) * 4 * stride + ((i >> 2) & 1) * 8 + (i >> 3) * 8 * stride for i in range(16)], np.int32)
        self.mb_off = ((inter // mb_w) * 16 * stride + (inter % mb_w) * 16).astype(np.int32)
        self.blocks = rng.integers(-60, 60, (len(inter), 256)).astype(np.int16)
        self.nnzc = np.zeros((len(inter), 40), np.uint8)
        for k, m in enumerate(inter):
            for i in range(16):
                r = rng.random()
                if r < .5:
                    self.blocks[k, 16 * i:16 * i + 16] = 0
                elif r < .7:
                    self.blocks[k, 16 * i + 1:16 * i + 16] = 0
                nz = int(np.count_nonzero(self.blocks[k, 16 * i:16 * i + 16]))
                self.nnzc[k, SCAN8[i]] = nz
                if nz:
                    pic.mb["nnz"][m] |= 1 << ((i & 1) + 2 * ((i >> 2) & 1) + 4 * (((i >> 1) & 1) + 2 * (i >> 3)))
        pic.mb["qp"] = rng.integers(26, 44, n)
        # what the planes hold before: the intra macroblocks' samples stay
        self.before = [smooth(h, w) for h, w in ((16 * mb_h, 16 * mb_w), (8 * mb_h, 8 * mb_w), (8 * mb_h, 8 * mb_w))]
        a, b = G.model(pic)[0], G.model(pic, fill=G.POISON ^ 0xFF)[0]
        want = [np.where(x == y, x, z) for x, y, z in zip(a, b, self.before)]
        O = ffi.oracle()
        u8p, i16p, i32p = ffi.u8p, C.POINTER(C.c_int16), C.POINTER(C.c_int32)
        wb = self.blocks.copy()
        for k in range(len(inter)):
            O.ffo_h264_idct_add16(C.cast(want[0].ctypes.data + int(self.mb_off[k]), u8p), ffi.ptr(self.bo, i32p), ffi.ptr(wb[k], i16p), stride,
                                  ffi.ptr(self.nnzc[k]))
        self.predicted = [w.copy() for w in want]
        bs = self.bs = B.blank(mb_w, mb_h)
        bs.mb, bs.mvf = pic.mb, pic.mvf
        bs.slices = np.zeros(pic.nslices, h264.BS_SLICE_DTYPE)
        bs.slices["ref"], bs.slices["num_ref"], bs.slices["flags"] = pic.slices["ref"], pic.slices["num_ref"], pic.is_b
        bs.nslices = pic.nslices
        self.tables = B.model_a(bs)
        for p, t in enumerate(("luma", "cb", "cr")):
            e = C.c_void_p(np.ascontiguousarray(self.tables[t]).ctypes.data)
            at = C.cast(want[p].ctypes.data, u8p)
            (O.ffo_h264_deblock_frame_chroma if p else O.ffo_h264_deblock_frame)(at, want[p].strides[0], mb_w, mb_h, e)
        self.want = want
        assert all((w != q).sum() > 50 for w, q in zip(want, self.predicted)), "the filter changed next to nothing"
        return self

    def fresh(self):
        return copy.copy(self)

    def upload(self, torch):
        pic = self.pic
        m = self.bs.maps()
        self.planes = [_dev(torch, b) for b in self.before]
        self.refs = [[_dev(torch, r[p]) for p in range(3)] for r in pic.refs]
        typed = lambda a: torch.from_numpy(a.copy()).cuda()        # idct_add_mb_batch() counts the macroblocks by mb_off.numel()
        self.ins = dict(mb=_dev(torch, pic.mb), mvf=_dev(torch, pic.mvf), slices=_dev(torch, pic.slices), bs_slices=_dev(torch, self.bs.slices),
                        chroma_qp=_dev(torch, m["chroma_qp"]), mb_off=typed(self.mb_off), bo=typed(self.bo), nnzc=typed(self.nnzc))
        self.blocks_d = typed(self.blocks)
        assert self.ins["mb_off"].dtype == torch.int32 and self.ins["mb_off"].numel() == len(self.mb_off) == len(self.blocks) == len(self.nnzc)
        assert int(self.mb_off.max()) + 15 * self.stride + 16 <= self.before[0].size and self.blocks.shape[1] == 256 and self.nnzc.shape[1] == 40
        n = self.mb_w * self.mb_h
        self.edges = [torch.full((n * per * 12,), 0xEE, dtype=torch.uint8, device="cuda") for per in (8, 4, 4)]

    def call(self, stream):
        pic, i = self.pic, self.ins
        strides = [b.strides[0] for b in self.before]
        h264.inter_pictures([dict(dst=self.planes, dst_stride=strides, mb=i["mb"], mvf=i["mvf"], slices=i["slices"], mvf_stride=pic.w4,
                                  nslices=pic.nslices, refs=[dict(base=r, stride=strides) for r in self.refs])], pic.mb_w, pic.mb_h, 8, 1, stream=stream)
        h264.idct_add_mb_batch(0, self.planes[0], self.stride, i["mb_off"], i["bo"], self.blocks_d, i["nnzc"], stream=stream)
        h264.edge_params_pictures([dict(mb=i["mb"], mvf=i["mvf"], slices=i["bs_slices"], chroma_qp=i["chroma_qp"], luma=self.edges[0],
                                        cb=self.edges[1], cr=self.edges[2], mvf_stride=pic.w4, nslices=pic.nslices)], pic.mb_w, pic.mb_h, stream=stream)
        for p, (pl, e) in enumerate(zip(self.planes, self.edges)):
            h, s = self.before[p].shape[0], strides[p]
            (h264.deblock_frames_chroma if p else h264.deblock_frames)(pl, h * s, 1, s, pic.mb_w, pic.mb_h, e, stream=stream)

    def inputs(self):
        return list(self.ins.values()) + [t for r in self.refs for t in r]

    def outputs(self):
        return list(self.planes) + list(self.edges) + [self.blocks_d]

    def compare(self, view=lambda t: t):
        for t, e in zip(("luma", "cb", "cr"), self.edges):
            assert np.array_equal(view(e).cpu().numpy().view(h264.EDGE_DTYPE), self.tables[t]), "%s: the %s table differs from model A" % (self.name, t)
        for p, (pl, w) in enumerate(zip(self.planes, self.want)):
            got = view(pl).cpu().numpy().reshape(w.shape)
            assert np.array_equal(got, w), "%s: plane %d: %d samples differ from the oracle's serial sequence" % (self.name, p, (got != w).sum())


def test_chained_into_the_residual_the_edge_parameters_and_the_filter_on_one_stream():
    """Chain on the NULL stream (tests/test_gpu_h264_inter_picture_streams.py runs it on a created one)"""
    torch = _torch()
    chain = Chain().build()
    chain.upload(torch)
    torch.cuda.synchronize()
    chain.call(None)
    assert _lib.lib().ffhip_stream_synchronize(None) == 0, _lib.lib().ffhip_last_error()
    torch.cuda.synchronize()
    chain.compare()
