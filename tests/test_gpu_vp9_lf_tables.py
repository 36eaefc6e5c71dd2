"""The VP9 loop-filter tables of whole frames on the GPU (ffhip_vp9_lf_tables_pictures_dev), byte for byte against the device-free host
face and the model of vp9_lf_tab_gen.py, guard regions included and every output pre-filled with 0xA5; and chained into
ffhip_vp9_loopfilter_frames_dev / _ssc_dev on one stream with no host synchronisation in between, against the oracle filtering
superblock by superblock from the model's VP9Filter."""
import copy

import numpy as np
import pytest

import vp9_lf_tab_gen as G
from ffmpeg_amd import _lib, vp9

pytestmark = pytest.mark.gpu

SS_IDS = ["420", "444", "422", "440"]
#: cols x rows in 8x8 blocks: 1 x 1 superblocks three ways, 2 x 13 and 9 x 5 superblocks with both edges cut at an odd block
SHAPES = [(1, 1), (5, 3), (8, 8), (13, 99), (67, 37)]


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def upload(torch, m):
    """the face's dict with device tensors: every array of maps() whole ("_name") and the payload view inside it ("name")"""
    d = dict(m)
    g = G.TabPicture.GUARD_BYTES
    for k in G.INPUTS + G.OUTPUTS:
        if m.get(k) is None:
            continue
        d["_" + k] = torch.from_numpy(m["_" + k].copy()).cuda()
        d[k] = d["_" + k][g:g + len(m[k])]
    return d


def compare(pics, ds, ms, models=None, view=lambda t: t):
    """device == host face == model on the whole allocations; the inputs unchanged"""
    P0 = pics[0]
    vp9.lf_tables_pictures_host(ms, P0.cols, P0.rows, P0.ss)
    for k, (pic, d, m) in enumerate(zip(pics, ds, ms)):
        model = models[k] if models is not None else pic.model()
        for name, e in G.expected(m, model).items():
            assert np.array_equal(m["_" + name], e), "picture %d %s: the host face differs from the model" % (k, name)
            got = view(d["_" + name]).cpu().numpy()
            bad = np.nonzero(got != e)[0]
            assert not len(bad), "picture %d %s: %d bytes differ, first at %s (payload from %d): got %s want %s" % (
                k, name, len(bad), bad[:4].tolist(), pic.GUARD_BYTES, got[bad[:4]], e[bad[:4]])
        for name in G.INPUTS:
            assert np.array_equal(d["_" + name].cpu().numpy(), m["_" + name]), "picture %d: %s was written" % (k, name)


def run(pics, models=None, filters=True, maps_kw=None, stream=None):
    torch = _torch()
    P0 = pics[0]
    ms = [p.maps(filters=filters, **(maps_kw or {})) for p in pics]
    ds = [upload(torch, m) for m in ms]
    torch.cuda.synchronize()
    vp9.lf_tables_pictures(ds, P0.cols, P0.rows, P0.ss, stream=stream)
    assert _lib.lib().ffhip_stream_synchronize(stream) == 0, _lib.lib().ffhip_last_error()
    torch.cuda.synchronize()
    compare(pics, ds, ms, models)
    return ds


@pytest.mark.parametrize("npics", [1, 3, 16])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("ss", G.SS, ids=SS_IDS)
def test_pictures(ss, shape, npics):
    """a partition of its own per picture"""
    run([G.TabPicture.random(9800 + 20 * shape[0] + k, shape[0], shape[1], ss) for k in range(npics)])


@pytest.mark.parametrize("ss", G.SS, ids=SS_IDS)
def test_crowded_whole_and_empty_superblocks_side_by_side(ss):
    """64 8x8 blocks | one 64x64 block | nothing"""
    a = [G.rec(i >> 3, i & 7, 9, i % 2, i % 3 == 0, i) for i in range(64)]
    pic = G.TabPicture(24, 8, ss, [a, [G.rec(0, 0, 0, 3, 0, 7)], []], level=np.arange(64) % 63 + 1, sharp=1)
    ds = run([pic])
    g = pic.GUARD_BYTES
    assert not ds[0]["_tables"][g + 2 * 1280:g + 3 * 1280].any() and ds[0]["_tables"][g:g + 2 * 1280].any()


@pytest.mark.parametrize("ss", G.SS, ids=SS_IDS)
def test_malformed_records_and_sb_first(ss):
    """the malformed-record set of the CPU tier in one picture, more than 64 records in a superblock, and sb_first with a decreasing
    pair and entries beyond nblocks: the result equals the host face and the model, the guard regions are intact"""
    clean = G.TabPicture.random(9700, 13, 11, ss, level=np.arange(64) % 63 + 1)
    recs = [list(r) for r in clean.sb_records]
    for _, sb, bad in G.malformed_cases():
        recs[sb].insert(len(recs[sb]) // 2, bad)
    dirty = G.TabPicture(13, 11, ss, recs, level=clean.level)
    dirty.lim, dirty.mblim = clean.lim, clean.mblim
    run([dirty], [clean.model()])

    import test_vp9_lf_tables_cpu as T
    run([T.crowded(ss)])

    pic = G.TabPicture.random(9710, 24, 8, ss)
    n, f = pic.nblocks, pic.sb_first
    flat = [tuple(int(v) for v in r) for r in pic.blocks]
    recs = [[], flat[f[0]:f[2]], flat[f[2]:n]]
    # the records of superblock 0 read as superblock 1's: where two of them overlap they must agree on the level
    lvl = np.full(64, 17, np.uint8)
    pic.level = lvl
    run([pic], [pic.model(recs)], maps_kw={"sb_first": np.array([f[1], f[0], f[2], 0xFFFFFFF0], np.uint32)})
    cut = int(f[2]) + 1
    run([pic], [pic.model([flat[f[0]:f[1]], flat[f[1]:f[2]], flat[f[2]:cut]])], maps_kw={"nblocks": cut})
    run([pic], [pic.model([[], [], []])], maps_kw={"sb_first": np.array([0xFFFFFFFF, 0x80000000, 5, 2], np.uint32)})


@pytest.mark.parametrize("ss", G.SS, ids=SS_IDS)
def test_without_filters_the_tables_are_the_same(ss):
    run([G.TabPicture.random(9810 + k, 19, 13, ss) for k in range(2)], filters=False)


@pytest.mark.parametrize("ss", G.SS, ids=SS_IDS)
def test_zero_levels_give_zero_tables(ss):
    ds = run([G.TabPicture.random(9820, 19, 13, ss, level=np.zeros(64, np.uint8))])
    g = G.TabPicture.GUARD_BYTES
    for name in G.OUTPUTS:
        if ds[0].get(name) is not None:
            assert not ds[0]["_" + name][g:-g].any() and (ds[0]["_" + name][:g] == G.GUARD).all()


# ------------------------------------------------------------------------------------------------ the chain
class Face:
    """the face alone, with the steps tests/picture_faces.py gives its adapters"""
    name, codec = "vp9_lf_tables", "vp9"

    def build(self, seed):
        self.pic = G.TabPicture.random(seed, 67, 37, (1, 1))
        self.model = self.pic.model()
        return self

    def fresh(self):
        return copy.copy(self)

    def upload(self, torch):
        self.m = self.pic.maps()
        self.d = upload(torch, self.m)

    def call(self, stream):
        vp9.lf_tables_pictures([self.d], self.pic.cols, self.pic.rows, self.pic.ss, stream=stream)

    def inputs(self):
        return [self.d["_" + k] for k in G.INPUTS]

    def outputs(self):
        return [self.d["_" + k] for k in G.OUTPUTS if self.d.get(k) is not None]

    def compare(self, view=lambda t: t):
        compare([self.pic], [self.d], [self.m], [self.model], view)


class Chain:
    """_dev -> ffhip_vp9_loopfilter_frames_dev (4:2:0) / _ssc_dev (4:2:2, with ctables) with no synchronisation between them: the planes
    equal the oracle's ffo_vp9_loopfilter_sb run superblock by superblock on the model's VP9Filter"""
    cols, rows = 21, 13          # 3 x 2 superblocks, both edges cut at an odd block

    def __init__(self, bit_depth=8, ss=(1, 1)):
        self.bd, self.ss = bit_depth, tuple(ss)
        self.name = "vp9_lf_tables+loopfilter_%d_%d%d" % (bit_depth, ss[0], ss[1])

    def build(self, seed=9830):
        import test_gpu_vp9_lf_frame as F
        rng = np.random.default_rng(seed + self.bd + 2 * self.ss[1])
        self.pic = G.TabPicture.random(seed + self.bd, self.cols, self.rows, self.ss)
        self.model = self.pic.model()
        sbc, sbr, (ss_h, ss_v) = self.pic.sb_cols, self.pic.sb_rows, self.ss
        cw, ch = 64 >> ss_h, 64 >> ss_v
        self.src = [F._plane(rng, 64 * sbr, 64 * sbc, 12, self.bd), F._plane(rng, ch * sbr, cw * sbc, 4, self.bd),
                    F._plane(rng, ch * sbr, cw * sbc, 4, self.bd)]
        self.filtered = [s.copy() for s in self.src]
        F.oracle_frame(self.filtered, self.model[0], sbc, sbr, self.bd, self.ss, self.pic.lim, self.pic.mblim)
        return self

    def fresh(self):
        return copy.copy(self)

    def upload(self, torch):
        if not hasattr(self, "pic"):
            self.build()
        self.m = self.pic.maps(filters=False)
        self.d = upload(torch, self.m)
        self.planes = [torch.from_numpy(s.view(np.uint8).reshape(-1).copy()).cuda() for s in self.src]

    def call(self, stream):
        p, d = self.pic, self.d
        vp9.lf_tables_pictures([d], p.cols, p.rows, p.ss, stream=stream)
        sy, suv = self.src[0].strides[0], self.src[1].strides[0]
        if self.ss[0] == self.ss[1]:
            vp9.loopfilter_frames([(*self.planes, d["tables"])], sy, suv, p.cols, p.rows, stream=stream, bit_depth=self.bd, ss=self.ss)
        else:
            vp9.loopfilter_frames_ssc([(*self.planes, d["tables"], d["ctables"])], sy, suv, p.cols, p.rows, self.ss, stream=stream,
                                      bit_depth=self.bd)

    def inputs(self):
        return [self.d["_" + k] for k in G.INPUTS]

    def outputs(self):
        return [self.d["_" + k] for k in G.OUTPUTS if self.d.get(k) is not None] + list(self.planes)

    def compare(self, view=lambda t: t):
        import test_gpu_vp9_lf_frame as F
        compare([self.pic], [self.d], [self.m], [self.model], view)
        F.compare([view(p) for p in self.planes], self.filtered, self.src, self.cols, self.rows, self.ss)
        changed = sum(int((w != s).sum()) for w, s in zip(self.filtered, self.src))
        assert changed > 100, "%s: the filter changed next to nothing" % self.name


CHAINS = [(8, (1, 1)), (10, (1, 1)), (8, (1, 0))]


@pytest.mark.parametrize("bit_depth,ss", CHAINS, ids=["420_8", "420_10", "422_8"])
def test_chained_into_the_loop_filter_on_one_stream(bit_depth, ss):
    """Chain on the NULL stream (tests/test_gpu_vp9_lf_tables_streams.py runs it on a created one)"""
    torch = _torch()
    chain = Chain(bit_depth, ss).build()
    chain.upload(torch)
    torch.cuda.synchronize()
    chain.call(None)
    assert _lib.lib().ffhip_stream_synchronize(None) == 0, _lib.lib().ffhip_last_error()
    torch.cuda.synchronize()
    chain.compare()
