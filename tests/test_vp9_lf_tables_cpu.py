"""CPU tier of the VP9 loop-filter table face (ffhip_vp9_lf_tables_pictures_dev / _host): the record ABI, the device-free host face
against the model of vp9_lf_tab_gen.py byte for byte (guard regions included), a single-record sweep, one hand-written case per
branch of mask_edges, malformed records and sb_first arrays, empty superblocks, the argument refusals with their texts, and the
coverage of the picture set."""
import ctypes as C

import numpy as np
import pytest

import vp9_lf_tab_gen as G
from ffmpeg_amd import _lib, vp9

SIZES = [(1, 1), (8, 8), (3, 5), (67, 37), (13, 100)]        # cols x rows in 8x8 blocks
SS_IDS = ["420", "444", "422", "440"]


def test_record_size_matches_the_c_struct():
    assert _lib.lib().ffhip_vp9_lf_block_record_size() == vp9.LF_BLOCK_DTYPE.itemsize == G.BLOCK_DT.itemsize == 4
    assert C.sizeof(vp9.LfTabPic) == 2 * 8 + 4 + 3 * 64 + 4 + 3 * 8


def check_host(pic, model=None, filters=True, **maps_kw):
    """the host face on the picture's arrays == the model, every allocation whole: guards intact, inputs unchanged"""
    m = pic.maps(filters=filters, **maps_kw)
    before = {k: m["_" + k].copy() for k in G.INPUTS}
    vp9.lf_tables_pictures_host([m], pic.cols, pic.rows, pic.ss)
    model = pic.model() if model is None else model
    for name, e in G.expected(m, model).items():
        bad = np.nonzero(m["_" + name] != e)[0]
        assert not len(bad), "%s: %d bytes differ from the model, first at %s (payload starts at %d)" % (name, len(bad), bad[:4], pic.GUARD_BYTES)
    for k, b in before.items():
        assert np.array_equal(m["_" + k], b), "%s was written" % k
    return m


_MODELS = {}


def picture_and_model(ss, size):
    key = (tuple(ss), tuple(size))
    if key not in _MODELS:
        pic = G.TabPicture.random(9500 + 100 * size[0] + size[1], size[0], size[1], ss)
        _MODELS[key] = (pic, pic.model())
    return _MODELS[key]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("ss", G.SS, ids=SS_IDS)
def test_host_face_equals_the_model(ss, size):
    pic, model = picture_and_model(ss, size)
    check_host(pic, model)
    check_host(pic, model, filters=False)


@pytest.mark.parametrize("ss", G.SS, ids=SS_IDS)
def test_pictures_of_one_call(ss):
    """three pictures with a partition each in one call"""
    pics = [G.TabPicture.random(9600 + k, 13, 11, ss) for k in range(3)]
    ms = [p.maps() for p in pics]
    vp9.lf_tables_pictures_host(ms, 13, 11, ss)
    for p, m in zip(pics, ms):
        for name, e in G.expected(m, p.model()).items():
            assert np.array_equal(m["_" + name], e), name


# ------------------------------------------------------------------------------------------------ the single-record sweep
def _lone(ss, cols, rows, record, level=None):
    sbc, sbr = (cols + 7) >> 3, (rows + 7) >> 3
    recs = [[] for _ in range(sbc * sbr)]
    recs[0] = [record]
    return G.TabPicture(cols, rows, ss, recs, level=np.full(64, 33) if level is None else level, sharp=3)


@pytest.mark.parametrize("ss", G.SS, ids=SS_IDS)
def test_single_record_sweep(ss):
    """every bs, every valid tx, both skip_inter, every aligned pos: a lone block in the first superblock of a picture whose right or
    bottom edge cuts it at every remainder (and the uncut block).  Blocks that touch no edge of the sweep are the same for every
    picture size, so only the uncut picture runs for them."""
    n = 0
    for bs, (w8, h8) in enumerate(G.BS_WH):
        for tx in range(G.max_tx(bs) + 1):
            for skip in (0, 1):
                for r7 in range(0, 8, h8):
                    for c7 in range(0, 8, w8):
                        sizes = {(c7 + w8, r7 + h8), (16, 16)}
                        sizes |= {(c7 + k, r7 + h8) for k in range(1, w8)} | {(c7 + w8, r7 + j) for j in range(1, h8)}
                        if w8 > 1 and h8 > 1:
                            sizes.add((c7 + w8 - 1, r7 + h8 - 1))
                        for cols, rows in sorted(sizes):
                            check_host(_lone(ss, cols, rows, G.rec(r7, c7, bs, tx, skip, 9)))
                            n += 1
    assert n > 1500


# ------------------------------------------------------------------------------------------------ mask_edges by hand
def _filter_of(ss, cols, rows, record):
    pic = _lone(ss, cols, rows, record)
    m = check_host(pic)
    return m["filters"].view(G.FILTER_DT)[0]


def _masks(entries):
    m = np.zeros((2, 2, 8, 4), np.uint8)
    for (pl, d, ys, k), v in entries.items():
        for y in ys:
            m[pl, d, y, k] = v
    return m


def _level(r7, c7, h8, w8, lvl=33):
    lv = np.zeros((8, 8), np.uint8)
    lv[r7:r7 + h8, c7:c7 + w8] = lvl
    return lv.reshape(64)


HAND = [
    # the 4x4 chroma transform of an 8x8 block (tx 8x8, uvtx 4x4) on an odd row / column: no chroma edge of its own
    ("early_return_odd_row", (1, 1), 8, 8, G.rec(1, 0, 9, 1, 0, 9), (1, 0, 1, 1), {(0, 0, (1,), 1): 1, (0, 1, (1,), 1): 1}),
    ("early_return_odd_col", (1, 1), 8, 8, G.rec(0, 1, 9, 1, 0, 9), (0, 1, 1, 1), {(0, 0, (0,), 1): 2, (0, 1, (0,), 1): 2}),
    # ... on an even row and column: h and w grow by one, the 8-wide filter on the 32-sample column, the 4-wide one on the other
    ("extension", (1, 1), 8, 8, G.rec(0, 0, 9, 1, 0, 9), (0, 0, 1, 1),
     {(0, 0, (0,), 1): 1, (0, 1, (0,), 1): 1, (1, 0, (0, 1), 1): 1, (1, 0, (0, 1), 2): 2, (1, 1, (0,), 1): 3, (1, 1, (1,), 2): 3}),
    # ... in a picture of one row of blocks: row_end is set, h stays
    ("no_extension_at_row_end", (1, 1), 8, 1, G.rec(0, 0, 9, 1, 0, 9), (0, 0, 1, 1),
     {(0, 0, (0,), 1): 1, (0, 1, (0,), 1): 1, (1, 0, (0,), 1): 1, (1, 0, (0,), 2): 2, (1, 1, (0,), 1): 3}),
    # a 64x64 block with 16x16 transforms cut to 5 columns: the last chroma column edge is 8 wide, the others 16
    ("odd_width_split", (1, 1), 5, 8, G.rec(0, 0, 0, 2, 0, 9), (0, 0, 8, 8),
     {(0, 0, range(8), 0): 0x15, (0, 1, (0, 2, 4, 6), 0): 0x1F, (1, 0, range(8), 0): 0x01, (1, 0, range(8), 1): 0x10, (1, 1, (0, 4), 0): 0x1F}),
    # ... cut to 5 rows: the last chroma row edge is 8 wide
    ("odd_height_split", (1, 1), 8, 5, G.rec(0, 0, 0, 2, 0, 9), (0, 0, 8, 8),
     {(0, 0, range(5), 0): 0x55, (0, 1, (0, 2, 4), 0): 0xFF, (1, 0, range(5), 0): 0x11, (1, 1, (0,), 0): 0xFF, (1, 1, (4,), 1): 0xFF}),
    # skipped inter blocks: the outer edges only
    ("skip_32x32_tx16", (1, 1), 8, 8, G.rec(4, 4, 3, 2, 1, 9), (4, 4, 4, 4),
     {(0, 0, range(4, 8), 0): 0x10, (0, 1, (4,), 0): 0xF0, (1, 0, range(4, 8), 0): 0x10, (1, 1, (4,), 0): 0xF0}),
    ("skip_8x8_tx4", (1, 1), 8, 8, G.rec(2, 2, 9, 0, 1, 9), (2, 2, 1, 1),
     {(0, 0, (2,), 2): 4, (0, 1, (2,), 2): 4, (1, 0, (2, 3), 2): 4, (1, 1, (2,), 2): 0xC}),
    # 4:4:4: mask[1] stays empty; 4x4 transforms set the inner edges too
    ("444_tx4", (0, 0), 8, 8, G.rec(0, 4, 9, 0, 0, 9), (0, 4, 1, 1),
     {(0, 0, (0,), 1): 0x10, (0, 0, (0,), 3): 0x10, (0, 1, (0,), 1): 0x10, (0, 1, (0,), 3): 0x10}),
]


@pytest.mark.parametrize("case", HAND, ids=[h[0] for h in HAND])
def test_mask_edges_by_hand(case):
    _, ss, cols, rows, record, (r7, c7, w8, h8), entries = case
    f = _filter_of(ss, cols, rows, record)
    want = _masks(entries)
    assert np.array_equal(f["mask"], want), "mask differs at [pl, dir, y, k] = %s" % np.argwhere(f["mask"] != want)[:6].tolist()
    assert np.array_equal(f["level"], _level(r7, c7, h8, w8))


# ------------------------------------------------------------------------------------------------ malformed input
@pytest.mark.parametrize("ss", G.SS, ids=SS_IDS)
@pytest.mark.parametrize("case", G.malformed_cases(), ids=lambda c: c[0])
def test_malformed_record_is_skipped(case, ss):
    """the tables equal those of the same picture without the record"""
    _, sb, bad = case
    clean = G.TabPicture.random(9700, 13, 11, ss, level=np.arange(64) % 63 + 1)
    recs = [list(r) for r in clean.sb_records]
    recs[sb].insert(len(recs[sb]) // 2, bad)
    dirty = G.TabPicture(13, 11, ss, recs, level=clean.level, sharp=0)
    dirty.lim, dirty.mblim = clean.lim, clean.mblim
    assert not G.record_ok(bad, sb // 2, sb % 2, 13, 11)
    check_host(dirty, clean.model())


def crowded(ss):
    """2 x 1 superblocks: 150 records in the first (64 distinct 8x8 blocks, then the same blocks again with other transforms but the
    same level, so a cell's level does not depend on which record wins), a 64x64 block in the second"""
    a = [G.rec(i >> 3, i & 7, 9, 1, 0, 8 * (i & 7) + 1) for i in range(64)]
    a += [G.rec(i >> 3, i & 7, 10 + i % 3, 0, i & 1, 8 * (i & 7) + 1) for i in range(64)]
    a += [G.rec(0, 0, 9, 0, 1, 1)] * 22
    return G.TabPicture(16, 8, ss, [a, [G.rec(0, 0, 0, 3, 0, 7)]], sharp=2, seed=5)


@pytest.mark.parametrize("ss", G.SS, ids=SS_IDS)
def test_more_than_64_records_in_a_superblock(ss):
    pic = crowded(ss)
    assert len(pic.sb_records[0]) == 150
    check_host(pic)


@pytest.mark.parametrize("ss", G.SS, ids=SS_IDS)
def test_sb_first_is_read_defensively(ss):
    """a decreasing pair is an empty superblock, entries beyond nblocks are clamped; nothing outside the arrays is touched"""
    pic = G.TabPicture.random(9710, 24, 8, ss)
    n = pic.nblocks
    f = pic.sb_first
    flat = [tuple(int(v) for v in r) for r in pic.blocks]
    # superblock 0: [f1, f0) decreasing -> empty; 1: [f0, f2) -> the records of 0 and 1 (those of 0 fall outside it or not: the model knows)
    sbf = np.array([f[1], f[0], f[2], 0xFFFFFFF0], np.uint32)
    recs = [[], flat[f[0]:f[2]], flat[f[2]:n]]
    check_host(pic, pic.model(recs), sb_first=sbf)
    # nblocks below what sb_first says: the records past it do not exist
    cut = int(f[2]) + 1
    recs = [flat[f[0]:f[1]], flat[f[1]:f[2]], flat[f[2]:cut]]
    check_host(pic, pic.model(recs), nblocks=cut)
    sbf = np.array([0xFFFFFFFF, 0x80000000, 5, 2], np.uint32)
    check_host(pic, pic.model([[], [], []]), sb_first=sbf)


# ------------------------------------------------------------------------------------------------ nothing to filter
@pytest.mark.parametrize("ss", G.SS, ids=SS_IDS)
def test_empty_superblocks_and_zero_levels_give_zero_tables(ss):
    """the outputs are pre-filled with 0xA5 (TabPicture.maps) and come out all zero"""
    empty = G.TabPicture(19, 9, ss, [[] for _ in range(6)])
    zero = G.TabPicture.random(9720, 19, 9, ss, level=np.zeros(64, np.uint8))
    some = G.TabPicture.random(9721, 19, 9, ss)
    some = G.TabPicture(19, 9, ss, [r if i % 2 else [] for i, r in enumerate(some.sb_records)], level=np.full(64, 20))
    for pic, all_zero in ((empty, True), (zero, True), (some, False)):
        m = check_host(pic)
        assert (m["_tables"][:4] == G.GUARD).all()
        for name in G.OUTPUTS:
            if m.get(name) is None:
                continue
            per = len(m[name]) // pic.nsb
            zeros = [not m[name][i * per:(i + 1) * per].any() for i in range(pic.nsb)]
            assert all(zeros) if all_zero else (all(zeros[0::2]) and not any(zeros[1::2])), name


# ------------------------------------------------------------------------------------------------ refusals
def _faces():
    L = _lib.lib()
    return (lambda sh, sv, c, r, n, p: L.ffhip_vp9_lf_tables_pictures_dev(sh, sv, c, r, n, p, None),
            lambda sh, sv, c, r, n, p: L.ffhip_vp9_lf_tables_pictures_host(sh, sv, c, r, n, p))


def _arr(ms):
    return vp9._lf_tab_pics(ms, lambda a: a.ctypes.data)


@pytest.mark.parametrize("which", [0, 1], ids=["dev", "host"])
def test_invalid_arguments(which):
    """one per FFHIP_EINVAL clause, each with its text; they come before the device check, so they hold on any machine, for both faces"""
    f = _faces()[which]
    L = _lib.lib()
    v = lambda a: C.cast(a, C.c_void_p)

    def refused(text, sh, sv, c, r, n, p):
        assert f(sh, sv, c, r, n, p) == _lib.EINVAL
        msg = L.ffhip_last_error().decode()
        assert text in msg and "ffhip_vp9_lf_tables_pictures_" + ("host" if which else "dev") in msg, msg

    pic = G.TabPicture.random(9730, 13, 11, (1, 1))
    m = pic.maps()
    ok = _arr([m])
    for c, r in ((0, 11), (13, 0), (-1, 11), (8 * 1364 + 1, 11), (13, 8 * 1364 + 1)):
        refused("8x8 blocks", 1, 1, c, r, 1, v(ok))
    for sh, sv in ((2, 1), (1, -1)):
        refused("subsampling", sh, sv, 13, 11, 1, v(ok))
    for n in (0, -1):
        refused("npics", 1, 1, 13, 11, n, v(ok))
    refused("npics = 17", 1, 1, 13, 11, 17, v(ok))
    refused("npics", 1, 1, 13, 11, 1, None)
    for field in ("sb_first", "tables", "blocks"):
        a = _arr([m])
        setattr(a[0], field, None)
        refused("NULL", 1, 1, 13, 11, 1, v(a))
    for field in ("blocks", "sb_first", "tables", "filters"):
        a = _arr([m])
        setattr(a[0], field, getattr(a[0], field) + 2)
        refused("4-byte aligned", 1, 1, 13, 11, 1, v(a))
    a = _arr([m])
    a[0].level[17] = 64
    refused("level[17] = 64", 1, 1, 13, 11, 1, v(a))
    # ctables against the sub-sampling
    m2 = G.TabPicture.random(9731, 13, 11, (1, 0)).maps()
    refused("ctables present", 1, 1, 13, 11, 1, v(_arr([m2])))
    refused("ctables present", 0, 0, 13, 11, 1, v(_arr([m2])))
    refused("ctables absent", 1, 0, 13, 11, 1, v(ok))
    refused("ctables absent", 0, 1, 13, 11, 1, v(ok))
    # overlaps: two pictures that share an output; an output inside an input
    refused("overlaps another output", 1, 1, 13, 11, 2, v(_arr([m, m])))
    other = pic.maps()
    a = _arr([m, other])
    a[1].filters = a[0].tables + 4 * 1280 - 192
    refused("overlaps another output", 1, 1, 13, 11, 2, v(a))
    for field in ("blocks", "sb_first"):
        a = _arr([m, other])
        setattr(a[1], field, a[0].tables + 1280)
        refused("an input overlaps an output", 1, 1, 13, 11, 2, v(a))
    # the same call, nothing wrong with it: the host face runs; the device face gets as far as looking for a device (with one, the host
    # arrays of this test are not for it)
    import torch
    if which:
        assert f(1, 1, 13, 11, 1, v(ok)) == 0
    elif not torch.cuda.is_available():
        assert f(1, 1, 13, 11, 1, v(ok)) == _lib.ENOSYS


# ------------------------------------------------------------------------------------------------ coverage
@pytest.mark.parametrize("ss", G.SS, ids=SS_IDS)
def test_the_picture_set_covers_the_entries(ss):
    """every table-entry width in both directions and the luma inner-4 entries occur, in luma and (where chroma has tables of its own)
    in chroma; no 16-wide chroma entry on a tile's last position"""
    seen, inner, wide_last = set(), set(), 0
    for size in SIZES:
        _, (f, tabs, ctabs) = picture_and_model(ss, size)
        s, i, w = G.entry_census(tabs, ctabs, tuple(ss))
        seen, inner, wide_last = seen | s, inner | i, wide_last + w
        if ss == (0, 0):
            assert not f["mask"][:, 1].any()
    want = {(d, w) for d in (0, 1) for w in (0, 1, 2)}
    if ss != (0, 0):
        want |= {("c", d, w) for d in (0, 1) for w in (0, 1, 2)}
    assert seen == want and inner == {0, 1} and wide_last == 0
