"""CPU tier of the VP9 intra frame face (ffhip_vp9_intra_frames_dev): the record ABI, the argument refusals, the refusal of a box without
a device, ffhip_vp9_intra_block_records against a restatement of intra_recon's loops, and what the generator and the plane model
reach: every (coded mode, tx, have_left, have_top) the partition allows, the top-right rule's x + 8 > dw case, and tile columns that
change the planes."""
import ctypes as C

import numpy as np
import pytest

import vp9_intra_frame_gen as G
from ffmpeg_amd import _lib, vp9


def test_record_size_matches_the_c_struct():
    assert _lib.lib().ffhip_vp9_intra_record_size() == vp9.INTRA_REC_DTYPE.itemsize == 12
    assert C.sizeof(vp9.IntraPlane) == 40 and C.sizeof(vp9.IntraPic) == 3 * 40 + 8


_BUFS = []


def _buf(n=1 << 14):
    b = (C.c_uint64 * n)()
    _BUFS.append(b)
    return C.addressof(b)


def _pics(n=1, stride=256):
    """n frames of 64 x 64 whose planes are distinct host buffers (only the face's host checks look at them)"""
    pics = (vp9.IntraPic * n)()
    for i in range(n):
        for p in range(3):
            pics[i].plane[p] = vp9.IntraPlane(_buf(), stride, _buf(16), _buf(16), _buf(16))
    return pics


def test_invalid_arguments():
    """FFHIP_EINVAL comes before the device check: these hold on any machine"""
    f = _lib.lib().ffhip_vp9_intra_frames_dev
    E = _lib.EINVAL
    v = lambda pics: C.cast(pics, C.c_void_p)
    ok = v(_pics())
    assert f(9, 1, 1, 64, 64, 1, ok, None) == E                 # depth
    assert f(16, 1, 1, 64, 64, 1, ok, None) == E
    assert f(8, 2, 1, 64, 64, 1, ok, None) == E                 # subsampling
    assert f(8, 1, -1, 64, 64, 1, ok, None) == E
    assert f(8, 1, 1, 0, 64, 1, ok, None) == E                  # frame size
    assert f(8, 1, 1, 64, -8, 1, ok, None) == E
    assert f(8, 1, 1, 65536, 64, 1, ok, None) == E
    assert f(8, 1, 1, 64, 65536, 1, ok, None) == E
    assert f(8, 1, 1, 64, 64, 0, ok, None) == E                 # npics
    assert f(8, 1, 1, 64, 64, -1, ok, None) == E
    assert f(8, 1, 1, 64, 64, 1, None, None) == E               # NULL array
    for field in ("base", "recs", "rec_sb_start", "coeffs"):    # NULL plane pointers
        pics = _pics()
        setattr(pics[0].plane[1], field, None)
        assert f(8, 1, 1, 64, 64, 1, v(pics), None) == E, field
    pics = _pics()
    pics[0].plane[0].base += 2                                   # misaligned base (4 samples)
    assert f(8, 1, 1, 64, 64, 1, v(pics), None) == E
    pics = _pics()
    pics[0].plane[2].stride = 258                                # misaligned stride
    assert f(8, 1, 1, 64, 64, 1, v(pics), None) == E
    pics = _pics(stride=132)
    assert f(10, 1, 1, 64, 64, 1, v(pics), None) == E            # 2-byte samples: 132 is not a multiple of 8
    pics = _pics(stride=60)
    assert f(8, 1, 1, 64, 64, 1, v(pics), None) == E             # stride below the decoded width
    pics = _pics(stride=64)
    assert f(8, 1, 1, 65, 64, 1, v(pics), None) == E             # 65 wide: the decoded width is 72
    for lt in (-1, 7):
        pics = _pics()
        pics[0].log2_tile_cols = lt
        assert f(8, 1, 1, 64, 64, 1, v(pics), None) == E, lt
    pics = _pics(2)
    pics[1].plane[2].base = pics[0].plane[0].base + 256 * 63     # two planes of the call overlap
    assert f(8, 1, 1, 64, 64, 2, v(pics), None) == E
    assert b"overlap" in _lib.lib().ffhip_last_error()


@pytest.mark.skipif(_lib.lib().ffhip_device_count() > 0, reason="a HIP device is present: the refusal path is not reachable")
def test_no_device_refusals():
    L = _lib.lib()
    ok = C.cast(_pics(), C.c_void_p)
    assert L.ffhip_vp9_intra_frames_dev(8, 1, 1, 64, 64, 1, ok, None) == _lib.ENOSYS
    assert L.ffhip_vp9_intra_frames_dev(12, 0, 0, 61, 57, 1, ok, None) == _lib.ENOSYS
    assert L.ffhip_vp9_intra_frames_dev(10, 1, 0, 1, 1, 1, ok, None) == _lib.ENOSYS


def _max_tx(bs):
    w, h = G.BS_DIMS[bs]
    return 0 if bs > 9 else min(3, int(np.log2(min(w, h))) - 2)


def _uv_tx(bs, tx, ss_h, ss_v):
    w, h = G.BS_DIMS[bs]
    return min(tx, int(np.log2(min(max(4, max(w, 8) >> ss_h), max(4, max(h, 8) >> ss_v)))) - 2)


@pytest.mark.parametrize("ss", [(1, 1), (1, 0), (0, 1), (0, 0)], ids=["420", "422", "440", "444"])
def test_block_records_match_intra_recon(ss):
    """every block size and allowed tx / uvtx, blocks clipped by end_x / end_y, skip, lossless"""
    rng = np.random.default_rng(11 + ss[0] * 2 + ss[1])
    cols, rows = 21, 13
    n = 0
    for bs in range(13):
        for tx in range(_max_tx(bs) + 1):
            for row, col in ((0, 0), (4, 8), (rows - 1, cols - 1), (rows - 2, cols - 3), (8, 16)):
                for lossless in ((False, True) if tx == 0 else (False,)):
                    for p in range(3):
                        t = tx if p == 0 else _uv_tx(bs, tx, *ss)
                        mode = [int(v) for v in rng.integers(0, 10, 4)]
                        eob = [int(v) for v in rng.choice([0, 1, 2, 7, 1024], 256)]
                        skip = bool(rng.random() < 0.2)
                        want = G.block_records(p, bs, t, row, col, mode if p == 0 else mode[:1], skip, eob, lossless, cols, rows, *ss)
                        got = vp9.intra_block_records(p, bs, t, row, col, mode if p == 0 else mode[:1], skip, eob, lossless, cols, rows,
                                                      ss)
                        assert len(got) == len(want), (bs, tx, row, col, p)
                        for g, w in zip(got, want):
                            assert tuple(int(g[f]) for f in G.REC_FIELDS) == tuple(w[f] for f in G.REC_FIELDS), (bs, tx, row, col, p)
                        n += len(want)
    assert n > 1000


def test_block_records_refusals():
    L = _lib.lib()
    out = np.zeros(256, vp9.INTRA_REC_DTYPE)
    mode = np.zeros(4, np.uint8)
    eob = np.zeros(256, np.uint16)
    f = lambda *a: L.ffhip_vp9_intra_block_records(out.ctypes.data, *a)
    ok = (0, 3, 1, 0, 0, mode.ctypes.data, 0, eob.ctypes.data, 0, 16, 16, 1, 1)
    assert f(*ok) == 16
    E = _lib.EINVAL
    for i, v in [(0, 3), (0, -1), (1, 13), (1, -1), (2, 4), (2, -1), (3, 16), (3, -1), (4, 16), (4, -1), (5, None), (8, 1), (9, 0),
                 (10, 0), (9, 8193), (11, 2), (12, -1)]:
        a = list(ok)
        a[i] = v
        assert f(*a) == E, (i, v)
    a = list(ok)
    a[7] = None                                                 # no eob array: fine when skipped
    a[6] = 1
    assert f(*a) == 16
    a[6] = 0
    assert f(*a) == E
    assert f(0, 9, 2, 0, 0, mode.ctypes.data, 0, eob.ctypes.data, 0, 16, 16, 1, 1) == E      # 16x16 transform in an 8x8 block
    assert L.ffhip_vp9_intra_block_records(None, *ok) == E


def test_coverage_of_modes_availability_and_the_top_right_rule():
    """the generated frames reach every (coded mode, tx, have_left, have_top) the partition allows, the 4x4 top-right fallback
    where x + 8 > dw with have_right, and a tile start with x > 0"""
    rng = np.random.default_rng(21)
    seen, tr_clip, tile_left = set(), 0, 0
    # one superblock per tile column: every superblock's first block has neither edge
    frames = [G.IntraFrame(rng, 4096, 64, 8, 0, 0, log2_tile_cols=6) for _ in range(6)]
    frames += [G.IntraFrame(rng, 4096, 64, 8, 0, 0, log2_tile_cols=6, lossless=True) for _ in range(2)]
    frames += [G.IntraFrame(rng, 203, 141, 8, 1, 1, log2_tile_cols=1), G.IntraFrame(rng, 300, 77, 8, 0, 0, log2_tile_cols=1)]
    for fr in frames:
        for p in range(3):
            for r in fr.recs[p]:
                x, y = r["x"], r["y"]
                sbx = x // (64 >> fr.hs[p])
                ts = max(s for s in G.tile_starts(fr.sb_w, fr.log2_tile_cols) if s <= sbx)
                hl, ht = x > (ts * 64) >> fr.hs[p], y > 0
                seen.add((r["mode"], r["tx"], hl, ht))
                N = 4 if r["tx"] == 4 else 4 << r["tx"]
                if N == 4 and r["flags"] & G.HAVE_RIGHT and ht and x + 8 > fr.dw[p]:
                    tr_clip += 1
                if x > 0 and not hl:
                    tile_left += 1
    want = {(m, t, l, u) for m in range(10) for t in range(5) for l in (False, True) for u in (False, True)}
    assert want - seen == set(), sorted(want - seen)[:10]
    assert tr_clip > 0 and tile_left > 0
    fr = frames[-2]
    with_tiles, without = G.model(fr), G.model(fr, tiles=False)
    assert any((a != b).any() for a, b in zip(with_tiles, without))


@pytest.mark.parametrize("bd", (8, 10, 12))
def test_model_writes_only_records(bd):
    """samples no record covers keep their (garbage) values; covered samples are inside 0 .. maxv"""
    rng = np.random.default_rng(31 + bd)
    fr = G.IntraFrame(rng, 200, 136, bd, 1, 1, inter=True, p_intra=0.3)
    out = G.model(fr)
    for p in range(3):
        cov = np.zeros(fr.planes[p].shape, bool)
        for r in fr.recs[p]:
            N = 4 if r["tx"] == 4 else 4 << r["tx"]
            cov[r["y"]:r["y"] + N, r["x"]:r["x"] + N] = True
        assert (out[p][~cov] == fr.planes[p][~cov]).all()
        assert out[p].min() >= 0 and out[p].max() <= fr.maxv


SS4 = [(1, 1), (1, 0), (0, 1), (0, 0)]


@pytest.mark.parametrize("bd", (8, 10, 12))
@pytest.mark.parametrize("ss", SS4, ids=["420", "422", "440", "444"])
def test_plane_model_equals_the_pointer_form(bd, ss):
    """the plane-coordinate rules (model(), what the kernel implements) give the planes of the reference's own route (pointer_model():
    frame buffers with linesize padding, the overhang buffers and their copy-back, intra_pred_data under a loop filter that changes
    each finished superblock row, dst_edge / dst_inner, the top == topleft test) — odd sizes, 1, 2 and 4 tile columns, lossless
    frames, the intra holes of inter frames, and DC-heavy frames whose left edges need the bottom clamp"""
    rng = np.random.default_rng(4000 + bd * 10 + SS4.index(ss))
    frames = [(G.IntraFrame(rng, 203, 141, bd, *ss, log2_tile_cols=1), (0, 8)),
              (G.IntraFrame(rng, 77, 99, bd, *ss), (24, 40)),
              (G.IntraFrame(rng, 520, 72, bd, *ss, log2_tile_cols=2), (8, 0)),
              (G.IntraFrame(rng, 128, 64, bd, *ss, lossless=True), (0, 0)),
              (G.IntraFrame(rng, 200, 108, bd, *ss, modes=[2, 1, 8]), (0, 8)),
              (G.IntraFrame(rng, 200, 136, bd, *ss, inter=True, p_intra=0.3, log2_tile_cols=1), (16, 0))]
    clamp_left = 0
    for fr, pad in frames:
        want, got = G.model(fr), G.pointer_model(fr, pad=pad)
        for p in range(3):
            bad = np.argwhere(want[p] != got[p])
            assert not len(bad), "%dx%d plane %d: %d samples differ, first %s" % (fr.W, fr.H, p, len(bad), bad[:3].tolist())
            for r in fr.recs[p]:
                N = 4 if r["tx"] == 4 else 4 << r["tx"]
                clamp_left += r["x"] > 0 and r["y"] + N > fr.dh[p]
    assert clamp_left > 0
