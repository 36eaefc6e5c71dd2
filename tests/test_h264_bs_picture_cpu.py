"""CPU tier of the H.264 edge-parameter face (ffhip_h264_edge_params_pictures_dev / _host): the record ABI, the argument refusals, the
two models of h264_bs_picture_gen.py against each other, the device-free host face against model A byte for byte (guard records and
inputs included), one hand-written case per rule, the three tables, malformed input, and the coverage of the picture set."""
import ctypes as C

import numpy as np
import pytest

import h264_bs_picture_gen as G
from ffmpeg_amd import _lib, h264

E = h264.EDGE_DTYPE


def test_record_sizes_match_the_c_structs():
    L = _lib.lib()
    assert L.ffhip_h264_bs_mb_record_size() == h264.BS_MB_DTYPE.itemsize == 8
    assert L.ffhip_h264_bs_mvf_record_size() == h264.BS_MVF_DTYPE.itemsize == 12
    assert L.ffhip_h264_bs_slice_record_size() == h264.BS_SLICE_DTYPE.itemsize == 72
    assert C.sizeof(h264.BsPic) == 7 * 8 + 2 * 4


# ------------------------------------------------------------------------------------------------------------- refusals
_BUFS = []


def _buf(n=1 << 12):
    b = (C.c_uint64 * n)()
    _BUFS.append(b)
    return C.addressof(b)


def _pics(n=1):
    """n pictures of 4 x 4 macroblocks whose tables are distinct zeroed host buffers"""
    pics = (h264.BsPic * n)()
    for i in range(n):
        for f in ("mb", "mvf", "slices", "chroma_qp", "luma", "cb", "cr"):
            setattr(pics[i], f, _buf())
        pics[i].mvf_stride, pics[i].nslices = 16, 1
    return pics


def _faces():
    L = _lib.lib()
    return (lambda w, h, fi, bd, n, p: L.ffhip_h264_edge_params_pictures_dev(w, h, fi, bd, n, p, None),
            lambda w, h, fi, bd, n, p: L.ffhip_h264_edge_params_pictures_host(w, h, fi, bd, n, p))


@pytest.mark.parametrize("which", [0, 1])
def test_invalid_arguments(which):
    """one per FFHIP_EINVAL clause; they come before the device check, so they hold on any machine, for both faces"""
    f = _faces()[which]
    EINVAL = _lib.EINVAL
    v = lambda pics: C.cast(pics, C.c_void_p)
    ok = v(_pics())
    assert f(0, 4, 0, 0, 1, ok) == EINVAL and f(4, 0, 0, 0, 1, ok) == EINVAL                 # mb_w, mb_h outside 1..4096
    assert f(4097, 4, 0, 0, 1, ok) == EINVAL and f(4, 4097, 0, 0, 1, ok) == EINVAL and f(-1, 4, 0, 0, 1, ok) == EINVAL
    for bd in (-6, 1, 18, 30, 42):
        assert f(4, 4, 0, bd, 1, ok) == EINVAL, bd                                            # another qp_bd_offset
    assert f(4, 4, 2, 0, 1, ok) == EINVAL and f(4, 4, -1, 0, 1, ok) == EINVAL                # field
    assert f(4, 4, 0, 0, 0, ok) == EINVAL and f(4, 4, 0, 0, -1, ok) == EINVAL                # npics
    assert f(4, 4, 0, 0, 1, None) == EINVAL
    for field in ("mb", "mvf", "slices", "luma"):
        pics = _pics()
        setattr(pics[0], field, None)
        assert f(4, 4, 0, 0, 1, v(pics)) == EINVAL, field
    for field in ("cb", "cr"):                                                                # only one of cb / cr
        pics = _pics()
        setattr(pics[0], field, None)
        assert f(4, 4, 0, 0, 1, v(pics)) == EINVAL, field
    pics = _pics()
    pics[0].chroma_qp = None                                                                  # cb without chroma_qp
    assert f(4, 4, 0, 0, 1, v(pics)) == EINVAL
    for field in ("mvf", "luma", "cb", "cr"):                                                 # misaligned
        pics = _pics()
        setattr(pics[0], field, getattr(pics[0], field) + 2)
        assert f(4, 4, 0, 0, 1, v(pics)) == EINVAL, field
    pics = _pics()
    pics[0].mvf_stride = 15
    assert f(4, 4, 0, 0, 1, v(pics)) == EINVAL
    for n in (0, -3):
        pics = _pics()
        pics[0].nslices = n
        assert f(4, 4, 0, 0, 1, v(pics)) == EINVAL
    # an output table over any input, or over another output table, of the same or another picture of the call
    for field, nbytes in (("mb", 16 * 8), ("mvf", 16 * 16 * 12), ("slices", 72), ("chroma_qp", 176)):
        for out in ("luma", "cb", "cr"):
            pics = _pics(2)
            setattr(pics[1], out, getattr(pics[0], field) + nbytes - 4)       # its first dword on the input's last
            assert f(4, 4, 0, 0, 2, v(pics)) == EINVAL, (field, out)
            assert b"overlaps" in _lib.lib().ffhip_last_error()
    pics = _pics()
    pics[0].cb = pics[0].luma + 16 * 8 * 12 - 12
    assert f(4, 4, 0, 0, 1, v(pics)) == EINVAL
    pics = _pics(3)
    pics[2].cr = pics[0].cb
    assert f(4, 4, 0, 0, 3, v(pics)) == EINVAL
    assert b"overlaps" in _lib.lib().ffhip_last_error()


@pytest.mark.skipif(_lib.lib().ffhip_device_count() > 0, reason="a HIP device is present: the refusal path is not reachable")
def test_no_device_refusals():
    f = _faces()[0]
    assert f(4, 4, 0, 0, 1, C.cast(_pics(), C.c_void_p)) == _lib.ENOSYS
    pics = _pics(17)
    pics[3].chroma_qp = pics[3].cb = pics[3].cr = None                                        # optional
    assert f(4, 4, 1, 12, 17, C.cast(pics, C.c_void_p)) == _lib.ENOSYS


def test_host_face_needs_no_device_and_adjacent_tables_are_accepted():
    pics = _pics()
    pics[0].cb = pics[0].luma + 16 * 8 * 12                                                   # back to back: no overlap
    pics[0].cr = pics[0].cb + 16 * 4 * 12
    assert _faces()[1](4, 4, 0, 0, 1, C.cast(pics, C.c_void_p)) == 0


# ------------------------------------------------------------------------------------------------ models and the host face
def _same(a, b, what):
    bad = np.nonzero(a != b)[0]
    assert not len(bad), "%s: %d records differ, first %s: %s against %s" % (what, len(bad), bad[:3].tolist(), a[bad[0]], b[bad[0]])


@pytest.mark.parametrize("i", range(len(G.SET)))
def test_model_a_equals_model_b(i):
    for k, pic in enumerate(G.picture_set(i)):
        a, b = G.model_a_of(pic), G.model_b(pic)
        for t in ("luma", "cb", "cr"):
            assert (t in a) == (t in b)
            if t in a:
                _same(a[t], b[t], "%s picture %d %s (A against B)" % (G.SET[i], k, t))


def run_host(pics, pad=0):
    """the host face on fresh maps of the pictures: the maps"""
    maps = [p.maps(pad) for p in pics]
    before = [{k: m[k].copy() for k in ("mb", "mvf", "slices", "chroma_qp") if m[k] is not None} for m in maps]
    P0 = pics[0]
    h264.edge_params_pictures_host(maps, P0.mb_w, P0.mb_h, P0.field, P0.bd_off)
    for m, b in zip(maps, before):
        for k, a in b.items():
            assert np.array_equal(m[k].view(np.uint8), a.view(np.uint8)), "input %s was written" % k
    return maps


def check_outputs(pics, maps, want=None):
    """every table equals model A, and the guard record on either side is untouched"""
    guard = np.full(12, G.GUARD, np.uint8).view(E)[0]
    for k, (pic, m) in enumerate(zip(pics, maps)):
        a = want[k] if want is not None else G.model_a_of(pic)
        assert ("cb" in m) == ("cb" in a)
        for t in ("luma", "cb", "cr"):
            if t in a:
                full = m["_" + t]
                assert full[0] == guard and full[-1] == guard, "picture %d %s: a guard record was written" % (k, t)
                _same(full[1:-1], a[t], "picture %d %s (the face against model A)" % (k, t))


@pytest.mark.parametrize("i", range(len(G.SET)))
def test_host_face_equals_model_a(i):
    pics = G.picture_set(i)
    check_outputs(pics, run_host(pics, G.set_pad(i)))


def test_the_set_covers_every_branch():
    """over the picture set: each bS 0..4 in each direction (0 on an edge that is not skipped), both kinds in each plane, skipped and
    unskipped records; asserted here so that a generator change cannot empty a branch"""
    seen = {(d, b): 0 for d in range(2) for b in range(5)}
    kinds, nskip, nlive = set(), 0, 0
    for i in range(len(G.SET)):
        for pic in G.picture_set(i):
            a = G.model_a_of(pic)
            live = ~a["skipped"]
            for d in range(2):
                bs = a["bs"][:, :, d][live[:, :, d]]
                for b in range(5):
                    seen[d, b] += int((bs == b).sum())
            nskip += int(a["skipped"].sum())
            nlive += int(live.sum())
            for t in ("luma", "cb", "cr"):
                if t in a:
                    kinds |= {(t, int(k)) for k in np.unique(a[t]["kind"])}
    assert all(n >= 20 for n in seen.values()), seen
    assert nskip >= 100 and nlive >= 1000
    assert kinds == {("luma", k) for k in (0, 1, 4, 5)} | {(t, k) for t in ("cb", "cr") for k in (2, 3, 6, 7)}, kinds


def test_mixed_slice_types_follow_the_macroblock_loop():
    """q in a P slice, p in a B slice: the reference compares list 0 alone (model A), the standard's wording compares what both
    blocks predict from (model B).  Same picture 10 and vector: p through list 1 alone, q through list 0.  The face follows A."""
    pic = G.blank(2, 1)
    pic.slices = np.concatenate([pic.slices, pic.slices])
    pic.nslices = 2
    pic.slices[0]["flags"] = h264.BS_SLICE_B
    pic.mb["slice"] = [0, 1]
    pic.mvf["ref_idx"][:, :4] = [-1, 0]                          # macroblock 0: list 1 only, picture 10
    a, b = G.model_a(pic), G.model_b(pic)
    e0 = (1 * 2 + 0) * 4                                         # macroblock 1, dir 0, edge 0
    assert a["luma"][e0]["alpha"] > 0 and a["luma"][e0]["tc0"].tolist() == [G.TC0[30][0]] * 4     # bS 1
    assert b["luma"][e0]["alpha"] == 0                                                             # bS 0
    check_outputs([pic], run_host([pic]), [a])


# ---------------------------------------------------------------------------------------------------- hand-written cases
def host(pic):
    """(luma (mb_h, mb_w, 2, 4), cb, cr (mb_h, mb_w, 2, 2)) of the host face, which must equal model A"""
    m = run_host([pic])
    check_outputs([pic], m, [G.model_a(pic)])
    sh = (pic.mb_h, pic.mb_w, 2)
    return (m[0]["luma"].reshape(sh + (4,)),) + ((m[0]["cb"].reshape(sh + (2,)), m[0]["cr"].reshape(sh + (2,))) if "cb" in m[0] else ())


def rec(kind, ia=None, ib=None, bs=None, chroma=False):
    """the record of an edge of bS bs (four values) at indexA ia / indexB ib; ia None: the skipped record"""
    if ia is None:
        return np.array((0, kind, 0, 0, 0, [0] * 4 if chroma else [-1] * 4), E)
    if bs[0] == 4:
        return np.array((0, kind, G.ALPHA[ia], G.BETA[ib], 0, [0] * 4), E)
    tc = [(G.TC0[ia][b - 1] + chroma if b else (0 if chroma else -1)) for b in bs]
    return np.array((0, kind, G.ALPHA[ia], G.BETA[ib], 0, tc), E)


H, V, HC, VC = h264.LF_H_LUMA, h264.LF_V_LUMA, h264.LF_H_CHROMA, h264.LF_V_CHROMA


def test_nothing_to_filter_and_the_picture_border():
    pic = G.blank(2, 2)
    pic.mb["flags"] = h264.BS_MB_INTRA                           # every edge is live but the border ones
    luma, cb, cr = host(pic)
    assert luma[0, 0, 0, 0] == rec(H) and luma[0, 0, 1, 0] == rec(V) and luma[0, 1, 1, 0] == rec(V) and luma[1, 0, 0, 0] == rec(H)
    assert cb[0, 0, 0, 0] == rec(HC, chroma=True) and cr[0, 0, 1, 0] == rec(VC, chroma=True)
    assert luma[0, 1, 0, 0] == rec(H + 4, 30, 30, [4] * 4) and luma[1, 0, 1, 0] == rec(V + 4, 30, 30, [4] * 4)
    assert luma[0, 0, 0, 1] == rec(H, 30, 30, [3] * 4)
    pic = G.blank(2, 2)
    luma, cb, cr = host(pic)
    assert (luma[:, :, 0] == rec(H)).all() and (luma[:, :, 1] == rec(V)).all()
    assert (cb[:, :, 0] == rec(HC, chroma=True)).all() and (cr[:, :, 1] == rec(VC, chroma=True)).all()


@pytest.mark.parametrize("field", [0, 1])
def test_idc(field):
    pic = G.blank(2, 2, field)
    pic.mb["flags"] = h264.BS_MB_INTRA
    pic.slices = np.concatenate([pic.slices] * 3)
    pic.nslices = 3
    pic.slices["idc"] = [0, 1, 2]
    pic.mb["slice"] = [0, 1, 2, 2]
    luma, cb, cr = host(pic)
    assert (luma[0, 1, 0] == rec(H)).all() and (luma[0, 1, 1] == rec(V)).all() and (cb[0, 1, 0] == rec(HC, chroma=True)).all()   # idc 1
    assert luma[1, 0, 1, 0] == rec(V) and cr[1, 0, 1, 0] == rec(VC, chroma=True)     # idc 2 at a slice border (slice 0 above)
    assert luma[1, 1, 1, 0] == rec(V)                                                 # ... (slice 1 above)
    assert luma[1, 1, 0, 0] == rec(H + 4, 30, 30, [4] * 4)                            # idc 2 inside the slice
    assert luma[1, 0, 0, 1] == rec(H, 30, 30, [3] * 4)


def test_transform_8x8_odd_edges_and_chroma_edge_1():
    pic = G.blank(1, 1)
    pic.mb["flags"] = h264.BS_MB_T8X8
    pic.mb["nnz"] = 0xFFFF
    luma, cb, cr = host(pic)
    for d, k, kc in ((0, H, HC), (1, V, VC)):
        assert luma[0, 0, d, 1] == rec(k) and luma[0, 0, d, 3] == rec(k)
        assert luma[0, 0, d, 2] == rec(k, 30, 30, [2] * 4)
        assert cb[0, 0, d, 1] == rec(kc, G.chroma_qp_table(0, 0)[30], G.chroma_qp_table(0, 0)[30], [2] * 4, chroma=True)


@pytest.mark.parametrize("field", [0, 1])
def test_intra_on_a_macroblock_edge_and_inside(field):
    for who in (0, 3):                                           # the macroblock to the left / above, or q itself
        pic = G.blank(2, 2, field)
        pic.mb["flags"][who] = h264.BS_MB_INTRA
        luma, cb, cr = host(pic)
        hor = 3 if field else 4                                  # the field picture's horizontal 3
        if who == 3:
            assert luma[1, 1, 0, 0] == rec(H + 4, 30, 30, [4] * 4) and luma[1, 1, 1, 0] == rec(V + (4 if hor == 4 else 0), 30, 30, [hor] * 4)
            assert luma[1, 1, 0, 2] == rec(H, 30, 30, [3] * 4) and luma[1, 1, 1, 3] == rec(V, 30, 30, [3] * 4)
            assert cb[1, 1, 1, 0] == rec(VC + (4 if hor == 4 else 0), 29, 29, [hor] * 4, chroma=True)
        else:
            assert luma[0, 1, 0, 0] == rec(H + 4, 30, 30, [4] * 4) and luma[1, 0, 1, 0] == rec(V + (4 if hor == 4 else 0), 30, 30, [hor] * 4)
            assert luma[0, 1, 0, 1] == rec(H) and luma[1, 1, 0, 0] == rec(H)


def test_nnz_bit_on_either_side():
    pic = G.blank(2, 1)
    pic.mb["nnz"][0] = 1 << (3 + 4 * 1)                          # the block left of macroblock 1's edge 0, group 1
    pic.mb["nnz"][1] = 1 << (2 + 4 * 3)                          # block (2, 3) of macroblock 1
    luma, cb, cr = host(pic)
    assert luma[0, 1, 0, 0] == rec(H, 30, 30, [0, 2, 0, 0])                          # p side
    assert luma[0, 1, 0, 2] == rec(H, 30, 30, [0, 0, 0, 2]) and luma[0, 1, 0, 3] == rec(H, 30, 30, [0, 0, 0, 2])    # q side, then p side
    assert luma[0, 1, 1, 3] == rec(V, 30, 30, [0, 0, 2, 0]) and luma[0, 1, 1, 2] == rec(V)
    assert cb[0, 1, 0, 1] == rec(HC, 29, 29, [0, 0, 0, 2], chroma=True)
    # block (3, 1) of macroblock 0: below horizontal edge 1, above edge 2
    assert luma[0, 0, 1, 1] == rec(V, 30, 30, [0, 0, 0, 2]) and luma[0, 0, 1, 2] == rec(V, 30, 30, [0, 0, 0, 2]) and luma[0, 0, 1, 3] == rec(V)


def _two(b=False, field=0):
    """two macroblocks side by side: the edge looked at is dir 0, edge 0 of macroblock 1"""
    return G.blank(2, 1, field, b=b)


def _bs_of(pic):
    r = host(pic)[0][0, 1, 0, 0]
    return [0] * 4 if r["alpha"] == 0 else [{-1: 0, 1: 1}[int(t)] for t in r["tc0"]]      # at index 30: tc0' = 1, 1, 2


def test_same_picture_through_another_ref_idx_or_slice():
    pic = _two()
    pic.mvf["ref_idx"][:, 4:, 0] = 3                             # ref[0][3] == ref[0][0] == picture 10
    assert _bs_of(pic) == [0] * 4
    pic.mvf["ref_idx"][:, 4:, 0] = 1                             # picture 11
    assert _bs_of(pic) == [1] * 4
    pic = _two()
    pic.slices = np.concatenate([pic.slices, pic.slices])
    pic.nslices = 2
    pic.slices[1]["ref"][0][:4] = [11, 12, 10, 10]
    pic.mb["slice"] = [0, 1]
    assert _bs_of(pic) == [1] * 4                                # ref_idx 0 names picture 10 on the left and 11 on the right
    pic.mvf["ref_idx"][:, 4:, 0] = 2                             # picture 10 through the other slice's list
    assert _bs_of(pic) == [0] * 4


def test_b_blocks_crossed_and_uni_l0_against_uni_l1():
    pic = _two(b=True)
    pic.mvf["ref_idx"][:] = [0, 1]                               # pictures 10 and 11
    pic.mvf["mv"][:, :4] = [[8, 0], [-4, 4]]
    pic.mvf["mv"][:, 4:] = [[8, 0], [-4, 4]]
    assert _bs_of(pic) == [0] * 4
    pic.mvf["ref_idx"][:, 4:] = [1, 0]                           # the same two pictures, lists swapped: vectors compared crosswise
    assert _bs_of(pic) == [1] * 4
    pic.mvf["mv"][:, 4:] = [[-4, 4], [8, 0]]
    assert _bs_of(pic) == [0] * 4
    pic.mvf["mv"][1, 4] = [[-4, 4], [8, 4]]                      # group 0 alone
    pic.mvf["mv"][0, 4] = [[-4, 4], [8, 3]]
    assert _bs_of(pic) == [0, 1, 0, 0]
    pic.mvf["ref_idx"][:, 4:] = [2, 0]                           # picture 12 in place of 11
    assert _bs_of(pic) == [1] * 4
    # both blocks predict twice from picture 10: different only if the straight and the crossed pairing both are
    pic = _two(b=True)
    pic.mvf["ref_idx"][:] = [0, 3]
    pic.mvf["mv"][:, :4] = [[0, 0], [16, 0]]
    pic.mvf["mv"][:, 4:] = [[16, 0], [0, 0]]
    assert _bs_of(pic) == [0] * 4
    pic.mvf["mv"][:, 4:] = [[16, 0], [4, 0]]
    assert _bs_of(pic) == [1] * 4
    # uni-L0 against uni-L1 of one picture: the unused lists compare equal with vector (0, 0), whatever the records hold
    pic = _two(b=True)
    pic.mvf["ref_idx"][:, :4] = [0, -1]
    pic.mvf["ref_idx"][:, 4:] = [-1, 3]
    pic.mvf["mv"][:, :4] = [[5, 5], [99, 99]]
    pic.mvf["mv"][:, 4:] = [[-77, 31], [5, 5]]
    assert _bs_of(pic) == [0] * 4
    pic.mvf["mv"][3, 4, 1] = [9, 5]
    assert _bs_of(pic) == [0, 0, 0, 1]
    pic.mvf["ref_idx"][:, 4:] = [-1, 1]                          # picture 11
    assert _bs_of(pic) == [1] * 4
    pic.mvf["ref_idx"][:, 4:] = [0, 3]                           # two vectors against one
    assert _bs_of(pic) == [1] * 4


@pytest.mark.parametrize("field", [0, 1])
def test_mv_thresholds(field):
    for dx, dy, want in ((3, 0, 0), (4, 0, 1), (-3, 0, 0), (-4, 0, 1), (0, 1, 0), (0, 2, field), (0, 3, field), (0, 4, 1), (0, -2, field),
                         (0, -4, 1), (3, 1, 0)):
        pic = _two(field=field)
        pic.mvf["mv"][:, :4, 0] = [-7, 11]
        pic.mvf["mv"][:, 4:, 0] = [-7 + dx, 11 + dy]
        assert _bs_of(pic) == [want] * 4, (dx, dy)


def test_qp_average_across_an_i_pcm_neighbour():
    pic = G.blank(2, 1, qp=33)
    pic.mb["flags"][0], pic.mb["qp"][0] = h264.BS_MB_INTRA, 0    # I_PCM
    pic.chroma_qp = np.stack([G.chroma_qp_table(2, 0), G.chroma_qp_table(-3, 0)])
    luma, cb, cr = host(pic)
    assert luma[0, 1, 0, 0] == rec(H + 4, 17, 17, [4] * 4)       # (0 + 33 + 1) >> 1
    assert luma[0, 0, 0, 1] == rec(H, 0, 0, [3] * 4) and luma[0, 0, 0, 1]["alpha"] == 0
    t = pic.chroma_qp.astype(int)
    for c, tab in ((0, cb), (1, cr)):                            # different Cb / Cr tables
        q = (t[c][0] + t[c][33] + 1) >> 1
        assert tab[0, 1, 0, 0] == rec(HC + 4, q, q, [4] * 4, chroma=True)
    assert cb[0, 1, 0, 0] != cr[0, 1, 0, 0]


@pytest.mark.parametrize("bd_off", [0, 6, 12, 24, 36])
def test_index_clipping_with_offsets(bd_off):
    for qp, ao, bo in ((5, -12, 12), (5, 12, -12), (48, 12, -12), (48, -12, 12), (0, -12, -12), (51, 12, 12), (26, 0, 0)):
        pic = G.blank(1, 1, bd_off=bd_off, qp=qp)
        pic.mb["flags"] = h264.BS_MB_INTRA
        pic.slices["alpha_c0_offset"], pic.slices["beta_offset"] = ao, bo
        luma, cb, cr = host(pic)
        ia, ib = min(max(qp + ao, 0), 51), min(max(qp + bo, 0), 51)
        assert luma[0, 0, 0, 1] == rec(H, ia, ib, [3] * 4), (qp, ao, bo)
        qc = int(G.chroma_qp_table(0, bd_off)[qp + bd_off]) - bd_off
        assert cb[0, 0, 1, 1] == rec(VC, min(max(qc + ao, 0), 51), min(max(qc + bo, 0), 51), [3] * 4, chroma=True)


def test_table_pins():
    """the three tables, read back through the face: row 0 intra (bS 3 inside), row 1 non-zero bits (2), row 2 motion (1); macroblock
    i has qp i"""
    assert G.ALPHA[16:] == [4, 4, 5, 6, 7, 8, 9, 10, 12, 13, 15, 17, 20, 22, 25, 28, 32, 36, 40, 45, 50, 56, 63, 71, 80, 90, 101, 113, 127, 144,
                            162, 182, 203, 226, 255, 255] and not any(G.ALPHA[:16])
    assert G.BETA[16:] == [2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13, 14, 14, 15, 15, 16, 16, 17, 17,
                           18, 18] and not any(G.BETA[:16])
    pic = G.blank(52, 3, chroma=False)
    pic.mb["qp"] = np.tile(np.arange(52), 3)
    pic.mb["flags"][:52] = h264.BS_MB_INTRA
    pic.mb["nnz"][52:104] = 0xFFFF
    pic.mvf["mv"][8:, 1::2, 0] = [40, 0]
    luma = host(pic)[0]
    for name, got, want in (("alpha", luma[0, :, 0, 1]["alpha"], G.ALPHA), ("beta", luma[0, :, 0, 1]["beta"], G.BETA),
                            ("tc0 bS 3", luma[0, :, 0, 1]["tc0"][:, 0], [t[2] for t in G.TC0]),
                            ("tc0 bS 2", luma[1, :, 0, 1]["tc0"][:, 2], [t[1] for t in G.TC0]),
                            ("tc0 bS 1", luma[2, :, 0, 1]["tc0"][:, 3], [t[0] for t in G.TC0])):
        assert got.tolist() == list(want), name
        assert all(a <= b for a, b in zip(want, want[1:])), name + " decreases"
    assert (G.ALPHA[51], G.BETA[51], G.TC0[51]) == (255, 18, (13, 17, 25))
    assert (luma[1, :, 0, 1]["alpha"] == luma[0, :, 0, 1]["alpha"]).all() and (luma[2, :, 1, 1]["alpha"] == 0).all()


@pytest.mark.parametrize("field", [0, 1])
def test_malformed_input_gives_the_defined_output(field):
    """slice >= nslices, ref_idx out of range, num_ref 33, an idc above 2, a qp above 87: model A's bytes, and nothing outside the maps
    is read (the tables are exactly as large as the geometry says; the stand-alone sanitizer program runs the same picture)"""
    pic = G.malformed(np.random.default_rng(9410 + field), field=field)
    a = G.model_a(pic)
    assert (a["skipped"][pic.mb["slice"].reshape(pic.mb_h, pic.mb_w) >= pic.nslices]).all()
    check_outputs([pic], run_host([pic], pad=2), [a])
    # an out-of-range ref_idx differs from every picture and from another such one; an unused list equals another unused one
    pic = _two(b=True)
    pic.mvf["ref_idx"][:] = [4, -1]                              # num_ref is 4
    assert _bs_of(pic) == [1] * 4
    pic.mvf["ref_idx"][:] = [0, 40]
    assert _bs_of(pic) == [1] * 4
    pic.mvf["ref_idx"][:] = [0, -5]
    assert _bs_of(pic) == [0] * 4
    pic.mb["slice"][0] = 9                                       # p without a slice: no reference resolves
    assert _bs_of(pic) == [1] * 4
