"""CPU tier of the HEVC boundary-strength face (ffhip_hevc_boundary_strengths_pictures_dev / _host, ffhip_hevc_bs_mark_tu): the
record ABI, the argument refusals, the refusal of a box without a device, the two models of hevc_bs_picture_gen.py against each
other, the device-free host face byte for byte against model A, hand-written cases for every rule, the defined results of malformed
input, the guard bytes, and the coverage of the generated set."""
import ctypes as C

import numpy as np
import pytest

import hevc_bs_picture_gen as G
from ffmpeg_amd import _lib, hevc

GUARD = 0x5A


def test_record_sizes_match_the_c_structs():
    L = _lib.lib()
    assert L.ffhip_hevc_bs_mvf_record_size() == hevc.BS_MVF_DTYPE.itemsize == 12
    assert L.ffhip_hevc_bs_slice_record_size() == hevc.BS_SLICE_DTYPE.itemsize == 36
    assert C.sizeof(hevc.BsPic) == 7 * 8 + 4 * 4 + 8


_BUFS = []


def _buf(n=1 << 12):
    b = (C.c_uint64 * n)()
    _BUFS.append(b)
    return C.addressof(b)


def _pics(n=1):
    """n pictures of 64 x 64 whose maps are distinct host buffers"""
    pics = (hevc.BsPic * n)()
    for i in range(n):
        for f in ("mvf", "tu", "ctb_slice", "ctb_tile", "slices", "bs_ver", "bs_hor"):
            setattr(pics[i], f, _buf())
        pics[i].mvf_stride = pics[i].tu_stride = pics[i].bs_stride = 16
        pics[i].nslices = 1
    return pics


def _faces():
    L = _lib.lib()
    return (lambda w, h, lc, n, p: L.ffhip_hevc_boundary_strengths_pictures_dev(w, h, lc, n, p, None),
            lambda w, h, lc, n, p: L.ffhip_hevc_boundary_strengths_pictures_host(w, h, lc, n, p))


@pytest.mark.parametrize("which", [0, 1])
def test_invalid_arguments(which):
    """FFHIP_EINVAL comes before the device check: these hold on any machine, for both faces"""
    f = _faces()[which]
    E = _lib.EINVAL
    v = lambda pics: C.cast(pics, C.c_void_p)
    ok = v(_pics())
    assert f(64, 64, 3, 1, ok) == E and f(64, 64, 7, 1, ok) == E          # CTB size
    assert f(60, 64, 5, 1, ok) == E and f(64, 0, 5, 1, ok) == E           # picture size
    assert f(65536, 64, 5, 1, ok) == E and f(64, 65540, 5, 1, ok) == E
    assert f(64, 64, 5, 0, ok) == E and f(64, 64, 5, -1, ok) == E         # npics
    assert f(64, 64, 5, 1, None) == E
    for field in ("mvf", "tu", "ctb_slice", "slices", "bs_ver", "bs_hor"):
        pics = _pics()
        setattr(pics[0], field, None)
        assert f(64, 64, 5, 1, v(pics)) == E, field
    for field in ("mvf_stride", "tu_stride", "bs_stride"):
        pics = _pics()
        setattr(pics[0], field, 15)                                        # below width / 4
        assert f(64, 64, 5, 1, v(pics)) == E, field
    for n in (0, -3):
        pics = _pics()
        pics[0].nslices = n
        assert f(64, 64, 5, 1, v(pics)) == E
    pics = _pics()
    pics[0].mvf += 2                                                       # records are read as dwords
    assert f(64, 64, 5, 1, v(pics)) == E
    # an output map over any input map, or over another output map, of the same or another picture of the call
    for field, nbytes in (("mvf", 16 * 16 * 12), ("tu", 256), ("ctb_slice", 8), ("ctb_tile", 8), ("slices", 36)):
        for out in ("bs_ver", "bs_hor"):
            pics = _pics(2)
            setattr(pics[1], out, getattr(pics[0], field) + nbytes - 1)    # its first byte on the input's last
            assert f(64, 64, 5, 2, v(pics)) == E, (field, out)
            assert b"overlaps" in _lib.lib().ffhip_last_error()
    pics = _pics()
    pics[0].bs_hor = pics[0].bs_ver + 255
    assert f(64, 64, 5, 1, v(pics)) == E
    pics = _pics(3)
    pics[2].bs_ver = pics[0].bs_hor
    assert f(64, 64, 5, 3, v(pics)) == E
    assert b"overlaps" in _lib.lib().ffhip_last_error()


@pytest.mark.skipif(_lib.lib().ffhip_device_count() > 0, reason="a HIP device is present: the refusal path is not reachable")
def test_no_device_refusals():
    f = _faces()[0]
    assert f(64, 64, 5, 1, C.cast(_pics(), C.c_void_p)) == _lib.ENOSYS
    pics = _pics(17)
    pics[3].ctb_tile = None                                                # optional
    assert f(64, 64, 4, 17, C.cast(pics, C.c_void_p)) == _lib.ENOSYS
    assert f(64, 64, 6, 1, C.cast(_pics(), C.c_void_p)) == _lib.ENOSYS


def test_host_face_needs_no_device_and_adjacent_maps_are_accepted():
    pics = _pics()
    pics[0].bs_hor = pics[0].bs_ver + 256                                  # back to back: no overlap
    assert _faces()[1](64, 64, 5, 1, C.cast(pics, C.c_void_p)) == 0


def test_mark_tu_equals_a_numpy_restatement():
    rng = np.random.default_rng(9000)
    got = np.zeros((24, 40), np.uint8)
    want = np.zeros_like(got)
    for _ in range(200):
        log2 = int(rng.integers(2, 6))
        n = 1 << (log2 - 2)
        x4, y4 = int(rng.integers(0, 40 - n + 1)), int(rng.integers(0, 24 - n + 1))
        cbf = int(rng.integers(0, 2))
        hevc.bs_mark_tu(got, 4 * x4, 4 * y4, log2, cbf)
        want[y4:y4 + n, x4] |= 1
        want[y4, x4:x4 + n] |= 2
        if cbf:
            want[y4:y4 + n, x4:x4 + n] |= 4
    assert np.array_equal(got, want) and {1, 2, 3, 4, 5, 6, 7} <= set(got.ravel().tolist())
    hevc.bs_mark_tu(got, 0, 0, 6, 1)                                       # no luma TU of 64: nothing is marked
    hevc.bs_mark_tu(got, 2, 0, 2, 1)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("i", range(len(G.SET)))
def test_model_a_equals_model_b(i):
    for k, pic in enumerate(G.picture_set(i)):
        av, ah, _, _ = G.model_a_of(pic)
        bv, bh = G.model_b(pic)
        assert np.array_equal(av, bv), (G.SET[i], k, np.argwhere(av != bv)[:4].tolist())
        assert np.array_equal(ah, bh), (G.SET[i], k, np.argwhere(ah != bh)[:4].tolist())


def check_outputs(pics, maps, pad):
    """every picture's maps equal model A inside w4 x h4, and the guard rows and the stride padding are untouched"""
    for k, (pic, m) in enumerate(zip(pics, maps)):
        av, ah, _, _ = G.model_a_of(pic)
        for name, full, want in (("bs_ver", m["_ver"], av), ("bs_hor", m["_hor"], ah)):
            exp = np.full_like(full, GUARD)
            exp[1:-1, :pic.w4] = want
            bad = np.argwhere(full != exp)
            assert not len(bad), "picture %d %s: %d mismatches, first (row, col) %s" % (k, name, len(bad), (bad[:3] - [1, 0]).tolist())


@pytest.mark.parametrize("i", range(len(G.SET)))
def test_host_face_equals_model_a(i):
    """one call per entry of the set: npics 1, 3 and 17 occur, as do all three CTB sizes and sizes that are not CTB multiples"""
    W, H, lc = G.SET[i][:3]
    pics = G.picture_set(i)
    pad = (0, 3, 5)[i % 3]
    maps = [p.maps(pad=pad, guard=GUARD) for p in pics]
    inputs = [(m["mvf"].copy(), m["tu"].copy()) for m in maps]
    hevc.boundary_strengths_pictures_host(maps, W, H, lc)
    check_outputs(pics, maps, pad)
    for m, (mvf, tu) in zip(maps, inputs):
        assert np.array_equal(m["mvf"], mvf) and np.array_equal(m["tu"], tu)


def test_set_covers_the_sizes_the_issue_names():
    assert {s[2] for s in G.SET} == {4, 5, 6} and {s[5] for s in G.SET} >= {1, 3, 17}
    assert (8, 8) in {s[:2] for s in G.SET} and (1920, 1080) in {s[:2] for s in G.SET}
    assert any(s[0] % (1 << s[2]) and s[1] % (1 << s[2]) for s in G.SET)
    parts = set()
    for i in range(len(G.SET)):
        for p in G.picture_set(i):
            parts |= p.parts
    assert parts == set(G.PARTS)


def test_every_outcome_class_occurs_on_50_segments():
    """the coverage condition: over the generated set, by model A alone"""
    n = np.zeros(19, np.int64)
    for i in range(len(G.SET)):
        for pic in G.picture_set(i):
            _, _, cv, ch = G.model_a_of(pic)
            n += np.bincount(cv.ravel(), minlength=19) + np.bincount(ch.ravel(), minlength=19)
    classes = {"bS 2": n[G.CLS_INTRA], "bS 1 by cbf": n[G.CLS_CBF], "bS 1 by different slots": n[G.CLS_SLOTS],
               "bS 1 by MV distance": n[G.CLS_MV], "bS 0 by equal motion": n[G.CLS_EQUAL],
               "bi, one picture four times: 0": n[G.CLS_BI1_0], "bi, one picture four times: 1": n[G.CLS_BI1_1],
               "bi, lists straight: 0": n[G.CLS_BI2_0], "bi, lists straight: 1": n[G.CLS_BI2_1],
               "bi, lists crossed": n[G.CLS_BI3_0] + n[G.CLS_BI3_1], "suppressed by slice": n[G.CLS_SLICE],
               "suppressed by tile": n[G.CLS_TILE], "suppressed by a disabled slice": n[G.CLS_DISABLED]}
    print({k: int(v) for k, v in classes.items()})
    assert not {k: int(v) for k, v in classes.items() if v < 50}
    assert n[G.CLS_BAD_SLICE] == 0                                         # the generator makes well-formed pictures


# ================================================================================================================================
# hand-written cases: two units, p = unit 3 and q = unit 4 of row (column) 0 of a 32 x 8 (8 x 32) picture with 16-sample CTBs, so
# that p and q lie in different CTBs; every other unit is intra with no TU edge marked
# ================================================================================================================================
def _slices():
    s = np.zeros(2, hevc.BS_SLICE_DTYPE)
    s[0]["ref"][0][:4], s[0]["ref"][1][:4], s[0]["num_ref"], s[0]["flags"] = [0, 1, 2, 0], [1, 0, 2, 2], [4, 4], hevc.BS_SLICE_ACROSS
    s[1]["ref"][0][:2], s[1]["ref"][1][:1], s[1]["num_ref"], s[1]["flags"] = [2, 0], [0], [2, 1], hevc.BS_SLICE_ACROSS
    return s


def U(pred=0, ref=(0, 0), mv0=(0, 0), mv1=(0, 0), tu=0):
    r = np.zeros((), hevc.BS_MVF_DTYPE)
    r["pred_flag"], r["ref_idx"], r["mv"] = pred, ref, (mv0, mv1)
    return r, tu


def two_units(p, q, want, ctb_slice=(0, 0), ctb_tile=(0, 0), across_tiles=1, slices=None):
    """the segment between p and q is `want` in both directions, by the host face and by model A; everything else is 0"""
    slices = _slices() if slices is None else slices
    for d in range(2):
        shape = (2, 8) if d == 0 else (8, 2)
        mvf, tu = np.zeros(shape, hevc.BS_MVF_DTYPE), np.zeros(shape, np.uint8)
        at = lambda k: (0, k) if d == 0 else (k, 0)
        mvf[at(3)], mvf[at(4)] = p[0], q[0]
        tu[at(3)] = p[1] & 4                                   # of p only its cbf matters
        tu[at(4)] = (q[1] & 4) | ((1 << d) if q[1] & 1 else 0)             # bit 0 of the case: q's side towards p is a TU edge
        cs, ct = np.array(ctb_slice, np.uint16), np.array(ctb_tile, np.uint16)
        ver, hor = np.full(shape, GUARD, np.uint8), np.full(shape, GUARD, np.uint8)
        m = dict(mvf=mvf, tu=tu, ctb_slice=cs, ctb_tile=ct, slices=slices, bs_ver=ver, bs_hor=hor, mvf_stride=shape[1], tu_stride=shape[1],
                 bs_stride=shape[1], nslices=len(slices), loop_filter_across_tiles=across_tiles)
        W, H = shape[1] * 4, shape[0] * 4
        hevc.boundary_strengths_pictures_host([m], W, H, 4)
        exp = [np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)]
        exp[d][at(4)] = want
        assert np.array_equal(ver, exp[0]) and np.array_equal(hor, exp[1]), (d, ver.tolist(), hor.tolist())
        av, ah, _, _ = G.model_a(mvf, tu, cs, ct, slices, across_tiles, 4)
        assert np.array_equal(av, exp[0]) and np.array_equal(ah, exp[1]), ("model A", d)


EDGE, CBF = 1, 4
A, B = (10, -6), (-30, 17)


def test_rule_4_intra_on_a_tu_edge():
    two_units(U(0), U(1, tu=EDGE), 2)
    two_units(U(1), U(0, tu=EDGE), 2)
    two_units(U(0), U(0, tu=EDGE), 2)
    two_units(U(0), U(0), 0)                                               # inside one intra TU


def test_rule_5_cbf_on_a_tu_edge():
    two_units(U(1, mv0=A, tu=CBF), U(1, mv0=A, tu=EDGE), 1)
    two_units(U(1, mv0=A), U(1, mv0=A, tu=EDGE | CBF), 1)
    two_units(U(1, mv0=A), U(1, mv0=A, tu=EDGE), 0)
    two_units(U(1, mv0=A, tu=CBF), U(1, mv0=A, tu=CBF), 0)                 # cbf without a TU edge: the motion rule, equal motion


def test_rule_2_the_slice_of_q_decides_disabling():
    s = _slices()
    s[1]["flags"] |= hevc.BS_SLICE_DEBLOCK_OFF
    two_units(U(0), U(0, tu=EDGE), 0, ctb_slice=(0, 1), slices=s)          # q's slice disabled
    two_units(U(0), U(0, tu=EDGE), 2, ctb_slice=(1, 0), slices=s)          # p's slice disabled, q's not
    two_units(U(0), U(0, tu=EDGE), 0, ctb_slice=(1, 1), slices=s)


def test_rule_3_slices_and_tiles():
    s = _slices()
    s[1]["flags"] = 0                                                      # slice 1: not across slices
    two_units(U(0), U(0, tu=EDGE), 0, ctb_slice=(0, 1), slices=s)          # q's slice forbids it
    two_units(U(0), U(0, tu=EDGE), 2, ctb_slice=(1, 0), slices=s)          # p's would, q's decides
    two_units(U(0), U(0, tu=EDGE), 2, ctb_slice=(1, 1), slices=s)          # the same slice
    two_units(U(0), U(0, tu=EDGE), 0, ctb_tile=(0, 1), across_tiles=0)
    two_units(U(0), U(0, tu=EDGE), 2, ctb_tile=(0, 1), across_tiles=1)
    two_units(U(0), U(0, tu=EDGE), 2, ctb_tile=(3, 3), across_tiles=0)
    two_units(U(1, mv0=A), U(1, mv0=B), 0, ctb_tile=(0, 1), across_tiles=0)   # the motion rule is suppressed too


def test_rule_6_one_side_intra_without_a_tu_edge():
    two_units(U(0), U(1, mv0=A), 2)
    two_units(U(2, mv1=A), U(0), 2)


def test_rule_6_uni_predicted():
    # slot 0 is L0 ref_idx 0 and 3, and L1 ref_idx 1; slot 1 is L0 ref_idx 1 and L1 ref_idx 0
    two_units(U(1, (3, 0), mv0=A), U(1, (0, 0), mv0=A), 0)                 # the same slot under two ref_idx
    two_units(U(1, (3, 0), mv0=(13, -6)), U(1, (0, 0), mv0=A), 0)          # 3 apart
    two_units(U(1, (3, 0), mv0=(14, -6)), U(1, (0, 0), mv0=A), 1)          # 4 apart in x
    two_units(U(1, (3, 0), mv0=(6, -6)), U(1, (0, 0), mv0=A), 1)           # -4 in x
    two_units(U(1, (3, 0), mv0=(10, -2)), U(1, (0, 0), mv0=A), 1)          # 4 apart in y
    two_units(U(1, (3, 0), mv0=(13, -9)), U(1, (0, 0), mv0=A), 0)          # 3 and 3
    two_units(U(2, (0, 0), mv1=A, mv0=B), U(1, (1, 0), mv0=A, mv1=(99, 99)), 0)   # slot 1 from L1 and from L0: each side's one MV
    two_units(U(2, (0, 0), mv1=B), U(1, (1, 0), mv0=A), 1)
    two_units(U(1, (1, 0), mv0=A), U(1, (0, 0), mv0=A), 1)                 # slots 1 and 0
    two_units(U(1, (0, 99), mv0=A), U(1, (0, -7), mv0=A), 0)               # the unused list's ref_idx is not read
    # across slices: slice 1 has L0 = [2, 0]
    two_units(U(1, (0, 0), mv0=A), U(1, (0, 0), mv0=A), 1, ctb_slice=(1, 0))    # ref_idx 0 is slot 2 there, slot 0 here
    two_units(U(1, (1, 0), mv0=A), U(1, (0, 0), mv0=A), 0, ctb_slice=(1, 0))    # ref_idx 1 there is slot 0
    two_units(U(1, (0, 0), mv0=A), U(1, (1, 0), mv0=A), 0, ctb_slice=(0, 1))    # q in slice 1: its ref_idx 1 is slot 0


def test_rule_6_bi_against_uni():
    two_units(U(3, (0, 0), A, A), U(1, (0, 0), A), 1)
    two_units(U(2, (0, 0), A, A), U(3, (0, 0), A, A), 1)


def test_rule_6_bi_one_picture_in_all_four():
    q = U(3, (0, 1), A, B)                                                 # slot 0 twice
    two_units(U(3, (3, 1), A, B), q, 0)
    two_units(U(3, (3, 1), B, A), q, 0)                                    # crossed MVs match
    two_units(U(3, (3, 1), (14, -6), B), q, 1)                             # neither pairing matches
    two_units(U(3, (3, 1), A, A), q, 1)
    two_units(U(3, (3, 1), (13, -6), (-30, 20)), q, 0)                     # straight, 3 apart
    two_units(U(3, (3, 1), (-27, 17), (10, -9)), q, 0)                     # crossed, 3 apart


def test_rule_6_bi_lists_straight():
    q = U(3, (0, 0), A, B)                                                 # slots 0, 1
    two_units(U(3, (3, 0), A, B), q, 0)
    two_units(U(3, (3, 0), A, (-30, 21)), q, 1)
    two_units(U(3, (3, 0), (6, -6), B), q, 1)
    two_units(U(3, (3, 0), B, A), q, 1)                                    # crossed MVs do not count here


def test_rule_6_bi_lists_crossed():
    q = U(3, (0, 0), A, B)                                                 # slots 0, 1
    two_units(U(3, (1, 1), B, A), q, 0)                                    # p: slots 1, 0
    two_units(U(3, (1, 1), (-30, 14), (10, -3)), q, 0)
    two_units(U(3, (1, 1), A, B), q, 1)
    two_units(U(3, (1, 1), B, (14, -6)), q, 1)


def test_rule_6_bi_other_pictures():
    two_units(U(3, (0, 2), A, B), U(3, (0, 0), A, B), 1)                   # p: slots 0, 2; q: 0, 1
    two_units(U(3, (2, 2), A, B), U(3, (0, 0), A, B), 1)                   # p: 2, 2
    two_units(U(3, (0, 1), A, B), U(3, (0, 0), A, B), 1)                   # p: 0, 0; q: 0, 1


def test_malformed_input_has_defined_results():
    two_units(U(0), U(0, tu=EDGE), 0, ctb_slice=(0, 5))                    # q's slice index out of range
    two_units(U(1, mv0=A), U(1, mv0=B), 0, ctb_slice=(0, 65535))
    two_units(U(0), U(0, tu=EDGE), 2, ctb_slice=(5, 0))                    # p's is, q's slice allows crossing
    two_units(U(1, mv0=A), U(1, mv0=A), 1, ctb_slice=(5, 0))               # p has no resolvable reference
    s = _slices()
    s[0]["flags"] = 0
    two_units(U(1, mv0=A), U(1, mv0=A), 0, ctb_slice=(5, 0), slices=s)     # different slices, not across
    two_units(U(1, (4, 0), mv0=A), U(1, (4, 0), mv0=A), 1)                 # ref_idx == num_ref on both sides: two different pictures
    two_units(U(1, (-1, 0), mv0=A), U(1, (0, 0), mv0=A), 1)
    two_units(U(1, (16, 0), mv0=A), U(1, (0, 0), mv0=A), 1)
    two_units(U(3, (0, 100), A, B), U(3, (0, 0), A, B), 1)
    two_units(U(3, (4, 4), A, B), U(3, (4, 4), A, B), 1)
    s = _slices()
    s[0]["num_ref"][0] = 17
    two_units(U(1, (0, 0), mv0=A), U(1, (0, 0), mv0=A), 1, slices=s)       # num_ref > 16
    two_units(U(7, mv0=A), U(1, mv0=A, tu=EDGE), 2)                        # pred_flag 7 counts as intra
    two_units(U(4, mv0=A), U(1, mv0=A), 2)
    two_units(U(255), U(200), 0)


def test_guard_bytes_around_the_maps_stay_untouched():
    """one buffer holds guard | bs_ver | guard | bs_hor | guard with nothing in between"""
    pic = G.picture_set(5)[0]
    m = pic.maps(pad=0)
    n = pic.w4 * pic.h4
    buf = np.full(3 * 64 + 2 * n, GUARD, np.uint8)
    m["bs_ver"], m["bs_hor"] = buf[64:64 + n], buf[128 + n:128 + 2 * n]
    hevc.boundary_strengths_pictures_host([m], pic.W, pic.H, pic.log2_ctb)
    av, ah, _, _ = G.model_a_of(pic)
    assert np.array_equal(buf[64:64 + n].reshape(pic.h4, pic.w4), av) and np.array_equal(buf[128 + n:].reshape(-1)[:n].reshape(pic.h4, pic.w4), ah)
    assert (buf[:64] == GUARD).all() and (buf[64 + n:128 + n] == GUARD).all() and (buf[128 + 2 * n:] == GUARD).all()
