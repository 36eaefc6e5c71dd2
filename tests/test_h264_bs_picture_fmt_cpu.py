"""CPU tier of the H.264 edge-parameter faces with a chroma format (ffhip_h264_edge_params_pictures_fmt_dev / _fmt_host) and of the
argument checks of ffhip_h264_deblock_pictures_fmt_dev: the record ABI, one assertion per refusal, the device-free host face against
models A and B of h264_bs_fmt_gen.py byte for byte (guard records and inputs included) at formats 0 .. 3, the existing host face's
bytes at 0 / 1, one hand-written picture per new rule, and the coverage of the picture set.

Two mutations of kernels/h264_bs_rules.h were tried by hand; each makes tests of this file fail:
 * applying the 8x8-transform skip to the horizontal chroma edges of 4:2:2 (h264bs_edge_bs ignoring c422h): the 4:2:2 entries of
   test_host_face_equals_both_models (but 1 x 1) and of test_malformed_input_gives_the_defined_output,
   test_422_8x8_transform_keeps_the_odd_horizontal_chroma_edges and test_422_intra_8x8_transform_macroblock fail;
 * adding 1 to the tc0 of 4:4:4 chroma records (h264bs_pack called with chroma = true at format 3): the 4:4:4 entries of
   test_host_face_equals_both_models and of test_malformed_input_gives_the_defined_output and
   test_444_planes_use_luma_conventions_with_their_own_qp fail."""
import ctypes as C

import numpy as np
import pytest

import h264_bs_fmt_gen as F
import h264_bs_picture_gen as G
from ffmpeg_amd import _lib, h264

E = h264.EDGE_DTYPE
EINVAL = _lib.EINVAL
H, V, HC, VC = h264.LF_H_LUMA, h264.LF_V_LUMA, h264.LF_H_CHROMA, h264.LF_V_CHROMA


def test_record_sizes_match_the_c_structs():
    L = _lib.lib()
    assert L.ffhip_h264_lf_pic_record_size() == C.sizeof(h264.LfPic) == 6 * 8
    assert L.ffhip_h264_bs_mb_record_size() == 8 and L.ffhip_h264_bs_mvf_record_size() == 12 and L.ffhip_h264_bs_slice_record_size() == 72
    assert C.sizeof(h264.BsPic) == 7 * 8 + 2 * 4                 # no record of the existing face changed
    assert h264.EDGE_CHROMA_RECORDS == (0, 4, 6, 8)


# ------------------------------------------------------------------------------------------------------------- refusals
_BUFS = []


def _buf(n=1 << 12):
    b = (C.c_uint64 * n)()
    _BUFS.append(b)
    return C.addressof(b)


def _pics(n=1):
    """n pictures of 4 x 4 macroblocks whose tables are distinct zeroed host buffers (32 KiB each: room for every format)"""
    pics = (h264.BsPic * n)()
    for i in range(n):
        for f in ("mb", "mvf", "slices", "chroma_qp", "luma", "cb", "cr"):
            setattr(pics[i], f, _buf())
        pics[i].mvf_stride, pics[i].nslices = 16, 1
    return pics


def _faces():
    L = _lib.lib()
    return (lambda fmt, w, h, fi, bd, n, p: L.ffhip_h264_edge_params_pictures_fmt_dev(fmt, w, h, fi, bd, n, p, None),
            lambda fmt, w, h, fi, bd, n, p: L.ffhip_h264_edge_params_pictures_fmt_host(fmt, w, h, fi, bd, n, p))


v = lambda pics: C.cast(pics, C.c_void_p)
HAVE_DEVICE = _lib.lib().ffhip_device_count() > 0


def accepted(which, call):
    """the arguments pass the checks: 0 from the host face, FFHIP_ENOSYS from the device face on a machine without a device; with a
    device the device face is not called at all, since these tables are host memory"""
    if which == 0 and HAVE_DEVICE:
        return
    assert call() == (0 if which else _lib.ENOSYS)


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("fmt", [1, 2, 3])
def test_invalid_arguments(which, fmt):
    """one per FFHIP_EINVAL clause of the face without a format, at every format with chroma tables; before the device check"""
    f = _faces()[which]
    ok = v(_pics())
    assert f(-1, 4, 4, 0, 0, 1, ok) == EINVAL and f(4, 4, 4, 0, 0, 1, ok) == EINVAL          # the format
    assert b"chroma_format_idc" in _lib.lib().ffhip_last_error()
    assert f(fmt, 0, 4, 0, 0, 1, ok) == EINVAL and f(fmt, 4, 0, 0, 0, 1, ok) == EINVAL
    assert f(fmt, 4097, 4, 0, 0, 1, ok) == EINVAL and f(fmt, 4, 4097, 0, 0, 1, ok) == EINVAL and f(fmt, -1, 4, 0, 0, 1, ok) == EINVAL
    for bd in (-6, 1, 18, 30, 42):
        assert f(fmt, 4, 4, 0, bd, 1, ok) == EINVAL, bd
    assert f(fmt, 4, 4, 2, 0, 1, ok) == EINVAL and f(fmt, 4, 4, -1, 0, 1, ok) == EINVAL
    assert f(fmt, 4, 4, 0, 0, 0, ok) == EINVAL and f(fmt, 4, 4, 0, 0, -1, ok) == EINVAL
    assert f(fmt, 4, 4, 0, 0, 1, None) == EINVAL
    for field in ("mb", "mvf", "slices", "luma", "cb", "cr", "chroma_qp"):                    # NULL; one of cb / cr; cb without chroma_qp
        pics = _pics()
        setattr(pics[0], field, None)
        assert f(fmt, 4, 4, 0, 0, 1, v(pics)) == EINVAL, field
    for field in ("mvf", "luma", "cb", "cr"):                                                 # misaligned
        pics = _pics()
        setattr(pics[0], field, getattr(pics[0], field) + 2)
        assert f(fmt, 4, 4, 0, 0, 1, v(pics)) == EINVAL, field
    pics = _pics()
    pics[0].mvf_stride = 15
    assert f(fmt, 4, 4, 0, 0, 1, v(pics)) == EINVAL
    pics = _pics()
    pics[0].nslices = 0
    assert f(fmt, 4, 4, 0, 0, 1, v(pics)) == EINVAL
    for field, nbytes in (("mb", 16 * 8), ("mvf", 16 * 16 * 12), ("slices", 72), ("chroma_qp", 176)):
        for out in ("luma", "cb", "cr"):
            pics = _pics(2)
            setattr(pics[1], out, getattr(pics[0], field) + nbytes - 4)
            assert f(fmt, 4, 4, 0, 0, 2, v(pics)) == EINVAL, (field, out)
            assert b"overlaps" in _lib.lib().ffhip_last_error()
    pics = _pics(3)
    pics[2].cr = pics[0].cb
    assert f(fmt, 4, 4, 0, 0, 3, v(pics)) == EINVAL
    assert b"overlaps" in _lib.lib().ffhip_last_error()


@pytest.mark.parametrize("which", [0, 1])
def test_overlap_spans_follow_the_format(which):
    """cr right behind the 16 * 4 records a 4:2:0 cb holds: no overlap at format 1, one at 4:2:2 (16 * 6) and 4:4:4 (16 * 8); behind
    16 * 6 records: an overlap at 4:4:4 alone.  An input behind cb the same way.  The host face accepts what does not overlap."""
    f = _faces()[which]
    for per, bad in ((4, (2, 3)), (6, (3,)), (8, ())):
        for fmt in (1, 2, 3):
            for field in ("cr", "mb"):
                pics = _pics()
                setattr(pics[0], field, pics[0].cb + 16 * per * 12)
                if fmt in bad:
                    assert f(fmt, 4, 4, 0, 0, 1, v(pics)) == EINVAL, (per, fmt, field)
                    assert b"overlaps" in _lib.lib().ffhip_last_error()
                else:
                    accepted(which, lambda: f(fmt, 4, 4, 0, 0, 1, v(pics)))


@pytest.mark.parametrize("which", [0, 1])
def test_format_0_does_not_look_at_the_chroma_pointers(which):
    f = _faces()[which]
    pics = _pics()
    pics[0].cb, pics[0].cr, pics[0].chroma_qp = pics[0].luma + 2, None, None                  # misaligned, over luma, without cr / chroma_qp
    accepted(which, lambda: f(0, 4, 4, 0, 0, 1, v(pics)))
    assert f(1, 4, 4, 0, 0, 1, v(pics)) == EINVAL


@pytest.mark.skipif(HAVE_DEVICE, reason="a HIP device is present: the refusal path is not reachable")
def test_no_device_refusals():
    f = _faces()[0]
    for fmt in range(4):
        assert f(fmt, 4, 4, 0, 0, 1, v(_pics())) == _lib.ENOSYS
    pics = _pics(17)
    pics[3].chroma_qp = pics[3].cb = pics[3].cr = None
    assert f(2, 4, 4, 1, 12, 17, v(pics)) == _lib.ENOSYS
    lf = _lf()
    assert _deblock(8, 2, 4, 4, 64, 32, 1, lf) == _lib.ENOSYS


# ---- the deblock face's checks (addresses are only looked at, never followed, before the device check)
def _lf(n=1, base=0x10000):
    pics = (h264.LfPic * n)()
    for i in range(n):
        for p in range(3):
            pics[i].plane[p] = base + (i * 6 + p) * 0x1000
            pics[i].edges[p] = base + (i * 6 + 3 + p) * 0x1000
    return pics


def _deblock(bd, fmt, w, h, sy, sc, n, pics):
    return _lib.lib().ffhip_h264_deblock_pictures_fmt_dev(bd, fmt, w, h, sy, sc, n, None if pics is None else v(pics), None)


def test_deblock_face_invalid_arguments():
    err = lambda: _lib.lib().ffhip_last_error()
    for bd in (7, 11, 16):
        assert _deblock(bd, 1, 4, 4, 64, 32, 1, _lf()) == EINVAL and b"bit depth" in err()
    for fmt in (-1, 4):
        assert _deblock(8, fmt, 4, 4, 64, 32, 1, _lf()) == EINVAL and b"chroma_format_idc" in err()
    for w, h in ((0, 4), (4, 0), (4097, 4), (4, 4097)):
        assert _deblock(8, 1, w, h, 64, 32, 1, _lf()) == EINVAL and b"macroblocks" in err()
    assert _deblock(8, 1, 4, 4, 64, 32, 0, _lf()) == EINVAL and _deblock(8, 1, 4, 4, 64, 32, 1, None) == EINVAL
    for p in range(3):                                           # a table without its plane
        lf = _lf()
        lf[0].plane[p] = None
        assert _deblock(8, 2, 4, 4, 64, 32, 1, lf) == EINVAL and b"NULL" in err(), p
    # alignment: (bit depth, format, plane, the plane's and the stride's, the table's)
    for bd, fmt, p, pa, ea in ((8, 1, 0, 4, 4), (8, 1, 1, 4, 4), (8, 2, 2, 4, 4), (8, 3, 1, 4, 4), (10, 1, 0, 16, 16), (10, 1, 2, 16, 16),
                               (10, 2, 0, 16, 16), (10, 2, 1, 8, 4), (10, 3, 2, 16, 16)):
        lf = _lf(2)
        lf[1].plane[p] += pa // 2
        assert _deblock(bd, fmt, 4, 4, 128, 128, 2, lf) == EINVAL and b"aligned" in err(), (bd, fmt, p)
        lf = _lf(2)
        lf[1].edges[p] += ea // 2
        assert _deblock(bd, fmt, 4, 4, 128, 128, 2, lf) == EINVAL and b"aligned" in err(), (bd, fmt, p)
        sy, sc = (128 + pa // 2, 128) if p == 0 else (128, 128 + pa // 2)
        assert _deblock(bd, fmt, 4, 4, sy, sc, 2, _lf(2)) == EINVAL and b"stride" in err(), (bd, fmt, p)
    if not HAVE_DEVICE:                                          # what is not refused, where no kernel can follow the made-up addresses
        good = _lib.ENOSYS
        lf = _lf()
        lf[0].plane[1] = lf[0].plane[2] = None                   # format 0 ignores planes 1 and 2
        lf[0].edges[1] += 2
        assert _deblock(8, 0, 4, 4, 64, 2, 1, lf) == good
        lf = _lf()
        lf[0].plane[1], lf[0].edges[1] = None, None              # a NULL table skips its plane
        assert _deblock(8, 2, 4, 4, 64, 32, 1, lf) == good
        lf = _lf()
        lf[0].plane[1] += 8
        assert _deblock(10, 2, 4, 4, 64, 40, 1, lf) == good      # 4:2:2 chroma above 8 bits: 8 bytes are enough


# ------------------------------------------------------------------------------------------------ models and the host face
def _same(a, b, what):
    bad = np.nonzero(a != b)[0]
    assert not len(bad), "%s: %d records differ, first %s: %s against %s" % (what, len(bad), bad[:3].tolist(), a[bad[0]], b[bad[0]])


def run_host(pics, pad=0, fmt=None):
    """the host face on fresh maps of the pictures: the maps; the inputs are unchanged"""
    fmt = pics[0].fmt if fmt is None else fmt
    maps = [F.fmt_maps(p, fmt, pad) for p in pics]
    before = [{k: m[k].copy() for k in ("mb", "mvf", "slices", "chroma_qp")} for m in maps]
    P0 = pics[0]
    h264.edge_params_pictures_fmt_host(maps, P0.mb_w, P0.mb_h, P0.field, P0.bd_off, fmt)
    for m, b in zip(maps, before):
        for k, a in b.items():
            assert np.array_equal(m[k].view(np.uint8), a.view(np.uint8)), "input %s was written" % k
    return maps


def check_outputs(maps, wants, what="the face against model A"):
    """every table equals the model's and the guard record on either side is untouched; a table the model does not have (format 0) is
    all guard bytes"""
    for k, (m, a) in enumerate(zip(maps, wants)):
        for t in ("luma", "cb", "cr"):
            full = m["_" + t]
            if t not in a:
                assert (full.view(np.uint8) == F.GUARD).all(), "picture %d %s: written at format 0" % (k, t)
                continue
            guard = np.full(12, F.GUARD, np.uint8).view(E)[0]
            assert full[0] == guard and full[-1] == guard, "picture %d %s: a guard record was written" % (k, t)
            assert len(full) - 2 == len(a[t]), "picture %d %s: %d records, the model has %d" % (k, t, len(full) - 2, len(a[t]))
            _same(full[1:-1], a[t], "picture %d %s (%s)" % (k, t, what))


@pytest.mark.parametrize("i", range(len(F.SET)))
def test_host_face_equals_both_models(i):
    pics = F.picture_set(i)
    maps = run_host(pics, F.set_pad(i))
    check_outputs(maps, [F.model_a_of(p) for p in pics])
    check_outputs(maps, [F.model_b(p) for p in pics], "the face against model B")


@pytest.mark.parametrize("i", [i for i, s in enumerate(F.SET) if s[0] < 2])
def test_formats_0_and_1_give_the_existing_host_face(i):
    pics = F.picture_set(i)
    fmt, pad = F.SET[i][0], F.set_pad(i)
    new = run_host(pics, pad)
    old = [F.fmt_maps(p, fmt, pad) for p in pics]
    for m in old:
        if fmt == 0:
            m["chroma_qp"] = m["cb"] = m["cr"] = None
    P0 = pics[0]
    h264.edge_params_pictures_host(old, P0.mb_w, P0.mb_h, P0.field, P0.bd_off)
    for a, b in zip(new, old):
        for t in ("_luma", "_cb", "_cr"):
            assert np.array_equal(a[t], b[t]), t


@pytest.mark.parametrize("fmt", range(4))
@pytest.mark.parametrize("field", [0, 1])
def test_malformed_input_gives_the_defined_output(fmt, field):
    pic = F.malformed(np.random.default_rng(9710 + field), fmt, field=field)
    check_outputs(run_host([pic], pad=2), [F.model_a(pic)])


def test_the_set_covers_the_new_rules():
    """counts over model A's intermediate bS: 4:2:2 odd horizontal edges of 8x8-transform macroblocks whose luma record is skipped
    while the chroma one has bS 2 (non-intra) and bS 3 (intra), and bS 1 there; vertical chroma edges with three different bS along
    them; 4:4:4 odd edges skipped by the 8x8 transform, and Cb / Cr records of one edge with different alpha"""
    n = {"422 bs2": 0, "422 bs3": 0, "422 bs1": 0, "422 vertical mixed": 0, "444 t8 skipped": 0, "444 cb != cr": 0, "444 live tc0 -1": 0}
    for i, s in enumerate(F.SET):
        for pic in F.picture_set(i):
            a = F.model_a_of(pic)
            t8 = (pic.mb["flags"].reshape(pic.mb_h, pic.mb_w) & h264.BS_MB_T8X8) != 0
            if s[0] == 2:
                for e in (1, 3):
                    lost = a["skipped"][:, :, 1, e] & t8
                    ch = a["bs_ch"][:, :, e][lost]
                    for b in (1, 2, 3):
                        n["422 bs%d" % b] += int((ch == b).any(-1).sum())
                    assert (a["bs"][:, :, 1, e][lost] == 0).all()
                for e in (0, 2):
                    bs = a["bs"][:, :, 0, e].reshape(-1, 4)
                    n["422 vertical mixed"] += sum(len(set(r.tolist())) == 3 for r in bs)
            if s[0] == 3:
                n["444 t8 skipped"] += int((a["skipped"][:, :, :, 1::2] & t8[:, :, None, None]).sum())
                live = a["cb"]["alpha"] > 0
                n["444 cb != cr"] += int((live & (a["cb"]["alpha"] != a["cr"]["alpha"])).sum())
                n["444 live tc0 -1"] += int((live[:, None] & (a["cb"]["kind"] < 4)[:, None] & (a["cb"]["tc0"] == -1)).sum())
                assert set(np.unique(a["cb"]["kind"])) <= {H, V, H + 4, V + 4}
    assert all(c >= 5 for c in n.values()), n


# ---------------------------------------------------------------------------------------------------- hand-written cases
def host(pic):
    """(luma (mb_h, mb_w, 2, 4), cb, cr (mb_h, mb_w, per)) of the host face, which must equal model A"""
    m = run_host([pic])
    check_outputs(m, [F.model_a(pic)])
    sh = (pic.mb_h, pic.mb_w)
    return m[0]["luma"].reshape(sh + (2, 4)), m[0]["cb"].reshape(sh + (-1,)), m[0]["cr"].reshape(sh + (-1,))


def rec(kind, ia=None, ib=None, bs=None, chroma=False):
    """the record of an edge of bS bs (four values) at indexA ia / indexB ib; ia None: the skipped record"""
    if ia is None:
        return np.array((0, kind, 0, 0, 0, [0] * 4 if chroma else [-1] * 4), E)
    if bs[0] == 4:
        return np.array((0, kind, G.ALPHA[ia], G.BETA[ib], 0, [0] * 4), E)
    tc = [(G.TC0[ia][b - 1] + chroma if b else (0 if chroma else -1)) for b in bs]
    return np.array((0, kind, G.ALPHA[ia], G.BETA[ib], 0, tc), E)


QC30 = int(G.chroma_qp_table(0, 0)[30])      # 29


def test_422_8x8_transform_keeps_the_odd_horizontal_chroma_edges():
    """a non-intra 8x8-transform macroblock with non-zero bits in its lower half: luma H1 / H3 are skipped records, chroma H1 carries
    nothing (no bit on either side), chroma H3 carries bS 2, and so does H2 (the bits below it)"""
    pic = F.with_fmt(G.blank(1, 2), 2)
    pic.mb["flags"][1] = h264.BS_MB_T8X8
    pic.mb["nnz"][1] = 0xFF00
    luma, cb, cr = host(pic)
    assert luma[1, 0, 1, 1] == rec(V) and luma[1, 0, 1, 3] == rec(V)
    assert luma[1, 0, 1, 2] == rec(V, 30, 30, [2] * 4)
    for tab in (cb, cr):
        assert tab[1, 0, 2] == rec(VC, chroma=True)                                  # H0: nothing on either side
        assert tab[1, 0, 2 + 1] == rec(VC, chroma=True)                              # H1: no bit above or below it
        assert tab[1, 0, 2 + 2] == rec(VC, QC30, QC30, [2] * 4, chroma=True)
        assert tab[1, 0, 2 + 3] == rec(VC, QC30, QC30, [2] * 4, chroma=True)         # H3: luma's record is the skipped one
        assert tab[1, 0, 0] == rec(HC, chroma=True) and tab[1, 0, 1] == rec(HC, QC30, QC30, [0, 0, 2, 2], chroma=True)
    pic.mb["nnz"][1] = 0x00FF                                                        # the upper half: H1 carries it, H3 does not
    luma, cb, cr = host(pic)
    assert luma[1, 0, 1, 1] == rec(V) and cb[1, 0, 3] == rec(VC, QC30, QC30, [2] * 4, chroma=True) and cb[1, 0, 5] == rec(VC, chroma=True)
    assert cb[1, 0, 2] == rec(VC, QC30, QC30, [2] * 4, chroma=True)                  # H0 against the macroblock above
    pic.mb["nnz"][1] = 0x3333                                                        # the left half, both rows of 8x8 blocks
    luma, cb, cr = host(pic)
    assert cr[1, 0, 3] == rec(VC, QC30, QC30, [2, 2, 0, 0], chroma=True) and cr[1, 0, 5] == rec(VC, QC30, QC30, [2, 2, 0, 0], chroma=True)


@pytest.mark.parametrize("field", [0, 1])
def test_422_intra_8x8_transform_macroblock(field):
    """chroma H1 / H3 at bS 3 (the normal kind, tc0'[..][2] + 1), H0 at 4 in a frame and 3 in a field picture"""
    pic = F.with_fmt(G.blank(1, 2, field), 2)
    pic.mb["flags"][1] = h264.BS_MB_T8X8 | h264.BS_MB_INTRA
    luma, cb, cr = host(pic)
    assert luma[1, 0, 1, 1] == rec(V) and luma[1, 0, 1, 3] == rec(V)
    for tab in (cb, cr):
        for k in (3, 4, 5):
            assert tab[1, 0, k] == rec(VC, QC30, QC30, [3] * 4, chroma=True)
            assert tab[1, 0, k]["tc0"].tolist() == [G.TC0[QC30][2] + 1] * 4
        assert tab[1, 0, 2] == (rec(VC, QC30, QC30, [3] * 4, chroma=True) if field else rec(VC + 4, QC30, QC30, [4] * 4, chroma=True))
        assert tab[1, 0, 0] == rec(HC, chroma=True)                                  # the picture border
        assert tab[1, 0, 1] == rec(HC, QC30, QC30, [3] * 4, chroma=True)             # x = 4: luma edge 2


def test_422_vertical_chroma_edge_has_a_tc0_per_four_lines():
    """bS 0, 1, 2, 2 down the edge x = 0 and 2, 0, 0, 1 down x = 4 (luma edge 2) land in tc0[0..3] in that order"""
    pic = F.with_fmt(G.blank(2, 1), 2)
    pic.mvf["mv"][1, 4:, 0] = [40, 0]                            # block row 1 of macroblock 1 moves: bS 1 in group 1 of its edge 0
    pic.mb["nnz"][1] = (1 << (0 + 4 * 2)) | (1 << (0 + 4 * 3)) | (1 << (2 + 4 * 0))
    pic.mvf["mv"][3, 6:, 0] = [-40, 0]                           # blocks (2, 3), (3, 3) against (1, 3): bS 1 in group 3 of edge 2
    luma, cb, cr = host(pic)
    t1, t2 = G.TC0[QC30][0] + 1, G.TC0[QC30][1] + 1
    for tab in (cb, cr):
        assert tab[0, 1, 0] == rec(HC, QC30, QC30, [0, 1, 2, 2], chroma=True) and tab[0, 1, 0]["tc0"].tolist() == [0, t1, t2, t2]
        assert tab[0, 1, 1] == rec(HC, QC30, QC30, [2, 0, 0, 1], chroma=True) and tab[0, 1, 1]["tc0"].tolist() == [t2, 0, 0, t1]
    assert luma[0, 1, 0, 0] == rec(H, 30, 30, [0, 1, 2, 2]) and luma[0, 1, 0, 2] == rec(H, 30, 30, [2, 0, 0, 1])


def test_444_planes_use_luma_conventions_with_their_own_qp():
    """Cb and Cr tables with different chroma_qp give different alpha / beta; tc0 has no + 1 and is -1 at bS 0; the odd edges of an
    8x8-transform macroblock are skipped on all three planes"""
    pic = F.with_fmt(G.blank(2, 1, qp=33), 3)
    pic.chroma_qp = np.stack([G.chroma_qp_table(4, 0), G.chroma_qp_table(-6, 0)])
    pic.mb["qp"][0] = 25
    pic.mb["flags"][1] = h264.BS_MB_T8X8
    pic.mb["nnz"][1] = 0x3333                                    # the 8x8 blocks of the left half
    luma, cb, cr = host(pic)
    cb, cr = cb.reshape(1, 2, 2, 4), cr.reshape(1, 2, 2, 4)
    t = pic.chroma_qp.astype(int)
    for c, tab in ((0, cb), (1, cr)):
        q0, q = (t[c][25] + t[c][33] + 1) >> 1, t[c][33]
        assert tab[0, 1, 0, 0] == rec(H, q0, q0, [2] * 4)                            # the luma kind at the averaged chroma qp
        assert tab[0, 1, 0, 0]["tc0"].tolist() == [G.TC0[q0][1]] * 4                 # no + 1
        assert tab[0, 1, 1, 2] == rec(V, q, q, [2, 2, 0, 0]) and tab[0, 1, 1, 2]["tc0"].tolist() == [G.TC0[q][1]] * 2 + [-1] * 2
        for d, k in ((0, H), (1, V)):
            assert tab[0, 1, d, 1] == rec(k) and tab[0, 1, d, 3] == rec(k)           # skipped by the 8x8 transform: tc0 -1
            assert luma[0, 1, d, 1] == rec(k) and luma[0, 1, d, 3] == rec(k)
        assert tab[0, 1, 0, 2] == rec(H, q, q, [2] * 4)                              # x = 8: the bits to its left
    assert cb[0, 1, 0, 0]["alpha"] != cr[0, 1, 0, 0]["alpha"] and cb[0, 1, 0, 0]["beta"] != cr[0, 1, 0, 0]["beta"]
    assert luma[0, 1, 0, 0] == rec(H, 29, 29, [2] * 4)
    pic.mb["flags"][0] = h264.BS_MB_INTRA                                            # bS 4: the luma intra kind
    luma, cb, cr = host(pic)
    q0 = (t[0][25] + t[0][33] + 1) >> 1
    assert cb.reshape(1, 2, 2, 4)[0, 1, 0, 0] == rec(H + 4, q0, q0, [4] * 4)
