"""CPU tier of the _fmt faces of the H.264 whole-picture residual (ffhip_h264_residual_pictures_fmt_host, and the argument checks of
ffhip_h264_residual_pictures_fmt_dev): the host face byte for byte against the models of h264_fmt_picture_gen.py at 4:2:2 and 4:4:4
(poisoned stride padding and guard rows, guarded inputs), against ffhip_h264_residual_pictures_host at 4:2:0 and monochrome, the
coverage of the sets, hand-written cases for the rules the formats add, and every refusal with the format's plane sizes."""
import ctypes as C

import numpy as np
import pytest

import h264_fmt_picture_gen as F
import h264_res_picture_gen as GR
import test_h264_res_picture_cpu as T
from ffmpeg_amd import _lib, h264

EINVAL, ENOSYS = _lib.EINVAL, _lib.ENOSYS


def test_records_keep_their_sizes_and_the_new_fields_mirror_the_c_struct():
    L = _lib.lib()
    assert L.ffhip_h264_res_mb_record_size() == h264.RES_MB_DTYPE.itemsize == h264.RES_MB_FMT_DTYPE.itemsize == 16
    assert L.ffhip_h264_res_pic_record_size() == C.sizeof(h264.ResPic) == 80
    f, g = h264.RES_MB_FMT_DTYPE.fields, h264.RES_MB_DTYPE.fields
    assert f["chroma_lo422"][1] == g["pad"][1] == 6 and f["pad"][1] == 7              # the byte that was pad[0]
    assert f["nnz444"][1] == f["qmul"][1] == g["qmul"][1] == 8 and f["nnz444"][0].base == np.uint32
    for k in ("coeff_offset", "chroma", "chroma_dc", "qmul"):
        assert f[k][:2] == g[k][:2]


def run_host(pics, fmt, pad=0, face=h264.residual_pictures_fmt_host):
    """T.run_host through a face that takes the format"""
    args, keep = [], []
    for p in pics:
        npl = len(p.before)
        bufs = [T.padded(b, pad) for b in p.before]
        ins = [T.guarded(p.mb, 2), T.guarded(p.res, 4), T.guarded(p.coeffs, 16)]
        keep.append((bufs, ins, [r.copy() for r, _ in ins]))
        args.append(dict(dst=[v.ctypes.data for _, v in bufs] + [None] * (3 - npl), dst_stride=[v.strides[0] for _, v in bufs] + [0] * (3 - npl),
                         mb=ins[0][1], res=ins[1][1], coeffs=ins[2][1], ncoeffs=p.ncoeffs))
    face(args, pics[0].mb_w, pics[0].mb_h, pics[0].bd, fmt)
    for bufs, ins, before in keep:
        for (raw, _), b in zip(ins, before):
            assert np.array_equal(raw, b), "an input or its guard was written"
    return [bufs for bufs, _, _ in keep]


def host_planes(pic, fmt=None):
    """the planes the host face leaves, without padding"""
    return [v.copy() for _, v in run_host([pic], pic.fmt if fmt is None else fmt)[0]]


@pytest.mark.parametrize("fmt", [2, 3])
def test_host_face_equals_the_model(fmt):
    """every set of the format (one case per format: the sets are small and their models shared), tight rows and rows 8 samples wider"""
    for name in F.RES_CPU_NAMES:
        pics, models = F.res_set(name)
        if pics[0].fmt == fmt:
            for pad in (0, 8):
                T.check(run_host(pics, fmt, pad), models, pics, pad, name)


def test_at_420_and_monochrome_the_fmt_host_face_is_the_existing_host_face():
    for name in GR.CPU_NAMES:
        pics, models = GR.picture_set(name)
        cfi = int(pics[0].chroma)
        got = run_host(pics, cfi, 4)
        old = T.run_host(pics, 4)
        for a, b in zip(got, old):
            for (x, _), (y, _) in zip(a, b):
                assert np.array_equal(x, y), name
        T.check(got, models, pics, 4, name)


def test_the_byte_of_422_is_without_effect_at_420_and_monochrome():
    for name in ("3x2", "5x4_10", "3x2_mono"):
        pics, models = GR.picture_set(name)
        noisy = []
        for p in pics:
            q = GR.ResPicture.__new__(GR.ResPicture)
            q.__dict__.update(p.__dict__)
            q.res = p.res.copy()
            q.res.view(h264.RES_MB_FMT_DTYPE)["chroma_lo422"] = 0xFF
            noisy.append(q)
        T.check(run_host(noisy, int(pics[0].chroma), 0), models, pics, 0, name)
        if not pics[0].chroma:
            T.check(run_host(noisy, 1, 0), models, pics, 0, name + " idc 1, NULL chroma")


def test_the_sets_cover_every_outcome():
    tot = {}
    for name in F.RES_CPU_NAMES:
        pics, models = F.res_set(name)
        for p, (_, c) in zip(pics, models):
            t = tot.setdefault((p.fmt, min(p.bd, 10) if p.bd in (8, 10) else 0), {})
            for k, v in c.items():
                t[k] = t.get(k, 0) + int(v)
            if p.bd in (9, 12, 14):                               # the clips at both ends, at each of these depths
                assert c["clip_lo"] > 0 and c["clip_hi"] > 0, (name, c)
    for bd in (8, 10):
        t = tot[(2, bd)]
        for k in ("intra", "none", "luma_only", "with_chroma", "t8", "cdc", "dc_up_with", "dc_up_without", "dc_lo_with", "dc_lo_without", "c_up",
                  "c_lo", "dc_bound", "clip_lo", "clip_hi"):
            assert t.get(k, 0) >= 1, (2, bd, k)
        assert bd != 8 or t["dc_trunc"] >= 1
        t = tot[(3, bd)]
        for k in ("intra", "none", "luma_only", "with_chroma", "t8", "plane4", "plane8", "t8_planes_differ", "clip_lo", "clip_hi"):
            assert t.get(k, 0) >= 1, (3, bd, k)


# -------------------------------------------------------------------------------------------------------- hand-written cases
def test_422_dc_with_and_without_each_blocks_bit():
    """one macroblock, Cb with its DC bit: for every block j of the eight, its bit alone set and its bit alone clear"""
    for bd in (8, 10):
        for j in range(8):
            for bits in ([j], [k for k in range(8) if k != j]):
                pic = F.res_blank(1, 1, 2, bd, seed=9910 + j)
                pic.set_chroma422(0, 0, dc=True, bits=bits)
                pic.set_chroma422(0, 1, dc=False, bits=[7 - j])
                pic.layout()
                want, cover = F.res_model(pic)
                assert cover["cdc"] == 1 and cover["dc_up_with"] + cover["dc_lo_with"] == len(bits)
                got = host_planes(pic)
                for p in range(3):
                    assert np.array_equal(got[p], want[p]), (bd, j, bits, p)
                assert np.array_equal(got[0], pic.before[0])       # no luma residual
                # Cr without its DC bit: only block 7 - j changes
                y, x = 4 * ((7 - j) >> 1), 4 * ((7 - j) & 1)
                diff = got[2] != pic.before[2]
                assert not diff[:y].any() and not diff[y + 4:].any() and not diff[:, :x].any() and not diff[:, x + 4:].any()


def test_444_planes_have_bits_of_their_own_with_and_without_the_8x8_flag():
    for bd in (8, 10):
        for t8 in (0, 1):
            pic = F.res_blank(2, 1, 3, bd, seed=9920 + t8)
            pic.mb["flags"][:] = t8 << 1
            if t8:
                pic.set_luma8(0, 0)
                pic.set_plane8(0, 1, [1, 2])
                pic.set_plane8(0, 2, [3])
                pic.set_plane8(1, 2, [0])                          # no luma bits at all: need is 768 by nnz444 alone
            else:
                pic.set_luma4(0, 5)
                pic.set_plane4(0, 1, [0, 15])
                pic.set_plane4(0, 2, [6, 9, 10])
                pic.set_plane4(1, 1, [3])
            pic.res["chroma"], pic.res["chroma_dc"] = 0xFF, 3      # not read at 4:4:4
            pic.resf["chroma_lo422"] = 0xFF
            pic.layout()
            want, cover = F.res_model(pic)
            assert cover["with_chroma"] == 2 and (not t8 or cover["t8_planes_differ"] == 1)
            got = host_planes(pic)
            for p in range(3):
                assert np.array_equal(got[p], want[p]), (bd, t8, p)
                assert (got[p] != pic.before[p]).any()
            assert np.array_equal(got[0][:, 16:], pic.before[0][:, 16:])   # macroblock 1 has no luma residual


def test_444_without_chroma_planes_ignores_nnz444():
    pic = F.res_blank(1, 1, 3, 8, chroma=False, seed=9930)
    pic.set_luma4(0, 3)
    pic.resf["nnz444"] = 0xFFFF
    pic.layout()
    assert pic.need(0) == 256
    want, _ = F.res_model(pic)
    assert np.array_equal(host_planes(pic)[0], want[0]) and (want[0] != pic.before[0]).any()


@pytest.mark.parametrize("fmt", [2, 3])
def test_need_boundaries_against_ncoeffs(fmt):
    """768 / 256 / 0: with ncoeffs one short of offset + need every plane of the macroblock is dropped; need 0 reads no offset"""
    def build(kind):
        pic = F.res_blank(1, 1, fmt, 8, seed=9940)
        if kind != "none":
            pic.set_luma4(0, 2, kind="many")
        if kind == "chroma":
            pic.set_chroma422(0, 1, dc=True, bits=[6]) if fmt == 2 else pic.set_plane4(0, 2, [7])
        pic.layout(shuffle=False)
        return pic
    for kind, need in (("chroma", 768), ("luma", 256), ("none", 0)):
        pic = build(kind)
        assert pic.need(0) == need
        if not need:
            assert all(np.array_equal(a, b) for a, b in zip(host_planes(pic), pic.before))
            continue
        off = int(pic.res["coeff_offset"][0])
        assert pic.ncoeffs == off + need
        want, _ = F.res_model(pic)
        got = host_planes(pic)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)) and (got[0] != pic.before[0]).any()
        pic.coeffs = np.concatenate([pic.coeffs, np.zeros(16, pic.coeffs.dtype)])     # the memory stays; only the count shrinks
        pic.ncoeffs -= 1
        assert F.res_model(pic)[1]["malformed"] == 1
        assert all(np.array_equal(a, b) for a, b in zip(host_planes(pic), pic.before)), "a malformed macroblock wrote a plane"
        for bad in (-16, off + 8):
            pic.ncoeffs = off + need + 16
            pic.res["coeff_offset"][0] = bad
            assert all(np.array_equal(a, b) for a, b in zip(host_planes(pic), pic.before)), bad


def test_intra_macroblocks_are_left_alone():
    for fmt in (2, 3):
        pics, _ = F.res_set("3x2_%d_8" % fmt)
        pic = pics[1]
        got = host_planes(pic)
        n = 0
        for m in np.nonzero(pic.mb["flags"] & 1)[0]:
            my, mx = divmod(int(m), pic.mb_w)
            for p in range(3):
                h, w = (16, 16) if p == 0 or fmt == 3 else (16, 8)
                assert np.array_equal(got[p][my * h:my * h + h, mx * w:mx * w + w], pic.before[p][my * h:my * h + h, mx * w:mx * w + w])
            n += 1
        assert n or not (pic.mb["flags"] & 1).any()


# ------------------------------------------------------------------------------------------------------------------ refusals
CW = {0: 8, 1: 8, 2: 8, 3: 16}
CH = {0: 8, 1: 8, 2: 16, 3: 16}


def _args(fmt, bd=8, mb_w=2, mb_h=2, n=1):
    """a well-formed call on host memory at a format: (dicts, what keeps the memory alive)"""
    ps = 2 if bd > 8 else 1
    args, keep = [], []
    for _ in range(n):
        planes = [np.zeros((h * mb_h, w * mb_w * ps + 16), np.uint8) for w, h in ((16, 16), (CW[fmt], CH[fmt]), (CW[fmt], CH[fmt]))]
        raw, co = T.guarded(np.zeros(768 * mb_w * mb_h, GR.coef_dtype(bd)), 16)
        mb, res = np.zeros(mb_w * mb_h, GR.MB), np.zeros(mb_w * mb_h, GR.RES)
        keep += planes + [raw, mb, res]
        args.append(dict(dst=[p.ctypes.data for p in planes], dst_stride=[p.strides[0] for p in planes], mb=mb, res=res, coeffs=co, ncoeffs=co.size))
    return args, keep


def _call(face, args, bd=8, cfi=1, mb_w=2, mb_h=2, n=None):
    arr = h264.res_pics(args, lambda a: a.ctypes.data)
    L = _lib.lib()
    a = (bd, cfi, mb_w, mb_h, len(args) if n is None else n, C.cast(arr, C.c_void_p))
    r = L.ffhip_h264_residual_pictures_fmt_host(*a) if face == "host" else L.ffhip_h264_residual_pictures_fmt_dev(*a, None)
    return r, L.ffhip_last_error().decode()


@pytest.mark.parametrize("face", ["host", "dev"])
def test_every_refusal_with_its_text(face):
    who = "ffhip_h264_residual_pictures_fmt_" + face
    keep = []

    def refused(text, args, **kw):
        r, msg = _call(face, args, **kw)
        assert r == EINVAL and msg.startswith(who + ":") and text in msg, (r, msg)

    def fresh(fmt, **kw):
        a, k = _args(fmt, **kw)
        keep.extend(k)
        return a
    for fmt in range(4):
        if face == "host":                                        # the well-formed call passes every check
            assert _call(face, fresh(fmt), cfi=fmt)[0] == 0
    refused("chroma_format_idc -1 (0..3)", fresh(1), cfi=-1)
    refused("chroma_format_idc 4 (0..3)", fresh(1), cfi=4)
    refused("bit depth 11 (8, 9, 10, 12 or 14)", fresh(2), cfi=2, bd=11)
    refused("0 x 2 macroblocks (1..4096 each)", fresh(3), cfi=3, mb_w=0)
    refused("npics = 0", fresh(2), cfi=2, n=0)
    for fmt in (1, 2, 3):
        for bd, ps in ((8, 1), (10, 2)):
            for p in (1, 2):                                      # a stride below the format's plane width
                a = fresh(fmt, bd=bd)
                a[0]["dst_stride"][p] = (2 * CW[fmt] - 4) * ps
                refused("dst plane %d" % p, a, cfi=fmt, bd=bd)
                refused("is below the plane's %d samples" % (2 * CW[fmt]), a, cfi=fmt, bd=bd)
        for p in (1, 2):                                          # only one of Cb / Cr
            a = fresh(fmt)
            a[0]["dst"][p] = None
            refused("one of Cb / Cr without the other", a, cfi=fmt)
        a = fresh(fmt)
        a[0]["res"] = a[0]["res"].ctypes.data + 2
        refused("a res that is not 4-byte aligned", a, cfi=fmt)
        # the row-overlap rule and the input spans with the format's rows: the last row of a chroma plane of picture 0
        rows = 2 * CH[fmt]
        two = fresh(fmt, n=2)
        two[1]["dst"][2] = two[0]["dst"][1] + (rows - 1) * two[0]["dst_stride"][1] + 4
        refused("a destination plane overlaps another destination plane", two, cfi=fmt)
        two = fresh(fmt, n=2)
        two[1]["coeffs"] = two[0]["dst"][2] + (rows - 1) * two[0]["dst_stride"][2]
        refused("picture 1: mb, res or coeffs overlaps a destination plane", two, cfi=fmt)
    # the planes of 4:2:0 are too small a stride for 4:4:4
    a = fresh(1)
    a[0]["dst_stride"][1] = 16
    refused("is below the plane's 32 samples", a, cfi=3)
    # the two fields of a frame interleaved at the format's row length are accepted; a byte into each other's rows they are not
    for fmt in (2, 3):
        a = fresh(fmt, n=2)
        frame = [np.zeros((2 * h * 2, w * 2 + 8), np.uint8) for w, h in ((16, 16), (CW[fmt], CH[fmt]), (CW[fmt], CH[fmt]))]
        keep.extend(frame)
        for par in range(2):
            a[par]["dst"] = [f.ctypes.data + par * f.strides[0] for f in frame]
            a[par]["dst_stride"] = [2 * f.strides[0] for f in frame]
        if face == "host":
            assert _call(face, a, cfi=fmt)[0] == 0
        a[1]["dst"][1] -= 12
        refused("a destination plane overlaps another destination plane", a, cfi=fmt)


@pytest.mark.skipif(_lib.lib().ffhip_device_count() > 0, reason="a HIP device is present: the refusal path is not reachable")
def test_no_device_comes_after_the_argument_checks():
    for fmt in range(4):
        a, keep = _args(fmt)
        assert _call("dev", a, cfi=fmt)[0] == ENOSYS
        a[0]["ncoeffs"] = -1
        assert _call("dev", a, cfi=fmt)[0] == EINVAL
