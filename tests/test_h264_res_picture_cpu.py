"""CPU tier of the H.264 whole-picture residual face: ffhip_h264_residual_pictures_host (the rules of kernels/h264_res_rules.h compiled
for the CPU) against the model of h264_res_picture_gen.py (the oracle's dispatchers in decoder order), byte for byte on whole buffers:
every plane with its stride padding and a guard row on either side, and guard bytes round coeffs, mb and res, which must come back
unchanged.  Then one hand-written macroblock per rule, every malformed case alone, every refusal of both faces with its text, the
record ABI and the coverage of the sets.  The _dev face is only ever called with arguments it must refuse, so the tier also runs
where a device exists."""
import ctypes as C

import numpy as np
import pytest

import h264_res_picture_gen as G
from ffmpeg_amd import _lib, h264

EINVAL, ENOSYS = _lib.EINVAL, _lib.ENOSYS
GUARD = 0x5A


def test_record_sizes_match_the_c_structs():
    L = _lib.lib()
    assert L.ffhip_h264_res_mb_record_size() == h264.RES_MB_DTYPE.itemsize == 16
    assert L.ffhip_h264_res_pic_record_size() == C.sizeof(h264.ResPic) == 80
    assert h264.RES_PICS_PER_LAUNCH * 80 <= 8192 * 4              # a launch's pictures travel in one staging slot
    assert [h264.RES_MB_DTYPE.fields[k][1] for k in ("coeff_offset", "chroma", "chroma_dc", "qmul")] == [0, 4, 5, 8]


def _poison(dtype):
    return np.frombuffer(bytes([G.POISON]) * 2, dtype)[0]


def padded(plane, pad):
    """the plane in rows `pad` samples wider with a guard row above and below, padding and guards poisoned; (buffer, view of the plane)"""
    a = np.full((plane.shape[0] + 2, plane.shape[1] + pad), _poison(plane.dtype), plane.dtype)
    a[1:-1, :plane.shape[1]] = plane
    return a, a[1:-1]


def guarded(a, align=16):
    """a copy of `a` with GUARD bytes on either side, the copy `align`-byte aligned; (buffer, the copy)"""
    raw = np.full(a.nbytes + 64 + align, GUARD, np.uint8)
    at = 32 + (-(raw.ctypes.data + 32)) % align
    v = raw[at:at + a.nbytes].view(a.dtype)
    v[:] = a.reshape(-1)
    return raw, v


def run_host(pics, pad=0, cfi=None):
    """the host face on the pictures; returns the padded buffers' planes [(buffer, view)] per picture after the checks of the guards"""
    args, keep = [], []
    for p in pics:
        npl = len(p.before)
        bufs = [padded(b, pad) for b in p.before[:npl]]
        ins = [guarded(p.mb, 2), guarded(p.res, 4), guarded(p.coeffs, 16)]
        keep.append((bufs, ins, [r.copy() for r, _ in ins]))
        args.append(dict(dst=[v.ctypes.data for _, v in bufs] + [None] * (3 - npl), dst_stride=[v.strides[0] for _, v in bufs] + [0] * (3 - npl),
                         mb=ins[0][1], res=ins[1][1], coeffs=ins[2][1], ncoeffs=p.ncoeffs))
    P0 = pics[0]
    h264.residual_pictures_host(args, P0.mb_w, P0.mb_h, P0.bd, int(P0.chroma) if cfi is None else cfi)
    for bufs, ins, before in keep:
        for (raw, _), b in zip(ins, before):
            assert np.array_equal(raw, b), "an input or its guard was written"
    return [bufs for bufs, _, _ in keep]


def check(got, models, pics, pad, what=""):
    for k, (bufs, (want, _)) in enumerate(zip(got, models)):
        for p, (buf, _) in enumerate(bufs):
            exp, _ = padded(want[p], pad)
            bad = np.argwhere(buf != exp)
            assert not len(bad), "%s picture %d plane %d: %d samples differ, first at row %d column %d: got %d want %d" % (
                what, k, p, len(bad), bad[0][0] - 1, bad[0][1], buf[tuple(bad[0])], exp[tuple(bad[0])])


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("name", G.CPU_NAMES)
def test_host_face_equals_the_model(name, pad):
    pics, models = G.picture_set(name)
    check(run_host(pics, pad), models, pics, pad, name)


def test_monochrome_through_chroma_format_idc_1_with_null_chroma_and_through_0_with_chroma_pointers():
    pics, models = G.picture_set("3x2_mono")
    check(run_host(pics, 4, cfi=1), models, pics, 4, "NULL chroma")
    full, _ = G.picture_set("3x2")                                # chroma_format_idc 0: Cb / Cr and the chroma fields are ignored
    mono = [G.model(p, has_chroma=False) for p in full]
    check(run_host(full, 4, cfi=0), mono, full, 4, "chroma_format_idc 0")
    assert any((a[0][1] != b[0][1]).any() for a, b in zip(mono, G.picture_set("3x2")[1]))        # the chroma residual was there to ignore


def test_the_sets_cover_every_outcome():
    tot = {8: {}, 10: {}}
    for name in G.CPU_NAMES:
        pics, models = G.picture_set(name)
        for p, (_, c) in zip(pics, models):
            t = tot[8 if p.bd == 8 else 10]
            for k, v in c.items():
                t[k] = t.get(k, 0) + int(v)
    for depth, t in tot.items():
        for k in ("intra", "none", "luma_only", "with_chroma", "t8", "blk4_dc", "blk4_ac1", "blk4_many", "blk8_dc", "blk8_ac1", "blk8_many",
                  "blk8_off", "cdc", "cdc_block_without_bit", "cdc_block_with_bit", "c_block", "dc_bound"):
            assert t.get(k, 0) >= 1, (depth, k)
    assert tot[8]["dc_trunc"] >= 1
    assert {p[0].chroma for p, _ in map(G.picture_set, G.NAMES)} == {True, False}
    assert {p[0].bd for p, _ in map(G.picture_set, G.CPU_NAMES)} == {8, 9, 10, 12, 14}
    assert {len(p) for p, _ in map(G.picture_set, G.NAMES)} >= {1, 3, h264.RES_PICS_PER_LAUNCH + 1}
    big = [p for name in G.CPU_NAMES for p in G.picture_set(name)[0] if p.bd == 8]
    assert any(np.abs(p.coeffs.astype(np.int64)).max() > 32000 for p in big)


# ---------------------------------------------------------------------------------------------------- hand-written cases
def changed(pic, pad=4):
    """(per plane: which samples differ from `before`, the planes) after the host face, checked against the model"""
    pic.layout()
    m = G.model(pic)
    got = run_host([pic], pad)
    check(got, [m], [pic], pad)
    return [v[:, :b.shape[1]] != b for (_, v), b in zip(got[0], pic.before)], m[1]


def only(mask, y, x, h, w):
    rest = mask.copy()
    rest[y:y + h, x:x + w] = False
    return not rest.any()


@pytest.mark.parametrize("bd", [8, 10])
def test_rule_2_no_residual(bd):
    pic = G.blank(2, 2, bd)
    d, c = changed(pic)
    assert not any(x.any() for x in d) and c["none"] == 4


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("i", range(16))
def test_rule_4_a_single_4x4_block_in_each_position(bd, i):
    pic = G.blank(2, 2, bd)
    v = np.arange(16) * 37 - 200
    pic.set_luma4(3, i, values=v << (bd - 8))
    d, c = changed(pic)
    x, y = 16 + 4 * G.X4[i], 16 + 4 * G.Y4[i]
    assert d[0][y:y + 4, x:x + 4].sum() >= 8 and only(d[0], y, x, 4, 4) and not d[1].any() and not d[2].any()
    assert c["luma_only"] == 1 and c["blk4_many"] == 1


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("k", range(4))
def test_rule_5_a_single_8x8_block_in_each_position(bd, k):
    pic = G.blank(2, 2, bd)
    pic.mb["flags"][1] = h264.BS_MB_T8X8
    pic.set_luma8(1, k, values=(np.arange(64) * 29 % 301 - 150) << (bd - 8))
    d, c = changed(pic)
    x, y = 16 + 8 * (k & 1), 8 * (k >> 1)
    assert d[0][y:y + 8, x:x + 8].sum() >= 32 and only(d[0], y, x, 8, 8) and c["blk8_many"] == 1


@pytest.mark.parametrize("bd", [8, 10])
def test_rule_5_only_the_top_left_bit_counts(bd):
    pic = G.blank(1, 1, bd)
    pic.mb["flags"][0] = h264.BS_MB_T8X8
    pic.mb["nnz"][0] = 0xFFFF & ~(1 | 1 << 2 | 1 << 8 | 1 << 10)  # every bit but the four top-left ones
    pic.blocks[0][:256] = 99
    d, c = changed(pic)
    assert not d[0].any() and c["blk8_off"] == 4 and c["luma_only"] == 1
    pic.mb["nnz"][0] = 1 << 10                                    # the top-left bit of 8x8 block 3 alone
    d, c = changed(pic)
    assert d[0][8:, 8:].sum() >= 16 and only(d[0], 8, 8, 8, 8)


@pytest.mark.parametrize("bd", [8, 10])
def test_rules_6_and_7_chroma(bd):
    pic = G.blank(2, 1, bd)                                       # Cb DC alone
    pic.set_chroma(1, 0, dc=True, bits=[])
    pic.blocks[1][256:512:16][:4] = np.array([900, -300, 200, 100]) << (bd - 8)
    pic.res["qmul"][1] = [640, 1]
    d, c = changed(pic)
    assert d[1][:, 8:].sum() >= 32 and only(d[1], 0, 8, 8, 8) and not d[0].any() and not d[2].any()
    assert c["cdc"] == 1 and c["cdc_block_without_bit"] == 4 and c["with_chroma"] == 1
    for j in range(4):                                            # Cr AC alone, on each block
        pic = G.blank(2, 1, bd)
        pic.set_chroma(0, 1, dc=False, bits=[j])
        pic.blocks[0][512 + 16 * j:512 + 16 * j + 16] = (np.arange(16) * 41 - 300) << (bd - 8)
        d, c = changed(pic)
        assert d[2][4 * (j >> 1):4 * (j >> 1) + 4, 4 * (j & 1):4 * (j & 1) + 4].sum() >= 8 and only(d[2], 4 * (j >> 1), 4 * (j & 1), 4, 4)
        assert not d[0].any() and not d[1].any() and c["c_block"] == 1 and c["cdc"] == 0


@pytest.mark.parametrize("bd", [8, 14])
def test_everything_coded_and_an_intra_macroblock_full_of_bits(bd):
    pic = G.blank(2, 1, bd)
    for m in range(2):
        for i in range(16):
            pic.set_luma4(m, i, kind="many")
        for c in range(2):
            pic.set_chroma(m, c, dc=True, bits=[0, 1, 2, 3])
    pic.mb["flags"][1] = h264.BS_MB_INTRA | h264.BS_MB_T8X8
    d, c = changed(pic)
    assert c["intra"] == 1 and c["with_chroma"] == 1 and c["blk4_many"] == 16 and c["cdc_block_with_bit"] == 8
    for p, w in enumerate((16, 8, 8)):
        assert not d[p][:, w:].any() and d[p][:, :w].mean() > 0.5


def test_rule_9_a_dc_the_coefficient_type_wraps():
    """at 8 bits block[0] + 32 wraps in the transform for 32736 .. 32767 and not in *_dc_add: a luma block with nothing but the DC
    and a chroma block without its bit take the latter, a chroma block with its bit the former, as the reference's dispatchers do"""
    pic = G.blank(1, 1, 8)
    pic.before = [np.full_like(b, 128) for b in pic.before]
    dc = np.zeros(16, np.int64)
    dc[0] = 32760
    pic.set_luma4(0, 0, values=dc)                                # *_dc_add: + 512
    ac = dc.copy()
    ac[5] = 1
    pic.set_luma4(0, 1, values=ac)                                # the transform: block[0] wraps to -32744
    pic.set_chroma(0, 0, dc=False, bits=[0])                      # idct_add8 with the bit: the transform, wrapped: - 512
    pic.blocks[0][256:272] = dc
    pic.set_chroma(0, 1, dc=True, bits=[])                        # under the DC bit, no block bit: idct_dc_add, not wrapped
    pic.blocks[0][512:768:16][:4] = [32760, 0, 0, 0]
    pic.res["qmul"][0][1] = 128                                   # (a * 128) >> 7 = a on all four blocks
    pic.layout()
    want, _ = G.model(pic)
    got = run_host([pic], 0)
    check(got, [(want, None)], [pic], 0)
    assert (want[0][:4, :4] == 255).all() and (want[0][:4, 4:8] == 0).all() and (want[1][:4, :4] == 0).all() and (want[2] == 255).all()


# ------------------------------------------------------------------------------------------------------------- malformed
@pytest.mark.parametrize("bd", [8, 10])
def test_rule_3_each_malformed_case_alone_and_the_exact_fit(bd):
    def pic_with(need768):
        pic = G.blank(2, 1, bd)
        for m in range(2):
            pic.set_luma4(m, 5, kind="many")
            if need768:
                pic.set_chroma(m, 0, dc=True, bits=[3])
        pic.layout(shuffle=False)
        return pic
    for need768 in (False, True):
        need = 768 if need768 else 256
        pic = pic_with(need768)
        pic.layout = lambda: None                                 # changed() keeps the offsets set below
        good, _ = changed(pic)
        assert good[0][:, :16].any() and good[0][:, 16:].any()
        last = int(np.argmax(pic.res["coeff_offset"]))
        assert int(pic.res["coeff_offset"][last]) + need == pic.ncoeffs      # the exact fit is accepted
        first = 1 - last
        for off in (-16, -1, int(pic.res["coeff_offset"][first]) + 8, int(pic.res["coeff_offset"][first]) + 1):
            keep = int(pic.res["coeff_offset"][first])
            pic.res["coeff_offset"][first] = off
            d, c = changed(pic)
            assert c["malformed"] == 1 and not any(x[:, (8 if p else 16) * first:(8 if p else 16) * (first + 1)].any() for p, x in enumerate(d))
            assert d[0][:, 16 * last:16 * last + 16].any()
            pic.res["coeff_offset"][first] = keep
        pic.ncoeffs -= 1                                          # one coefficient past the end
        d, c = changed(pic)
        assert c["malformed"] == 1 and not any(x[:, (8 if p else 16) * last:(8 if p else 16) * (last + 1)].any() for p, x in enumerate(d))
        assert d[0][:, 16 * first:16 * first + 16].any()


# -------------------------------------------------------------------------------------------------------------- refusals
def _args(bd=8, mb_w=2, mb_h=2, n=1, mono=False):
    """a well-formed call on host memory: (dicts, what keeps the memory alive)"""
    ps = 2 if bd > 8 else 1
    args, keep = [], []
    for _ in range(n):
        planes = [np.zeros((h * mb_h, w * mb_w * ps + 16), np.uint8) for w, h in ((16, 16), (8, 8), (8, 8))[:1 if mono else 3]]
        raw, co = guarded(np.zeros(768 * mb_w * mb_h, G.coef_dtype(bd)), 16)
        mb, res = np.zeros(mb_w * mb_h, G.MB), np.zeros(mb_w * mb_h, G.RES)
        keep += planes + [raw, mb, res]
        args.append(dict(dst=[p.ctypes.data for p in planes] + [None] * (3 - len(planes)), dst_stride=[p.strides[0] for p in planes] + [0] * (3 - len(planes)),
                         mb=mb, res=res, coeffs=co, ncoeffs=co.size))
    return args, keep


def _call(face, args, bd=8, cfi=1, mb_w=2, mb_h=2, n=None):
    arr = h264.res_pics(args, lambda a: a.ctypes.data)
    L = _lib.lib()
    a = (bd, cfi, mb_w, mb_h, len(args) if n is None else n, C.cast(arr, C.c_void_p) if args is not None else None)
    r = L.ffhip_h264_residual_pictures_host(*a) if face == "host" else L.ffhip_h264_residual_pictures_dev(*a, None)
    return r, L.ffhip_last_error().decode()


@pytest.mark.parametrize("face", ["host", "dev"])
def test_every_refusal_with_its_text(face):
    who = "ffhip_h264_residual_pictures_" + face

    def refused(rc, text, args, **kw):
        r, msg = _call(face, args, **kw)
        assert r == rc and msg.startswith(who + ":") and text in msg, (r, msg)
    ok, keep = _args()
    if face == "host":                                            # the well-formed call passes every check (the device face would launch)
        assert _call(face, ok)[0] == 0
    for cfi in (2, 3):
        refused(ENOSYS, "4:2:2 and 4:4:4 are not implemented", ok, cfi=cfi)
    for bd in (7, 11, 16):
        refused(EINVAL, "bit depth %d (8, 9, 10, 12 or 14)" % bd, ok, bd=bd)
    refused(EINVAL, "chroma_format_idc -1 (0 or 1)", ok, cfi=-1)
    refused(EINVAL, "chroma_format_idc 4 (0 or 1)", ok, cfi=4)
    for w, h in ((0, 2), (2, 0), (4097, 2), (2, 4097)):
        refused(EINVAL, "%d x %d macroblocks (1..4096 each)" % (w, h), ok, mb_w=w, mb_h=h)
    refused(EINVAL, "npics = 0", ok, n=0)
    refused(EINVAL, "npics = -1", ok, n=-1)
    r, msg = (_lib.lib().ffhip_h264_residual_pictures_host(8, 1, 2, 2, 1, None) if face == "host" else
              _lib.lib().ffhip_h264_residual_pictures_dev(8, 1, 2, 2, 1, None, None)), _lib.lib().ffhip_last_error().decode()
    assert r == EINVAL and "NULL picture array" in msg

    def edited(**kw):
        a, k = _args(**{x: kw.pop(x) for x in ("bd", "n") if x in kw})
        keep.extend(k)
        for key, val in kw.items():
            a[-1][key] = val(a[-1]) if callable(val) else val
        return a
    refused(EINVAL, "dst plane 0 is NULL", edited(dst=lambda a: [None] + a["dst"][1:]))
    for key in ("mb", "res", "coeffs"):
        refused(EINVAL, "a NULL mb, res or coeffs", edited(**{key: None}))
    refused(EINVAL, "one of Cb / Cr without the other", edited(dst=lambda a: a["dst"][:2] + [None]))
    refused(EINVAL, "one of Cb / Cr without the other", edited(dst=lambda a: [a["dst"][0], None, a["dst"][2]]))
    refused(EINVAL, "dst plane 0 is NULL, its base or stride", edited(dst=lambda a: [a["dst"][0] + 2] + a["dst"][1:]))
    refused(EINVAL, "dst plane 2 is NULL, its base or stride", edited(bd=10, dst=lambda a: a["dst"][:2] + [a["dst"][2] + 4]), bd=10)
    refused(EINVAL, "stride 50 is not a multiple of 4 samples", edited(dst_stride=lambda a: [50] + a["dst_stride"][1:]))
    refused(EINVAL, "is below the plane's 16 samples", edited(dst_stride=lambda a: [a["dst_stride"][0], 12, a["dst_stride"][2]]))
    refused(EINVAL, "is below the plane's 32 samples", edited(dst_stride=lambda a: [-a["dst_stride"][0]] + a["dst_stride"][1:]))   # negative strides
    refused(EINVAL, "a res that is not 4-byte aligned", edited(res=lambda a: a["res"].ctypes.data + 2))
    refused(EINVAL, "a coeffs that is not 16-byte aligned", edited(coeffs=lambda a: a["coeffs"].ctypes.data + 8))
    refused(EINVAL, "ncoeffs -1 (>= 0)", edited(ncoeffs=-1))
    # overlaps: two destination planes; an input inside a destination span
    refused(EINVAL, "a destination plane overlaps another destination plane", edited(dst=lambda a: [a["dst"][0], a["dst"][0] + 16, a["dst"][2]]))
    two = edited(n=2)
    two[1]["dst"] = [two[0]["dst"][0] + 4] + two[1]["dst"][1:]
    refused(EINVAL, "a destination plane overlaps another destination plane", two)
    for key in ("mb", "res", "coeffs"):
        refused(EINVAL, "picture 0: mb, res or coeffs overlaps a destination plane", edited(**{key: lambda a: a["dst"][1] + 16}))
    two = edited(n=2)
    two[1]["coeffs"] = two[0]["dst"][2] + 15 * two[0]["dst_stride"][2]       # the first picture's last Cr row
    refused(EINVAL, "picture 1: mb, res or coeffs overlaps a destination plane", two)


def test_both_fields_of_one_buffer_in_one_call():
    """the two fields of a frame are two pictures of the call whose planes interleave row by row: accepted by the row rule, and each
    field gets its own residual; shifted by a byte into each other's rows they are refused"""
    for bd in (8, 10):
        rng = np.random.default_rng(9790 + bd)
        mb_w, mb_h, pad = 3, 2, 8
        top, bot = G.ResPicture(rng, mb_w, mb_h, bd), G.ResPicture(rng, mb_w, mb_h, bd)
        frame = []
        for p in range(3):
            f = np.full((2 * top.before[p].shape[0], top.before[p].shape[1] + pad), _poison(top.before[p].dtype), top.before[p].dtype)
            f[0::2, :-pad], f[1::2, :-pad] = top.before[p], bot.before[p]
            frame.append(f)
        exp = [f.copy() for f in frame]
        for par, pic in enumerate((top, bot)):
            for p, w in enumerate(G.model(pic)[0]):
                exp[p][par::2, :-pad] = w
        args = [dict(dst=[f.ctypes.data + par * f.strides[0] for f in frame], dst_stride=[2 * f.strides[0] for f in frame], mb=pic.mb, res=pic.res,
                     coeffs=guarded(pic.coeffs)[1], ncoeffs=pic.ncoeffs) for par, pic in enumerate((top, bot))]
        h264.residual_pictures_host(args, mb_w, mb_h, bd, 1)
        for p in range(3):
            assert np.array_equal(frame[p], exp[p]), "plane %d" % p
        args[1]["dst"][0] -= 12 * (2 if bd > 8 else 1)            # past the 8 samples of padding: into the top field's rows
        r, msg = _call("host", args, bd=bd, mb_w=mb_w, mb_h=mb_h)
        assert r == EINVAL and "a destination plane overlaps another destination plane" in msg
