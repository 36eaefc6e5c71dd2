"""CPU tier of the H.264 whole-picture inter prediction face (ffhip_h264_inter_pictures_dev) and its device-free plan face
(ffhip_h264_inter_plan_pictures_host): the record ABI, the plan face against the decisions of the model of h264_inter_picture_gen.py
over the picture sets (guard records round the output, inputs untouched), one hand-written case per line of rules 1, 2 and 5 to 8,
every malformed case alone, every refusal of both faces with its text, the row-overlap rule in both directions, and the coverage of
the sets.  The _dev face is only ever called with arguments it must refuse, so the tier also runs where a device exists."""
import ctypes as C

import numpy as np
import pytest

import h264_inter_picture_gen as G
from ffmpeg_amd import _lib, h264

EINVAL, ENOSYS = _lib.EINVAL, _lib.ENOSYS
SKIP, UNI, UNI_W, BI_AVG, BI_W = range(5)


def test_record_sizes_match_the_c_structs():
    L = _lib.lib()
    assert L.ffhip_h264_inter_slice_record_size() == h264.INTER_SLICE_DTYPE.itemsize == 2888
    assert L.ffhip_h264_inter_ref_record_size() == C.sizeof(h264.InterRef) == 56
    assert L.ffhip_h264_inter_pic_record_size() == C.sizeof(h264.InterPic) == 1880
    assert L.ffhip_h264_inter_plan_record_size() == h264.INTER_PLAN_DTYPE.itemsize == 28
    assert L.ffhip_h264_inter_plan_pic_record_size() == C.sizeof(h264.InterPlanPic) == 48
    assert h264.INTER_PICS_PER_LAUNCH * 1880 <= 8192 * 4          # a launch's pictures travel in one staging slot
    assert (h264.INTER_SKIP, h264.INTER_UNI, h264.INTER_UNI_W, h264.INTER_BI_AVG, h264.INTER_BI_W) == (SKIP, UNI, UNI_W, BI_AVG, BI_W)


# ------------------------------------------------------------------------------------------------------------- the plan face
GUARD = 0x5A


def run_plan(pics, pad=0):
    """the plan face on the pictures (an mvf stride `pad` records wider than the picture): the plans (h4, w4) per picture; a guard
    record on either side of the output and the inputs must come back untouched"""
    args, keep = [], []
    for p in pics:
        mvf = np.zeros((p.h4, p.w4 + pad), h264.BS_MVF_DTYPE)
        mvf.view(np.uint8)[:] = 0x7F                              # ref_idx 127 beside the picture: malformed if ever read
        mvf[:, :p.w4] = p.mvf
        full = np.zeros(p.h4 * p.w4 + 2, G.PLAN)
        full.view(np.uint8)[:] = GUARD
        ins = (p.mb.copy(), mvf, p.slices.copy())
        keep.append((full, ins, [a.copy() for a in ins]))
        args.append(dict(mb=ins[0], mvf=mvf, slices=ins[2], plans=full[1:-1], mvf_stride=p.w4 + pad, nslices=p.nslices, nrefs=p.nrefs))
    h264.inter_plan_host(args, pics[0].mb_w, pics[0].mb_h)
    guard = np.full(28, GUARD, np.uint8).view(G.PLAN)[0]
    for full, ins, before in keep:
        assert full[0] == guard and full[-1] == guard, "a guard record was written"
        for a, b in zip(ins, before):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "an input was written"
    return [full[1:-1].reshape(p.h4, p.w4) for (full, _, _), p in zip(keep, pics)]


@pytest.mark.parametrize("name", G.NAMES)
def test_plan_face_equals_the_models_decisions(name):
    pics, models = G.picture_set(name)
    for k, (got, (_, plans, _)) in enumerate(zip(run_plan(pics, pad=k_pad(name)), models)):
        bad = np.argwhere(got != plans)
        assert not len(bad), "%s picture %d: %d plans differ, first at %s: %s against %s" % (
            name, k, len(bad), bad[0].tolist(), got[tuple(bad[0])], plans[tuple(bad[0])])


def k_pad(name):
    return len(name) % 3                                          # mvf strides of 4 mb_w, + 1 and + 2 records over the sets


def test_the_sets_cover_every_branch():
    """no mcxy at any block size, chroma fraction, mode, partition shape or picture side may be missing; 8-bit and 10-bit sets each
    have every mcxy at 8x8 and at 4x4 and every chroma fraction"""
    tot = {}
    for depth in (8, 10):
        cov = {k: set() for k in ("mcxy", "cfrac", "modes", "parts", "sides")}
        nskip = nlive = 0
        for name in G.NAMES:
            pics, models = G.picture_set(name)
            if pics[0].bd != depth:
                continue
            for pic, (_, plans, c) in zip(pics, models):
                for k in cov:
                    cov[k] |= c[k]
                inter = np.repeat(np.repeat((pic.mb["flags"] & 1).reshape(pic.mb_h, pic.mb_w) == 0, 4, 0), 4, 1)
                nlive += int((plans["mode"] != SKIP).sum())
                nskip += int((plans["mode"][~inter] == SKIP).sum())
                assert (plans["mode"][inter] != SKIP).all()      # the generator's content is legal
        assert {(s, m) for s in (4, 8) for m in range(16)} <= cov["mcxy"], depth
        assert cov["cfrac"] == {(x, y) for x in range(8) for y in range(8)}, depth
        assert cov["modes"] == {UNI, UNI_W, BI_AVG, BI_W}, depth
        assert cov["sides"] == {"left", "top", "right", "bottom"}, depth
        assert nskip >= 16 and nlive >= 500, depth
        tot[depth] = cov
    assert {(16, m) for m in range(16)} <= tot[8]["mcxy"] | tot[10]["mcxy"]
    assert tot[8]["parts"] == {"16x16", "16x8", "8x16", "8x8", "8x4", "4x8", "4x4"} == tot[10]["parts"]
    assert {pics[0].chroma for pics, _ in map(G.picture_set, G.NAMES)} == {True, False}
    assert {len(pics) for pics, _ in map(G.picture_set, G.NAMES)} >= {1, 3, h264.INTER_PICS_PER_LAUNCH + 1}


# ---------------------------------------------------------------------------------------------------- hand-written cases
def plan_of(pic):
    """the face's plan of block (0, 0), which must equal the model's decision"""
    got = run_plan([pic])[0]
    want = np.array([[G.decide(pic, pic.mb[(y >> 2) * pic.mb_w + (x >> 2)], pic.mvf[y, x]) for x in range(pic.w4)] for y in range(pic.h4)])
    assert (got == want).all()
    return got[0, 0]


def _weights(pic):
    """explicit tables with a different value in every entry"""
    s = pic.slices[0]
    s["luma_log2_denom"], s["chroma_log2_denom"] = 3, 6
    s["luma_weight"] = (np.arange(128) - 60).reshape(32, 2, 2)
    s["chroma_weight"] = (np.arange(256) - 120).reshape(32, 2, 2, 2)
    return s


def _zero_but(p, **kw):
    z = np.zeros((), G.PLAN)
    for k, v in kw.items():
        z[k] = v
    assert p == z, "%s against %s" % (p, z)


def test_rule_1_intra():
    pic = G.blank(2, 1)
    pic.mb["flags"][0] = h264.BS_MB_INTRA | h264.BS_MB_T8X8
    got = run_plan([pic])[0]
    assert (got[:, :4]["mode"] == SKIP).all() and (got[:, 4:]["mode"] == UNI).all()
    _zero_but(got[0, 0])
    pic.mb["flags"][1] = h264.BS_MB_T8X8                          # bit 1 alone is not intra
    assert (run_plan([pic])[0][:, 4:]["mode"] == UNI).all()


def test_rule_6_one_list_and_two_lists():
    pic = G.blank(1, 1, nrefs=3)
    pic.slices[0]["ref"][0][:3] = [2, 0, 1]
    pic.slices[0]["ref"][1][:3] = [1, 1, 2]
    pic.mvf["ref_idx"] = [1, -1]
    _zero_but(plan_of(pic), mode=UNI, list=0, slot=[0, 0])
    pic.mvf["ref_idx"] = [0, -1]
    _zero_but(plan_of(pic), mode=UNI, list=0, slot=[2, 0])
    pic.mvf["ref_idx"] = [-1, 2]
    _zero_but(plan_of(pic), mode=UNI, list=1, slot=[2, 0])
    pic.mvf["ref_idx"] = [-128, 0]
    _zero_but(plan_of(pic), mode=UNI, list=1, slot=[1, 0])
    pic.mvf["ref_idx"] = [0, 2]
    _zero_but(plan_of(pic), mode=BI_AVG, slot=[2, 2])             # the same slot in both lists
    pic.mvf["ref_idx"] = [2, 0]
    _zero_but(plan_of(pic), mode=BI_AVG, slot=[1, 1])
    _weights(pic)                                                 # use_weight 0: the tables are not read
    pic.slices[0]["use_weight_chroma"] = 1
    _zero_but(plan_of(pic), mode=BI_AVG, slot=[1, 1])


def test_rule_5_and_7_implicit():
    pic = G.blank(1, 1, nrefs=3)
    s = _weights(pic)
    s["use_weight"] = 2
    s["implicit_weight"] = 32
    s["implicit_weight"][1][2] = 33
    s["implicit_weight"][2][1] = -64
    s["implicit_weight"][0][0] = 128
    pic.mvf["ref_idx"] = [1, 1]
    _zero_but(plan_of(pic), mode=BI_AVG, slot=[1, 1])             # implicit 32: the plain average
    pic.mvf["ref_idx"] = [1, 2]
    _zero_but(plan_of(pic), mode=BI_W, slot=[1, 2], chroma_weighted=1, luma_log2_denom=5, chroma_log2_denom=5, luma_weight=[33, 31],
              chroma_weight=[[33, 31], [33, 31]])                 # ... against 33
    pic.mvf["ref_idx"] = [2, 1]
    _zero_but(plan_of(pic), mode=BI_W, slot=[2, 1], chroma_weighted=1, luma_log2_denom=5, chroma_log2_denom=5, luma_weight=[-64, 128],
              chroma_weight=[[-64, 128], [-64, 128]])
    pic.mvf["ref_idx"] = [0, 0]
    _zero_but(plan_of(pic), mode=BI_W, slot=[0, 0], chroma_weighted=1, luma_log2_denom=5, chroma_log2_denom=5, luma_weight=[128, -64],
              chroma_weight=[[128, -64], [128, -64]])
    for ri, L, slot in (([1, -1], 0, 1), ([-1, 2], 1, 2)):        # use_weight 2 with one list: not weighted
        pic.mvf["ref_idx"] = ri
        _zero_but(plan_of(pic), mode=UNI, list=L, slot=[slot, 0])


@pytest.mark.parametrize("uwc", [0, 1])
def test_rule_7_and_8_explicit(uwc):
    pic = G.blank(1, 1, nrefs=3)
    s = _weights(pic)
    s["use_weight"], s["use_weight_chroma"] = 1, uwc
    s["implicit_weight"] = 77                                     # not read
    lw, cw = s["luma_weight"].astype(int), s["chroma_weight"].astype(int)
    pic.mvf["ref_idx"] = [2, 1]                                   # two lists: chroma is weighted whatever use_weight_chroma says
    _zero_but(plan_of(pic), mode=BI_W, slot=[2, 1], chroma_weighted=1, luma_log2_denom=3, chroma_log2_denom=6,
              luma_weight=[lw[2][0][0], lw[1][1][0]], luma_offset=lw[2][0][1] + lw[1][1][1],
              chroma_weight=[[cw[2][0][c][0], cw[1][1][c][0]] for c in range(2)],
              chroma_offset=[cw[2][0][c][1] + cw[1][1][c][1] for c in range(2)])
    for ri, L, r in (([2, -1], 0, 2), ([-1, 1], 1, 1)):           # one list: chroma only with use_weight_chroma
        pic.mvf["ref_idx"] = ri
        want = dict(mode=UNI_W, list=L, slot=[r, 0], luma_log2_denom=3, luma_weight=[lw[r][L][0], 0], luma_offset=lw[r][L][1])
        if uwc:
            want.update(chroma_weighted=1, chroma_log2_denom=6, chroma_weight=[[cw[r][L][c][0], 0] for c in range(2)],
                        chroma_offset=[cw[r][L][c][1] for c in range(2)])
        _zero_but(plan_of(pic), **want)


def test_explicit_offsets_sum_outside_int8():
    pic = G.blank(1, 1)
    s = _weights(pic)
    s["use_weight"] = 1
    s["luma_weight"][..., 1] = -128
    s["chroma_weight"][..., 1] = 127
    s["luma_log2_denom"], s["chroma_log2_denom"] = 0, 7
    pic.mvf["ref_idx"] = [0, 1]
    p = plan_of(pic)
    assert p["luma_offset"] == -256 and p["chroma_offset"].tolist() == [254, 254] and (p["luma_log2_denom"], p["chroma_log2_denom"]) == (0, 7)


MALFORMED = {
    "slice >= nslices": lambda p: p.mb["slice"].__setitem__(0, 1),
    "no list used": lambda p: p.mvf["ref_idx"].__setitem__((0, 0), [-1, -3]),
    "ref_idx >= num_ref, list 0": lambda p: p.mvf["ref_idx"].__setitem__((0, 0), [2, -1]),
    "ref_idx >= num_ref, list 1 of two": lambda p: p.mvf["ref_idx"].__setitem__((0, 0), [0, 2]),
    "ref_idx >= 32": lambda p: (p.slices["num_ref"].__setitem__(0, [32, 32]), p.slices["ref"].__setitem__(0, 0),
                                p.mvf["ref_idx"].__setitem__((0, 0), [32, -1])),
    "ref_idx 127 with num_ref 255": lambda p: (p.slices["num_ref"].__setitem__(0, [2, 255]), p.mvf["ref_idx"].__setitem__((0, 0), [-1, 127])),
    "num_ref > 32": lambda p: p.slices["num_ref"].__setitem__(0, [33, 2]),
    "slot >= nrefs": lambda p: p.slices["ref"][0][0].__setitem__(0, 2),
    "slot 255": lambda p: p.slices["ref"][0][0].__setitem__(0, 255),
    "luma denominator 8": lambda p: p.slices["luma_log2_denom"].__setitem__(0, 8),
    "chroma denominator 8": lambda p: p.slices["chroma_log2_denom"].__setitem__(0, 8),
    "use_weight 3": lambda p: p.slices["use_weight"].__setitem__(0, 3),
}


@pytest.mark.parametrize("case", list(MALFORMED))
def test_rule_2_each_malformed_case_alone(case):
    pic = G.blank(1, 1)
    assert plan_of(pic)["mode"] == UNI
    MALFORMED[case](pic)
    got = run_plan([pic])[0]
    _zero_but(got[0, 0])
    whole = case.split()[0] in ("slice", "num_ref", "slot", "luma", "chroma", "use_weight")
    assert (got["mode"] == SKIP).sum() == (16 if whole else 1)    # a slice's fault takes every block of it, a block's fault itself
    assert plan_of(pic)["mode"] == SKIP


def test_malformed_values_at_the_limits_are_well_formed():
    pic = G.blank(1, 1)
    s = pic.slices[0]
    s["num_ref"] = [32, 32]
    s["ref"][:] = 1
    s["luma_log2_denom"] = s["chroma_log2_denom"] = 7
    s["use_weight"] = 2
    pic.mvf["ref_idx"] = [31, 31]
    assert plan_of(pic)["mode"] == BI_AVG                          # implicit_weight is 32 everywhere in blank()'s slice
    pic.nrefs = 1                                                 # slot 1 with one reference
    assert plan_of(pic)["mode"] == SKIP


# ------------------------------------------------------------------------------------------------------------- refusals
_BUFS = []


def _buf(n=1 << 13):
    b = (C.c_uint64 * n)()
    _BUFS.append(b)
    return C.addressof(b)


def err():
    return _lib.lib().ffhip_last_error().decode()


def _plan_pics(n=1):
    """n plan pictures of 2 x 2 macroblocks whose tables are distinct zeroed host buffers"""
    pics = (h264.InterPlanPic * n)()
    for i in range(n):
        for f in ("mb", "mvf", "slices", "plans"):
            setattr(pics[i], f, _buf())
        pics[i].mvf_stride, pics[i].nslices, pics[i].nrefs = 8, 1, 2
    return pics


def plan_face(w, h, n, pics):
    return _lib.lib().ffhip_h264_inter_plan_pictures_host(w, h, n, C.cast(pics, C.c_void_p) if pics is not None else None)


def test_plan_face_refusals():
    who = "ffhip_h264_inter_plan_pictures_host"
    ok = _plan_pics()
    assert plan_face(2, 2, 1, ok) == 0
    for w, h in ((0, 2), (2, 0), (4097, 2), (2, 4097), (-1, 2)):
        assert plan_face(w, h, 1, ok) == EINVAL and who in err() and "1..4096" in err()
    for n in (0, -1):
        assert plan_face(2, 2, n, ok) == EINVAL and "npics" in err()
    assert plan_face(2, 2, 1, None) == EINVAL and "npics" in err()
    for field in ("mb", "mvf", "slices", "plans"):
        pics = _plan_pics()
        setattr(pics[0], field, None)
        assert plan_face(2, 2, 1, pics) == EINVAL and who in err() and "NULL" in err(), field
    pics = _plan_pics()
    pics[0].mvf += 2
    assert plan_face(2, 2, 1, pics) == EINVAL and "4-byte aligned" in err()
    for field, bad, word in (("mvf_stride", 7, "mvf_stride 7 (>= 8)"), ("nslices", 0, "nslices 0 (>= 1)"), ("nslices", -2, "nslices -2"),
                             ("nrefs", -1, "nrefs -1 (0..32)"), ("nrefs", 33, "nrefs 33 (0..32)")):
        pics = _plan_pics()
        setattr(pics[0], field, bad)
        assert plan_face(2, 2, 1, pics) == EINVAL and word in err(), (field, err())
    for field, nbytes in (("mb", 4 * 8), ("mvf", 8 * 8 * 12), ("slices", 2888)):
        pics = _plan_pics(2)
        pics[1].plans = getattr(pics[0], field) + nbytes - 4
        assert plan_face(2, 2, 2, pics) == EINVAL and "overlaps" in err(), field
        pics[1].plans = getattr(pics[0], field) + nbytes          # back to back: accepted
        assert plan_face(2, 2, 2, pics) == 0, field
    pics = _plan_pics(2)
    pics[1].plans = pics[0].plans + 64 * 28 - 4
    assert plan_face(2, 2, 2, pics) == EINVAL and "overlaps another plans array" in err()
    for nrefs in (0, 32):
        pics = _plan_pics()
        pics[0].nrefs = nrefs
        assert plan_face(2, 2, 1, pics) == 0


def _dev_pics(n=1, mb_w=2, mb_h=2, ps=1, nrefs=2, chroma=True):
    """n pictures whose planes and tables are distinct host buffers (never dereferenced: every call below is refused, or ends at the
    device check); tight strides"""
    pics = (h264.InterPic * n)()
    for i in range(n):
        P = pics[i]
        for p in range(3 if chroma else 1):
            P.dst[p], P.dst_stride[p] = _buf(), (16 if p == 0 else 8) * mb_w * ps
        P.mb, P.mvf, P.slices = _buf(), _buf(), _buf()
        P.mvf_stride, P.nslices, P.nrefs = 4 * mb_w, 1, nrefs
        for k in range(nrefs):
            for p in range(3):
                P.ref[k].base[p], P.ref[k].stride[p] = _buf(), (16 if p == 0 else 8) * mb_w * ps
    return pics


def dev_face(bd, cfi, w, h, n, pics):
    return _lib.lib().ffhip_h264_inter_pictures_dev(bd, cfi, w, h, n, C.cast(pics, C.c_void_p) if pics is not None else None, None)


def _would_accept(bd, cfi, w, h, n, pics):
    """where a device exists the face would launch on pointers that are host memory, so acceptance is only asserted without one"""
    if _lib.lib().ffhip_device_count() > 0:
        return True
    return dev_face(bd, cfi, w, h, n, pics) == ENOSYS


def test_dev_face_refusals():
    who = "ffhip_h264_inter_pictures_dev"
    ok = _dev_pics()
    assert _would_accept(8, 1, 2, 2, 1, ok)
    for cfi in (2, 3):
        assert dev_face(8, cfi, 2, 2, 1, ok) == ENOSYS and who in err() and "chroma_format_idc %d" % cfi in err() and "not implemented" in err()
    for bd in (0, 7, 11, 13, 15, 16):
        assert dev_face(bd, 1, 2, 2, 1, ok) == EINVAL and "bit depth %d (8, 9, 10, 12 or 14)" % bd in err()
    for cfi in (-1, 4):
        assert dev_face(8, cfi, 2, 2, 1, ok) == EINVAL and "chroma_format_idc %d (0 or 1)" % cfi in err()
    for w, h in ((0, 2), (2, 0), (4097, 2), (2, 4097), (-3, 2)):
        assert dev_face(8, 1, w, h, 1, ok) == EINVAL and who in err() and "1..4096" in err()
    for n in (0, -1):
        assert dev_face(8, 1, 2, 2, n, ok) == EINVAL and "npics" in err()
    assert dev_face(8, 1, 2, 2, 1, None) == EINVAL and "npics" in err()
    pics = _dev_pics()
    pics[0].dst[0] = None
    assert dev_face(8, 1, 2, 2, 1, pics) == EINVAL and "dst plane 0 is NULL" in err()
    for p in (1, 2):                                              # only one of Cb / Cr
        pics = _dev_pics()
        pics[0].dst[p] = None
        assert dev_face(8, 1, 2, 2, 1, pics) == EINVAL and "one of Cb / Cr without the other" in err()
    for bd, ps in ((8, 1), (10, 2)):
        for p in range(3):
            pics = _dev_pics(ps=ps)
            pics[0].dst[p] += 2 * ps                              # base not a multiple of 4 samples
            assert dev_face(bd, 1, 2, 2, 1, pics) == EINVAL and "dst plane %d" % p in err() and "multiple of 4 samples" in err()
            pics = _dev_pics(ps=ps)
            pics[0].dst_stride[p] += 2 * ps                       # stride not a multiple of 4 samples
            assert dev_face(bd, 1, 2, 2, 1, pics) == EINVAL and "dst plane %d" % p in err()
            pics = _dev_pics(ps=ps)
            pics[0].dst_stride[p] -= 4 * ps                       # stride below the width
            assert dev_face(bd, 1, 2, 2, 1, pics) == EINVAL and "below the plane's %d samples" % (32 if p == 0 else 16) in err()
    for field in ("mb", "mvf", "slices"):
        pics = _dev_pics()
        setattr(pics[0], field, None)
        assert dev_face(8, 1, 2, 2, 1, pics) == EINVAL and who in err() and "NULL mb, mvf or slices" in err(), field
    pics = _dev_pics()
    pics[0].mvf += 2
    assert dev_face(8, 1, 2, 2, 1, pics) == EINVAL and "4-byte aligned" in err()
    for field, bad, word in (("mvf_stride", 7, "mvf_stride 7 (>= 8)"), ("nslices", 0, "nslices 0 (>= 1)"), ("nrefs", -1, "nrefs -1 (0..32)"),
                             ("nrefs", 33, "nrefs 33 (0..32)")):
        pics = _dev_pics()
        setattr(pics[0], field, bad)
        assert dev_face(8, 1, 2, 2, 1, pics) == EINVAL and word in err(), (field, err())
    for p in range(3):                                            # a NULL plane among the first nrefs references
        pics = _dev_pics()
        pics[0].ref[1].base[p] = None
        assert dev_face(8, 1, 2, 2, 1, pics) == EINVAL and "reference 1: plane %d is NULL" % p in err()
    pics = _dev_pics(ps=2)
    pics[0].ref[0].base[0] += 1                                   # 16-bit samples at an odd address
    assert dev_face(10, 1, 2, 2, 1, pics) == EINVAL and "multiple of the sample size" in err()
    # what is not refused: references beyond nrefs, chroma of a luma-only picture or of chroma_format_idc 0, nrefs 0 and 32
    pics = _dev_pics()
    pics[0].ref[2].base[0] = None
    assert _would_accept(8, 1, 2, 2, 1, pics)
    pics = _dev_pics(chroma=False)
    for k in range(2):
        pics[0].ref[k].base[1] = pics[0].ref[k].base[2] = None
    assert _would_accept(8, 1, 2, 2, 1, pics) and _would_accept(8, 0, 2, 2, 1, pics)
    pics = _dev_pics()
    pics[0].dst[1] = None                                         # chroma_format_idc 0: Cb / Cr are ignored
    assert _would_accept(8, 0, 2, 2, 1, pics)
    pics = _dev_pics(nrefs=0)
    assert _would_accept(8, 1, 2, 2, 1, pics)
    for bd in (9, 12, 14):
        assert _would_accept(bd, 1, 2, 2, 1, _dev_pics(ps=2))


def _frame(ps=1, mb_w=2, mb_h=2):
    """a frame buffer of 2 * 16 mb_h luma rows whose fields are pictures of mb_w x mb_h macroblocks: (bases of the three planes, strides)"""
    return [_buf(), _buf(), _buf()], [16 * mb_w * ps + 32, 8 * mb_w * ps + 16, 8 * mb_w * ps + 16]


def _field_pic(P, bases, strides, parity, as_dst=True, k=0):
    for p in range(3):
        if as_dst:
            P.dst[p], P.dst_stride[p] = bases[p] + parity * strides[p], 2 * strides[p]
        else:
            P.ref[k].base[p], P.ref[k].stride[p] = bases[p] + parity * strides[p], 2 * strides[p]


def test_row_overlap_rule_in_both_directions():
    # the second field of a frame predicted from the first, and the other way round: rows interleave, no byte is shared
    for ps, bd in ((1, 8), (2, 10)):
        for parity in (0, 1):
            pics = _dev_pics(ps=ps)
            bases, strides = _frame(ps)
            _field_pic(pics[0], bases, strides, parity)
            _field_pic(pics[0], bases, strides, 1 - parity, as_dst=False, k=1)
            assert _would_accept(bd, 1, 2, 2, 1, pics), (ps, parity)
            # the same field as destination and reference: every row is shared
            _field_pic(pics[0], bases, strides, parity, as_dst=False, k=1)
            assert dev_face(bd, 1, 2, 2, 1, pics) == EINVAL and "reference 1: a row of plane 0 overlaps a destination row" in err()
    # a reference whose rows begin inside the destination's rows (d < dst_row_bytes) or run into the next one (d + ref_row_bytes > s)
    for shift, plane in ((36, 0), (-36, 0), (20, 1), (-20, 2)):
        pics = _dev_pics()
        bases, strides = _frame()
        _field_pic(pics[0], bases, strides, 0)
        _field_pic(pics[0], bases, strides, 1, as_dst=False, k=0)
        pics[0].ref[0].base[plane] += shift
        assert dev_face(8, 1, 2, 2, 1, pics) == EINVAL and "reference 0: a row of plane %d overlaps" % plane in err(), (shift, plane)
    # d exactly at the end of the destination's row bytes: disjoint; one byte less: shared
    pics = _dev_pics()
    bases, strides = _frame()
    for p in range(3):
        pics[0].dst[p], pics[0].dst_stride[p] = bases[p], 2 * strides[p]
        pics[0].ref[0].base[p], pics[0].ref[0].stride[p] = bases[p] + (32 if p == 0 else 16), 2 * strides[p]
    assert _would_accept(8, 1, 2, 2, 1, pics)
    pics[0].ref[0].base[0] -= 1
    assert dev_face(8, 1, 2, 2, 1, pics) == EINVAL and "overlaps a destination row" in err()
    # overlapping spans with unequal strides are refused, rows disjoint or not
    pics = _dev_pics()
    bases, strides = _frame()
    _field_pic(pics[0], bases, strides, 0)
    _field_pic(pics[0], bases, strides, 1, as_dst=False, k=0)
    pics[0].ref[0].stride[0] += 4
    assert dev_face(8, 1, 2, 2, 1, pics) == EINVAL and "overlaps a destination row" in err()
    # the destination of one picture is a reference of another picture of the call
    pics = _dev_pics(2)
    for p in range(3):
        pics[1].ref[1].base[p], pics[1].ref[1].stride[p] = pics[0].dst[p], pics[0].dst_stride[p]
    assert dev_face(8, 1, 2, 2, 2, pics) == EINVAL and "picture 1: reference 1" in err()
    # two destinations: the two fields of a frame are accepted, the same field twice is not
    pics = _dev_pics(2)
    bases, strides = _frame()
    _field_pic(pics[0], bases, strides, 0)
    _field_pic(pics[1], bases, strides, 1)
    assert _would_accept(8, 1, 2, 2, 2, pics)
    _field_pic(pics[1], bases, strides, 0)
    assert dev_face(8, 1, 2, 2, 2, pics) == EINVAL and "a destination plane overlaps another destination plane" in err()
    pics = _dev_pics(3)
    pics[2].dst[2] = pics[0].dst[1] + 8
    assert dev_face(8, 1, 2, 2, 3, pics) == EINVAL and "destination plane overlaps another" in err()
    # an input table inside a destination plane
    for field in ("mb", "mvf", "slices"):
        pics = _dev_pics(2)
        setattr(pics[1], field, pics[0].dst[0] + 64)
        assert dev_face(8, 1, 2, 2, 2, pics) == EINVAL and "an input table overlaps a destination plane" in err(), field


@pytest.mark.skipif(_lib.lib().ffhip_device_count() > 0, reason="a HIP device is present: the refusal path is not reachable")
def test_no_device_comes_after_the_argument_checks():
    assert dev_face(8, 1, 2, 2, 1, _dev_pics()) == ENOSYS
    assert dev_face(14, 0, 2, 2, 17, _dev_pics(17, ps=2, chroma=False)) == ENOSYS
    pics = _dev_pics()
    pics[0].nrefs = 33
    assert dev_face(8, 1, 2, 2, 1, pics) == EINVAL
