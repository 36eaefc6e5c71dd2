"""VP8 whole-frame reconstruction without a GPU: the two statements of the model agree on generated frames, the device-free faces
ffhip_vp8_mb_preds / ffhip_vp8_intra_modes (the rules the kernels run, on the host) equal the model's, the record's size, and every
refusal of ffhip_vp8_recon_frames_dev."""
import collections
import ctypes as C
import itertools

import numpy as np
import pytest

from ffmpeg_amd import _lib, vp8

import vp8_recon_gen as G
import vp8_recon_model as RM

EINVAL = -22
CASES = [  # seed, mb_w, mb_h, keyframe, kwargs
    (1, 5, 4, True, {}), (2, 4, 5, True, {}), (3, 1, 1, True, {}), (4, 1, 4, True, {}), (5, 4, 1, True, {}),
    (11, 6, 5, False, dict(intra=0.25)), (12, 5, 6, False, dict(intra=0.25, far=0.3)), (13, 4, 4, False, dict(intra=0.2, fullpel=1)),
    (14, 4, 4, False, dict(intra=0.2, bilinear=1)), (15, 1, 1, False, dict(intra=0.0)), (16, 5, 5, False, dict(intra=0.3, mv_range=7)),
] + [(20 + i, 3, 3, True, {}) for i in range(40)]   # 3 x 3: every border class once per frame
CASES += [(200 + i, 8, 8, False, dict(intra=0.05, mv_range=12)) for i in range(4)]   # every partitioning x [v][h] slot
CASES += [(100 + i, 1, 1, True, dict(i4=1.0)) for i in range(80)]        # one I4x4 macroblock: every sub-block border class


def _case(seed, mb_w, mb_h, key, kw):
    kw = dict(kw)
    bil, full = kw.pop("bilinear", 0), kw.pop("fullpel", 0)
    mbs, co = G.frame(seed, mb_w, mb_h, keyframe=key, **kw)
    refs = [G.planes(100 * seed + r, mb_w, mb_h) for r in range(3)]
    return mbs, co, refs, bil, full


@pytest.mark.parametrize("seed,mb_w,mb_h,key,kw", CASES)
def test_plane_rule_equals_pointer_route(seed, mb_w, mb_h, key, kw):
    mbs, co, refs, bil, full = _case(seed, mb_w, mb_h, key, kw)
    a = RM.recon_frame(G.planes(7, mb_w, mb_h), mbs, co, refs, mb_w, mb_h, bil, full)
    b = RM.recon_frame_ptr(G.planes(7, mb_w, mb_h), mbs, co, refs, mb_w, mb_h, bil, full)
    for p in range(3):
        assert np.array_equal(a[p], b[p]), "plane %d" % p


def test_generated_frames_cover_every_case():
    """coverage is a condition: every (mode x border class), partitioning x [v][h] slot, block code, y2 value and reference is met"""
    n16, nch, n4 = collections.Counter(), collections.Counter(), collections.Counter()
    slots, codes, y2, refs = collections.Counter(), collections.Counter(), collections.Counter(), collections.Counter()
    for seed, mb_w, mb_h, key, kw in CASES:
        mbs, co, _, bil, full = _case(seed, mb_w, mb_h, key, kw)
        for m, mb in enumerate(mbs):
            mb_x, mb_y = m % mb_w, m // mb_w
            cls = G.border_class(mb_x, mb_y, mb_w, mb_h)
            y2[int(mb["y2"])] += 1
            for b in range(24):
                codes[RM.code(mb, b)] += 1
            if mb["ref_frame"]:
                refs[int(mb["ref_frame"])] += 1
                for c in RM.mb_preds(mb, mb_x, mb_y, full):
                    slots[(int(mb["partitioning"]), c["vslot"], c["hslot"])] += 1
            else:
                nch[(int(mb["chroma_mode"]), cls)] += 1
                if mb["mode"] == RM.MODE_I4x4:
                    for i in range(16):
                        bx, by = 4 * mb_x + (i & 3), 4 * mb_y + (i >> 2)
                        c4 = 3 * (0 if by == 0 else 2 if by == 4 * mb_h - 1 else 1) + (0 if bx == 0 else 2 if bx == 4 * mb_w - 1 else 1)
                        n4[(int(mb["sub_mode"][i]), c4)] += 1
                else:
                    n16[(int(mb["mode"]), cls)] += 1
    for mode, cls in itertools.product(range(4), range(9)):
        assert n16[(mode, cls)] > 0 and nch[(mode, cls)] > 0, (mode, cls)
    for mode, cls in itertools.product(range(10), range(9)):
        assert n4[(mode, cls)] > 0, (mode, cls)
    for part, v, h in itertools.product(range(5), range(3), range(3)):
        assert slots[(part, v, h)] > 0, (part, v, h)
    assert all(codes[c] > 0 for c in range(3)) and all(y2[v] > 0 for v in range(3)) and all(refs[r] > 0 for r in (1, 2, 3))


def test_record_size_is_the_dtype():
    assert vp8.mb_record_size() == vp8.MB_DTYPE.itemsize == 96


def _same_calls(mb, mb_x, mb_y, full):
    got, want = vp8.mb_preds(mb, mb_x, mb_y, full), RM.mb_preds(mb, mb_x, mb_y, full)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert {k: int(g[k]) for k in w} == w


def test_mb_preds_equals_the_model():
    mb = np.zeros(1, vp8.MB_DTYPE)[0]
    mb["ref_frame"] = 1
    rng = np.random.default_rng(5)
    for part in range(5):
        mb["partitioning"] = part
        for full in (0, 1):
            # both signs and all eight fractions per axis (luma quarters doubled: 0, 2, 4, 6; chroma eighths: 0..7)
            for fx, fy in itertools.product(range(8), range(8)):
                for sx, sy in itertools.product((-1, 1), (-1, 1)):
                    base = np.array([sx * (8 * 3 + fx), sy * (8 * 2 + fy)])
                    mb["mv"] = base[None, :] + (rng.integers(-3, 4, (16, 2)) if part == RM.PART_4x4 else 0)
                    _same_calls(mb, 2, 1, full)
            for _ in range(50):
                mb["mv"] = rng.integers(-32768, 32768, (16, 2))
                _same_calls(mb, int(rng.integers(0, 1024)), int(rng.integers(0, 1024)), full)
    # the 4x4 chroma rounding at negative sums: (s + 2 + (s >> 31)) >> 2 for s = -1 .. -9
    mb["partitioning"] = RM.PART_4x4
    for s in range(-9, 10):
        mb["mv"] = 0
        mb["mv"][0] = (s, -s)
        _same_calls(mb, 0, 0, 0)
        want = (s + 2 + (-1 if s < 0 else 0)) >> 2
        c = vp8.mb_preds(mb, 0, 0, 0)[16]
        assert (int(c["sx"]) * 8 + int(c["mx"])) == want
    mb["ref_frame"] = 0
    with pytest.raises(RuntimeError):
        vp8.mb_preds(mb, 0, 0, 0)


def test_intra_modes_equals_the_model():
    mb = np.zeros(1, vp8.MB_DTYPE)[0]
    for mb_x, mb_y in itertools.product((0, 1, 7), (0, 1, 7)):   # the nine border classes of an 8 x 8 frame
        for mode, ch in itertools.product(range(4), range(4)):
            mb["mode"], mb["chroma_mode"] = mode, ch
            got, want = vp8.intra_modes(mb, mb_x, mb_y), RM.intra_modes(mb, mb_x, mb_y)
            assert (int(got["mode16"]), int(got["chroma"])) == (want["mode16"], want["chroma"])
            assert not got["sub"].any() and not got["copy"].any()
        mb["mode"] = RM.MODE_I4x4
        for sub in range(10):
            mb["sub_mode"] = sub
            got, want = vp8.intra_modes(mb, mb_x, mb_y), RM.intra_modes(mb, mb_x, mb_y)
            assert int(got["mode16"]) == RM.PRED_NONE == 255
            assert got["sub"].tolist() == want["sub"] and got["copy"].tolist() == want["copy"]
    mb["sub_mode"] = 10
    with pytest.raises(RuntimeError):
        vp8.intra_modes(mb, 0, 0)


def test_refusals_need_no_device():
    """every refusal is FFHIP_EINVAL before any device check (the pointers are never dereferenced on the host)"""
    L = _lib.lib()
    W, H, sy, suv = 4, 3, 64, 32
    ysz, csz = sy * 16 * H, suv * 8 * H

    def pic(**kw):
        base = 0x10000000
        p = vp8.ReconPic()
        p.y, p.u, p.v = base, base + ysz, base + ysz + csz
        for k in range(3):
            p.ref[0][k] = base + 0x100000 + (0, ysz, ysz + csz)[k]
        p.mbs, p.coeffs, p.coeff_count = base + 0x200000, base + 0x300000, 400 * W * H
        for k, v in kw.items():
            if k == "ref0":
                p.ref[0][v[0]] = v[1]
            else:
                setattr(p, k, v)
        return p

    def call(p, mb_w=W, mb_h=H, bil=0, full=0, n=1, s_y=sy, s_uv=suv, null=False):
        arr = (vp8.ReconPic * max(n, 1))(*([p] * max(n, 1)))
        return L.ffhip_vp8_recon_frames_dev(mb_w, mb_h, bil, full, n, None if null else C.cast(arr, C.c_void_p), s_y, s_uv, None)

    good = pic()
    assert call(good, null=True) == EINVAL and call(good, n=0) == EINVAL and call(good, n=-1) == EINVAL
    for bad in (0, 1025):
        assert call(good, mb_w=bad, s_y=16 * 1025 + 4 - (16 * 1025 + 4) % 4) == EINVAL and call(good, mb_h=bad) == EINVAL
    assert call(good, bil=2) == EINVAL and call(good, full=2) == EINVAL
    assert call(good, s_y=sy + 2) == EINVAL and call(good, s_uv=suv + 1) == EINVAL
    assert call(good, s_y=16 * W - 4) == EINVAL and call(good, s_uv=8 * W - 4) == EINVAL
    for name in ("y", "u", "v", "mbs", "coeffs"):
        assert call(pic(**{name: None})) == EINVAL, name
    for name in ("y", "u", "v"):
        assert call(pic(**{name: getattr(good, name) + 2})) == EINVAL, name
    assert call(pic(ref0=(1, good.ref[0][1] + 1))) == EINVAL                 # a misaligned reference plane
    assert call(pic(ref0=(0, good.y + 16))) == EINVAL                         # a reference inside a destination
    assert call(pic(ref0=(2, good.v - 8 * suv))) == EINVAL                    # ... reaching into one from before it
    assert call(pic(u=good.y + 16 * sy)) == EINVAL                            # destinations overlap
    assert call(good, n=2) == EINVAL                                          # the same frame twice
    # and a well-formed call gets past them: no device here means FFHIP_ENOSYS, a device means it would run (not tried)
    if L.ffhip_device_count() == 0:
        assert call(good) == -38
