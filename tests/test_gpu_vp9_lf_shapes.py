"""The VP9 whole-frame loop filter faces at the launch shapes test_gpu_vp9_lf_frame.py does not reach, byte for byte against the oracle's
ffo_vp9_loopfilter_sb called superblock by superblock: calls that the height splits into launches of 31 + 1 pictures (4:2:0 at 8 and 10
bits, 4:4:4 with a partial last workgroup) with twice the workgroups the device holds by LDS, 4:2:2 / 4:4:0 calls of 21 + 11 pictures with
8064 one-wave workgroups in the first launch, and the tallest picture every face takes.  The product build, no FFHIP_* variable.  Each
case first asserts, with the compute-unit count of the device it runs on, that its shape reaches its branch (row_shapes.py).

The pictures of a batch share one set of filter tables (structured masks, so the row edges read the rows above; the first and the last
superblock row with a strong filter on every block) and differ in their planes.  In every picture the filter must have changed samples in
the first and in the last superblock row."""
import numpy as np
import pytest

import row_shapes as S
import vp9_lf_gen as G
from test_gpu_vp9_lf_frame import compare, oracle_frame

pytestmark = pytest.mark.gpu
_FILTERS = {}


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _cus():
    return _torch().cuda.get_device_properties(0).multi_processor_count


def _reaches(why):
    assert why is None, "the shape no longer reaches its branch on this device (%d CUs): %s" % (_cus(), why)


def _plane(rng, h, w, pad, bd):
    """the smooth plane of test_gpu_vp9_lf_frame.py with its random walk folded into 32 .. 224: down thousands of rows the unfolded walk
    leaves the sample range, and a plane clipped flat gives the filter nothing to change"""
    walk = np.cumsum(rng.integers(-2, 3, (h, w + pad)), axis=1) + np.cumsum(rng.integers(-2, 3, (h, 1)), axis=0)
    base = np.abs(walk % 384 - 192) + 32
    base = (base << (bd - 8)) + rng.integers(0, (1 << (bd - 8)) + 1, (h, w + pad))
    base[rng.integers(0, h, 40 + h // 50), :] += 9 << (bd - 8)                      # real edges
    return np.clip(base, 0, (1 << bd) - 1).astype(np.uint8 if bd == 8 else np.uint16)


def _filters(sbc, cols, rows, ss):
    """the VP9Filter records of a picture, made once for every test of the same geometry and left unchanged"""
    key = (sbc, cols, rows, ss)
    if key not in _FILTERS:
        rng = np.random.default_rng(5000 + rows + 10 * ss[0] + ss[1])
        sbr = (rows + 7) >> 3
        filt = np.zeros(sbr * sbc, G.FILTER_DT)
        for r in range(sbr):
            for c in range(sbc):
                for _ in range(200):    # the first and the last row are drawn until every block of theirs has a strong filter
                    f = G.structured(rng, r, c, cols, rows, *ss, p_zero=.1 if 0 < r < sbr - 1 else 0.)
                    coded = f["level"][f["level"] > 0]
                    if 0 < r < sbr - 1 or (coded.size and coded.min() >= 24):
                        break
                else:
                    raise AssertionError("no strong filter drawn")
                filt[r * sbc + c] = f
        filt.setflags(write=False)
        _FILTERS[key] = filt
    return _FILTERS[key]


def _host(sbc, rows, npics, bd, ss, seed):
    """(cols, filters, planes before, planes as the oracle leaves them) of npics pictures; asserts that the pictures differ and that the
    filter changed samples in the first and in the last superblock row of every picture"""
    rng = np.random.default_rng(seed)
    lim, mblim = G.filter_lut(3)
    sbr, cols = (rows + 7) >> 3, 8 * sbc - 3
    cw, ch = 64 >> ss[0], 64 >> ss[1]
    filt = _filters(sbc, cols, rows, ss)
    before, want = [], []
    for i in range(npics):
        planes = [_plane(rng, 64 * sbr, 64 * sbc, 12, bd), _plane(rng, ch * sbr, cw * sbc, 4, bd), _plane(rng, ch * sbr, cw * sbc, 4, bd)]
        before.append([p.copy() for p in planes])
        oracle_frame(planes, filt, sbc, sbr, bd, ss, lim, mblim)
        want.append(planes)
        diff = [planes[k] != before[i][k] for k in range(3)]       # the filter worked in the first and in the last superblock row
        assert any(d[:64 if k == 0 else ch].any() for k, d in enumerate(diff)), "picture %d: the first superblock row is unchanged" % i
        assert any(d[(64 if k == 0 else ch) * (sbr - 1):].any() for k, d in enumerate(diff)), "picture %d: the last superblock row is unchanged" % i
        assert sum(int(d.sum()) for d in diff) > 20 * sbc * sbr
        assert i == 0 or all((before[i][k] != before[0][k]).any() for k in range(3))
    return cols, filt, before, want


def _case(face, sbc, rows, npics, bd, ss, seed):
    """face: 'frames' (ffhip_vp9_loopfilter_frames_dev / _frames_ssc_dev) or 'lone' (the single-picture face of the format)"""
    from ffmpeg_amd import vp9, _lib
    torch = _torch()
    L = _lib.lib()
    lim, mblim = G.filter_lut(3)
    sbr, ssc = (rows + 7) >> 3, ss[0] != ss[1]
    cols, filt, before, want = _host(sbc, rows, npics, bd, ss, seed)
    fbytes = filt.view(np.uint8).reshape(sbr * sbc, 192)
    if ssc:
        tabs, ctabs = vp9.lf_sb_tables_ss(fbytes, sbc, sbr, lim, mblim, ss)
        d_tabs = (torch.from_numpy(tabs.view(np.int32)).cuda(), torch.from_numpy(ctabs.view(np.int32)).cuda())
    else:
        d_tabs = (torch.from_numpy(vp9.lf_sb_tables(fbytes, sbc, sbr, lim, mblim).view(np.int32)).cuda(),)
    dev = [[torch.from_numpy(p.view(np.uint8).reshape(-1).copy()).cuda() for p in b] for b in before]
    sy, suv = before[0][0].strides[0], before[0][1].strides[0]
    if face == "frames" and ssc:
        vp9.loopfilter_frames_ssc([tuple(d) + d_tabs for d in dev], sy, suv, cols, rows, ss, bit_depth=bd)
    elif face == "frames":
        vp9.loopfilter_frames([tuple(d) + d_tabs for d in dev], sy, suv, cols, rows, bit_depth=bd, ss=ss)
    else:
        assert npics == 1
        if ssc:
            vp9.loopfilter_frame_ssc(dev[0][0], dev[0][1], dev[0][2], sy, suv, cols, rows, d_tabs[0], d_tabs[1], ss, bit_depth=bd)
        else:
            vp9.loopfilter_frame(dev[0][0], dev[0][1], dev[0][2], sy, suv, cols, rows, d_tabs[0], bit_depth=bd, ss=ss)
    torch.cuda.synchronize()
    assert L.ffhip_stream_synchronize(None) == 0, L.ffhip_last_error()
    for i in range(npics):          # every picture: the one that starts a second launch and the last one of the call among them
        try:
            compare(dev[i], want[i], before[i], cols, rows, ss)
        except AssertionError as e:
            raise AssertionError("picture %d of %d: %s" % (i, npics, e))


@pytest.mark.parametrize("name,ss", [("VLF_SPLIT_420", (1, 1)), ("VLF_SPLIT_420_HBD", (1, 1)), ("VLF_SPLIT_444", (0, 0))])
def test_tall_frames_split_their_counters(name, ss):
    """32 pictures of 128 superblock rows (4:4:4: 86): launches of 31 + 1; the first holds 1984 (10 bits: 3968, 4:4:4: 2046) workgroups of
    44 KB of LDS, at least twice what fits the device: a row's upper neighbour is resident only by the order of dispatch"""
    g = getattr(S, name)
    _reaches(S.vlf_split(g, _cus(), (31, 1), workgroups={"VLF_SPLIT_420": 1984, "VLF_SPLIT_420_HBD": 3968, "VLF_SPLIT_444": 2046}[name]))
    d = S.vp9_lf(cus=_cus(), **g)
    assert (d["W"], d["nwg"]) == {"VLF_SPLIT_420": (4, 32), "VLF_SPLIT_420_HBD": (2, 64), "VLF_SPLIT_444": (4, 22)}[name]
    assert name != "VLF_SPLIT_444" or d["sb_rows"] % d["W"], "a partial last workgroup"
    _case("frames", 2 if g.get("planes444") else 1, g["rows"], g["npics"], g.get("bd", 8), ss, 5100 + g["rows"] + g.get("bd", 8))


@pytest.mark.parametrize("bd,ss", [(8, (1, 0)), (10, (0, 1))], ids=["8-422", "10-440"])
def test_tall_ssc_frames_split_their_counters(bd, ss):
    """32 pictures of 128 superblock rows at 4:2:2 / 4:4:0: 384 counters a picture, launches of 21 + 11, dim3(384, 21) one-wave workgroups"""
    g = S.VLF_SSC_SPLIT
    _reaches(S.vlf_ssc_split(g, _cus(), (21, 11), (384, 21)))
    _case("frames", 1, g["rows"], g["npics"], bd, ss, 5200 + bd)


@pytest.mark.parametrize("face,bd,ss", [("lone_420", 8, (1, 1)), ("frames_420", 8, (1, 1)), ("frames_444", 8, (0, 0)), ("frames_ssc", 8, (1, 0)),
                                        ("lone_444", 10, (0, 0)), ("lone_ssc", 10, (0, 1))])
def test_the_tallest_picture_of_every_face(face, bd, ss):
    """2047 superblock rows through the lone 4:2:0 face, 1364 through every other: accepted and correct; the frames faces with one picture
    more than a launch holds (3 / 2 / 2), so the tallest picture also starts a second launch"""
    rows, per = S.VLF_TALLEST[face]
    _reaches(S.vlf_tallest(rows, face == "lone_420", ss == (0, 0), ss[0] != ss[1], per))
    lone = face.startswith("lone")
    _case("lone" if lone else "frames", 1, rows, 1 if lone else per + 1, bd, ss, 5300 + bd + rows)
