"""The frame-order H.264 deblocking faces at the launch shapes the content tests of test_gpu_h264.py and test_gpu_h264_hbd.py do not
reach, byte for byte against the oracle's serial order (ffo_h264_deblock_frame, _chroma, _bd, one call a picture): workgroups of
k_h264_deblock_skew that walk several super-bands, the floor on the waves of a picture, calls whose counters take several slots (the
offsets of a second launch), 16-bit luma with three waves a workgroup, the 16-row band kernel chosen by the size of the call alone, and the
byte-path row kernel split by height.  The product build, no FFHIP_* variable.  Each case first asserts, with the compute-unit count of
the device it runs on, that its shape reaches the branch it is meant to reach (row_shapes.py).

Planes and edge records are made as test_gpu_h264.py::test_deblock_frame makes them: smooth planes, the alpha / beta ladder, 25 % intra
edges, 15 % skipped; whole buffers are compared, stride padding included, and every picture must have been changed by the filter."""
import ctypes as C

import numpy as np
import pytest

import ffi
import row_shapes as S
from ffi import u8p
from test_gpu_h264 import EDGE_DT, LADDER, _torch
from test_gpu_h264_picture import _record_one

pytestmark = pytest.mark.gpu


def _cus():
    return _torch().cuda.get_device_properties(0).multi_processor_count


def _reaches(why):
    assert why is None, "the shape no longer reaches its branch on this device (%d CUs): %s" % (_cus(), why)


def _stride(g):
    """bytes: the macroblocks of a row and the smallest padding (0, 8, 4 or 3 bytes) that gives the stride the alignment of the shape"""
    ps, n = (2 if g.get("bd", 8) > 8 else 1), (8 if g.get("chroma") else 16)
    for pad in (0, 8, 4, 3):
        stride = g["mb_w"] * n * ps + pad
        if min(16, stride & -stride) == g.get("align", 16):
            return stride
    raise AssertionError("no stride of alignment %d" % g.get("align", 16))


def _host(g, seed):
    """(stride, planes, edge records, planes as the oracle leaves them) of the nf pictures; asserts that the filter changed every picture"""
    O = ffi.oracle()
    O.ffo_h264_deblock_frame_bd.argtypes = [C.c_int, C.c_int, u8p, C.c_ssize_t, C.c_int, C.c_int, C.c_void_p]
    mb_w, mb_h, nf, chroma, bd = g["mb_w"], g["mb_h"], g["nf"], bool(g.get("chroma")), g.get("bd", 8)
    rng = np.random.default_rng(seed)
    ps, n_s = (2 if bd > 8 else 1), (8 if chroma else 16)
    h, stride = mb_h * n_s, _stride(g)
    assert min(16, (stride | h * stride) & -(stride | h * stride)) == g.get("align", 16)
    # smooth planes (small steps, so that |p0 - q0| < alpha fires often); the padding of a row holds samples of the same kind
    cols = stride // ps if ps == 2 else stride
    base = rng.integers(0, 1 << bd, (nf, h // 8 + 1, cols // 8 + 1)).astype(np.int32)
    step = 6 << (bd - 8)
    planes = np.clip(np.kron(base, np.ones((8, 8), np.int32))[:, :h, :cols] + rng.integers(-step, step + 1, (nf, h, cols)), 0, (1 << bd) - 1)
    planes = np.ascontiguousarray(planes.astype(np.uint16 if ps == 2 else np.uint8))
    ne = 4 if chroma else 8
    n = mb_w * mb_h * ne
    ed = np.zeros(nf * n, EDGE_DT)
    lad = np.array(LADDER)
    sel = rng.integers(0, len(LADDER), nf * n)
    ed["alpha"], ed["beta"] = lad[sel, 0], lad[sel, 1]
    ed["kind"] = np.where(rng.random(nf * n) < .25, 6 if chroma else 4, 2 if chroma else 0)
    ed["tc0"] = rng.integers(-1, 5, (nf * n, 4))
    ed["alpha"][rng.random(nf * n) < .15] = 0            # skipped edges
    want = planes.copy()
    for f in range(nf):
        at, e = C.cast(want[f].ctypes.data, u8p), C.c_void_p(ed[f * n:].ctypes.data)
        if bd > 8:
            O.ffo_h264_deblock_frame_bd(bd, int(chroma), at, stride, mb_w, mb_h, e)
        elif chroma:
            O.ffo_h264_deblock_frame_chroma(at, stride, mb_w, mb_h, e)
        else:
            O.ffo_h264_deblock_frame(at, stride, mb_w, mb_h, e)
        assert (want[f] != planes[f]).sum() > 10 * mb_h, "picture %d: the filter changed next to nothing" % f
    return stride, planes, ed, want


def _case(g, seed):
    """nf pictures at a constant pitch through the face of their depth == the oracle picture by picture"""
    from ffmpeg_amd import h264, _lib
    torch = _torch()
    mb_w, mb_h, nf, chroma, bd = g["mb_w"], g["mb_h"], g["nf"], bool(g.get("chroma")), g.get("bd", 8)
    stride, planes, ed, want = _host(g, seed)
    h = mb_h * (8 if chroma else 16)
    d = torch.from_numpy(planes.view(np.uint8).reshape(nf, h, stride)).cuda()
    d_ed = torch.from_numpy(ed.view(np.uint8).reshape(-1, 12)).cuda()
    assert d.data_ptr() % 16 == 0 and d_ed.data_ptr() % 16 == 0
    if bd > 8:
        h264.deblock_frames_hbd(bd, d, h * stride, nf, stride, mb_w, mb_h, d_ed, chroma=chroma)
    elif chroma:
        h264.deblock_frames_chroma(d, h * stride, nf, stride, mb_w, mb_h, d_ed)
    elif nf == 1:
        h264.deblock_frame(d, stride, mb_w, mb_h, d_ed)
    else:
        h264.deblock_frames(d, h * stride, nf, stride, mb_w, mb_h, d_ed)
    torch.cuda.synchronize()
    L = _lib.lib()
    assert L.ffhip_stream_synchronize(None) == 0, L.ffhip_last_error()
    got = d.cpu().numpy().view(planes.dtype).reshape(planes.shape)
    for f in range(nf):             # every picture: the one that starts a second launch and the last one of the call among them
        bad = np.argwhere(got[f] != want[f])
        assert bad.size == 0, "picture %d of %d: %d mismatches, first (row, column) %s" % (f, nf, len(bad), bad[:4].tolist())


@pytest.mark.parametrize("name,kw", [("DB_SUPERBANDS", {}), ("DB_SUPERBANDS_RAGGED", dict(ragged=2)), ("DB_SUPERBANDS_ODD", dict(idle=True))])
def test_a_workgroup_walks_several_super_bands(name, kw):
    """a lone picture of 511 / 512 bands: 128 waves, 32 workgroups that each reuse their strip and count their LDS hand-offs across 4
    super-bands; the last band 2 rows high; the last super-band with an idle wave"""
    g = getattr(S, name)
    _reaches(S.db_superbands(g, _cus(), **kw))
    _case(g, 3000 + g["mb_h"])


def test_the_floor_on_the_waves_of_a_picture():
    """9 pictures, two an XCD: 128 / 2 = 64 waves a picture lose against a quarter of the 512 bands; 7 of the 16 picture places of the
    grid hold no picture and their workgroups leave at once"""
    g = S.DB_FLOOR
    _reaches(S.db_floor(g, _cus()))
    _case(g, 3100)


@pytest.mark.parametrize("name,kernel,launches", [("DB_SPLIT", "skew", (16, 1)), ("DB_SPLIT_CHROMA", "skew", (16, 1)), ("DB_ROW_SPLIT", "row", (13, 1))])
def test_a_call_of_several_slots(name, kernel, launches):
    """the second launch starts at plane + f0 * frame_pitch and edges + f0 * mb_w * mb_h * ne: luma and chroma on the skewed-rows kernel,
    and the row kernel of the byte path (a counter a row and one more a frame)"""
    g = getattr(S, name)
    _reaches(S.db_split(g, _cus(), launches, kernel))
    _case(g, 3200 + g["nf"] + g["mb_h"])


def test_three_waves_a_workgroup_at_16_bits():
    """10-bit luma: 250 bands in 84 super-bands of three (the last with two idle waves) on 43 workgroups"""
    g = S.DB_HBD_WPB3
    _reaches(S.db_hbd_wpb3(g, _cus()))
    _case(g, 3300)


@pytest.mark.parametrize("name,partial", [("DB_BAND16", True), ("DB_BAND16_CHROMA", False)])
def test_the_16_row_band_kernel_by_the_size_of_the_call(name, partial):
    """dword-aligned strides: k_h264_deblock_band<., 16>, for luma through 2057 rows (129 bands, the last of 9 rows), for chroma through
    33 pictures of 70 rows"""
    g = getattr(S, name)
    _reaches(S.db_band16(g, _cus(), partial))
    _case(g, 3400 + g["nf"])


class _FilterWatch:
    """the oracle, noting how many samples each of its whole-plane deblocking calls changes (_record_one ends a picture with three)"""

    def __init__(self, O):
        self._O, self.changed = O, []

    def __getattr__(self, name):
        return getattr(self._O, name)

    def _run(self, fn, rows, p, stride, mb_w, mb_h, ed):
        a = np.ctypeslib.as_array(p, shape=(mb_h * rows * stride,))
        before = a.copy()
        fn(p, stride, mb_w, mb_h, ed)
        self.changed.append(int((a != before).sum()))

    def ffo_h264_deblock_frame(self, *a):
        self._run(self._O.ffo_h264_deblock_frame, 16, *a)

    def ffo_h264_deblock_frame_chroma(self, *a):
        self._run(self._O.ffo_h264_deblock_frame_chroma, 8, *a)


def test_one_picture_more_than_the_pointer_table_holds():
    """33 picture objects flushed together (ffhip_h264_pictures_flush): their luma planes, and beside them their 66 chroma planes, go
    through ffhip_launch_h264_deblock_pictures_bd, whose table of 32 planes and edge-record pointers, not the slot, cuts the calls into
    launches of 32 + 1 and 32 + 32 + 2; the later launches read the host tables from f0 on.  Every picture == the oracle's decode of it
    (prediction, residual, then ffo_h264_deblock_frame and _chroma), whole planes with their padding; the planes of the pictures differ"""
    from ffmpeg_amd import h264, _lib
    torch = _torch()
    O, L = _FilterWatch(ffi.oracle()), _lib.lib()
    g, gc = S.DB_PTRS_SPLIT, S.DB_PTRS_SPLIT_CHROMA
    mb_w, mb_h, n = g["mb_w"], g["mb_h"], g["nf"]
    P = 32
    W, H = mb_w * 16, mb_h * 16
    sy, sc = W + 2 * P, W // 2 + P
    strides = [sy, sc, sc]
    assert sy % 16 == 0 and sc % 8 == 0 and gc["nf"] == 2 * n and (gc["mb_w"], gc["mb_h"]) == (mb_w, mb_h)
    _reaches(S.db_ptrs(g, _cus(), (32, 1)))
    _reaches(S.db_ptrs(gc, _cus(), (32, 32, 2)))
    rng = np.random.default_rng(3500)
    refs = [rng.integers(0, 256, (2 * (H + 2 * P), sy), dtype=np.uint8), rng.integers(0, 256, (2 * (H // 2 + P), sc), dtype=np.uint8),
            rng.integers(0, 256, (2 * (H // 2 + P), sc), dtype=np.uint8)]
    d_refs = [torch.from_numpy(r).cuda() for r in refs]
    pics, wants, dsts = [], [], []
    for it in range(n):
        pic = h264.Picture(mb_w, mb_h)
        dst0, want = _record_one(pic, rng, O, h264, mb_w, mb_h, P, refs, strides, 0.0)
        # (random references predict rough planes: few chroma edges pass their thresholds, but more than a handful in every plane)
        assert len(O.changed) == 3 * (it + 1) and O.changed[-3] > 10 * mb_h and min(O.changed[-2:]) > mb_h, \
            "picture %d: the filter changed next to nothing: %s" % (it, O.changed[-3:])
        pics.append(pic)
        wants.append(want)
        dsts.append([torch.from_numpy(a.copy()).cuda() for a in dst0])
    assert all(t.data_ptr() % 16 == 0 for d in dsts for t in d)
    h264.pictures_flush(pics, dsts, strides, [d_refs] * n)
    torch.cuda.synchronize()
    assert L.ffhip_stream_synchronize(None) == 0, L.ffhip_last_error()
    assert all(L.ffhip_h264_picture_status(p_._p) == 0 for p_ in pics)
    for it in range(n):             # every picture: those that start the later launches (32; chroma planes 64 and 65) among them
        for pl in range(3):
            bad = np.argwhere(dsts[it][pl].cpu().numpy() != wants[it][pl])
            assert bad.size == 0, "picture %d of %d, plane %d: %d mismatches, first (row, column) %s" % (it, n, pl, len(bad), bad[:4].tolist())
    for p_ in pics:
        p_.close()
