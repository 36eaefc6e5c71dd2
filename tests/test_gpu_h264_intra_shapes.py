"""ffhip_h264_intra_frames_dev at the launch shapes test_gpu_h264_intra_batch.py does not reach: one workgroup set that reconstructs
luma and chroma (parts == 3: 32 pictures of 10 workgroups are past the 576 up to which chroma gets a wavefront of its own), a call the
height splits into launches of 31 + 1 pictures with three times the workgroups the device holds with the kernel as compiled, and the widths at which the launcher
itself takes 3 and 2 rows a workgroup for the LDS of the line buffers.  The product build, no FFHIP_* variable.  Each case first asserts,
with the compute-unit count of the device it runs on, that its shape reaches its branch (row_shapes.py).

Every picture of a batch equals a launch of its own (ffhip_h264_intra_frame_dev[_hbd]: one picture always takes the split path, so the
unsplit batches pit the two paths against each other) and a reference that knows nothing of the launcher's W, LDS and split: at 8 bits
the oracle's hl_decode_mb() macroblock by macroblock, above 8 bits the kernel's per-macroblock logic run serially on the CPU
(oracle/libffemul.so, which test_h264_intra_cpu.py pins to the reference's ff_h264_hl_decode_mb() at depth).  The pictures
of a batch share their records and coefficient runs (the host-side generation is the cost of these tests) and differ in their planes:
a third of the macroblocks are inter, so what every intra macroblock next to one predicts from is the picture's own."""
import ctypes as C
import os

import numpy as np
import pytest

import ffi
import h264_intra_gen as G
import row_shapes as S
from test_gpu_h264_intra_batch import IntraPic, _pack_picture

pytestmark = pytest.mark.gpu
FRAC = 0.67
EMUL_SO = os.path.join(ffi.ROOT, "oracle", "libffemul.so")


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _cus():
    return _torch().cuda.get_device_properties(0).multi_processor_count


def _reaches(why):
    assert why is None, "the shape no longer reaches its branch on this device (%d CUs): %s" % (_cus(), why)


def _case(g, seed):
    from ffmpeg_amd import _lib
    torch = _torch()
    L = _lib.lib()
    L.ffhip_h264_intra_pack.restype = C.c_int
    L.ffhip_h264_intra_pack_hbd.restype = C.c_int
    mb_w, mb_h, npics, depth = g["mb_w"], g["mb_h"], g["npics"], g.get("bd", 8)
    rng = np.random.default_rng(seed)
    ps = 2 if depth > 8 else 1
    sy, sc = mb_w * 16 * ps, mb_w * 8 * ps
    dt = np.uint16 if depth > 8 else np.uint8
    rec, rows, coefs, states = _pack_picture(L, rng, mb_w, mb_h, FRAC, depth)
    assert len(states) > mb_w * mb_h // 2 and (np.diff(rows) > 0).sum() > mb_h // 2 and (np.diff(rows) < mb_w).any()
    d_rec = torch.from_numpy(rec.view(np.uint8).reshape(-1, 108).copy()).cuda()
    d_rows, d_coef = torch.from_numpy(rows).cuda(), torch.from_numpy(coefs).cuda()
    shapes = [(mb_h * 16, mb_w * 16), (mb_h * 8, mb_w * 8), (mb_h * 8, mb_w * 8)]
    before, batch, single, pics = [], [], [], []
    for i in range(npics):
        planes = [rng.integers(0, 1 << depth, s).astype(dt) for s in shapes]
        a = [torch.from_numpy(p.view(np.uint8).reshape(p.shape[0], -1).copy()).cuda() for p in planes]
        before.append(planes)
        batch.append(a)
        single.append([t.clone() for t in a])
        pics.append(IntraPic(a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), d_rec.data_ptr(), d_rows.data_ptr(), d_coef.data_ptr()))
    arr = (IntraPic * npics)(*pics)
    _lib.check(L.ffhip_h264_intra_frames_dev(depth, npics, C.cast(arr, C.c_void_p), sy, sc, mb_w, mb_h, None), "ffhip_h264_intra_frames_dev")
    for b in single:
        if depth > 8:
            _lib.check(L.ffhip_h264_intra_frame_dev_hbd(depth, b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), sy, sc, mb_w, mb_h, d_rec.data_ptr(),
                                                        d_rows.data_ptr(), d_coef.data_ptr(), None), "ffhip_h264_intra_frame_dev_hbd")
        else:
            _lib.check(L.ffhip_h264_intra_frame_dev(b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), sy, sc, mb_w, mb_h, d_rec.data_ptr(),
                                                    d_rows.data_ptr(), d_coef.data_ptr(), None), "ffhip_h264_intra_frame_dev")
    torch.cuda.synchronize()
    assert L.ffhip_stream_synchronize(None) == 0, L.ffhip_last_error()
    O = ffi.oracle() if depth == 8 else None
    E = None if depth == 8 else C.CDLL(EMUL_SO)
    if E is not None:
        E.ffemul_h264_intra_set_split(0)
        E.ffemul_h264_intra_frame_bd.argtypes = [C.c_int] + [C.c_void_p] * 3 + [C.c_ssize_t] * 2 + [C.c_int] * 2 + [C.c_void_p] * 3
    for i in range(npics):          # every picture: the one that starts a second launch and the last one of the call among them
        got = [t.cpu().numpy() for t in batch[i]]
        for pl in range(3):
            b = single[i][pl].cpu().numpy()
            bad = np.argwhere(got[pl] != b)
            assert bad.size == 0, "picture %d of %d, plane %d: %d bytes differ from its own launch, first %s" % (i, npics, pl, len(bad), bad[:3].tolist())
            assert (got[pl] != before[i][pl].view(np.uint8).reshape(got[pl].shape)).sum() > got[pl].size // 4, (i, pl)
        want = [p.copy() for p in before[i]]
        if O is not None:
            for d in states:
                G.oracle_decode(O, d, want, [sy, sc, sc])
        else:
            assert E.ffemul_h264_intra_frame_bd(depth, want[0].ctypes.data, want[1].ctypes.data, want[2].ctypes.data, sy, sc, mb_w, mb_h,
                                                rec.ctypes.data, rows.ctypes.data, coefs.ctypes.data) == 0
        for pl in range(3):
            bad = np.argwhere(got[pl] != want[pl].view(np.uint8).reshape(got[pl].shape))
            assert bad.size == 0, "picture %d of %d, plane %d: %d bytes differ from the %s, first %s" % (
                i, npics, pl, len(bad), "oracle" if O is not None else "serial emulation", bad[:3].tolist())


@pytest.mark.parametrize("name", ["IF_UNSPLIT", "IF_UNSPLIT_HBD"])
def test_one_workgroup_set_for_luma_and_chroma(name):
    g = getattr(S, name)
    _reaches(S.if_unsplit(g, _cus()))
    _case(g, 4000 + g["mb_w"])


def test_tall_pictures_split_their_counters():
    """32 pictures of 256 rows: 257 counters a picture, launches of 31 + 1; the first has 31 x 64 = 1984 workgroups against the 2 a CU
    that the kernel's register count leaves as it is compiled (row_shapes.INTRA_WG_PER_CU; its launch bounds only keep that achievable and
    cap nothing, and by waves and LDS a CU could hold 8, 2048 at 256 CUs, so this is not proved from an upper bound): with most workgroups
    waiting to be dispatched, a row's upper neighbour is resident only because workgroups are dispatched x-fastest"""
    g = S.IF_HEIGHT_SPLIT
    _reaches(S.if_height_split(g, _cus(), (31, 1)))
    _case(g, 4100)


@pytest.mark.parametrize("depth,W", sorted(S.IF_WIDTHS))
def test_the_rows_of_a_workgroup_by_the_width(depth, W):
    """the last width at which the line buffers of 4 rows fit beside the static tiles in 64 KB of LDS, the first of 3 rows and the first
    of 2, at 8 and 10 bits: the launcher's own W and its dynamic LDS"""
    g = dict(mb_w=S.IF_WIDTHS[depth, W], mb_h=S.IF_W_ROWS, npics=S.IF_W_PICS, bd=depth)
    _reaches(S.if_w(g, _cus(), W))
    _case(g, 4200 + 10 * depth + W)
