"""ffhip_hevc_intra_pictures_dev at the launch shapes the content tests (test_gpu_hevc_intra_picture.py) do not reach, byte for byte
against the same sequential model: tall pictures whose counters split a call into launches of fewer than 16 pictures; the tallest
picture the face takes, and the first one it refuses; and one launch of as many waves as a launch can have, several times what the
device holds at once, with CTB rows that hold no record between rows that do.  k_hevc_intra_pic has no ticket: it counts on
workgroups being dispatched in the order of their linear id, which only such a grid puts to the test.  Each case first asserts that
its shape reaches the branch it is meant to reach (row_shapes.py), with the compute-unit count of the device where that matters.

run() asserts that ffhip_stream_synchronize returns 0 (a lost hand-off is FFHIP_EIO there) and compares whole buffers, the stride
padding with its sentinel included; the records, CTB starts and residuals are read-only inputs that it uploads per call."""
import ctypes as C

import numpy as np
import pytest

import hevc_intra_picture_gen as G
import row_shapes as S
from ffmpeg_amd import _lib, hevc
from test_gpu_hevc_intra_picture import SENT, _torch, run

pytestmark = pytest.mark.gpu


def _cus():
    return _torch().cuda.get_device_properties(0).multi_processor_count


def _reaches(why):
    assert why is None, "the shape no longer reaches its branch on this device (%d CUs): %s" % (_cus(), why)


def test_tall_420_pictures_split_their_counters():
    """512 CTB rows x 3 planes: five pictures a launch, 11 pictures in launches of 5 + 5 + 1"""
    g = S.HEVC_SPLIT_420
    _reaches(S.hevc_split(g["height"], g["log2_ctb"], g["cfi"], g["npics"], g["launches"]))
    rng = np.random.default_rng(3100)
    run([G.Picture(rng, 16, g["height"], g["log2_ctb"], 8, g["cfi"], p_intra=0.8) for _ in range(g["npics"])])


def test_tall_400_pictures_split_just_below_16():
    """513 CTB rows of one plane: 15 pictures a launch, 16 pictures in launches of 15 + 1"""
    g = S.HEVC_SPLIT_400
    _reaches(S.hevc_split(g["height"], g["log2_ctb"], g["cfi"], g["npics"], g["launches"]))
    rng = np.random.default_rng(3200)
    run([G.Picture(rng, 16, g["height"], g["log2_ctb"], 10, g["cfi"], p_intra=0.8) for _ in range(g["npics"])])


def test_the_tallest_picture_the_face_takes():
    """8190 counters, one picture a launch; two pictures, so the second launch follows the first on a slot of its own"""
    g = S.HEVC_LIMIT
    assert S.hevc_accepted(**g) and not S.hevc_accepted(**S.HEVC_PAST_LIMIT) and S.hevc_per(**g) == 1
    assert S.hevc_rows(**g) + 3 > S.SLOT_INTS, "one more CTB row no longer fits"
    rng = np.random.default_rng(3300)
    run([G.Picture(rng, 16, g["height"], g["log2_ctb"], 8, g["cfi"], p_intra=0.7),
         G.Picture(rng, 16, g["height"], g["log2_ctb"], 8, g["cfi"], p_intra=0.7)])


def test_one_ctb_row_more_is_refused():
    """8193 counters: FFHIP_EINVAL, and the plane is not written.  The face's comparison (rows > FFHIP_PROGRESS_SLOT_INTS) agrees with
    the launcher's per = FFHIP_PROGRESS_SLOT_INTS / rows: whatever is accepted gets per >= 1."""
    torch = _torch()
    g = S.HEVC_PAST_LIMIT
    assert not S.hevc_accepted(**g) and S.hevc_accepted(g["height"] - 16, g["log2_ctb"], g["cfi"])
    W, H = 16, g["height"]
    keep, planes = [], []
    for p in range(3):
        h, w = (H, W) if p == 0 else (H // 2, W // 2)
        keep.append([torch.full((h * 64,), SENT, dtype=torch.uint8).cuda(), torch.zeros(16, dtype=torch.uint8).cuda(),
                     torch.zeros(((H + 15) // 16) + 1, dtype=torch.int32).cuda(), torch.zeros(16, dtype=torch.int16).cuda()])
        planes.append(hevc.IntraPlane(keep[p][0].data_ptr(), 64, keep[p][1].data_ptr(), keep[p][2].data_ptr(), keep[p][3].data_ptr()))
    arr = (hevc.IntraPic * 1)()
    for p in range(3):
        arr[0].plane[p] = planes[p]
    rc = _lib.lib().ffhip_hevc_intra_pictures_dev(8, g["cfi"], W, H, g["log2_ctb"], 1, C.cast(arr, C.c_void_p), None)
    assert rc == _lib.EINVAL, rc
    assert b"progress pool" in _lib.lib().ffhip_last_error()
    assert _lib.lib().ffhip_stream_synchronize(None) == 0
    for p in range(3):
        assert bool((keep[p][0] == SENT).all())


@pytest.mark.parametrize("bd", [8, 10])
def test_a_grid_far_past_residency(bd):
    """16 pictures x 512 CTB rows in one launch: 8192 workgroups, every counter of the slot, at least four times what the device
    holds; CTB rows 5, 9, 10 of every 16 hold no record (k0 == k1 across the row) and still publish"""
    g = S.HEVC_RESIDENCY
    _reaches(S.hevc_past_residency(cus=_cus(), **g))
    ctb_h = g["height"] >> g["log2_ctb"]
    quiet = [r for r in range(ctb_h) if r % 16 in (5, 9, 10)]
    rng = np.random.default_rng(3400 + bd)
    pics = [G.Picture(rng, 32, g["height"], g["log2_ctb"], bd, g["cfi"], p_intra=1.0, inter_rows=quiet) for _ in range(g["npics"])]
    for pic in pics:
        assert pic.ctb_w == 2 and pic.ctb_h == ctb_h
        per_row = np.diff(pic.pack(0, dtype=hevc.INTRA_TU_DTYPE)[1].astype(np.int64)).reshape(ctb_h, pic.ctb_w)
        assert not per_row[quiet].any() and per_row[[r for r in range(ctb_h) if r not in quiet]].all()
    run(pics)
