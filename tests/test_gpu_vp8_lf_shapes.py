"""ffhip_vp8_loopfilter_frames_dev at the launch shapes the frame-filter tests of test_gpu_vp8dsp.py do not reach, byte for byte
against vp8dsp_model.loop_filter_frame: a launch of more units than the grid holds (one wave of k_vp8_lf_frame walks several rows), and
calls that the height splits into launches of fewer than 16 frames.  Normal and simple filter, key and inter frames, the content and
the strengths of the frame-filter tests; one more case has rows in which no record filters anything.  Each case first asserts, with
the compute-unit count of the device it runs on, that its shape reaches the branch it is meant to reach (row_shapes.py).

_frame_case asserts that ffhip_stream_synchronize returns 0 and compares whole buffers, stride padding and the rows below included."""
import numpy as np
import pytest

import row_shapes as S
import test_gpu_vp8dsp as D
from test_gpu_vp8dsp import _frame_case, _torch

pytestmark = pytest.mark.gpu

assert (S.V8F_PICS, S.V8F_PER_CU) == (S.V8R_PICS, S.V8R_PER_CU)    # the vp8_* functions of row_shapes take the recon launcher's by default
KINDS = [(0, 1), (0, 0), (1, 1), (1, 0)]    # filter_type (0 normal, 1 simple), keyframe


def _cus():
    return _torch().cuda.get_device_properties(0).multi_processor_count


def _reaches(why):
    assert why is None, "the shape no longer reaches its branch on this device (%d CUs): %s" % (_cus(), why)


@pytest.mark.parametrize("filter_type,keyframe", KINDS)
def test_a_wave_walks_several_rows(filter_type, keyframe):
    g = S.VP8_REUSE
    _reaches(S.vp8_ticket_reuse(g["mb_w"], g["mb_h"], g["npics"], _cus()))
    _frame_case(_torch(), np.random.default_rng(2000 + 2 * filter_type + keyframe), g["npics"], g["mb_w"], g["mb_h"], filter_type, keyframe)


@pytest.mark.parametrize("filter_type,keyframe", KINDS)
@pytest.mark.parametrize("g", [S.VP8_SPLIT_600, S.VP8_SPLIT_1024], ids=["600x16", "1024x8"])
def test_tall_frames_split_their_counters(g, filter_type, keyframe):
    _reaches(S.vp8_height_split(g["mb_h"], g["npics"], _cus(), g["launches"]))
    if g is S.VP8_SPLIT_1024:
        _reaches(S.vp8_many_tickets(g["mb_h"], g["npics"], _cus()))
    _frame_case(_torch(), np.random.default_rng(2100 + g["mb_h"] + 2 * filter_type + keyframe), g["npics"], g["mb_w"], g["mb_h"], filter_type,
                keyframe)


@pytest.mark.parametrize("filter_type", [0, 1])
def test_rows_that_filter_nothing_still_hand_off(filter_type, monkeypatch):
    """every record of the middle rows has filter_level 0, in every frame of a launch whose waves walk several rows: those rows write
    nothing and the rows below them still start"""
    g = S.VP8_REUSE
    mb_w, mb_h = g["mb_w"], g["mb_h"]
    _reaches(S.vp8_ticket_reuse(mb_w, mb_h, g["npics"], _cus()))
    strengths, made = D._strengths, []

    def quiet_middle(rng, h, w):
        st = strengths(rng, h, w)
        st["filter_level"][h // 4:h - h // 4] = 0
        made.append(st)
        return st

    monkeypatch.setattr(D, "_strengths", quiet_middle)
    _frame_case(_torch(), np.random.default_rng(2200 + filter_type), g["npics"], mb_w, mb_h, filter_type, 0)
    assert len(made) == g["npics"]
    for st in made:
        assert not st["filter_level"][mb_h // 4:mb_h - mb_h // 4].any() and st["filter_level"][:mb_h // 4].any() and st["filter_level"][-(mb_h // 4):].any()
