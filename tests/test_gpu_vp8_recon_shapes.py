"""ffhip_vp8_recon_frames_dev at the launch shapes its content tests (test_gpu_vp8_recon.py) do not reach, byte for byte against the
same model: a launch of more units than the grid holds, so that one wave of k_vp8_recon_intra walks several rows; calls that the height
splits into launches of fewer than 16 frames; frame widths at the edges of the 64-record ballot chunks of the intra search, with the
intra macroblocks placed; the widest frame.  Each case first asserts, with the compute-unit count of the device it runs on, that its
shape reaches the branch it is meant to reach (row_shapes.py), and fails if it does not.

_run asserts that ffhip_stream_synchronize returns 0 (a lost hand-off is FFHIP_EIO there), that the stride padding keeps its sentinel
and that references and coefficients are unchanged."""
import numpy as np
import pytest

import row_shapes as S
import vp8_recon_gen as G
import vp8_recon_model as RM
from test_gpu_vp8_recon import _check, _frame, _run, _torch, _want

pytestmark = pytest.mark.gpu


def _cus():
    return _torch().cuda.get_device_properties(0).multi_processor_count


def _reaches(why):
    assert why is None, "the shape no longer reaches its branch on this device (%d CUs): %s" % (_cus(), why)


def _all(frames, mb_w, mb_h):
    got = _run(frames, mb_w, mb_h)
    for i, fr in enumerate(frames):
        _check(got[i], _want(fr, mb_w, mb_h), "frame %d" % i)


@pytest.mark.parametrize("key", [True, False])
def test_a_wave_walks_several_rows(key):
    """16 frames in one launch whose units are at least twice the grid: every wave takes a second ticket, some a third"""
    g = S.VP8_REUSE
    mb_w, mb_h, npics = g["mb_w"], g["mb_h"], g["npics"]
    _reaches(S.vp8_ticket_reuse(mb_w, mb_h, npics, _cus()))
    lo, hi = S.tickets_per_wave(S.vp8_units(mb_h, npics)[0], S.vp8_grids(mb_h, npics, _cus())[0])
    assert lo >= 2 and hi >= 3
    _all([_frame(200 + 20 * key + i, mb_w, mb_h, key, intra=0.3) for i in range(npics)], mb_w, mb_h)


@pytest.mark.parametrize("g", [S.VP8_SPLIT_600, S.VP8_SPLIT_1024], ids=["600x16", "1024x8"])
def test_tall_frames_split_their_counters(g):
    """launches of fewer than 16 frames, the last the shorter one; every frame its own seed, key and inter frames mixed"""
    mb_w, mb_h, npics = g["mb_w"], g["mb_h"], g["npics"]
    _reaches(S.vp8_height_split(mb_h, npics, _cus(), g["launches"]))
    if g is S.VP8_SPLIT_1024:
        _reaches(S.vp8_many_tickets(mb_h, npics, _cus()))
    _all([_frame(300 + mb_h + i, mb_w, mb_h, i % 3 == 0, intra=0.3) for i in range(npics)], mb_w, mb_h)


def _placed(seed, mb_w, mb_h, intra, i4):
    place = np.zeros((mb_h, mb_w), bool)
    for r, c in intra:
        place[r, c] = True
    mbs, co = G.frame(seed, mb_w, mb_h, intra=0.0, place=place.reshape(-1), place_i4={r * mb_w + c for r, c in i4})
    for r, c in i4:     # the sub-blocks of the last column read above-right of the macroblock in every row
        mb = mbs[r * mb_w + c]
        assert mb["mode"] == RM.MODE_I4x4
        sub = mb["sub_mode"].copy()
        sub[[3, 7, 11, 15]] = [RM.B_DDL, RM.B_VL, RM.B_DDL, RM.B_VL]
        mb["sub_mode"] = sub
    assert np.array_equal(mbs["ref_frame"].reshape(mb_h, mb_w) == 0, place)
    refs = [G.planes(100 * seed + r, mb_w, mb_h) for r in range(3)]
    return mbs, co, refs, G.planes(7 + seed, mb_w, mb_h)


@pytest.mark.parametrize("mb_w", S.CHUNK_EDGE_WIDTHS)
def test_ballot_chunk_edges(mb_w):
    """inter frames of three rows, one per placement of the intra macroblocks (row_shapes.chunk_patterns), in one call"""
    mb_h = 3
    assert mb_w % S.CHUNK in (S.CHUNK - 1, 0, 1)
    pats = S.chunk_patterns(mb_w, mb_h)
    assert len(pats) >= (7 if mb_w > S.CHUNK else 5)
    frames = [_placed(400 + 10 * mb_w + k, mb_w, mb_h, intra, i4) for k, (name, intra, i4) in enumerate(pats)]
    got = _run(frames, mb_w, mb_h)
    for (name, intra, i4), fr, g in zip(pats, frames, got):
        _check(g, _want(fr, mb_w, mb_h), "%s, %d wide:" % (name, mb_w))


@pytest.mark.parametrize("mb_w,mb_h", S.VP8_WIDEST)
def test_widest_key_frames(mb_w, mb_h):
    assert mb_w == S.VP8_MAX_MB
    _all([_frame(500 + mb_h, mb_w, mb_h, True)], mb_w, mb_h)
