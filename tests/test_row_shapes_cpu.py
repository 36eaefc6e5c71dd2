"""The shapes of the geometry tests (the tables of row_shapes.py, run by test_gpu_vp8_recon_shapes.py, test_gpu_vp8_lf_shapes.py and
test_gpu_hevc_intra_picture_shapes.py) reach the launcher branches they are meant to reach: conditions on the inputs, computed from
the launch arithmetic restated in row_shapes.py, at 256 compute units and at 304 so that a slightly larger part does not void a case.
The GPU tests assert the same conditions with the compute-unit count of the device they run on."""
import os
import re

import pytest

import row_shapes as S

CUS = [256, 304]
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ffmpeg_amd", "csrc")


@pytest.mark.parametrize("path,name,value", [
    ("kernels/progress_pool.h", "FFHIP_PROGRESS_SLOT_INTS", S.SLOT_INTS),
    ("kernels/vp8_recon_frame.hip", "V8R_PICS", S.V8R_PICS), ("kernels/vp8_recon_frame.hip", "V8R_PER_CU", S.V8R_PER_CU),
    ("kernels/vp8_lf_frame.hip", "V8F_PICS", S.V8F_PICS), ("kernels/vp8_lf_frame.hip", "V8F_PER_CU", S.V8F_PER_CU),
    ("kernels/hevc_intra_pic.hip", "HIP_PICS", S.HIP_PICS)])
def test_constants_are_the_sources(path, name, value):
    text = open(os.path.join(CSRC, path)).read()
    m = re.search(r"^#define %s (\d+)" % name, text, re.M)
    assert m, "%s no longer defines %s" % (path, name)
    assert int(m.group(1)) == value


def test_the_arithmetic_on_the_shapes_the_suite_already_runs():
    """17 frames of 4 rows: the 16 + 1 split of test_frames_per_call; one 1080p frame: 68 units, a grid of 68"""
    assert S.vp8_launches(4, 17) == [16, 1] and S.vp8_units(4, 17) == [64, 4] and S.vp8_grids(4, 17, 256) == [64, 4]
    assert S.vp8_launches(68, 1) == [1] and S.vp8_grids(68, 1, 256) == [68]
    assert S.vp8_per(511) == 16 and S.vp8_per(512) == 15 and S.vp8_per(1024) == 7
    assert S.hevc_per(1088, 6, 1) == 16 and S.hevc_per(16 * 170, 4, 1) == 16 and S.hevc_per(16 * 171, 4, 1) == 15
    assert S.tickets_per_wave(4096, 2048) == (2, 2) and S.tickets_per_wave(5120, 2048) == (2, 3)


@pytest.mark.parametrize("cus", CUS)
def test_vp8_ticket_reuse(cus):
    g = S.VP8_REUSE
    assert g["mb_h"] <= 511 and g["npics"] == 16
    assert S.vp8_ticket_reuse(g["mb_w"], g["mb_h"], g["npics"], cus) is None
    lo, hi = S.tickets_per_wave(S.vp8_units(g["mb_h"], g["npics"])[0], S.vp8_grids(g["mb_h"], g["npics"], cus)[0])
    assert lo >= 2 and hi >= 3, "every wave a second ticket, some a third"
    # what the suite ran before does not reach it
    assert S.vp8_ticket_reuse(120, 68, 1, cus) is not None and S.vp8_ticket_reuse(5, 4, 16, cus) is not None


@pytest.mark.parametrize("cus", CUS)
def test_vp8_height_splits(cus):
    for g in (S.VP8_SPLIT_600, S.VP8_SPLIT_1024):
        assert g["mb_h"] <= S.VP8_MAX_MB
        assert S.vp8_height_split(g["mb_h"], g["npics"], cus, g["launches"]) is None
        assert all(u + 1 <= S.SLOT_INTS for u in S.vp8_units(g["mb_h"], g["npics"]))
    g = S.VP8_SPLIT_1024
    assert S.vp8_units(g["mb_h"], g["npics"]) == [7168, 1024]
    assert S.vp8_many_tickets(g["mb_h"], g["npics"], cus) is None
    assert S.vp8_height_split(68, 17, cus, (16, 1)) is not None, "the 16 + 1 split is not a height split"


def test_vp8_chunk_edges():
    assert S.CHUNK == 64
    assert {w % S.CHUNK for w in S.CHUNK_EDGE_WIDTHS} == {63, 0, 1} and max(S.CHUNK_EDGE_WIDTHS) > 2 * S.CHUNK
    assert set(S.CHUNK_EDGE_WIDTHS) == {63, 64, 65, 128, 129}
    for w in S.CHUNK_EDGE_WIDTHS:
        pats = dict((name, (intra, i4)) for name, intra, i4 in S.chunk_patterns(w))
        assert {"column 0", "last column", "every column", "inter middle row", "inter first row"} <= set(pats)
        assert not any(r == 1 for r, c in pats["inter middle row"][0]) and not any(r == 0 for r, c in pats["inter first row"][0])
        assert all(0 <= r < 3 and 0 <= c < w for intra, i4 in pats.values() for r, c in intra)
        if w > S.CHUNK:
            assert {c for r, c in pats["columns 63 and 64"][0]} == {63, 64}
            intra, i4 = pats["I4x4 at a chunk's end"]
            for r, c in i4:
                assert (r, c) in intra and c % S.CHUNK == S.CHUNK - 1 and r > 0
                if c + 1 < w:   # its above-right macroblock is intra and the first record of the next ballot
                    assert (r - 1, c + 1) in intra and (c + 1) // S.CHUNK == c // S.CHUNK + 1
            assert any(c + 1 < w for r, c in i4)
    for w, h in S.VP8_WIDEST:
        assert w == S.VP8_MAX_MB and h in (1, 2)


def test_hevc_splits():
    g = S.HEVC_SPLIT_420
    assert S.hevc_rows(g["height"], g["log2_ctb"], g["cfi"]) == 1536 and S.hevc_per(g["height"], g["log2_ctb"], g["cfi"]) == 5
    assert S.hevc_split(g["height"], g["log2_ctb"], g["cfi"], g["npics"], g["launches"]) is None
    g = S.HEVC_SPLIT_400
    assert S.hevc_per(g["height"], g["log2_ctb"], g["cfi"]) == 15, "just below 16"
    assert S.hevc_per(g["height"] - 16, g["log2_ctb"], g["cfi"]) == 16, "one CTB row less does not split"
    assert S.hevc_split(g["height"], g["log2_ctb"], g["cfi"], g["npics"], g["launches"]) is None
    assert S.hevc_split(1080, 6, 1, 17, (16, 1)) is not None


def test_hevc_limit():
    """no picture has exactly FFHIP_PROGRESS_SLOT_INTS counters: three planes give multiples of 3, one plane at most 4096 rows"""
    g, b = S.HEVC_LIMIT, S.HEVC_PAST_LIMIT
    assert S.SLOT_INTS % 3 and (65535 // 8 * 8 + 15) // 16 < S.SLOT_INTS
    assert S.hevc_rows(**g) == S.SLOT_INTS // 3 * 3 == 8190 and S.hevc_accepted(**g) and S.hevc_per(**g) == 1
    assert S.hevc_rows(**b) == 8193 and not S.hevc_accepted(**b)
    assert b["height"] <= 65535 and b["height"] % 8 == 0, "refused for its counters, not for its size"
    # the face's comparison against the launcher's division: whatever is accepted gets at least one picture a launch
    for rows in (S.SLOT_INTS - 1, S.SLOT_INTS):
        assert S.SLOT_INTS // rows >= 1
    assert S.SLOT_INTS // (S.SLOT_INTS + 1) == 0


@pytest.mark.parametrize("cus", CUS)
def test_hevc_past_residency(cus):
    """A launch has at most FFHIP_PROGRESS_SLOT_INTS waves (a counter each), which is four times what 256 CUs hold and 3.4 times what
    304 hold: the shape is the largest launch there is, and the factor 4 of the GPU test is reachable up to 256 CUs."""
    g = S.HEVC_RESIDENCY
    assert S.hevc_units(**g) == [S.SLOT_INTS]
    if 4 * S.hevc_resident(cus) <= S.SLOT_INTS:
        assert S.hevc_past_residency(cus=cus, **g) is None
    else:
        assert S.hevc_past_residency(cus=cus, factor=3, **g) is None
        assert S.hevc_past_residency(cus=cus, **g) is not None
    assert S.hevc_past_residency(1080, 6, 1, 1, cus) is not None
