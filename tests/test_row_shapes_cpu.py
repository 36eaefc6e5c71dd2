"""The shapes of the geometry tests (the tables of row_shapes.py, run by test_gpu_vp8_recon_shapes.py, test_gpu_vp8_lf_shapes.py,
test_gpu_hevc_intra_picture_shapes.py, test_gpu_h264_deblock_shapes.py, test_gpu_h264_intra_shapes.py and
test_gpu_vp9_lf_shapes.py) reach the launcher branches they are meant to reach: conditions on the inputs, computed from the launch
arithmetic restated in row_shapes.py, at 256 compute units and at 304 so that a slightly larger part does not void a case.  The GPU
tests assert the same conditions with the compute-unit count of the device they run on."""
import ctypes as C
import os
import re
import subprocess

import pytest

import row_shapes as S

CUS = [256, 304]
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ffmpeg_amd", "csrc")


@pytest.mark.parametrize("path,name,value", [
    ("kernels/progress_pool.h", "FFHIP_PROGRESS_SLOT_INTS", S.SLOT_INTS),
    ("kernels/vp8_recon_frame.hip", "V8R_PICS", S.V8R_PICS), ("kernels/vp8_recon_frame.hip", "V8R_PER_CU", S.V8R_PER_CU),
    ("kernels/vp8_lf_frame.hip", "V8F_PICS", S.V8F_PICS), ("kernels/vp8_lf_frame.hip", "V8F_PER_CU", S.V8F_PER_CU),
    ("kernels/hevc_intra_pic.hip", "HIP_PICS", S.HIP_PICS), ("kernels/h264_kernels.h", "FFHIP_DB_PTRS", S.DB_PTRS),
    ("kernels/h264_kernels.h", "FFHIP_INTRA_PICS", S.INTRA_PICS), ("kernels/h264_kernels.h", "FFHIP_VP9_LF_PICS", S.VP9_LF_PICS)])
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


# ---- the H.264 deblocking, H.264 intra and VP9 loop filter launchers -------------------------------------------------------------------
@pytest.mark.parametrize("path,pattern,value", [
    ("kernels/h264_deblock.hip", r"\(long long\)nframes \* mb_h > (\d+) \? 16 : 4;", S.DB_BAND_ROWS),
    ("kernels/h264_deblock.hip", r"int bwaves = .* : (\d+) / per_xcd;", S.DB_XCD_SIMDS),
    ("kernels/h264_deblock.hip", r"const int per_xcd = cdiv\(nf, (\d+)\);", S.DB_XCDS),
    ("kernels/h264_deblock.hip", r"if \(bwaves < cdiv\(nbands, (\d+)\)\) bwaves = cdiv\(nbands, 4\);", 4),
    ("kernels/h264_intra.hip", r"bool split = !luma_only && \(size_t\)npics \* nwg \* 2 <= (\d+);", S.INTRA_SPLIT_WGS),
    ("kernels/h264_intra.hip", r"while \(W > 1 && fixed \+ \(size_t\)\(W - 1\) \* line > (\d+) \* 1024\)", S.INTRA_LDS // 1024),
    ("kernels/h264_intra.hip", r"__launch_bounds__\(256, (\d+)\) void k_h264_intra_frame", S.INTRA_WG_PER_CU),
    ("kernels/h264_intra.hip", r"\? sizeof\(ImbTileT<uint16_t>\) \* 4 \+ sizeof\(FFHipH264IntraMB\) \* 8 \+ 4 \* 2 \* (\d+) \* 256 \+ 64 \+ IMB_TABS \* 4", 7),
    ("kernels/h264_intra.hip", r": sizeof\(ImbTileT<uint8_t>\) \* 4 \+ sizeof\(FFHipH264IntraMB\) \* 8 \+ 4 \* 2 \* (\d+) \* 256 \+ 64 \+ IMB_TABS \* 4", 3),
    ("kernels/vp9_lf.hip", r"const int wmax = bd == 8 \? (\d+) : 2;", 4),
    ("h264_api.hip", r"if \(rows > 8 \* (\d+)\) \{\n        ffhip_set_error\(\"ffhip_vp9_loopfilter_frame_dev:", S.VLF_ROWS_420 // 8)])
def test_literals_of_the_launchers_are_the_sources(path, pattern, value):
    m = re.search(pattern, open(os.path.join(CSRC, path)).read())
    assert m, "%s no longer has a line like %s: restate the launcher in row_shapes.py" % (path, pattern)
    assert int(m.group(1)) == value


def test_the_other_faces_share_one_limit():
    text = open(os.path.join(CSRC, "h264_api.hip")).read()
    assert re.findall(r"if \(rows > 8 \* (\d+)\) \{", text) == [str(S.VLF_ROWS_420 // 8)] + 4 * [str(S.VLF_ROWS // 8)]
    assert text.count("rows > 8 *") == 5


def test_the_intra_kernels_static_lds_is_the_compilers(tmp_path):
    """the sizes behind `fixed` (h264_intra.hip:385-386), from a host-only translation unit of the header the kernel shares with the CPU
    emulation: a tile that grows, a longer record or another table moves the widths at which W shrinks"""
    src = tmp_path / "sizes.cpp"
    src.write_text('#include <cstdio>\n#include "kernels/h264_intra_mb.h"\n'
                   'int main() { std::printf("%zu %zu %zu %d\\n", sizeof(ImbTileT<uint8_t>), sizeof(ImbTileT<uint16_t>), sizeof(FFHipH264IntraMB), '
                   '(int)IMB_TABS); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(CSRC, "..", "..", "include"), "-I", CSRC, "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert got == [S.IMB_TILE[1], S.IMB_TILE[2], S.IMB_REC, S.IMB_TABS], "ImbTileT<uint8_t>, ImbTileT<uint16_t>, FFHipH264IntraMB, IMB_TABS: %s" % got
    assert (S.h264_intra_fixed(8), S.h264_intra_fixed(10)) == (19744, 31392)


def test_the_new_arithmetic_on_the_shapes_the_suite_already_runs():
    """what the content tests reach: a wave a band, one launch, chroma on a wavefront of its own, W = 4"""
    d = S.h264_deblock(60, 34, 24)                  # test_deblock_frames_batch: the largest call before these tests
    assert (d["kernel"], d["nbands"], d["launches"], d["per_xcd"], d["bwaves"], d["walked"]) == ("skew", 9, [24], [3], [12], [(1, 1)])
    d = S.h264_deblock(240, 135, 1)
    assert d["bwaves"] == [36] and d["walked"] == [(1, 1)] and d["grids"] == [72]
    assert S.h264_deblock(9, 8, 1, align=4)["bw"] == 4 and S.h264_deblock(7, 4, 1, align=1)["kernel"] == "row"
    assert S.h264_deblock(2, 2, 1, chroma=True, align=1) is None and S.h264_deblock(2, 2, 1, bd=10, align=8) is None
    assert S.h264_deblock(6, 16, 1, chroma=True, align=4)["kernel"] == "band" and S.h264_deblock(6, 16, 1, chroma=True, align=8)["kernel"] == "skew"
    assert S.h264_deblock(1, 2048, 33, ptrs=True)["launches"] == [16, 16, 1] and S.h264_deblock(4, 4, 33, ptrs=True)["launches"] == [32, 1]
    # test_gpu_h264_picture.py::test_pictures_flush_batch[11-7-35-1.0]: 35 picture objects, their luma and their 70 chroma planes by table
    assert S.h264_deblock(11, 7, 35, ptrs=True)["launches"] == [32, 3]
    assert S.h264_deblock(11, 7, 70, chroma=True, align=8, ptrs=True)["launches"] == [32, 32, 6]
    d = S.h264_intra(13, 7, 37)                     # test_intra_frames_batch_equals_single_launches: 37 x 2 x 2 = 148 workgroups
    assert d["split"] and d["launches"] == [32, 5] and d["grids"] == [(4, 32), (4, 5)] and d["W"] == 4
    assert S.h264_intra(120, 68, 3)["split"] and S.h264_intra(120, 68, 3)["lds"] == 3 * 120 * 32
    assert S.h264_intra(20, 9, 5, luma_only=True)["parts"] == (1,)
    d = S.vp9_lf(8 * 17, 2)
    assert (d["per"], d["launches"], d["grids"], d["lds"], d["wg_per_cu"]) == (32, [2], [(10, 2)], 44256, 3)
    assert S.vp9_lf(8 * 2, 70)["launches"] == [32, 32, 6] and S.vp9_lf_ssc(8 * 2, 40)["launches"] == [32, 8]
    assert S.vp9_lf(8 * 6, 3, bd=10)["lds"] == 43408


@pytest.mark.parametrize("cus", CUS)
def test_h264_deblock_shapes(cus):
    assert S.db_superbands(S.DB_SUPERBANDS, cus) is None
    d = S.h264_deblock(cus=cus, **S.DB_SUPERBANDS)
    assert (d["nbands"], d["bwaves"], d["wgs"], d["walked"], d["grids"]) == (512, [128], [32], [(4, 4)], [256])
    assert S.db_superbands(S.DB_SUPERBANDS_RAGGED, cus, ragged=2) is None
    assert S.db_superbands(S.DB_SUPERBANDS_ODD, cus, idle=True) is None
    assert S.h264_deblock(cus=cus, **S.DB_SUPERBANDS_ODD)["nbands"] % 4 == 3
    assert S.db_superbands(S.DB_SUPERBANDS, cus, idle=True) is not None and S.db_superbands(S.DB_SUPERBANDS, cus, ragged=2) is not None
    assert S.db_floor(S.DB_FLOOR, cus) is None
    d = S.h264_deblock(cus=cus, **S.DB_FLOOR)
    assert (d["per_xcd"], d["bwaves"], d["grids"], d["launches"]) == ([2], [128], [512], [9])
    assert S.db_floor(S.DB_SUPERBANDS, cus) is not None, "a lone picture: 128 waves are the floor, it does not win"
    assert S.db_split(S.DB_SPLIT, cus, (16, 1)) is None and S.db_split(S.DB_SPLIT_CHROMA, cus, (16, 1)) is None
    assert S.h264_deblock(cus=cus, **S.DB_SPLIT_CHROMA)["nbands"] == 512
    assert S.db_split(S.DB_ROW_SPLIT, cus, (13, 1), "row") is None
    assert S.h264_deblock(cus=cus, **S.DB_ROW_SPLIT)["per_frame"] == 601
    assert S.db_hbd_wpb3(S.DB_HBD_WPB3, cus) is None
    d = S.h264_deblock(cus=cus, **S.DB_HBD_WPB3)
    assert (d["wpb"], d["nbands"], d["superbands"], d["wgs"], d["idle_waves"]) == (3, 250, 84, [43], 2)
    assert S.db_hbd_wpb3(dict(S.DB_HBD_WPB3, bd=8), cus) is not None
    assert S.db_band16(S.DB_BAND16, cus, True) is None and S.db_band16(S.DB_BAND16_CHROMA, cus, False) is None
    assert S.db_band16(dict(S.DB_BAND16, mb_h=2048), cus, True) is not None, "2048 rows keep bands of 4"
    assert S.db_band16(dict(S.DB_BAND16_CHROMA, nf=29), cus, False) is not None
    assert S.db_ptrs(S.DB_PTRS_SPLIT, cus, (32, 1)) is None and S.db_ptrs(S.DB_PTRS_SPLIT_CHROMA, cus, (32, 32, 2)) is None
    assert S.DB_PTRS_SPLIT_CHROMA["nf"] == 2 * S.DB_PTRS_SPLIT["nf"], "Cb and Cr of every picture"
    d = S.h264_deblock(cus=cus, **S.DB_PTRS_SPLIT)
    assert (d["nbands"], d["last_band_rows"], d["per_xcd"], d["bwaves"], d["grids"]) == (3, 1, [4, 1], [4, 4], [32, 8])
    assert S.db_ptrs(dict(S.DB_PTRS_SPLIT, ptrs=False), cus, (32, 1)) is not None, "at a constant pitch a slot holds all 33"
    assert S.db_ptrs(dict(S.DB_PTRS_SPLIT, mb_h=2048), cus, (16, 16, 1)) is not None, "512 counters a picture: the slot cuts, not the table"
    assert S.db_ptrs(dict(S.DB_PTRS_SPLIT, align=4), cus, (32, 1)) is not None, "the table is for the skewed-rows kernel only"
    # what the suite ran before reaches none of them
    old = dict(mb_w=60, mb_h=34, nf=24)
    assert S.db_superbands(old, cus) and S.db_floor(old, cus) and S.db_split(old, cus, (16, 1))


@pytest.mark.parametrize("cus", CUS)
def test_h264_intra_shapes(cus):
    for g in (S.IF_UNSPLIT, S.IF_UNSPLIT_HBD):
        assert S.if_unsplit(g, cus) is None
        d = S.h264_intra(cus=cus, **g)
        assert (d["nwg"], d["parts"], d["launches"], d["grids"]) == (10, (3,), [32], [(10, 32)])
    assert S.if_unsplit(dict(S.IF_UNSPLIT, npics=28), cus) is not None, "28 x 10 x 2 = 560 workgroups keep the split"
    assert S.if_unsplit(dict(mb_w=13, mb_h=7, npics=37), cus) is not None
    assert S.if_height_split(S.IF_HEIGHT_SPLIT, cus, (31, 1)) is None
    assert S.if_height_split(dict(S.IF_HEIGHT_SPLIT, mb_h=255), cus, (31, 1)) is not None, "255 rows: 32 pictures fit a slot"
    # "three times past residency" holds for the kernel as compiled (two workgroups a CU by its registers), not from an upper bound:
    # by waves and LDS a CU could hold 8, and a launch has a counter a row in one slot, so at most about 8192 / 4 workgroups
    d = S.h264_intra(cus=cus, **S.IF_HEIGHT_SPLIT)
    assert d["grids"][0] == (64, 31) and d["resident"] == 2 * cus and d["resident_bound"] == 8 * cus
    assert 3 * d["resident"] <= 64 * 31 < d["resident_bound"]
    assert S.IF_W_ROWS >= 4, "the picture does not cap W itself"
    for bd in (8, 10):
        assert S.h264_intra_widths(bd) == tuple(S.IF_WIDTHS[bd, W] for W in (4, 3, 2))
        for W in (4, 3, 2):
            g = dict(mb_w=S.IF_WIDTHS[bd, W], mb_h=S.IF_W_ROWS, npics=S.IF_W_PICS, bd=bd)
            assert S.if_w(g, cus, W) is None
            assert S.h264_intra(cus=cus, **g)["split"], "two pictures of three workgroups: luma and chroma apart"
    assert S.h264_intra(240, 135, 1, bd=10)["W"] == 3, "a 4K-wide picture at 10 bits is past W = 4"
    assert S.h264_intra(240, 135, 1)["W"] == 4 and S.h264_intra(120, 68, 1, bd=10)["W"] == 4


def test_h264_intra_split_and_height_split_exclude_each_other():
    """a call of more than one picture whose chroma has its own wavefront is never split by the height: split needs
    npics * nwg * 2 <= 576 with nwg >= mb_h / 4, a slot holds 8192 / (2 * (mb_h + 1)) such pictures, and that is always more"""
    for mb_w in (1, 177, 178, 267, 477, 478, 716, 2000):
        for bd in (8, 10):
            for mb_h in range(1, S.SLOT_INTS):
                nwg = S.h264_intra(mb_w, mb_h, 1, bd=bd)["nwg"]
                most = S.INTRA_SPLIT_WGS // (2 * nwg)      # the most pictures that keep the split
                if most < 2:
                    continue
                d = S.h264_intra(mb_w, mb_h, most, bd=bd)
                # the slot holds them all, or the 32 of a launch: no launch is cut short by the height
                assert d["split"] and d["per"] >= min(most, S.INTRA_PICS), (mb_w, mb_h, bd, d)
                assert d["launches"] == S._split(most, S.INTRA_PICS)


@pytest.mark.parametrize("cus", CUS)
def test_vp9_lf_shapes(cus):
    assert S.VLF_SPLIT_420["rows"] % 8 and S.VLF_SPLIT_444["rows"] % 8
    assert S.vlf_split(S.VLF_SPLIT_420, cus, (31, 1), workgroups=1984) is None
    assert S.vlf_split(S.VLF_SPLIT_420_HBD, cus, (31, 1), workgroups=3968) is None
    assert S.vlf_split(S.VLF_SPLIT_444, cus, (31, 1), workgroups=2046) is None
    d = S.vp9_lf(cus=cus, **S.VLF_SPLIT_444)
    assert (d["per_pic"], d["per"], d["nwg"], d["sb_rows"] % d["W"]) == (258, 31, 22, 2)
    assert S.vp9_lf(cus=cus, **S.VLF_SPLIT_420_HBD)["W"] == 2 and S.vp9_lf(cus=cus, **S.VLF_SPLIT_420)["wg_per_cu"] == 3
    assert S.vlf_split(dict(rows=8 * 17, npics=32), cus, (32,)) is not None and S.vlf_split(dict(rows=8 * 2, npics=70), cus, (32, 32, 6)) is not None
    assert S.vlf_ssc_split(S.VLF_SSC_SPLIT, cus, (21, 11), (384, 21)) is None
    d = S.vp9_lf_ssc(cus=cus, **S.VLF_SSC_SPLIT)
    assert d["grids"][0][0] * d["grids"][0][1] == 8064
    # a launch of one-wave workgroups has a counter each: never more than a slot, which 256 CUs of 32 waves hold at once
    assert S.SLOT_INTS <= d["resident"]
    assert S.vlf_ssc_split(dict(rows=8 * 2, npics=40), cus, (32, 8), (6, 32)) is not None
    for face, (rows, per) in S.VLF_TALLEST.items():
        ssc, p444 = face.endswith("ssc"), face.endswith("444")
        assert S.vlf_tallest(rows, face == "lone_420", p444, ssc, per) is None, face
        assert S.vlf_tallest(rows - 8, face == "lone_420", p444, ssc, per) is not None
    assert [S.VLF_TALLEST[f][1] for f in ("frames_420", "frames_444", "frames_ssc")] == [3, 2, 2]
    # the limits are the faces' contract, not the launchers': a slot would hold a taller lone 4:4:4 or 4:2:2 picture
    assert S.vp9_lf(S.VLF_ROWS + 8, 1, planes444=True) is not None and S.vp9_lf_ssc(S.VLF_ROWS + 8, 1) is not None
    assert S.vp9_lf(S.VLF_ROWS_420 + 8, 1) is not None and S.vp9_lf(8 * 4096, 1) is None


@pytest.mark.parametrize("name,value,conditions", [
    ("SLOT_INTS", 4096, ["db_split(DB_SPLIT)", "db_split(DB_ROW_SPLIT)", "if_height_split", "vlf_split(VLF_SPLIT_420)", "vlf_ssc_split"]),
    ("SLOT_INTS", 16384, ["db_split(DB_SPLIT)", "db_split(DB_SPLIT_CHROMA)", "db_split(DB_ROW_SPLIT)", "if_height_split", "vlf_split(VLF_SPLIT_420)",
                          "vlf_split(VLF_SPLIT_444)", "vlf_ssc_split"]),
    ("INTRA_SPLIT_WGS", 640, ["if_unsplit(IF_UNSPLIT)", "if_unsplit(IF_UNSPLIT_HBD)"]),
    ("DB_XCD_SIMDS", 256, ["db_superbands", "db_floor"]),
    ("DB_BAND_ROWS", 4096, ["db_band16(DB_BAND16)", "db_band16(DB_BAND16_CHROMA)"]),
    ("INTRA_LDS", 48 * 1024, ["if_w(8, 4)", "if_w(10, 3)", "if_w(10, 2)"]),
    ("IMB_REC", 140, ["if_w(8, 4)", "if_w(10, 4)"]),
    ("INTRA_WG_PER_CU", 4, ["if_height_split"]),
    ("DB_PTRS", 16, ["db_ptrs(DB_PTRS_SPLIT)", "db_ptrs(DB_PTRS_SPLIT_CHROMA)"]),
    ("DB_PTRS", 64, ["db_ptrs(DB_PTRS_SPLIT)", "db_ptrs(DB_PTRS_SPLIT_CHROMA)"]),
    ("CU_LDS", 256 * 1024, ["vlf_split(VLF_SPLIT_420)"]),
    ("VP9_LF_PICS", 16, ["vlf_split(VLF_SPLIT_420)", "vlf_ssc_split"])])
def test_a_perturbed_constant_is_noticed(name, value, conditions, monkeypatch):
    """a launcher that changes one of its constants is restated here, and the shapes that no longer reach their branch say so"""
    conds = {
        "db_superbands": lambda: S.db_superbands(S.DB_SUPERBANDS, 256),
        "db_floor": lambda: S.db_floor(S.DB_FLOOR, 256),
        "db_split(DB_SPLIT)": lambda: S.db_split(S.DB_SPLIT, 256, (16, 1)),
        "db_split(DB_SPLIT_CHROMA)": lambda: S.db_split(S.DB_SPLIT_CHROMA, 256, (16, 1)),
        "db_split(DB_ROW_SPLIT)": lambda: S.db_split(S.DB_ROW_SPLIT, 256, (13, 1), "row"),
        "db_ptrs(DB_PTRS_SPLIT)": lambda: S.db_ptrs(S.DB_PTRS_SPLIT, 256, (32, 1)),
        "db_ptrs(DB_PTRS_SPLIT_CHROMA)": lambda: S.db_ptrs(S.DB_PTRS_SPLIT_CHROMA, 256, (32, 32, 2)),
        "db_band16(DB_BAND16)": lambda: S.db_band16(S.DB_BAND16, 256, True),
        "db_band16(DB_BAND16_CHROMA)": lambda: S.db_band16(S.DB_BAND16_CHROMA, 256, False),
        "if_unsplit(IF_UNSPLIT)": lambda: S.if_unsplit(S.IF_UNSPLIT, 256),
        "if_unsplit(IF_UNSPLIT_HBD)": lambda: S.if_unsplit(S.IF_UNSPLIT_HBD, 256),
        "if_height_split": lambda: S.if_height_split(S.IF_HEIGHT_SPLIT, 256, (31, 1)),
        "vlf_split(VLF_SPLIT_420)": lambda: S.vlf_split(S.VLF_SPLIT_420, 256, (31, 1)),
        "vlf_split(VLF_SPLIT_444)": lambda: S.vlf_split(S.VLF_SPLIT_444, 256, (31, 1)),
        "vlf_ssc_split": lambda: S.vlf_ssc_split(S.VLF_SSC_SPLIT, 256, (21, 11), (384, 21)),
    }
    for (bd, W), mb_w in S.IF_WIDTHS.items():
        conds["if_w(%d, %d)" % (bd, W)] = lambda bd=bd, W=W, mb_w=mb_w: S.if_w(dict(mb_w=mb_w, mb_h=S.IF_W_ROWS, npics=S.IF_W_PICS, bd=bd), 256, W)
    for c in conds.values():
        assert c() is None
    monkeypatch.setattr(S, name, value)
    for c in conditions:
        why = conds[c]()
        assert isinstance(why, str) and why, "%s = %s: %s still holds" % (name, value, c)


_KEEP = []


def _addr(n=64):
    b = (C.c_uint64 * n)()
    _KEEP.append(b)
    return C.addressof(b)


def test_vp9_lf_too_tall_is_refused_with_a_text():
    """VLF_TOO_TALL: one block row more than each face's limit is FFHIP_EINVAL with the face and the limit in the error text.  The check
    comes before the device is looked for, so nothing is launched and this holds on any machine"""
    from ffmpeg_amd import _lib
    L = _lib.lib()
    y, u, v, t, ct = (_addr() for _ in range(5))
    pics = (C.c_void_p * 5)(y, u, v, t, ct)
    _KEEP.append(pics)
    pv = C.cast(pics, C.c_void_p)
    lo, hi = S.VLF_ROWS + 1, S.VLF_ROWS_420 + 1
    calls = [
        ("ffhip_vp9_loopfilter_frame_dev", hi, S.VLF_ROWS_420, lambda r: L.ffhip_vp9_loopfilter_frame_dev(8, y, u, v, 64, 32, 8, r, t, None)),
        ("ffhip_vp9_loopfilter_frame_dev", hi, S.VLF_ROWS_420, lambda r: L.ffhip_vp9_loopfilter_frame_ss_dev(8, 1, 1, y, u, v, 64, 32, 8, r, t, None)),
        ("ffhip_vp9_loopfilter_frame_ss_dev", lo, S.VLF_ROWS, lambda r: L.ffhip_vp9_loopfilter_frame_ss_dev(10, 0, 0, y, u, v, 64, 64, 8, r, t, None)),
        ("ffhip_vp9_loopfilter_frame_ssc_dev", lo, S.VLF_ROWS, lambda r: L.ffhip_vp9_loopfilter_frame_ssc_dev(8, 1, 0, y, u, v, 64, 32, 8, r, t, ct, None)),
        ("ffhip_vp9_loopfilter_frame_ssc_dev", lo, S.VLF_ROWS, lambda r: L.ffhip_vp9_loopfilter_frame_ssc_dev(12, 0, 1, y, u, v, 64, 64, 8, r, t, ct, None)),
        ("ffhip_vp9_loopfilter_frames_dev", lo, S.VLF_ROWS, lambda r: L.ffhip_vp9_loopfilter_frames_dev(8, 1, 1, 1, pv, 64, 32, 8, r, None)),
        ("ffhip_vp9_loopfilter_frames_dev", lo, S.VLF_ROWS, lambda r: L.ffhip_vp9_loopfilter_frames_dev(8, 0, 0, 1, pv, 64, 64, 8, r, None)),
        ("ffhip_vp9_loopfilter_frames_ssc_dev", lo, S.VLF_ROWS, lambda r: L.ffhip_vp9_loopfilter_frames_ssc_dev(8, 1, 0, 1, pv, 64, 32, 8, r, None)),
    ]
    for face, rows, limit, call in calls:
        for r in (rows, rows + 7, 8 * 8192, 2 ** 31 - 1):
            assert call(r) == _lib.EINVAL, (face, r)
            text = L.ffhip_last_error().decode()
            assert text.startswith(face + ":") and "%d rows" % r in text and "the supported %d" % limit in text and \
                "(%d superblock rows)" % (limit // 8) in text, (face, r, text)
    assert not S.vp9_lf_face_accepts(hi, True) and not S.vp9_lf_face_accepts(lo, False)
    assert S.vp9_lf_face_accepts(hi - 1, True) and S.vp9_lf_face_accepts(lo - 1, False) and S.vp9_lf_face_accepts(lo, True)
