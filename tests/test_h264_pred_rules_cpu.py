"""kernels/h264_pred_rules.h, the one statement of the H.264 intra-prediction arithmetic, compiled for the host and walked against the
oracle (oracle/ffo_h264pred.c, 8 bits) by tests/h264_pred_rules_check.cpp: hp_dir_sample / hp_dir_dc against pred4x4 (12 modes), the same
over hp_filter8's line against pred8x8l (12 modes x has_topleft x has_topright), the filtered VERT / HOR lines against
pred8x8l_filter_add without a residual, the block rules (needs, plane, 16x16 DC, cell DC) against pred8x8 and pred8x16 (modes 0..10) and
pred16x16 (0..6) on every sample; every one of these a second time with the neighbours the mode's mask does not name given other values;
the table forms of h264_intra_mb.h decoded against the rules; mid and maxv at 9 / 10 / 12 / 14 bits; the whole-block DC against
pred16x16 and the RV40 rule text of h264_pred_codec.inc.  Windows: random, all 0, all 255, a 0 / 255 checkerboard, two ramps on which
the plane predictor overshoots both ends of the range.  Undefined behaviour ends the program."""
import os
import subprocess

import ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ffmpeg_amd", "csrc")

NRAND = 4                               # random windows (the program's argument)
FIXED_WINDOWS = 5                       # 0, 255, checkerboard, ramp up, ramp down
TWICE = 2                               # against the oracle, and again with the unnamed neighbours disturbed
DIR_MODES, CORNERS = 12, 2 * 2          # pred4x4 / pred8x8l modes; has_topleft x has_topright
ADD_MODES = 2                           # VERT, HOR
BLK8_MODES, BLK16_MODES = 11, 7
S4, S8, S8x16, S16 = 4 * 4, 8 * 8, 8 * 16, 16 * 16                 # samples of a block
SIDES_DC = 4 + 3                        # pred16x16 modes 0, 4, 5, 6; RV40's three pred8x8 DCs
TABLE_MODES = 8                         # the directional modes that are table rules
EDGE_ENTRIES = CORNERS * 25             # imb_p8_edge_tab
DEPTHS = 4                              # 9, 10, 12, 14 bits
MID = 2 + 1 + 2 + 8 + 2 + 2             # DC_128 of 4x4, 8x8l; 16x16; whole-block 8, 16; the 8 cells; L00's and 0L0's two mid cells
DEPTH_WINDOWS = 4                       # 0, the maximum, the two ramps


def test_the_header_equals_the_oracle(tmp_path):
    assert os.path.exists(ffi.ORACLE_SO), "oracle/liboracle.so missing - run build()"
    exe = tmp_path / "h264_pred_rules_check"
    oracle = os.path.join(ROOT, "oracle")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
                    "-I", CSRC, "-I", oracle, "-o", str(exe), os.path.join(ROOT, "tests", "h264_pred_rules_check.cpp"), ffi.ORACLE_SO,
                    "-Wl,-rpath," + oracle], check=True)
    r = subprocess.run([str(exe), str(NRAND)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    windows = NRAND + FIXED_WINDOWS
    per_window = DIR_MODES * S4 * TWICE + DIR_MODES * CORNERS * S8 * TWICE                      # pred4x4, pred8x8l
    per_window += ADD_MODES * CORNERS * S8                                                      # pred8x8l_filter_add
    per_window += (BLK8_MODES * S8 + BLK8_MODES * S8x16 + BLK16_MODES * S16) * TWICE            # pred8x8, pred8x16, pred16x16
    per_window += SIDES_DC
    want = windows * per_window
    want += NRAND * (TABLE_MODES * (S4 + S8) + EDGE_ENTRIES)                                    # the tables, over NRAND random lines
    want += DEPTHS * (MID + (S8 + S8x16 + S16) * (DEPTH_WINDOWS + windows))                     # plane samples: in range; equal to the 8-bit oracle's
    assert r.stdout == "%d comparisons, no disagreement\n" % want, r.stdout
