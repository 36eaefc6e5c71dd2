"""kernels/hevc_mc_rules.h, the one statement of the HEVC motion-compensation arithmetic, compiled for the host and walked against
the oracle by tests/hevc_mc_rules_check.cpp: hevcmc_sample at all 16 luma and 64 chroma fractions (8, 10, 12 bits; random windows,
windows of 0 and of the maximum, the two sign-matched extremes of each fraction's filters) against ffo_hevc_mc_bd in put and uni mode,
hevcmc_out's uni_w / bi / bi_w over the weight sets of tests/mc_matrix.py:weights() against ffo_hevc_mc_w_bd, and the generated
v_dot2 operand and byte tables against the taps (the operand layout also against words written out by hand).  Undefined behaviour
(a shift of a negative offset, say) ends the program."""
import os
import subprocess

import ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ffmpeg_amd", "csrc")

NRAND = 20                              # random windows per fraction (the program's argument)
DEPTHS, FRACTIONS, FIXED_WINDOWS, BLOCK = 3, 16 + 64, 4, 2 * 2      # 8 / 10 / 12 bits; luma + chroma; 0, max, two extremes; 2 x 2 samples
WEIGHT_SETS = 3 * 3 * 3 * 2 + 8 * 3 * 3 * 3                         # the two kinds of mc_matrix.weights() as grids
HAND_WORDS = 6                          # dot2 operand words the program has as literals
OTHER_LIST, WEIGHTED_MODES = 4, 3                                   # -8192, 0, the largest, random; uni_w, bi, bi_w


def table_checks(taps):
    """per fraction: two parities of taps / 2 + 1 pairs of two halves, two padding words, the byte row"""
    return (32 // taps) * (2 * (taps // 2 + 1) * 2 + 2 + taps)


def test_the_header_equals_the_oracle(tmp_path):
    assert os.path.exists(ffi.ORACLE_SO), "oracle/liboracle.so missing - run build()"
    exe = tmp_path / "hevc_mc_rules_check"
    oracle = os.path.join(ROOT, "oracle")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
                    "-I", CSRC, "-I", oracle, "-o", str(exe), os.path.join(ROOT, "tests", "hevc_mc_rules_check.cpp"), ffi.ORACLE_SO,
                    "-Wl,-rpath," + oracle], check=True)
    r = subprocess.run([str(exe), str(NRAND)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    want = DEPTHS * FRACTIONS * (NRAND + FIXED_WINDOWS) * BLOCK * 2     # put and uni
    want += DEPTHS * 2 * WEIGHT_SETS * OTHER_LIST * WEIGHTED_MODES * BLOCK
    want += table_checks(8) + table_checks(4) + HAND_WORDS
    assert r.stdout == "%d comparisons, no disagreement\n" % want, r.stdout
