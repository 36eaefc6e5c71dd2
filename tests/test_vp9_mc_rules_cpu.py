"""kernels/vp9_mc_rules.h, the one statement of the VP9 motion-compensation arithmetic, compiled for the host and walked against the
oracle by tests/vp9_mc_rules_check.cpp: vp9mc_pass and the 2-D form through clipped temporaries against ffo_vp9_mc_bd (filters 0..3,
all 16 x 16 fractions, 8 / 10 / 12 bits, 4 x 4 blocks; random windows, windows of 0 and of the maximum, the two sign-matched extremes
of each fraction's taps; put and avg), the scaled walk with vp9mc_pass0 against ffo_vp9_smc_bd (steps 1, 8, 11, 16, 24, 32 on each
axis, all start fractions, steps of 16 also against the unscaled oracle; one 4 x 64 block at 2x down, whole and in strips of 32 rows),
the generated dword and v_dot2 operand tables against the taps (a few words also against literals of the tables they replaced; every
tap row sums to 128), and vp9mc_avg4 against vp9mc_avg on all byte pairs.  Undefined behaviour ends the program."""
import os
import subprocess

import ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ffmpeg_amd", "csrc")

NRAND = 4                               # random windows per fraction of the unscaled walk (the program's argument)
DEPTHS, FILTERS, FRACTIONS, BLOCK = 3, 4, 16 * 16, 4 * 4            # 8 / 10 / 12 bits; smooth, regular, sharp, bilinear; (mx, my); 4 x 4
FIXED_WINDOWS, PUT_AVG = 4, 2                                       # 0, max, two extremes
STEPS = 6                               # 1, 8, 11, 16, 24, 32 on each axis
TALL = 4 * 64                           # the 134-row block
TABLE_ROWS = 3 * 16                     # filter sets x fractions
HAND_WORDS = 12                         # table words the program has as literals
BYTE_PAIRS, LANES = 256 * 256, 4


def test_the_header_equals_the_oracle(tmp_path):
    assert os.path.exists(ffi.ORACLE_SO), "oracle/liboracle.so missing - run build()"
    exe = tmp_path / "vp9_mc_rules_check"
    oracle = os.path.join(ROOT, "oracle")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
                    "-I", CSRC, "-I", oracle, "-o", str(exe), os.path.join(ROOT, "tests", "vp9_mc_rules_check.cpp"), ffi.ORACLE_SO,
                    "-Wl,-rpath," + oracle], check=True)
    r = subprocess.run([str(exe), str(NRAND)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    want = DEPTHS * FILTERS * FRACTIONS * (NRAND + FIXED_WINDOWS) * BLOCK * PUT_AVG             # unscaled
    want += DEPTHS * FILTERS * FRACTIONS * (STEPS * STEPS * BLOCK * PUT_AVG + BLOCK)            # scaled; steps of 16 against the unscaled oracle
    want += DEPTHS * FILTERS * (1 + TALL * PUT_AVG + 1 + TALL)      # the row count, the block whole, the strips' rows, the strips
    want += TABLE_ROWS * (8 + 1 + 2 * 5 * 2 + 2)                    # bytes, the sum, two parities of five pairs of two halves, padding
    want += HAND_WORDS + BYTE_PAIRS * LANES
    assert r.stdout == "%d comparisons, no disagreement\n" % want, r.stdout
