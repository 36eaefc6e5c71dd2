"""kernels/h264_mc_rules.h, the one statement of the H.264 motion-compensation arithmetic, compiled for the host and walked against
the oracle by tests/h264_mc_rules_check.cpp: h264mc_luma at all 16 positions on 9 x 9 windows (8, 10, 14 bits; random windows and
windows of 0 and the maximum), h264mc_chroma at all 64 fractions, h264mc_weight / h264mc_biweight over the weight ladder at every
depth, h264mc_avg4 against h264mc_avg."""
import os
import subprocess

import ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ffmpeg_amd", "csrc")


def test_the_header_equals_the_oracle(tmp_path):
    assert os.path.exists(ffi.ORACLE_SO), "oracle/liboracle.so missing - run build()"
    exe = tmp_path / "h264_mc_rules_check"
    oracle = os.path.join(ROOT, "oracle")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-I", oracle, "-o", str(exe),
                    os.path.join(ROOT, "tests", "h264_mc_rules_check.cpp"), ffi.ORACLE_SO, "-Wl,-rpath," + oracle], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout
    assert r.stdout.endswith("comparisons, no disagreement\n") and int(r.stdout.split()[0]) > 500000, r.stdout
