#!/usr/bin/env python3
"""tools/bench_vp9_intra_frame.py — VP9 intra reconstruction of whole frames (ffhip_vp9_intra_frames_dev).

Inputs: 4:2:0 frames of tests/vp9_intra_frame_gen.py: keyframes (every block intra: the random partition down to 8 x 8, all ten
modes, every tx the block allows, 20 % skipped blocks) at 1920 x 1088 (8 and 10 bits) and 3840 x 2176 (8 bits), and 1920 x 1088
inter frames with about 5 % intra blocks, where the face only fills the holes; one tile column.  Runs: 1 and 16 frames per launch,
each frame of a launch with buffers of its own (planes, records, superblock starts, coefficients); HIP events after a warm-up, median
of --reps (>= 10).  Prints, per case, ms per frame and the records per frame.  Reruns of the face on its own output give the same
planes, so every run does the same work.  --quick: the 1080p 8-bit keyframe only, for a rocprofv3
--kernel-trace --stats run of its own (the kernel time)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import vp9_intra_frame_gen as G  # noqa: E402
import test_gpu_vp9_intra_frame as T  # noqa: E402  (its upload helper)
from ffmpeg_amd import _lib, vp9  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    assert _lib.lib().ffhip_stream_synchronize(None) == 0, _lib.lib().ffhip_last_error()
    return float(np.median(ms)), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    assert args.reps >= 10 or args.quick, "--reps: at least 10"
    cases = [("keyframe", 1920, 1088, 8), ("keyframe", 1920, 1088, 10), ("keyframe", 3840, 2176, 8), ("inter, 5 % intra", 1920, 1088, 8)]
    if args.quick:
        cases = cases[:1]
    for name, W, H, bd in cases:
        rng = np.random.default_rng(W + bd + len(name))
        inter = name != "keyframe"
        fr = G.IntraFrame(rng, W, H, bd, 1, 1, inter=inter, p_intra=0.05, min_log2=3)
        a, dst, keep = T.upload(torch, fr)
        res = {"case": "vp9 intra frames %dx%d 4:2:0 %d-bit, %s" % (W, H, bd, name), "records_per_frame": sum(len(r) for r in fr.recs)}
        for npics in (1, 16):
            # more frames: the same content, each frame with planes, records, superblock starts and coefficients of its own
            own = lambda: [(d.clone(), st, recs.clone(), starts.clone(), co.clone())
                           for (_, st, recs, starts, co), (_, d) in zip(a[0], dst)]
            extra = [(own(), a[1]) for _ in range(npics - 1)]
            pics = [a] + extra
            med, lo, hi = timed(lambda: vp9.intra_frames(pics, W, H, ss=(1, 1), bit_depth=bd), args.reps)
            res["ms_per_frame_%d" % npics] = round(med / npics, 4)
            res["ms_per_launch_min_max_%d" % npics] = [round(lo, 4), round(hi, 4)]
            del extra
        torch.cuda.synchronize()
        print(json.dumps(res), flush=True)
        del keep


if __name__ == "__main__":
    main()
