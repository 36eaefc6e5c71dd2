#!/usr/bin/env python3
"""tools/bench_hevc_bs_picture.py — HEVC deblocking boundary strengths of whole pictures (ffhip_hevc_boundary_strengths_pictures_dev).

Inputs: the test generator's pictures (tests/hevc_bs_picture_gen.py: CU quadtrees, every partition mode, transform trees, 4 slices,
3 x 2 tiles) with 64 x 64 CTBs at 1080p and 4K.
Runs: 1 and 16 pictures per launch, HIP events after warm-up, median of --reps (>= 20).  Prints, per size, ms per picture of the
face, a byte model (12 B motion field + 1 B tu in, 2 B out per 4 x 4 unit, the halo column and row of each 64 x 64 tile re-read)
over the 16-per-launch time as a share of the 8 TB/s HBM peak, the device-free host face on one CPU thread for the same pictures
(what the decoder stops paying), and the chain: the in-loop filter from two maps uploaded from host memory (upload included) against
boundary strengths made on the device followed by the same filter call.
--quick: the face alone at --pics pictures per launch, 1080p, for a rocprofv3 --kernel-trace --stats run of its own (the kernel
time)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
import bench_hevc_lf_picture as LB  # noqa: E402  (its numpy-drawn filter pictures and its timer)
import hevc_bs_picture_gen as G  # noqa: E402
import test_gpu_hevc_bs_picture as T  # noqa: E402  (its upload helper)
import test_gpu_hevc_lf_picture as TL  # noqa: E402
from ffmpeg_amd import hevc  # noqa: E402

HBM_PEAK = 8.0e12


def byte_model(pic):
    tiles = -(-pic.w4 // 16) * -(-pic.h4 // 16)
    return pic.w4 * pic.h4 * (12 + 1 + 2) + tiles * 33 * 12 + 2 * len(pic.ctb_slice) * 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--pics", type=int, default=16, help="--quick: pictures per launch")
    args = ap.parse_args()
    reps = max(20, args.reps)
    rows = []
    for W, H in [(1920, 1080)] if args.quick else [(1920, 1080), (3840, 2160)]:
        rng = np.random.default_rng(W)
        pics = [G.BsPicture(rng, W, H, 6, tiles=(3, 2), nslices=4) for _ in range(2)]
        ups = [T.upload(torch, pics[i % 2]) for i in range(16)]
        call = lambda n: hevc.boundary_strengths_pictures([u[0] for u in ups[:n]], W, H, 6)
        if args.quick:
            print(json.dumps(dict(case="%dx%d" % (W, H), pics=args.pics, ms=round(LB.timed(lambda: call(args.pics), reps), 4))))
            continue
        one = LB.timed(lambda: call(1), reps)
        sixteen = LB.timed(lambda: call(16), reps) / 16
        host = []
        for _ in range(5):
            t0 = time.perf_counter()
            hevc.boundary_strengths_pictures_host([ups[0][1]], W, H, 6)
            host.append((time.perf_counter() - t0) * 1e3)
        # the chain: the filter's pictures are bench_hevc_lf_picture's; only where the bS maps come from differs
        lf = LB.picture(np.random.default_rng(W + 8), W, H, 8)
        av, ah, _, _ = G.model_a_of(pics[0])
        (planes, maps), _ = TL.upload(torch, lf, bs=(av, ah))
        hv, hh = maps["bs_ver"].cpu().pin_memory(), maps["bs_hor"].cpu().pin_memory()
        d = dict(ups[0][0])
        d["bs_ver"], d["bs_hor"], d["bs_stride"] = maps["bs_ver"], maps["bs_hor"], maps["bs_stride"]
        filt = lambda: hevc.loop_filter_pictures([(planes, maps)], W, H, 6, 3, chroma_format_idc=1, bit_depth=8)
        uploaded = LB.timed(lambda: (maps["bs_ver"].copy_(hv, non_blocking=True), maps["bs_hor"].copy_(hh, non_blocking=True), filt()), reps)
        chained = LB.timed(lambda: (hevc.boundary_strengths_pictures([d], W, H, 6), filt()), reps)
        alone = LB.timed(filt, reps)
        row = dict(case="%dx%d CTB 64" % (W, H), face_ms_1=round(one, 4), face_ms_16=round(sixteen, 4), host_ms_1thread=round(float(np.median(host)), 3),
                   mbytes=round(byte_model(pics[0]) / 1e6, 2), hbm_share_16=round(byte_model(pics[0]) / (sixteen * 1e-3) / HBM_PEAK, 3),
                   lf_alone_ms=round(alone, 4), lf_uploaded_maps_ms=round(uploaded, 4), lf_device_maps_ms=round(chained, 4))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if rows:
        print("| case | face 1/launch ms | face 16/launch ms/pic | host face ms (1 thread) | MB model | share of 8 TB/s at 16 | filter alone ms | "
              "upload 2 maps + filter ms | bS on device + filter ms |")
        print("|---|---|---|---|---|---|---|---|---|")
        for r in rows:
            print("| %s | %.3f | %.4f | %.2f | %.2f | %.3f | %.3f | %.3f | %.3f |" % (
                r["case"], r["face_ms_1"], r["face_ms_16"], r["host_ms_1thread"], r["mbytes"], r["hbm_share_16"], r["lf_alone_ms"],
                r["lf_uploaded_maps_ms"], r["lf_device_maps_ms"]))


if __name__ == "__main__":
    main()
