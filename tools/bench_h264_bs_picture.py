#!/usr/bin/env python3
"""tools/bench_h264_bs_picture.py — H.264 deblocking edge parameters of whole pictures (ffhip_h264_edge_params_pictures_dev).

Inputs: the test generator's pictures (tests/h264_bs_picture_gen.py: 4 slices of both types, 20 % intra macroblocks, every
partition) at 1080p (120 x 68 macroblocks) and 2160p (240 x 135), with chroma tables.
Runs, after warm-up, median of --reps (>= 20):
  face_ms_1 / face_ms_16   the _dev face with 1 and 16 pictures per launch, ms per picture (HIP events);
  host_ms                  the device-free _host face on one CPU thread for one picture (wall clock);
  upload_ms                the copy of that picture's three tables from pinned host memory to the device (HIP events);
  replaced_ms              host_ms + upload_ms: the path the _dev face replaces, of the same commit's _host face.
One JSON line per size, then a table."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import h264_bs_picture_gen as G  # noqa: E402
import test_gpu_h264_bs_picture as T  # noqa: E402  (its upload helper)
from ffmpeg_amd import _lib, h264  # noqa: E402


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
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    reps = max(20, args.reps)
    rows = []
    for mb_w, mb_h in ((120, 68), (240, 135)):
        rng = np.random.default_rng(mb_w)
        pics = [G.BsPicture(rng, mb_w, mb_h, 0, 0, 4) for _ in range(2)]
        ups = [T.upload(torch, pics[i % 2]) for i in range(16)]
        call = lambda n: h264.edge_params_pictures([u[0] for u in ups[:n]], mb_w, mb_h)
        one = timed(lambda: call(1), reps)
        sixteen = timed(lambda: call(16), reps) / 16
        host = []
        for _ in range(reps):
            t0 = time.perf_counter()
            h264.edge_params_pictures_host([ups[0][1]], mb_w, mb_h)
            host.append((time.perf_counter() - t0) * 1e3)
        d, m = ups[0]
        pinned = [torch.from_numpy(m["_" + t].view(np.uint8)).pin_memory() for t in T.TABLES]
        upload = timed(lambda: [d["_" + t].copy_(p, non_blocking=True) for t, p in zip(T.TABLES, pinned)], reps)
        host_ms = float(np.median(host))
        row = dict(case="%dx%d" % (16 * mb_w, 16 * mb_h), face_ms_1=round(one, 4), face_ms_16=round(sixteen, 4), host_ms=round(host_ms, 3),
                   upload_ms=round(upload, 4), replaced_ms=round(host_ms + upload, 3), table_mbytes=round(sum(p.numel() for p in pinned) / 1e6, 2))
        rows.append(row)
        print(json.dumps(row), flush=True)
    print("| case | face 1/launch ms | face 16/launch ms/pic | host face ms (1 thread) | upload of 3 tables ms | host + upload ms | tables MB |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %.4f | %.4f | %.3f | %.4f | %.3f | %.2f |" % (r["case"], r["face_ms_1"], r["face_ms_16"], r["host_ms"], r["upload_ms"],
                                                               r["replaced_ms"], r["table_mbytes"]))


if __name__ == "__main__":
    main()
