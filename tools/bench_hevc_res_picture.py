#!/usr/bin/env python3
"""tools/bench_hevc_res_picture.py — HEVC residuals of whole pictures (ffhip_hevc_residual_pictures_dev).

Inputs: 4:2:0 pictures at 1080p and 4K, 8 and 10 bits, about 60 % of the area coded.  Luma area by TU size: 25 % 4x4, 35 % 8x8,
25 % 16x16, 15 % 32x32; chroma a quarter of the luma record counts per size.  Kinds per record (tests/hevc_res_picture_gen.py's
mix): about 55 % DCT (scan-consistent coefficients and col_limit), 20 % DC-only, 25 % of luma 4x4 the DST, 10 % transform skip
(rotation and RDPCM among them at 4x4), 8 % bypass, 7 % cbf-0 records.
Runs: 1 and 16 pictures per launch (16 pictures of two contents, each picture with buffers of its own, so that nothing is
read from a cache that another picture filled), HIP events after warm-up, median of --reps (>= 10).  Prints, per case, ms per picture of the
face and of the per-call path (tests/hevc_res_batch_path.py: idct_batch per (kind, size), then RDPCM_H / RDPCM_V, per plane; the
records it can express, which is all but rotation and the cbf-0 ones) with the launches each takes, and a byte model (coefficients
read, residuals written, 16-byte records) over the face's time at 16 pictures as a share of the 8 TB/s HBM peak.
--quick: 1080p only and the face alone at --pics pictures per launch, for a rocprofv3 --kernel-trace --stats run of its own (the
kernel time)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import hevc_res_batch_path as BP  # noqa: E402
import hevc_res_picture_gen as G  # noqa: E402
from ffmpeg_amd import _lib, hevc  # noqa: E402

HBM_PEAK = 8.0e12


def counts(W, H):
    """records per size of a picture with about 60 % of its luma coded"""
    a = W * H * 0.6
    luma = [int(a * f / (1 << (2 * (s + 2)))) for s, f in enumerate((0.25, 0.35, 0.25, 0.15))]
    return [luma, [c // 4 for c in luma], [c // 4 for c in luma]]


def upload(planes):
    return [(torch.from_numpy(D.coeffs.copy()).cuda(), torch.zeros(D.nres, dtype=torch.int16, device="cuda"),
             torch.from_numpy(np.ascontiguousarray(D.tus).view(np.uint8).copy()).cuda(), D.size_start) for D in planes]


def byte_model(planes):
    b = 0
    for D in planes:
        for t in D.tus:
            n = 1 << (2 * int(t["log2_size"]))
            b += 16 + 2 * n + (0 if int(t["kind_flags"]) & 7 == G.ZERO else 2 * n)
    return b


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
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--pics", type=int, default=16, help="--quick: pictures per launch")
    args = ap.parse_args()
    reps = max(10, args.reps)
    sizes = [(1920, 1080)] if args.quick else [(1920, 1080), (3840, 2160)]
    rows = []
    for W, H in sizes:
        for bd in (8, 10):
            rng = np.random.default_rng(W + bd)
            pics = [G.build_planes(rng, counts(W, H), 1, gap=0) for _ in range(2)]
            ups = [upload(pics[i % 2]) if i < 2 else None for i in range(16)]
            for i in range(2, 16):   # 16 pictures of two contents, each with its own coefficient, record and res buffers in HBM
                ups[i] = [(c.clone(), torch.zeros_like(r), t.clone(), ss) for c, r, t, ss in ups[i % 2]]
            call = lambda n: hevc.residual_pictures(ups[:n], chroma_format_idc=1, bit_depth=bd)
            if args.quick:
                print(json.dumps(dict(case="%dx%d %d-bit" % (W, H, bd), pics=args.pics, ms=round(timed(lambda: call(args.pics), reps), 4))))
                continue
            one = timed(lambda: call(1), reps)
            sixteen = timed(lambda: call(16), reps) / 16
            paths = [BP.BatchPath(torch, D, bd) for D in pics[0]]
            per_call = timed(lambda: [p.run() for p in paths], reps)
            copies = timed(lambda: [p.src.clone() for p in paths], reps)   # run() starts from a clone of the coefficients
            mb = byte_model(pics[0])
            row = dict(case="%dx%d %d-bit 4:2:0" % (W, H, bd), face_ms_1=round(one, 4), face_ms_16=round(sixteen, 4), face_launches=1,
                       per_call_ms=round(per_call - copies, 4), per_call_launches=sum(len(p.calls) for p in paths),
                       mbytes=round(mb / 1e6, 2), hbm_share_16=round(mb / (sixteen * 1e-3) / HBM_PEAK, 3))
            rows.append(row)
            print(json.dumps(row), flush=True)
    print("| case | face 1/launch ms | face 16/launch ms/pic | per-call path ms (launches) | MB model | share of 8 TB/s at 16 |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %.3f | %.3f | %.3f (%d) | %.2f | %.2f |" % (r["case"], r["face_ms_1"], r["face_ms_16"], r["per_call_ms"],
                                                               r["per_call_launches"], r["mbytes"], r["hbm_share_16"]))


if __name__ == "__main__":
    main()
