#!/usr/bin/env python3
"""tools/bench_vp8.py — the vp8dsp batch faces and the whole-frame VP8 loop filter.

Cases: the MC batch over every 16 x 16 position of 8 planes of 3840 x 2160 (one 2-D 6-tap call, put_vp8_epel_pixels_tab[0][2][2], per
position, mx / my random in 1..7; a bilinear run beside it); the IDCT batch over every 4 x 4 block of a 1920 x 1080 plane (half full
transforms, half dc-only); the frame loop filter at 1920 x 1088 (120 x 68 macroblocks), normal and simple, inter frames with levels
over 1..63 and inner edges everywhere, 1 and 16 frames per launch.  HIP events after a warm-up, median of --reps.  Each case prints ms
and the fraction of the 8 TB/s HBM peak that the bytes it must move at the least (every sample and record read once, every output
written once) would take at that time."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from ffmpeg_amd import _lib, vp8  # noqa: E402

HBM = 8e12


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


def report(case, ms, nbytes, **kw):
    print(json.dumps(dict(case=case, ms=round(ms, 4), hbm_fraction=round(nbytes / (ms * 1e-3) / HBM, 4), **kw)), flush=True)


def bench_mc(rng, reps, bilinear):
    W, H, B, NP = 3840, 2160, 16, 8
    SW = W + 2 * B
    src = torch.from_numpy(rng.integers(0, 256, (NP * (H + 2 * B), SW)).astype(np.uint8)).cuda()
    dst = torch.empty((NP * H, W), dtype=torch.uint8, device="cuda")
    by, bx = np.mgrid[0:H // 16, 0:W // 16]
    by, bx = by.reshape(-1), bx.reshape(-1)
    per = len(by)
    recs = np.zeros(NP * per, vp8.MC_DTYPE)
    for p in range(NP):
        r = recs[p * per:(p + 1) * per]
        r["dst_offset"] = (p * H + 16 * by) * W + 16 * bx
        r["src_offset"] = (p * (H + 2 * B) + B + 16 * by) * SW + B + 16 * bx
    recs["width"], recs["h"] = 16, 16
    recs["mx"], recs["my"] = rng.integers(1, 8, len(recs)), rng.integers(1, 8, len(recs))
    recs["htaps"], recs["vtaps"], recs["bilinear"] = 2, 2, int(bilinear)
    d_recs = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
    ms = timed(lambda: vp8.mc_batch(dst, W, src, SW, d_recs, len(recs)), reps)
    report("vp8 mc batch, %s 16x16 h 16 at every position of 8 planes 3840x2160" % ("bilinear hv" if bilinear else "epel h6v6"), ms,
           2 * NP * W * H + 16 * len(recs), records=len(recs))


def bench_idct(rng, reps):
    W, H = 1920, 1080
    n = (W // 4) * (H // 4)
    plane = torch.from_numpy(rng.integers(0, 256, (H, W)).astype(np.uint8)).cuda()
    co_h = rng.integers(-200, 200, (n, 16)).astype(np.int16)
    co = torch.from_numpy(co_h).cuda()
    by, bx = np.mgrid[0:H // 4, 0:W // 4]
    recs = np.zeros(n, vp8.IDCT_DTYPE)
    recs["dst_offset"] = (4 * by.reshape(-1)) * W + 4 * bx.reshape(-1)
    recs["coeff_offset"] = np.arange(n) * 32
    recs["dc_only"] = np.arange(n) & 1
    d_recs = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
    # the face consumes the coefficients: later runs transform zero blocks, the same loads, arithmetic and stores
    ms = timed(lambda: vp8.idct_add_batch(plane, W, co, d_recs, n), reps)
    report("vp8 idct_add batch, every 4x4 block of 1920x1080 (half dc-only)", ms, 2 * W * H + n * (32 + 32 + 12), records=n)


def bench_lf(rng, reps, filter_type):
    mb_w, mb_h = 120, 68
    sy, suv = 16 * mb_w + 64, 8 * mb_w + 32
    res = {}
    for npics in (1, 16):
        pics = []
        for _ in range(npics):
            yy, xx = np.mgrid[0:16 * mb_h, 0:sy]
            Y = np.clip(128 + 50 * np.sin(yy / 13.0) * np.cos(xx / 17.0) + rng.integers(-6, 7, yy.shape), 0, 255).astype(np.uint8)
            U = np.clip(128 + rng.integers(-8, 9, (8 * mb_h, suv)), 0, 255).astype(np.uint8)
            st = np.zeros((mb_h, mb_w), vp8.STRENGTH_DTYPE)
            st["filter_level"] = rng.integers(1, 64, (mb_h, mb_w))
            st["inner_limit"] = np.maximum(st["filter_level"] >> 1, 1)
            st["inner_filter"] = 1
            pics.append((torch.from_numpy(Y).cuda(), torch.from_numpy(U).cuda(), torch.from_numpy(U.copy()).cuda(),
                         torch.from_numpy(st.view(np.uint8).reshape(-1).copy()).cuda()))
        ms = timed(lambda: vp8.loopfilter_frames(pics, filter_type, 0, mb_w, mb_h, sy, suv), reps)
        planes = 1.5 if filter_type == 0 else 1.0
        res[npics] = ms
        report("vp8 frame loop filter 1920x1088 %s, %d frame%s per launch" % ("normal" if filter_type == 0 else "simple", npics,
                                                                              "s" if npics > 1 else ""),
               ms, npics * (2 * planes * 256 * mb_w * mb_h + 3 * mb_w * mb_h), ms_per_frame=round(ms / npics, 4))
        del pics
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    rng = np.random.default_rng(8)
    bench_mc(rng, args.reps, False)
    bench_mc(rng, args.reps, True)
    bench_idct(rng, args.reps)
    bench_lf(rng, args.reps, 0)
    bench_lf(rng, args.reps, 1)


if __name__ == "__main__":
    main()
