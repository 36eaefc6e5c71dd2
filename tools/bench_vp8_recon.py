#!/usr/bin/env python3
"""tools/bench_vp8_recon.py — VP8 reconstruction of whole frames (ffhip_vp8_recon_frames_dev) at 1920 x 1088 (120 x 68 macroblocks).

Cases: a key frame (every macroblock intra, a fifth of them I4x4) and an inter frame (about 10 % intra macroblocks, every
partitioning, one reference, MVs within +-10 samples), each alone and at 16 frames per call; the loop filter of the same frames beside
them (normal filter, levels over 1..63, inner edges everywhere).  HIP events after a warm-up, median of --reps.  With --route the
same two frames also go through the per-call batch faces, launch by launch (tests/vp8_recon_batch_path.py: the only device route
before the frame face), wall clock from the first launch to the end of the stream, and the ratio to the frame face is printed."""
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
from ffmpeg_amd import _lib, vp8  # noqa: E402
import vp8_recon_batch_path as BP  # noqa: E402
import vp8_recon_gen as G  # noqa: E402

MB_W, MB_H = 120, 68


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


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--route", action="store_true", help="also time the per-call batch-face route (seconds per frame)")
    a = ap.parse_args()
    sy, suv = 16 * MB_W, 8 * MB_W
    rng = np.random.default_rng(1)
    st = np.zeros((MB_H, MB_W), vp8.STRENGTH_DTYPE)
    st["filter_level"], st["inner_limit"], st["inner_filter"] = rng.integers(1, 64, st.shape), rng.integers(0, 10, st.shape), 1
    d_st = up(st)
    ref_host = G.planes(3, MB_W, MB_H)
    ref = [up(p) for p in ref_host]
    for name, key in (("keyframe", True), ("inter", False)):
        mbs, co = G.frame(5, MB_W, MB_H, keyframe=key, intra=0.1, mv_range=40, refs=(1,))
        d_mbs, d_co = up(mbs), torch.from_numpy(co).cuda()
        init = G.planes(4, MB_W, MB_H)
        frames = [[up(p) for p in init] for _ in range(16)]
        pics = [dict(y=f[0], u=f[1], v=f[2], refs=[ref, None, None], mbs=d_mbs, coeffs=d_co) for f in frames]
        lf = [(f[0], f[1], f[2], d_st) for f in frames]
        res = dict(case=name, intra_mbs=int((mbs["ref_frame"] == 0).sum()), i4x4_mbs=int(((mbs["ref_frame"] == 0) & (mbs["mode"] == 4)).sum()))
        for n in (1, 16):
            ms = timed(lambda: vp8.recon_frames(pics[:n], MB_W, MB_H, sy, suv), a.reps)
            res["recon_ms_per_call_of_%d" % n], res["recon_ms_per_frame_of_%d" % n] = round(ms, 4), round(ms / n, 4)
            ms = timed(lambda: vp8.loopfilter_frames(lf[:n], 0, int(key), MB_W, MB_H, sy, suv), a.reps)
            res["loopfilter_ms_per_call_of_%d" % n], res["loopfilter_ms_per_frame_of_%d" % n] = round(ms, 4), round(ms / n, 4)
        if a.route:
            t0 = time.perf_counter()
            route = BP.Frame(torch, mbs, co, [ref_host, None, None], init, MB_W, MB_H)
            res["route_plan_s"] = round(time.perf_counter() - t0, 2)
            walls = []
            for _ in range(3):
                route.reset()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                launches = route.issue()
                torch.cuda.synchronize()
                walls.append(time.perf_counter() - t0)
            assert _lib.lib().ffhip_stream_synchronize(None) == 0
            vp8.recon_frames(pics[:1], MB_W, MB_H, sy, suv)
            assert _lib.lib().ffhip_stream_synchronize(None) == 0
            same = all(np.array_equal(r, frames[0][p].cpu().numpy().reshape(r.shape)) for p, r in enumerate(route.result()))
            res.update(route_launches=launches, route_ms_per_frame=round(1e3 * float(np.median(walls)), 1), route_equals_face=bool(same),
                       route_over_face=round(1e3 * float(np.median(walls)) / res["recon_ms_per_call_of_1"], 1))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
