#!/usr/bin/env python3
"""tools/bench_vp9_scaled_frame.py — VP9 inter reconstruction of whole frames from references of another size
(ffhip_vp9_inter_frames_scaled_dev).

Inputs: 4:2:0 frames of tests/vp9_scaled_frame_gen.py with a smooth MV field, blocks of 8 x 8 and up, 5 % intra holes, 2 references
both of the other size: 1920x1088 from 1280x720 references (up), 1280x720 from 1920x1088 (down) and 960x544 from 1920x1088 (2x down,
the end where a call reads the most reference rows); 8 and 10 bits; single-reference and compound (85 % of the blocks).  Runs: 1 and
16 frames per launch, HIP events after warm-up, median of --reps (>= 10): ms per frame.  The same frame through the per-call batch
faces (tests/vp9_scaled_batch_path.py: padded references, scaled_mc_batch / mc_batch put / avg + itxfm_add_batch) gives the
comparison: launches and ms.  Destination planes are whole superblocks (the batch faces write a block's overhang).  --quick: the
two 8-bit single-reference cases of 1080p and 2x down, for a rocprofv3 --kernel-trace --stats run of its own (the kernel time)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import vp9_scaled_batch_path as BP  # noqa: E402
import vp9_scaled_frame_gen as S  # noqa: E402
import test_gpu_vp9_scaled_frame as T  # noqa: E402  (its upload helpers)
from ffmpeg_amd import _lib, vp9  # noqa: E402

CASES = {"single ref": dict(p_comp=0.0), "compound": dict(p_comp=0.85)}
SIZES = {"up": ((1920, 1088), (1280, 720)), "down": ((1280, 720), (1920, 1088)), "2x down": ((960, 544), (1920, 1088))}


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
    for kind, ((W, H), (rw, rh)) in SIZES.items():
        if args.quick and kind == "down":
            continue
        for bd in ((8,) if args.quick else (8, 10)):
            for name, kw in CASES.items():
                if args.quick and name != "single ref":
                    continue
                rng = np.random.default_rng(W + bd + len(name))
                fr = S.ScaledFrame(rng, W, H, bd, 1, 1, [(rw, rh), (rw, rh)], p_intra=0.05, p_far=0.0, p_edge=0.0, min_log2=3, smooth=True,
                                   **kw)
                big = [np.zeros(((fr.sb_h * 64) >> fr.vs[p], (fr.sb_w * 64) >> fr.hs[p]), np.int64) for p in range(3)]
                for p in range(3):
                    big[p][:fr.dh[p], :fr.dw[p]] = fr.planes[p]
                fr.planes = big
                a, dst, keep = T.upload(torch, fr)
                res = {"case": "vp9 scaled inter frames %dx%d from %dx%d 4:2:0 %d-bit, %s" % (W, H, rw, rh, bd, name),
                       "records_per_frame": len(fr.preds), "tus_per_frame": sum(len(t) for t in fr.tus)}
                for npics in (1, 16):
                    # more frames: the same records and references, destination planes of their own
                    extra = [([(d.clone(),) + pl[1:] for pl, (_, d) in zip(a[0], dst)],) + a[1:] for _ in range(npics - 1)]
                    pics = [a] + extra
                    med, lo, hi = timed(lambda: vp9.inter_frames_scaled(pics, [fr.ref_sizes] * npics, W, H, ss=(1, 1), bit_depth=bd),
                                        args.reps)
                    res["ms_per_frame_%d" % npics] = round(med / npics, 4)
                    res["ms_per_launch_min_max_%d" % npics] = [round(lo, 4), round(hi, 4)]
                    del extra
                if not args.quick:
                    path = BP.BatchPath(torch, fr, [pl[1] for pl in a[0]], overhang=True)
                    other = [torch.empty_like(d) for _, d in dst]
                    med, lo, hi = timed(lambda: path.run(other), args.reps)
                    res["batch_faces_launches"] = path.launches()
                    res["batch_faces_ms_per_frame"] = round(med, 4)
                    del path, other
                torch.cuda.synchronize()
                print(json.dumps(res), flush=True)
                del keep


if __name__ == "__main__":
    main()
