#!/usr/bin/env python3
"""tools/bench_vp9_inter_frame.py — VP9 inter reconstruction of whole frames (ffhip_vp9_inter_frames_dev).

Inputs: 4:2:0 frames of tests/vp9_inter_frame_gen.py with a smooth MV field (one vector per superblock plus a few eighth samples of
noise), blocks of 8 x 8 and up, 5 % intra holes, 3 references, frame sizes of whole superblocks; 1080p and 4K at 8 and 10 bits;
single-reference and compound (85 % of the blocks).  Runs: 1 and 16 frames per launch, HIP events after warm-up, median of --reps
(>= 10).  Prints, per case, ms per frame and a byte model over the launch time (planes written + coefficients read + the reference
windows the records need, (w + 7)(h + 7) samples per reference) as a share of the 8 TB/s HBM peak.  The same frame through the
per-call batch faces (tests/vp9_inter_batch_path.py: padded references, mc_batch put / avg + itxfm_add_batch) gives the comparison:
launches and ms.  --quick: one 1080p case each, for a rocprofv3 --kernel-trace --stats run of its own (the kernel time)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import vp9_inter_batch_path as BP  # noqa: E402
import vp9_inter_frame_gen as G  # noqa: E402
import test_gpu_vp9_inter_frame as T  # noqa: E402  (its upload helpers)
from ffmpeg_amd import _lib, vp9  # noqa: E402

HBM_PEAK = 8.0e12
CASES = {"single ref": dict(p_comp=0.0), "compound": dict(p_comp=0.85)}


def byte_model(fr):
    ps = 1 if fr.bd == 8 else 2
    cs = 2 if fr.bd == 8 else 4
    b = 0
    for p in range(3):
        for rec in fr.preds:
            if (rec["flags"] >> 1) & 1 != int(p > 0):
                continue
            w, h = rec["w"], rec["h"]
            b += w * h * ps                                                     # written
            b += (1 + (rec["flags"] & 1)) * (w + 7) * (h + 7) * ps              # reference windows
        b += sum((16 if t["tx"] == 4 else 16 << (2 * t["tx"])) * cs for t in fr.tus[p])   # coefficients
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
    return float(np.median(ms)), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    assert args.reps >= 10 or args.quick, "--reps: at least 10"
    sizes = ((1920, 1088),) if args.quick else ((1920, 1088), (3840, 2176))
    depths = (8,) if args.quick else (8, 10)
    for (W, H) in sizes:
        for bd in depths:
            for name, kw in CASES.items():
                rng = np.random.default_rng(W + bd + len(name))
                fr = G.InterFrame(rng, W, H, bd, 1, 1, nrefs=3, p_intra=0.05, p_far=0.0, p_edge=0.0, min_log2=3, smooth=True, **kw)
                nbytes = byte_model(fr)
                refs = T.upload_refs(torch, fr)
                a, dst, keep = T.upload(torch, fr, refs=refs)
                res = {"case": "vp9 inter frames %dx%d 4:2:0 %d-bit, %s" % (W, H, bd, name), "records_per_frame": len(fr.preds),
                       "tus_per_frame": sum(len(t) for t in fr.tus), "model_bytes_per_frame": nbytes}
                for npics in (1, 16):
                    # more frames: the same records and references, destination planes of their own
                    extra = [([(d.clone(),) + pl[1:] for pl, (_, d) in zip(a[0], dst)],) + a[1:] for _ in range(npics - 1)]
                    pics = [a] + extra
                    med, lo, hi = timed(lambda: vp9.inter_frames(pics, W, H, ss=(1, 1), bit_depth=bd), args.reps)
                    res["ms_per_frame_%d" % npics] = round(med / npics, 4)
                    res["ms_per_launch_min_max_%d" % npics] = [round(lo, 4), round(hi, 4)]
                    res["hbm_share_%d" % npics] = round(nbytes * npics / (med * 1e-3) / HBM_PEAK, 3)
                    del extra
                # the same frame through the batch faces
                path = BP.BatchPath(torch, fr, [pl[1] for pl in a[0]])
                other = [torch.empty_like(d) for _, d in dst]
                med, lo, hi = timed(lambda: path.run(other), args.reps)
                res["batch_faces_launches"] = path.launches()
                res["batch_faces_ms_per_frame"] = round(med, 4)
                torch.cuda.synchronize()
                print(json.dumps(res), flush=True)
                del keep, refs, path, other


if __name__ == "__main__":
    main()
