#!/usr/bin/env python3
"""tools/bench_hevc_inter_picture.py — HEVC inter reconstruction of whole pictures (ffhip_hevc_inter_pictures_dev).

Inputs: 4:2:0 pictures of tests/hevc_inter_picture_gen.py with a smooth MV field (one vector per 64 x 64 area plus a few quarter
samples of noise), 64 x 64 CTBs, 95 % inter CUs, 4 references; 1080p and 4K at 8 and 10 bits; P (uni), B (85 % bi) and B weighted.
Runs: 1 and 16 pictures per launch, HIP events after warm-up, median of --reps (>= 10).  Prints, per case, ms per picture and a byte
model over the launch time (planes written + residuals read + the reference windows the PUs need, (w + 7)(h + 7) luma and
(w + 3)(h + 3) chroma samples per list) as a share of the 8 TB/s HBM peak.  The same picture through the per-call batch faces
(tests/hevc_inter_batch_path.py: padded references, mc_batch / mc_w_batch + idct_batch add) gives the comparison: launches and ms.
--quick: one 1080p case each, for a rocprofv3 --kernel-trace --stats run of its own (the kernel time)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import hevc_inter_batch_path as BP  # noqa: E402
import hevc_inter_picture_gen as G  # noqa: E402
import test_gpu_hevc_inter_picture as T  # noqa: E402  (its upload helpers)
from ffmpeg_amd import _lib, hevc  # noqa: E402

HBM_PEAK = 8.0e12
CASES = {"P uni": dict(slice_types=["P"], weighted=False), "B bi": dict(slice_types=["B"], weighted=False, p_bi=0.85),
         "B weighted": dict(slice_types=["B"], weighted=True, p_bi=0.85)}


def byte_model(pic):
    ps = 1 if pic.bd == 8 else 2
    b = 0
    for p in range(pic.nplanes):
        taps = 4 if p else 8
        for pu in pic.pus:
            bw, bh = pu["w"] >> pic.hs[p], pu["h"] >> pic.vs[p]
            b += bw * bh * ps                                           # written
            b += bin(pu["flags"]).count("1") * (bw + taps - 1) * (bh + taps - 1) * ps   # reference windows
        b += sum(2 << (2 * t["log2_size"]) for t in pic.tus[p] if t["res_offset"] >= 0)  # residuals
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
    sizes = ((1920, 1080),) if args.quick else ((1920, 1080), (3840, 2160))
    depths = (8,) if args.quick else (8, 10)
    for (W, H) in sizes:
        for bd in depths:
            for name, kw in CASES.items():
                rng = np.random.default_rng(W + bd + len(name))
                pic = G.InterPicture(rng, W, H, 6, bd, 1, nrefs=4, nslices=2, p_inter=0.95, p_pcm=0.0, p_far=0.0, smooth=True, **kw)
                ps = 1 if bd == 8 else 2
                dt = np.uint8 if bd == 8 else np.uint16
                nbytes = byte_model(pic)
                refs = T.upload_refs(torch, pic)
                a, dst, keep = T.upload(torch, pic, refs=refs)
                res = {"case": "hevc inter pictures %dx%d 4:2:0 %d-bit, 64x64 CTBs, %s" % (W, H, bd, name), "pus_per_picture": len(pic.pus),
                       "model_bytes_per_picture": nbytes}
                for npics in (1, 16):
                    # more pictures: the same records and DPB, destination planes of their own
                    extra = [([(d.clone(),) + pl[1:] for pl, (_, d) in zip(a[0], dst)],) + a[1:] for _ in range(npics - 1)]
                    pics = [a] + extra
                    med, lo, hi = timed(lambda: hevc.inter_pictures(pics, W, H, 6, bit_depth=bd), args.reps)
                    res["ms_per_picture_%d" % npics] = round(med / npics, 4)
                    res["ms_per_launch_min_max_%d" % npics] = [round(lo, 4), round(hi, 4)]
                    res["hbm_share_%d" % npics] = round(nbytes * npics / (med * 1e-3) / HBM_PEAK, 3)
                    del extra
                # the same picture through the batch faces
                path = BP.BatchPath(torch, pic, [pl[1] for pl in a[0]])
                other = [torch.empty_like(d) for _, d in dst]
                med, lo, hi = timed(lambda: path.run(other), args.reps)
                res["batch_faces_launches"] = path.launches()
                res["batch_faces_ms_per_picture"] = round(med, 4)
                torch.cuda.synchronize()
                print(json.dumps(res), flush=True)
                del keep, refs, path, other


if __name__ == "__main__":
    main()
