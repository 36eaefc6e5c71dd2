#!/usr/bin/env python3
"""tools/bench_hevc_intra_picture.py — HEVC intra reconstruction of whole pictures (ffhip_hevc_intra_pictures_dev): all-intra 4:2:0
pictures of tests/hevc_intra_picture_gen.py (random CU / TU quadtrees, 64 x 64 CTBs, modes mixed, half the blocks with residuals),
1080p and 4K at 8 and 10 bits, 1 and 16 pictures per launch.  One GPU, HIP events; ms per launch and per picture.  The figure is a
dependency chain's latency (ctb_w + 2 ctb_h CTB steps, blocks one after another inside a CTB), not a bandwidth."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import hevc_intra_picture_gen as G  # noqa: E402
from ffmpeg_amd import _lib, hevc  # noqa: E402

dev = torch.device("cuda", 0)
for (W, H) in ((1920, 1080), (3840, 2160)):
    for bd in (8, 10):
        pic = G.Picture(np.random.default_rng(W + bd), W, H, 6, bd, 1, p_intra=1.0)
        ps = 1 if bd == 8 else 2
        dt = np.uint8 if bd == 8 else np.uint16
        side = []
        for p in range(3):
            arr, starts = pic.pack(p, dtype=hevc.INTRA_TU_DTYPE)
            side.append((torch.from_numpy(arr.view(np.uint8).copy()).to(dev), torch.from_numpy(starts).to(dev),
                         torch.from_numpy(pic.res[p]).to(dev)))
        nblk = sum(len(r) for r in pic.recs)
        n4 = sum(1 for r in pic.recs[0] if r["log2_size"] == 2)
        for npics in (1, 16):
            keep, pics = [], []
            for i in range(npics):
                planes = []
                for p in range(3):
                    h, w = pic.planes[p].shape
                    stride = (w * ps + 255) // 256 * 256
                    host = np.zeros((h, stride), np.uint8)
                    host[:, :w * ps] = pic.planes[p].astype(dt).view(np.uint8).reshape(h, w * ps)
                    d = torch.from_numpy(host).to(dev)
                    keep.append(d)
                    planes.append((d, stride) + side[p])
                pics.append(planes)
            hevc.intra_pictures(pics, W, H, 6, bit_depth=bd)
            assert _lib.lib().ffhip_stream_synchronize(None) == 0
            ms, reps = [], 10
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                hevc.intra_pictures(pics, W, H, 6, bit_depth=bd)
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
            assert _lib.lib().ffhip_stream_synchronize(None) == 0
            med = float(np.median(ms))
            print(json.dumps({"case": "hevc intra pictures %dx%d 4:2:0 %d-bit, 64x64 CTBs, all intra, %d per launch" % (W, H, bd, npics),
                              "blocks_per_picture": nblk, "luma_4x4_share": round(n4 / len(pic.recs[0]), 3),
                              "ms_per_launch": round(med, 3), "ms_per_picture": round(med / npics, 3),
                              "ms_min_max": [round(min(ms), 3), round(max(ms), 3)]}), flush=True)
