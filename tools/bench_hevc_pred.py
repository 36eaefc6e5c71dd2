#!/usr/bin/env python3
"""tools/bench_hevc_pred.py — HEVC intra prediction (ffhip_hevc_intra_batch_dev) over 8 4K planes: every block of one size tiles the
planes, modes mixed, prepared lines and raw ones (substitution + filtering on the device); depths 8 and 10.  One GPU, HIP events.
Every block of a plane goes in one launch, so the figure is the kernel's rate, not a decoder's: a real picture's wavefront hands
over far fewer blocks per launch.  Bytes = block writes + reference-line reads + records, against 8 TB/s."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from ffmpeg_amd import hevc  # noqa: E402

dev = torch.device("cuda", 0)
W, H, planes = 3840, 2160, 8
rng = np.random.default_rng(7)
for bd in (8, 10):
    ps = 1 if bd == 8 else 2
    pic = torch.zeros(planes * H * W * ps, dtype=torch.uint8, device=dev)
    for log2 in (2, 3, 4, 5):
        N = 1 << log2
        by, bx = np.meshgrid(np.arange(0, planes * H - N + 1, N), np.arange(0, W - N + 1, N), indexing="ij")
        nb = by.size
        ll = 4 * N + 1
        lines = torch.randint(0, 1 << bd, (nb * ll,), dtype=torch.int16 if ps == 2 else torch.uint8, device=dev)
        for raw in (False, True):
            rec = np.zeros(nb, hevc.INTRA_DTYPE)
            rec["dst_offset"] = ((by * W + bx) * ps).ravel()
            rec["edge_offset"] = np.arange(nb) * ll * ps
            rec["log2_size"] = log2
            rec["mode"] = rng.integers(0, 35, nb)
            rec["c_idx_unit"] = hevc.intra_c_idx_unit(0, 2, 2)
            if raw:
                nu = (2 * N) >> 2
                rec["flags"] = hevc.INTRA_RAW | hevc.INTRA_STRONG | (rng.integers(0, 2, nb) * hevc.INTRA_CORNER)
                rec["avail_left"] = rng.integers(0, 1 << nu, nb)
                rec["avail_top"] = rng.integers(0, 1 << nu, nb)
            d_rec = torch.from_numpy(rec.view(np.uint8).reshape(nb, 16)).to(dev)
            hevc.intra_batch(pic, W * ps, lines, d_rec, nb, bit_depth=bd)
            torch.cuda.synchronize()
            ms, reps = 0.0, 10
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                hevc.intra_batch(pic, W * ps, lines, d_rec, nb, bit_depth=bd)
                e1.record()
                torch.cuda.synchronize()
                ms += e0.elapsed_time(e1) / reps
            byt = nb * (N * N * ps + ll * ps + 16)
            print(json.dumps({"case": "hevc intra %dx%d, %d-bit, %s lines, modes mixed, %d 4K planes" % (N, N, bd, "raw" if raw else "prepared", planes),
                              "blocks": nb, "ms": round(ms, 4), "Mblocks/s": round(nb / ms / 1e3, 1), "Gsample/s": round(nb * N * N / ms / 1e6, 1),
                              "hbm_frac": round(byt / ms / 1e6 / 8000, 4)}), flush=True)
