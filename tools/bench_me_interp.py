#!/usr/bin/env python3
"""Times vf_minterpolate's compensation (ffhip_me_interp_sequence_dev, k_me_interp) on 4:2:0 pictures of 1920 x 1080 and 3840 x 2160,
16 x 16 blocks, mv_range 32, beside the two sequence searches that feed it.

Input: one sequence of 17 pictures, a smooth texture (box-filtered noise, stretched to the full range) that pans by a vector changing
from picture to picture (at most 3 samples a picture in x and y) plus noise of +-2; chroma is the luma averaged 2 x 2.  The fields are
those of ffhip_me_search_pred_sequence_dev (EPZS, SAD, search_param 32), direction 0 and direction 1, found on the device.  The window is
a separable linear ramp.  32 jobs are 2 instants per pair, 256 jobs 16 per pair, all MCI; a row "blend" times the same jobs as BLEND.

Per row: milliseconds per output picture (median of --rounds timed windows of at least --window seconds each, after two warm-up
launches; device events round whole windows), the spread of the windows, and the share of the HBM peak on the ALGORITHMIC bytes — pictures
A and B read once and the output written once, per plane: 3 * 1.5 * W * H bytes per job — against the 8.0 TB/s of the data sheet (6.29 TB/s
is what a float4 copy reaches on this part).  It is a call's share, not a kernel's: launch gaps are inside the window.  The rows "search"
give the time of the two sequence searches per pair, one call per direction, so a reader sees which stage dominates: a pair costs its two
searches once and an interpolation per output picture.  Before anything is timed, job 0 at 1920 x 1080 is checked against the host face.

    python tools/bench_me_interp.py [--out profiles/me_interp_bench.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_me_search import timed  # noqa: E402

NFRAMES, MB, R = 17, 16, 32
SIZES = ((1920, 1080), (3840, 2160))
JOBS = (32, 256)
HBM_PEAK = 8.0e12


def make_sequence(torch, W, H):
    """-> the planes of NFRAMES pictures: (NFRAMES, H, W), (NFRAMES, H / 2, W / 2) twice, uint8"""
    g = torch.Generator(device="cuda").manual_seed(17)
    m = 3 * NFRAMES + 8
    big = torch.rand((1, 1, H + 2 * m, W + 2 * m), device="cuda", generator=g)
    big = torch.nn.functional.avg_pool2d(big, 9, stride=1, padding=4)[0, 0]
    big = (big - big.amin()) / (big.amax() - big.amin()) * 255.0
    y8 = torch.empty((NFRAMES, H, W), dtype=torch.uint8, device="cuda")
    u8 = torch.empty((NFRAMES, H // 2, W // 2), dtype=torch.uint8, device="cuda")
    v8 = torch.empty_like(u8)
    x = y = m
    for p in range(NFRAMES):
        dx, dy = (int(v) for v in torch.randint(-3, 4, (2,), device="cuda", generator=g).cpu())
        x, y = x + dx, y + dy
        luma = (big[y:y + H, x:x + W] + torch.randint(-2, 3, (H, W), device="cuda", generator=g)).round().clamp(0, 255)
        y8[p] = luma.to(torch.uint8)
        c = torch.nn.functional.avg_pool2d(luma[None, None], 2)[0, 0]
        u8[p] = c.round().to(torch.uint8)
        v8[p] = (255 - c).round().to(torch.uint8)
    return y8, u8, v8


def ramp(mb):
    import numpy as np
    n = 2 * mb
    h = np.array([2 * min(i, n - 1 - i) + 1 for i in range(n)])
    return ((h[:, None] * h[None, :]) >> (2 if mb == 16 else 0)).astype(np.uint8).reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "me_interp_bench.txt"))
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_me_interp: no GPU: nothing is measured")
    from ffmpeg_amd import me
    window = ramp(MB)
    lines = ["# tools/bench_me_interp.py on %s: 4:2:0, %d x %d blocks, mv_range %d, a panning sequence of %d pictures, fields of the sequence "
             "face (EPZS, SAD); ms = median of %d windows of >= %.2f s" % (torch.cuda.get_device_name(0), MB, MB, R, NFRAMES, a.rounds, a.window),
             "# interp: ms per output picture and the call's share of the %.1f TB/s HBM peak on 4.5 * W * H algorithmic bytes per picture; "
             "search: ms per pair, both directions together (one call each)" % (HBM_PEAK / 1e12),
             "%-11s %-7s %5s %12s %18s %10s %9s" % ("size", "stage", "jobs", "ms", "windows min..max", "GB/s", "of peak")]
    for W, H in SIZES:
        planes = make_sequence(torch, W, H)
        np_ = NFRAMES - 1
        per = (W // MB) * (H // MB)
        mv = [torch.zeros((np_, per * 2), dtype=torch.int16, device="cuda") for _ in range(2)]
        cost = torch.zeros((np_, per), dtype=torch.int32, device="cuda")
        search = lambda: [me.search_pred_sequence(me.EPZS, planes[0], W, H, W, W * H, NFRAMES, NFRAMES * W * H, 1, d, MB, R, me.SAD, None, None,
                                                  mv[d], cost) for d in range(2)]
        search()
        torch.cuda.synchronize()
        strides, pitches = [W, W // 2, W // 2], [W * H, W * H // 4, W * H // 4]
        src = me.planes(planes, strides, pitches, [NFRAMES * p for p in pitches])
        if (W, H) == SIZES[0]:      # the device against the host face, one job
            hp = [p.cpu().numpy() for p in planes]
            hout = [np.zeros(p, np.uint8) for p in pitches]
            job = [(0, 3, 341, me.MCI)]
            me.interp_sequence_host(me.planes(hp, strides, pitches, [NFRAMES * p for p in pitches]), me.planes(hout, strides, pitches), 3, 1, 1, W, H,
                                    NFRAMES, 1, MB, R, window, mv[0].cpu().numpy(), mv[1].cpu().numpy(), job)
            dout = [torch.zeros(p, dtype=torch.uint8, device="cuda") for p in pitches]
            me.interp_sequence(src, me.planes(dout, strides, pitches), 3, 1, 1, W, H, NFRAMES, 1, MB, R, window, mv[0], mv[1], job)
            torch.cuda.synchronize()
            assert all(np.array_equal(d.cpu().numpy(), h) for d, h in zip(dout, hout)), "the device and the host face differ"
        t = [x / np_ for x in timed(torch, search, a.window, a.rounds)]
        lines.append("%-11s %-7s %5s %12.4f %8.4f..%-8.4f %10s %9s" % ("%dx%d" % (W, H), "search", "-", statistics.median(t), min(t), max(t), "-", "-"))
        print(lines[-1], flush=True)
        for njobs in JOBS:
            out = [torch.empty(njobs * p, dtype=torch.uint8, device="cuda") for p in pitches]
            dst = me.planes(out, strides, pitches)
            k = njobs // np_
            for stage, mode in (("interp", me.MCI), ("blend", me.BLEND)):
                jobs = [(0, j // k, (1024 * (j % k + 1)) // (k + 1), mode) for j in range(njobs)]
                call = lambda: me.interp_sequence(src, dst, 3, 1, 1, W, H, NFRAMES, 1, MB, R, window, mv[0], mv[1], jobs)
                t = [x / njobs for x in timed(torch, call, a.window, a.rounds)]
                ms = statistics.median(t)
                rate = 4.5 * W * H / (ms * 1e-3)
                lines.append("%-11s %-7s %5d %12.4f %8.4f..%-8.4f %10.1f %8.1f%%" % ("%dx%d" % (W, H), stage, njobs, ms, min(t), max(t), rate / 1e9,
                                                                                     100 * rate / HBM_PEAK))
                print(lines[-1], flush=True)
            del out, dst
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
