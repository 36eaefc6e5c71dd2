#!/usr/bin/env python
"""Timing of the bilateral motion search of whole sequences (ffhip_me_search_bilat_sequence_dev) beside the existing sequence face
(ffhip_me_search_pred_sequence_dev, SAD, direction 0) on the same pictures in the same process, in the manner of
tools/bench_me_interp.py: 3840 x 2160, 16 x 16 blocks, sequences of --pictures pictures (default 61), 1 sequence per call, EPZS and UMH,
search_param --R (default 32).  Per pair: the median of --rounds windows of at least --window seconds after two warm-up calls.

The bilateral face is checked equal to its host face on the first pair before it is timed.  costs/block is the host face's counter on
that pair; GB/s is the bytes the bilateral cost loads — 2 * (2 * mb)^2 per cost — over the time, the block SAD's mb^2 (the current
block stays in registers) for the existing face.

--variants runs the measurement build (libffhip_measure.so) instead and adds a third row per method: the bilateral kernel without the
early predictor pass (FFHIP_ME_BILAT_NO_EARLY=1), checked equal to the same host face — all three rows from the same build.

--interp runs another section instead (out: profiles/me_bilat_interp_bench.txt): the panning 4:2:0 sequence of 17 pictures of
tools/bench_me_interp.py, 16 x 16 blocks, search_param = mv_range 32.
  compensation: ms per 32 jobs (2 instants per pair, all MCI) at 1920 x 1080 and 3840 x 2160, ffhip_me_interp_sequence_dev (k_me_interp,
    the two EPZS fields of the sequence face) beside ffhip_me_interp_bilat_sequence_dev (k_me_interp_bilat, the one bilateral EPZS
    field), the latter checked against its host face on one job at 1080p first;
  conversion: wall-clock ms per sequence, the final synchronisation included, median of --rounds runs: the bidir chain — search,
    search, detection, interpolation with the flags — beside the bilat chain — search, detection, bilateral interpolation — on torch's
    current stream, 32 output pictures each.

    python tools/bench_me_bilat.py [--variants | --interp] [--out profiles/me_bilat_bench.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_me_search import H, MB, NAMES, W, make_sequences, timed  # noqa: E402


def interp_section(torch, np, me, a):
    import time

    import bench_me_interp as BI
    NF, R = BI.NFRAMES, BI.R
    window = BI.ramp(MB)
    lines = ["# tools/bench_me_bilat.py --interp on %s: 4:2:0, %d x %d blocks, mv_range %d, a panning sequence of %d pictures, EPZS fields; "
             "median of %d windows of >= %.2f s (compensation) or of %d runs (conversion)" % (torch.cuda.get_device_name(0), MB, MB, R, NF, a.rounds, a.window, a.rounds),
             "# bidir: ffhip_me_interp_sequence_scd_dev from two fields of ffhip_me_search_pred_sequence_dev; bilat: ffhip_me_interp_bilat_sequence_dev from one "
             "field of ffhip_me_search_bilat_sequence_dev",
             "%-11s %-13s %-6s %14s %20s %8s" % ("size", "stage", "mode", "ms", "min..max", "x bidir")]
    for W, H in BI.SIZES:
        planes = BI.make_sequence(torch, W, H)
        np_, per, plane = NF - 1, (W // MB) * (H // MB), W * H
        mv = [torch.zeros((np_, per * 2), dtype=torch.int16, device="cuda") for _ in range(3)]      # direction 0, direction 1, bilateral
        cost = torch.zeros((np_, per), dtype=torch.int32, device="cuda")
        flags = torch.zeros(np_, dtype=torch.uint8, device="cuda")
        strides, pitches = [W, W // 2, W // 2], [plane, plane // 4, plane // 4]
        src = me.planes(planes, strides, pitches, [NF * p for p in pitches])
        jobs = [(0, j // 2, (1024 * (j % 2 + 1)) // 3, me.MCI) for j in range(2 * np_)]
        out = [torch.empty(len(jobs) * p, dtype=torch.uint8, device="cuda") for p in pitches]
        dst = me.planes(out, strides, pitches)
        search2 = lambda: [me.search_pred_sequence(me.EPZS, planes[0], W, H, W, plane, NF, NF * plane, 1, d, MB, R, me.SAD, None, None, mv[d], cost)
                           for d in range(2)]
        search1 = lambda: me.search_bilat_sequence(me.EPZS, planes[0], W, H, W, plane, NF, NF * plane, 1, MB, R, None, None, mv[2], cost)
        scene = lambda: me.scene_sequence(planes[0], 8, W, H, W, plane, NF, NF * plane, 1, 10.0, flags_out=flags)
        comp2 = lambda: me.interp_sequence_scd(src, dst, 3, 1, 1, W, H, NF, 1, MB, R, window, mv[0], mv[1], jobs, flags)
        comp1 = lambda: me.interp_bilat_sequence(src, dst, 3, 1, 1, W, H, NF, 1, MB, R, window, mv[2], jobs, flags)
        search2(), search1(), scene()
        torch.cuda.synchronize()
        if (W, H) == BI.SIZES[0]:       # the bilateral compensation against its host face, one job
            hp = [p.cpu().numpy() for p in planes]
            hout = [np.zeros(p, np.uint8) for p in pitches]
            job = [(0, 3, 341, me.MCI)]
            me.interp_bilat_sequence_host(me.planes(hp, strides, pitches, [NF * p for p in pitches]), me.planes(hout, strides, pitches), 3, 1, 1, W, H, NF, 1,
                                          MB, R, window, mv[2].cpu().numpy(), job)
            dout = [torch.zeros(p, dtype=torch.uint8, device="cuda") for p in pitches]
            me.interp_bilat_sequence(src, me.planes(dout, strides, pitches), 3, 1, 1, W, H, NF, 1, MB, R, window, mv[2], job)
            torch.cuda.synchronize()
            assert all(np.array_equal(d.cpu().numpy(), h) for d, h in zip(dout, hout)), "the device and the host face differ"
        size, base = "%dx%d" % (W, H), None
        for mode, call in (("bidir", comp2), ("bilat", comp1)):
            t = timed(torch, call, a.window, a.rounds)
            ms = statistics.median(t)
            base = ms if base is None else base
            lines.append("%-11s %-13s %-6s %14.4f %9.4f..%-9.4f %8.3f" % (size, "comp/32 jobs", mode, ms, min(t), max(t), ms / base))
            print(lines[-1], flush=True)
        base = None
        for mode, chain in (("bidir", (search2, scene, comp2)), ("bilat", (search1, scene, comp1))):
            t = []
            for i in range(a.rounds + 2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for c in chain:
                    c()
                torch.cuda.synchronize()
                t.append((time.perf_counter() - t0) * 1e3)
            t = t[2:]                   # two warm-up runs
            ms = statistics.median(t)
            base = ms if base is None else base
            lines.append("%-11s %-13s %-6s %14.4f %9.4f..%-9.4f %8.3f" % (size, "conversion", mode, ms, min(t), max(t), ms / base))
            print(lines[-1], flush=True)
        del out, dst, planes
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--interp", action="store_true", help="the section on the compensation and the whole conversion instead")
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--pictures", type=int, default=61)
    ap.add_argument("--R", type=int, default=32)
    ap.add_argument("--variants", action="store_true", help="the measurement build, with the bilateral kernel without its early pass as a third row")
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_me_bilat: no GPU: nothing is measured")
    from ffmpeg_amd import _lib, me
    a.out = a.out or os.path.join(ROOT, "profiles", "me_bilat_interp_bench.txt" if a.interp else "me_bilat_bench.txt")
    if a.interp:
        lines = interp_section(torch, np, me, a)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return
    if a.variants:
        _lib.select("measure")
    nb, plane, np_ = (W // MB) * (H // MB), W * H, a.pictures - 1
    frames = make_sequences(torch, 1, a.pictures)
    h0, h1 = frames[0, 0].cpu().numpy(), frames[0, 1].cpu().numpy()
    mv = torch.empty((np_, 1, nb * 2), dtype=torch.int16, device="cuda")
    cost = torch.empty((np_, 1, nb), dtype=torch.int32, device="cuda")
    hmv, hcost = np.zeros(nb * 2, np.int16), np.zeros(nb, np.uint32)
    lines = ["# tools/bench_me_bilat.py on %s: 1 sequence of %d pictures of %d x %d, %d x %d blocks, search_param %d; ms per pair = median of %d windows of >= %.2f s"
             % (torch.cuda.get_device_name(0), a.pictures, W, H, MB, MB, a.R, a.rounds, a.window),
             "# build: %s" % ("measurement (libffhip_measure.so); bilat-ne: FFHIP_ME_BILAT_NO_EARLY=1, no early predictor pass" if a.variants else "product"),
             "# pred: ffhip_me_search_pred_sequence_dev, SAD, direction 0; bilat: ffhip_me_search_bilat_sequence_dev, checked equal to its host face on pair 0",
             "# costs/block: the host face's counters on pair 0; GB/s: costs * bytes loaded per cost (pred: mb^2, bilat: 2 * (2 mb)^2) over the time",
             "%-6s %-8s %12s %18s %12s %10s %8s" % ("method", "face", "ms/pair", "windows min..max", "costs/block", "GB/s", "x pred")]
    for method in (me.EPZS, me.UMH):
        base = None
        for face in ("pred", "bilat") + (("bilat-ne",) if a.variants else ()):
            os.environ.pop("FFHIP_ME_BILAT_NO_EARLY", None)
            if face == "bilat-ne":
                os.environ["FFHIP_ME_BILAT_NO_EARLY"] = "1"
            if face == "pred":
                call = lambda: me.search_pred_sequence(method, frames, W, H, W, plane, a.pictures, a.pictures * plane, 1, 0, MB, a.R, me.SAD, None, None, mv, cost)
                blocks, costs = me.search_pred_frames_host(method, h1, h0, W, H, W, plane, 1, MB, a.R, me.SAD, None, None, hmv, hcost)
                per_cost = MB * MB
            else:
                call = lambda: me.search_bilat_sequence(method, frames, W, H, W, plane, a.pictures, a.pictures * plane, 1, MB, a.R, None, None, mv, cost)
                blocks, costs = me.search_bilat_frames_host(method, h0, h1, W, H, W, plane, 1, MB, a.R, None, None, hmv, hcost)
                per_cost = 2 * (2 * MB) ** 2
            call()
            torch.cuda.synchronize()
            assert np.array_equal(mv[0, 0].cpu().numpy(), hmv) and np.array_equal(cost[0, 0].cpu().numpy().view(np.uint32), hcost), \
                "the device and the host face differ on pair 0"
            t = [x / np_ for x in timed(torch, call, a.window, a.rounds)]
            ms = statistics.median(t)
            base = ms if base is None else base
            lines.append("%-6s %-8s %12.4f %8.4f..%-8.4f %12.1f %10.1f %8.3f"
                         % (NAMES[method], face, ms, min(t), max(t), costs / blocks, costs * per_cost / (ms * 1e-3) / 1e9, ms / base))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
