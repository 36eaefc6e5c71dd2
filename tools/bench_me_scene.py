#!/usr/bin/env python3
"""Times the scene-change detection (ffhip_me_scene_sequence_dev: k_me_scene_sad and k_me_scene_flags) and the four-call frame-rate
conversion it completes.

First case: the detection alone on one sequence of 61 luma pictures of 3840 x 2160 (60 pairs, 506 MB at 8 bits: twice the Infinity
Cache, so every pass comes from HBM), at depth 8 and at depth 10, with a frame_pitch that is a multiple of 16 (the wide loads) and, at
depth 8, with one that is not (every sample loaded alone).  Per row: milliseconds per pair (median of --rounds timed windows of at least
--window seconds each, after warm-up launches; device events round whole windows), the spread of the windows, and the bytes per second
on the ALGORITHMIC bytes, 2 * W * H samples per pair (a picture in the middle of a sequence is read by two pairs; the second read may
come from a cache), against the 8.0 TB/s of the data sheet (6.29 TB/s is what a float4 copy reaches on this part).  It is a call's share,
not a kernel's: the memset of the sums, both kernels and the launch gaps are inside the window.  Before anything is timed the device's
sums, scores and flags are checked against the host face on 1920 x 1080.

Second case: the pipeline on the panning 4:2:0 sequence of tools/bench_me_interp.py (17 pictures, 2 instants per pair), with a hard cut
put in the middle: "device" is search forward, search backward, detection, interpolation with the flags, four calls and one
synchronisation at the end; "host decision" is what a caller had to do without the detection face: both searches, a synchronisation, the
luma planes copied back, the same rule on the CPU (the host face), the job table built with BLEND at the cut, then the interpolation.
Wall-clock milliseconds per sequence, median of --rounds runs.

    python tools/bench_me_scene.py [--out profiles/me_scene_bench.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_me_interp import MB, NFRAMES, R, make_sequence, ramp  # noqa: E402
from bench_me_search import timed  # noqa: E402

W, H, NPICS = 3840, 2160, 61
HBM_PEAK = 8.0e12
RECORDED = "recorded earlier on the same part: 0.141 ms per pair for a sequence search, 0.335 ms per output picture for the interpolation"


def check(torch, np, me):
    """the device against the host face: 4 pictures of 1920 x 1080 at both depths"""
    for depth in (8, 10):
        px = 2 if depth > 8 else 1
        w, h, n = 1920, 1080, 4
        frames = np.random.default_rng(depth).integers(0, 256, n * w * h * px, dtype=np.uint8)
        frames[2 * w * h * px:] >>= 2
        sad, score, flags, mafd = np.zeros(n - 1, np.uint64), np.zeros(n - 1, np.float32), np.zeros(n - 1, np.uint8), np.zeros(1)
        me.scene_sequence_host(frames, depth, w, h, w * px, w * h * px, n, 0, 1, 10.0, mafd_out=mafd, sad_out=sad, score_out=score, flags_out=flags)
        d = torch.from_numpy(frames).cuda()
        dsad = torch.zeros(n - 1, dtype=torch.int64, device="cuda")
        dscore = torch.zeros(n - 1, dtype=torch.float32, device="cuda")
        dflags = torch.zeros(n - 1, dtype=torch.uint8, device="cuda")
        dmafd = torch.zeros(1, dtype=torch.float64, device="cuda")
        me.scene_sequence(d, depth, w, h, w * px, w * h * px, n, 0, 1, 10.0, mafd_out=dmafd, sad_out=dsad, score_out=dscore, flags_out=dflags)
        torch.cuda.synchronize()
        assert np.array_equal(dsad.cpu().numpy().view(np.uint64), sad) and np.array_equal(dscore.cpu().numpy().view(np.uint32), score.view(np.uint32)) and \
            np.array_equal(dflags.cpu().numpy(), flags) and np.array_equal(dmafd.cpu().numpy().view(np.uint64), mafd.view(np.uint64)), \
            "the device and the host face differ at depth %d" % depth


def detection(torch, me, a, lines):
    for depth, extra, what in ((8, 0, "wide loads"), (10, 0, "wide loads"), (8, 4, "single samples")):
        px = 2 if depth > 8 else 1
        fp = W * H * px + extra
        g = torch.Generator(device="cuda").manual_seed(depth + extra)
        frames = torch.randint(0, 256, ((NPICS - 1) * fp + W * H * px,), dtype=torch.uint8, device="cuda", generator=g)
        flags = torch.zeros(NPICS - 1, dtype=torch.uint8, device="cuda")
        score = torch.zeros(NPICS - 1, dtype=torch.float32, device="cuda")
        call = lambda: me.scene_sequence(frames, depth, W, H, W * px, fp, NPICS, 0, 1, 10.0, score_out=score, flags_out=flags)
        t = [x / (NPICS - 1) for x in timed(torch, call, a.window, a.rounds)]
        ms = statistics.median(t)
        rate = 2.0 * W * H * px / (ms * 1e-3)
        lines.append("%-10s %5d %-15s %10.4f %8.4f..%-8.4f %10.1f %8.1f%%" % ("%dx%d" % (W, H), depth, what, ms, min(t), max(t), rate / 1e9,
                                                                              100 * rate / HBM_PEAK))
        print(lines[-1], flush=True)
        del frames


def pipeline(torch, np, me, a, lines):
    w, h = W, H
    planes = list(make_sequence(torch, w, h))
    cut = NFRAMES // 2
    for p in planes:
        p[cut:] = 255 - p[cut:]                        # a hard cut before picture `cut`
    npairs = NFRAMES - 1
    per = (w // MB) * (h // MB)
    mv = [torch.zeros((npairs, per * 2), dtype=torch.int16, device="cuda") for _ in range(2)]
    cost = torch.zeros((npairs, per), dtype=torch.int32, device="cuda")
    strides, pitches = [w, w // 2, w // 2], [w * h, w * h // 4, w * h // 4]
    src = me.planes(planes, strides, pitches, [NFRAMES * p for p in pitches])
    njobs = 2 * npairs
    out = [torch.empty(njobs * p, dtype=torch.uint8, device="cuda") for p in pitches]
    ref = [torch.empty_like(o) for o in out]
    window = ramp(MB)
    flags = torch.zeros(npairs, dtype=torch.uint8, device="cuda")
    instants = [(k, al) for k in range(npairs) for al in (341, 683)]
    mci_jobs = [(0, k, al, me.MCI) for k, al in instants]

    def search():
        for d in range(2):
            me.search_pred_sequence(me.EPZS, planes[0], w, h, w, w * h, NFRAMES, NFRAMES * w * h, 1, d, MB, R, me.SAD, None, None, mv[d], cost)

    def device():
        search()
        me.scene_sequence(planes[0], 8, w, h, w, w * h, NFRAMES, 0, 1, 10.0, flags_out=flags)
        me.interp_sequence_scd(src, me.planes(out, strides, pitches), 3, 1, 1, w, h, NFRAMES, 1, MB, R, window, mv[0], mv[1], mci_jobs, flags, me.SCENE_BLEND)
        torch.cuda.synchronize()

    hflags = np.zeros(npairs, np.uint8)

    def host_decision():
        search()
        torch.cuda.synchronize()
        luma = planes[0].cpu().numpy()
        me.scene_sequence_host(luma, 8, w, h, w, w * h, NFRAMES, 0, 1, 10.0, flags_out=hflags)
        jobs = [(0, k, al, me.BLEND if hflags[k] else me.MCI) for k, al in instants]
        me.interp_sequence(src, me.planes(ref, strides, pitches), 3, 1, 1, w, h, NFRAMES, 1, MB, R, window, mv[0], mv[1], jobs)
        torch.cuda.synchronize()

    device()
    host_decision()
    assert hflags[cut - 1] == 1 and np.array_equal(flags.cpu().numpy(), hflags), "the flags of the two routes differ"
    assert all(torch.equal(o, r) for o, r in zip(out, ref)), "the pictures of the two routes differ"
    for name, fn in (("device", device), ("host decision", host_decision)):
        t = []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        lines.append("%-10s %-15s %10.3f %8.3f..%-8.3f" % ("%dx%d" % (w, h), name, statistics.median(t), min(t), max(t)))
        print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "me_scene_bench.txt"))
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_me_scene: no GPU: nothing is measured")
    from ffmpeg_amd import me
    check(torch, np, me)
    lines = ["# tools/bench_me_scene.py on %s: the detection of one sequence of %d luma pictures (%d pairs), score_out and flags_out asked for; "
             "ms = median of %d windows of >= %.2f s" % (torch.cuda.get_device_name(0), NPICS, NPICS - 1, a.rounds, a.window),
             "# ms per pair and the call's share of the %.1f TB/s HBM peak on 2 * W * H samples per pair; %s" % (HBM_PEAK / 1e12, RECORDED),
             "%-10s %5s %-15s %10s %18s %10s %9s" % ("size", "depth", "loads", "ms", "windows min..max", "GB/s", "of peak")]
    detection(torch, me, a, lines)
    lines += ["# the pipeline on one 4:2:0 sequence of %d pictures with a hard cut, %d output pictures: wall-clock ms per sequence, median of %d runs"
              % (NFRAMES, 2 * (NFRAMES - 1), a.rounds),
              "%-10s %-15s %10s %18s" % ("size", "route", "ms", "runs min..max")]
    pipeline(torch, np, me, a, lines)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
