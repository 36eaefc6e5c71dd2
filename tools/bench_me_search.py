#!/usr/bin/env python3
"""Times the filter's per-block motion searches (ffhip_me_search_batch_dev, methods TSS .. HEXBS) and its predictive ones
(ffhip_me_search_pred_batch_dev, EPZS and UMH) beside the exhaustive face (ffhip_me_esa_batch_dev) on 3840 x 2160 frame pairs, 8 pairs
per launch, 16 x 16 blocks, at search_param 7 and 32, SAD and SATD.

Input: a smooth texture (box-filtered noise, stretched to the full range), the current frame = the reference moved by (3, -2) plus
noise of +-2: uniform noise alone has no slope for a pattern search to follow.  Per row: milliseconds per frame pair (median of
--rounds timed windows of at least --window seconds each, after two warm-up launches; device events round whole windows), the spread of
the windows, MB-searches/s, and the mean number of costs a block evaluates — the counters of ffhip_me_search_frames_host() on the FIRST
pair of the same input (the exhaustive rows: the window sizes, from the geometry).  The last column compares with the exhaustive face
at the same search_param and metric, from the same run.

EPZS and UMH search a pair in wavefront order (one wave per block row, each two blocks behind the row above), so a pair's time is a
chain of about b_w + 2 * b_h blocks, and pairs of one launch overlap: their rows come twice, at 8 pairs per launch and ("/1") at 1 pair
per launch, the latter with the chain's time per block.  prev1 = prev2 = the vectors EPZS finds without them (a sequence at rest).

    python tools/bench_me_search.py [--out profiles/me_search_bench.txt]

--sequences runs another section instead: whole sequences (2, 9, 17 and 61 pictures, 1 and 2 sequences per call) through
ffhip_me_search_pred_sequence_dev against the same pairs as chained calls of the pair face on one stream — the caller's only way before
that face — and, for EPZS, against the same number of independent pairs in one call (sequence_section()).

    python tools/bench_me_search.py --sequences [--out profiles/me_seq_search_bench.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, NF, MB = 3840, 2160, 8, 16
NAMES = {1: "esa", 2: "tss", 3: "tdls", 4: "ntss", 5: "fss", 6: "ds", 7: "hexbs", 8: "epzs", 9: "umh"}
SEQ_PICTURES, SEQ_NSEQ = (2, 9, 17, 61), (1, 2)     # the sequence section: pictures per sequence, sequences per call


def make_input(torch):
    g = torch.Generator(device="cuda").manual_seed(4)
    big = torch.rand((NF, 1, H + 16, W + 16), device="cuda", generator=g)
    big = torch.nn.functional.avg_pool2d(big, 9, stride=1, padding=4)
    big = (big - big.amin()) / (big.amax() - big.amin()) * 255.0
    ref = big[:, 0, 8:8 + H, 8:8 + W]
    cur = big[:, 0, 8 - 2:8 - 2 + H, 8 + 3:8 + 3 + W] + torch.randint(-2, 3, (NF, H, W), device="cuda", generator=g)
    to8 = lambda t: t.round().clamp(0, 255).to(torch.uint8).contiguous()
    return to8(cur), to8(ref)


def timed(torch, call, window, rounds):
    """-> the per-launch milliseconds of `rounds` windows"""
    ev = lambda: torch.cuda.Event(enable_timing=True)
    for _ in range(2):
        call()
    e0, e1 = ev(), ev()
    e0.record()
    for _ in range(3):
        call()
    e1.record()
    torch.cuda.synchronize()
    reps = max(3, min(2000, int(window * 1e3 / max(e0.elapsed_time(e1) / 3, 1e-3))))
    out = []
    for _ in range(rounds):
        e0, e1 = ev(), ev()
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return out


def pred_rows(torch, np, me, a, cur, ref, hcur, href, mv, cost, hmv, hcost, kind, kname, R, esa_ms):
    """the EPZS and UMH rows of one metric and search_param: 8 pairs per launch, then 1 pair per launch"""
    nb = (W // MB) * (H // MB)
    out = []
    prev = torch.empty_like(mv)
    me.search_pred_batch(me.EPZS, cur, ref, W, H, W, W * H, NF, MB, R, kind, None, None, prev, cost)
    torch.cuda.synchronize()
    hprev = prev[0].cpu().numpy()
    for method in (me.EPZS, me.UMH):
        blocks, costs = me.search_pred_frames_host(method, hcur, href, W, H, W, W * H, 1, MB, R, kind, hprev, hprev, hmv, hcost)
        me.search_pred_batch(method, cur, ref, W, H, W, W * H, NF, MB, R, kind, prev, prev, mv, cost)
        torch.cuda.synchronize()
        assert np.array_equal(mv[0].cpu().numpy(), hmv) and np.array_equal(cost[0].cpu().numpy().view(np.uint32), hcost), \
            "the device and the host face differ"
        for nf in (NF, 1):
            call = lambda: me.search_pred_batch(method, cur, ref, W, H, W, W * H, nf, MB, R, kind, prev, prev, mv, cost)
            t = [x / nf for x in timed(torch, call, a.window, a.rounds)]
            ms = statistics.median(t)
            out.append("%-6s %-5s %3d %12.4f %8.4f..%-8.4f %16.4g %12.1f %8.3f"
                       % (NAMES[method] + ("" if nf == NF else "/1"), kname, R, ms, min(t), max(t), nb / (ms * 1e-3), costs / blocks, ms / esa_ms))
            if nf == 1:
                out[-1] += "   chain: %.2f us per block over b_w + 2 * b_h = %d blocks" % (ms * 1e3 / (W // MB + 2 * (H // MB)), W // MB + 2 * (H // MB))
            print(out[-1], flush=True)
    return out


def esa_costs_per_block(R):
    """the start plus the window, averaged over the blocks of a frame"""
    bw, bh = W // MB, H // MB
    nx = [min(x * MB + R, (bw - 1) * MB) - max(0, x * MB - R) + 1 for x in range(bw)]
    ny = [min(y * MB + R, (bh - 1) * MB) - max(0, y * MB - R) + 1 for y in range(bh)]
    return 1 + sum(nx) * sum(ny) / (bw * bh)


def make_sequences(torch, nseq, nframes):
    """nseq sequences of nframes pictures: a smooth texture per sequence that drifts by a vector that changes from picture to picture
    (at most 3 samples a picture in x and y), plus noise of +-2 -> (nseq, nframes, H, W) uint8"""
    g = torch.Generator(device="cuda").manual_seed(61)
    frames = torch.empty((nseq, nframes, H, W), dtype=torch.uint8, device="cuda")
    m = 3 * nframes + 8
    for s in range(nseq):
        big = torch.rand((1, 1, H + 2 * m, W + 2 * m), device="cuda", generator=g)
        big = torch.nn.functional.avg_pool2d(big, 9, stride=1, padding=4)[0, 0]
        big = (big - big.amin()) / (big.amax() - big.amin()) * 255.0
        x = y = m
        for p in range(nframes):
            dx, dy = (int(v) for v in torch.randint(-3, 4, (2,), device="cuda", generator=g).cpu())
            x, y = x + dx, y + dy
            frames[s, p] = (big[y:y + H, x:x + W] + torch.randint(-2, 3, (H, W), device="cuda", generator=g)).round().clamp(0, 255).to(torch.uint8)
    return frames


def sequence_section(torch, me, a):
    """Sequences of 2, 9, 17 and 61 pictures, 1 and 2 sequences per call, EPZS and UMH, SAD and SATD, search_param a.R, per pair:
      (a) chained  np calls of ffhip_me_search_pred_batch_dev on one stream, one step (nseq pairs) each, prev fields the two steps before;
      (b) sequence one call of ffhip_me_search_pred_sequence_dev, checked equal to (a) before it is timed;
      (c) batch    EPZS only: the np * nseq pairs as INDEPENDENT pairs in one call of the pair face (prev NULL) — not the same result:
                   the bound a pipeline can approach, not a like-for-like figure."""
    nb = (W // MB) * (H // MB)
    longest = max(SEQ_PICTURES)
    all_frames = make_sequences(torch, 2, longest)
    plane = W * H
    lines = ["# tools/bench_me_search.py --sequences on %s: %d x %d, %d x %d blocks, search_param %d; ms per pair = median of %d windows of >= %.2f s"
             % (torch.cuda.get_device_name(0), W, H, MB, MB, a.R, a.rounds, a.window),
             "# chained: np calls of the pair face on one stream (one step of nseq pairs each); sequence: one call of the sequence face, checked equal to chained;",
             "# batch: the same pairs as independent ones in one call of the pair face (EPZS; another result: the bound, not a like-for-like figure)",
             "%-6s %-5s %4s %4s %-9s %12s %18s %10s" % ("method", "cost", "pics", "nseq", "path", "ms/pair", "windows min..max", "x chained")]
    for kind, kname in ((me.SAD, "sad"), (me.SATD, "satd")):
        for method in (me.EPZS, me.UMH):
            for nframes in SEQ_PICTURES:
                for nseq in SEQ_NSEQ:
                    np_ = nframes - 1
                    frames = all_frames[:nseq]          # seq_pitch stays that of the longest sequence
                    mv_a = torch.zeros((np_, nseq, nb * 2), dtype=torch.int16, device="cuda")
                    mv_b, mv_c = torch.ones_like(mv_a), torch.empty_like(mv_a)
                    cost_a = torch.zeros((np_, nseq, nb), dtype=torch.int32, device="cuda")
                    cost_b, cost_c = torch.ones_like(cost_a), torch.empty_like(cost_a)

                    def chained():
                        for k in range(np_):
                            me.search_pred_batch(method, frames[0, k + 1], frames[0, k], W, H, W, longest * plane, nseq, MB, a.R, kind,
                                                 mv_a[k - 1] if k >= 1 else None, mv_a[k - 2] if k >= 2 else None, mv_a[k], cost_a[k])

                    def sequence():
                        me.search_pred_sequence(method, frames, W, H, W, plane, nframes, longest * plane, nseq, 0, MB, a.R, kind, None, None, mv_b, cost_b)

                    def batch():
                        for s in range(nseq):
                            me.search_pred_batch(method, frames[s, 1], frames[s, 0], W, H, W, plane, np_, MB, a.R, kind, None, None, mv_c[:, s], cost_c[:, s])

                    chained()
                    sequence()
                    torch.cuda.synchronize()
                    assert torch.equal(mv_a, mv_b) and torch.equal(cost_a, cost_b), "the sequence face and the chained calls differ"
                    base = None
                    for path, call in (("chained", chained), ("sequence", sequence)) + ((("batch", batch),) if method == me.EPZS and nseq == 1 else ()):
                        t = [x / (np_ * nseq) for x in timed(torch, call, a.window, a.rounds)]
                        ms = statistics.median(t)
                        base = ms if base is None else base
                        lines.append("%-6s %-5s %4d %4d %-9s %12.4f %8.4f..%-8.4f %10.3f" % (NAMES[method], kname, nframes, nseq, path, ms, min(t), max(t), ms / base))
                        print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sequences", action="store_true", help="the section on whole sequences (the sequence face against chained calls) instead")
    ap.add_argument("--R", type=int, default=7, help="search_param of the sequence section")
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "me_seq_search_bench.txt" if a.sequences else "me_search_bench.txt")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_me_search: no GPU: nothing is measured")
    from ffmpeg_amd import me
    if a.sequences:
        lines = sequence_section(torch, me, a)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return
    cur, ref = make_input(torch)
    hcur, href = cur[0].cpu().numpy(), ref[0].cpu().numpy()
    nb = (W // MB) * (H // MB)
    mv = torch.empty((NF, nb * 2), dtype=torch.int16, device="cuda")
    cost = torch.empty((NF, nb), dtype=torch.int32, device="cuda")
    import numpy as np
    hmv, hcost = np.zeros(nb * 2, np.int16), np.zeros(nb, np.uint32)
    lines = ["# tools/bench_me_search.py on %s: %d pairs of %d x %d per launch, %d x %d blocks; ms per pair = median of %d windows of >= %.2f s"
             % (torch.cuda.get_device_name(0), NF, W, H, MB, MB, a.rounds, a.window),
             "# costs/block: the host face's counters on the first pair (esa: from the window sizes); x esa: this row's time over esa's at the same R and metric",
             "# epzs, umh: blocks in wavefront order; name/1: 1 pair per launch, with the time per block of the b_w + 2 * b_h chain; prev1 = prev2 = EPZS's vectors without them",
             "%-6s %-5s %3s %12s %18s %16s %12s %8s" % ("method", "cost", "R", "ms/pair", "windows min..max", "MB-searches/s", "costs/block", "x esa")]
    for kind, kname in ((me.SAD, "sad"), (me.SATD, "satd")):
        for R in (7, 32):
            esa_ms = None
            for method in range(1, 8):
                if method == me.ESA:
                    call = lambda: me.esa_batch(cur, ref, W, H, W, W * H, NF, MB, R, kind, mv, cost)
                    per_block = esa_costs_per_block(R)
                else:
                    call = lambda: me.search_batch(method, cur, ref, W, H, W, W * H, NF, MB, R, kind, mv, cost)
                    blocks, costs = me.search_frames_host(method, hcur, href, W, H, W, W * H, 1, MB, R, kind, hmv, hcost)
                    per_block = costs / blocks
                    call()
                    torch.cuda.synchronize()
                    assert np.array_equal(mv[0].cpu().numpy(), hmv) and np.array_equal(cost[0].cpu().numpy().view(np.uint32), hcost), \
                        "the device and the host face differ"
                t = [x / NF for x in timed(torch, call, a.window, a.rounds)]
                ms = statistics.median(t)
                if method == me.ESA:
                    esa_ms = ms
                lines.append("%-6s %-5s %3d %12.4f %8.4f..%-8.4f %16.4g %12.1f %8.3f"
                             % (NAMES[method], kname, R, ms, min(t), max(t), nb / (ms * 1e-3), per_block, ms / esa_ms))
                print(lines[-1], flush=True)
                if method == me.HEXBS:
                    lines.extend(pred_rows(torch, np, me, a, cur, ref, hcur, href, mv, cost, hmv, hcost, kind, kname, R, esa_ms))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
