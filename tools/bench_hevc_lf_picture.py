#!/usr/bin/env python3
"""tools/bench_hevc_lf_picture.py — HEVC in-loop filtering of whole pictures (ffhip_hevc_loop_filter_pictures_dev).

Inputs: 4:2:0 pictures of blocky content with 64 x 64 CTBs (min CB 8) at 1080p and 4K, 8 and 10 bits, and a realistic mix: about
40 % of the 8 x 8 grid's luma segments with bS > 0 (a quarter of them 2), QpY 22..37 per 8 x 8, SAO on in about 70 % of the CTBs
(band and edge over all classes, per component), no bypass CUs.  Maps are drawn with numpy, not by the test generator's quadtrees.
Runs: 1 and 16 pictures per launch, HIP events after warm-up, median of --reps (>= 10).  Prints, per case, ms per picture of the
face and of the per-call path (tests/hevc_lf_batch_path.py: loop_filter_batch x 2 -> copy -> sao_batch + sao_restore_batch ->
bypass copy-back, per plane) with the launches each takes, and a byte model over the face's launch time as a share of the 8 TB/s
HBM peak: src read once plus the halo re-read ((C + 8)^2 / C^2 of each plane), dst written, the bS / QP maps and CTB records.
--quick: 1080p only and the face alone at --pics pictures per launch, for a rocprofv3 --kernel-trace --stats run of its own (the
kernel time)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import hevc_lf_batch_path as BP  # noqa: E402
import hevc_lf_picture_gen as G  # noqa: E402
import test_gpu_hevc_lf_picture as T  # noqa: E402  (its upload helpers)
from ffmpeg_amd import _lib, hevc  # noqa: E402

HBM_PEAK = 8.0e12


def picture(rng, W, H, bd):
    """an LfPicture with numpy-drawn maps (the generator's quadtrees are too slow at 4K)"""
    pic = object.__new__(G.LfPicture)
    pic.rng, pic.W, pic.H, pic.log2_ctb, pic.bd, pic.cfi, pic.lmc = rng, W, H, 6, bd, 1, 3
    pic.C, pic.ctb_w, pic.ctb_h = 64, -(-W // 64), -(-H // 64)
    pic.nplanes, pic.hs, pic.vs, pic.maxv = 3, [0, 1, 1], [0, 1, 1], (1 << bd) - 1
    pic.src = [pic._content((H >> pic.vs[p], W >> pic.hs[p])) for p in range(3)]
    pic.cb_qp_offset, pic.cr_qp_offset = 0, 0
    pic.nb_w, pic.nb_h = W // 8, H // 8
    pic.qp = np.kron(rng.integers(22, 38, (pic.nb_h, pic.nb_w)), np.ones((1, 1), np.int64))
    pic.bypass = np.zeros((pic.nb_h, pic.nb_w), np.uint8)
    draw = lambda: np.where(rng.random((H // 4, W // 4)) < 0.4, rng.choice(np.array([1, 1, 1, 2], np.uint8), (H // 4, W // 4)), 0)
    pic.bs_ver, pic.bs_hor = draw().astype(np.uint8), draw().astype(np.uint8)
    pic.bs_ver[:, 1::2] = 0                                      # x % 8 == 0 only
    pic.bs_ver[:, 0] = 0
    pic.bs_hor[1::2, :] = 0
    pic.bs_hor[0, :] = 0
    pic.ctbs = []
    for a in range(pic.ctb_w * pic.ctb_h):
        on = rng.random() < 0.7
        t = [int(rng.integers(1, 3)) if on else 0 for _ in range(3)]
        pic.ctbs.append(dict(beta_offset=0, tc_offset=0, sao_type=t, sao_class=[int(rng.integers(0, 32 if x == 1 else 4)) for x in t],
                             sao_offset_val=np.array([[0] + list(rng.integers(-7, 8, 4)) for _ in range(3)]), restore=0, vert_edge=0,
                             horiz_edge=0, diag_edge=0))
    return pic


def byte_model(pic):
    ps = 1 if pic.bd == 8 else 2
    b = 0
    for p in range(pic.nplanes):
        ph, pw = pic.src[p].shape
        cw, ch = pic.C >> pic.hs[p], pic.C >> pic.vs[p]
        b += ph * pw * ps * (1 + (cw + 8) * (ch + 8) / (cw * ch))   # src with its halo, dst
    b += 2 * pic.bs_ver.size + 2 * pic.qp.size + 44 * len(pic.ctbs)
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
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--pics", type=int, default=16, help="--quick: pictures per launch")
    args = ap.parse_args()
    reps = max(10, args.reps)
    sizes = [(1920, 1080)] if args.quick else [(1920, 1080), (3840, 2160)]
    rows = []
    for W, H in sizes:
        for bd in (8, 10):
            rng = np.random.default_rng(W + bd)
            pics = [picture(rng, W, H, bd) for _ in range(2 if args.quick else 4)]
            ups = [T.upload(torch, pics[i % len(pics)]) for i in range(16)]
            call = lambda n: hevc.loop_filter_pictures([u[0] for u in ups[:n]], W, H, 6, 3, chroma_format_idc=1, bit_depth=bd)
            if args.quick:
                print(json.dumps(dict(case="%dx%d %d-bit" % (W, H, bd), pics=args.pics, ms=round(timed(lambda: call(args.pics), reps), 4))))
                continue
            one = timed(lambda: call(1), reps)
            sixteen = timed(lambda: call(16), reps) / 16
            path = BP.BatchPath(torch, pics[0])
            work = path.upload(pics[0].src)
            fresh = [w.clone() for w in work]
            per_call = timed(lambda: ([w.copy_(f) for w, f in zip(work, fresh)], path.run(work)), reps)
            copy = timed(lambda: [w.copy_(f) for w, f in zip(work, fresh)], reps)
            row = dict(case="%dx%d %d-bit 4:2:0 CTB 64" % (W, H, bd), face_ms_1=round(one, 4), face_ms_16=round(sixteen, 4),
                       face_launches=1, per_call_ms=round(per_call - copy, 4), per_call_launches=path.launches,
                       mbytes=round(byte_model(pics[0]) / 1e6, 2), hbm_share_16=round(byte_model(pics[0]) / (sixteen * 1e-3) / HBM_PEAK, 3))
            rows.append(row)
            print(json.dumps(row), flush=True)
    print("| case | face 1/launch ms | face 16/launch ms/pic | per-call path ms (launches) | MB model | share of 8 TB/s at 16 |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %.3f | %.3f | %.3f (%d) | %.2f | %.2f |" % (r["case"], r["face_ms_1"], r["face_ms_16"], r["per_call_ms"],
                                                               r["per_call_launches"], r["mbytes"], r["hbm_share_16"]))


if __name__ == "__main__":
    main()
