#!/usr/bin/env python3
"""tools/bench_h264_inter_picture.py — H.264 inter prediction of whole pictures (ffhip_h264_inter_pictures_dev) against the path it
replaces on the same commit: the same prediction recorded call by call into the picture object (h264.Picture) and flushed.

Inputs: the test generator's pictures (tests/h264_inter_picture_gen.py: every partition shape, 4 slices, 3 references, 10 % intra
macroblocks, vectors within +-10 samples and 2 % far outside) at 1080p (120 x 68 macroblocks) and 2160p (240 x 135), 8 bits 4:2:0, three
contents: P (one list, mixed fractions, no weights), B with about 60 % bi-prediction and implicit weights, B with explicit weights.
Before timing, the planes of the two paths are compared and must be identical.  Then, in one process, alternating, after warm-up,
medians of --reps (>= 20):
  face_ms_1 / face_ms_16   the face with 1 and 16 pictures per launch, ms per picture (HIP events);
  record_ms                the host's wall clock to put one picture's records into the picture object, one thread; the calls are made
                           from Python through ctypes, so null_ms, the same number of calls of a library function that does nothing,
                           is measured beside it and record_ms - null_ms is what the object's members cost;
  flush_ms                 ffhip_h264_picture_flush of those records (their upload, put, put into the scratch plane, avg, weight /
                           biweight), HIP events.
Algorithmic bytes per picture, from the shapes: every predicted sample written once, plus per motion call the reference window it
reads ((w + 5) x (h + 5) luma where the axis is fractional, (w + 1) x (h + 1) chroma); hbm_share is those bytes over face_ms_16 as a
share of the 8 TB/s HBM peak: a figure of the whole call, not of a kernel phase.  One JSON line per case, then a table."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import h264_inter_picture_gen as G  # noqa: E402
from ffmpeg_amd import _lib, h264  # noqa: E402

HBM_PEAK = 8.0e12
NPICS = h264.INTER_PICS_PER_LAUNCH
CONTENTS = {"P uni": dict(types="P", weights="none"), "B implicit": dict(types="B", weights="implicit", p_bi=0.6),
            "B explicit": dict(types="B", weights="explicit")}


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def packed(records):
    """the records as (ctypes function, leading arguments, address) triples: the loop below is then as thin as Python allows"""
    L = _lib.lib()
    fns = {"mc_luma": L.ffhip_h264_picture_mc_luma, "mc_chroma": L.ffhip_h264_picture_mc_chroma, "weight": L.ffhip_h264_picture_weight}
    keep = [r for _, _, r in records]
    return [(fns[name], lead, r.ctypes.data) for name, lead, r in records], keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="120x68,240x135")
    args = ap.parse_args()
    reps = max(20, args.reps)
    L = _lib.lib()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    rows = []
    for size in args.sizes.split(","):
        mb_w, mb_h = map(int, size.split("x"))
        for name, kw in CONTENTS.items():
            rng = np.random.default_rng(mb_w + len(name))
            pic = G.InterPicture(rng, mb_w, mb_h, 8, nslices=4, nrefs=3, p_intra=0.1, p_far=0.02, **kw)
            _, plans, cover = G.model(pic, oracle=False)
            calls = cover["calls"]
            strides = [16 * mb_w, 8 * mb_w, 8 * mb_w]
            step = [16 * mb_h * strides[0], 8 * mb_h * strides[1], 8 * mb_h * strides[2]]
            refs = [dev(np.concatenate([r[p] for r in pic.refs])) for p in range(3)]
            ins = [dev(pic.mb), dev(pic.mvf), dev(pic.slices)]
            dsts = [[torch.full((step[p],), G.POISON, dtype=torch.uint8, device="cuda") for p in range(3)] for _ in range(NPICS + 1)]
            arg = lambda d: dict(dst=d, dst_stride=strides, mb=ins[0], mvf=ins[1], slices=ins[2], mvf_stride=pic.w4, nslices=pic.nslices,
                                 refs=[dict(base=[refs[p].data_ptr() + k * step[p] for p in range(3)], stride=strides) for k in range(pic.nrefs)])
            face_args = [arg(d) for d in dsts[:NPICS]]
            obj = h264.Picture(mb_w, mb_h)
            recs, keep = packed(G.picture_records(pic, calls, strides, step))

            def record():
                obj.begin()
                p = obj._p
                for fn, lead, at in recs:
                    fn(p, *lead, at)

            def null():
                f = L.ffhip_h264_inter_plan_record_size
                for _ in recs:
                    f()

            flush = lambda: obj.flush(dsts[NPICS], strides, refs)
            face = lambda n: h264.inter_pictures(face_args[:n], mb_w, mb_h, 8, 1)
            # ---- the two paths give identical planes ----
            record()
            flush()
            face(NPICS)
            torch.cuda.synchronize()
            for p in range(3):
                assert torch.equal(dsts[NPICS][p], dsts[0][p]) and torch.equal(dsts[NPICS][p], dsts[NPICS - 1][p]), (size, name, p)
                assert (dsts[0][p] != G.POISON).float().mean() > 0.85
            # ---- timing ----
            t = {k: [] for k in ("face1", "faceN", "record", "null", "flush")}
            for _ in range(2):
                record(); flush(); face(1); face(NPICS)
            torch.cuda.synchronize()
            for _ in range(reps):
                t0 = time.perf_counter(); record(); t["record"].append((time.perf_counter() - t0) * 1e3)
                t["flush"].append(events(flush))
                t["face1"].append(events(lambda: face(1)))
                t["faceN"].append(events(lambda: face(NPICS)) / NPICS)
                t0 = time.perf_counter(); null(); t["null"].append((time.perf_counter() - t0) * 1e3)
            assert L.ffhip_stream_synchronize(None) == 0, L.ffhip_last_error()
            obj.close()
            med = {k: float(np.median(v)) for k, v in t.items()}
            nbytes = 0
            for c in calls:
                if c[0] == "mc":
                    _, pl, _, _, _, w, h, fx, fy = c[:9]
                    nbytes += (w + (5 if fx else 0)) * (h + (5 if fy else 0)) if pl == 0 else (w + (fx > 0)) * (h + (fy > 0))
            nbytes += int((plans["mode"] != 0).sum()) * 24             # 16 luma and 2 x 4 chroma samples written per block
            row = dict(case="%dx%d %s" % (16 * mb_w, 16 * mb_h, name), face_ms_1=round(med["face1"], 4), face_ms_16=round(med["faceN"], 4),
                       record_ms=round(med["record"], 2), null_ms=round(med["null"], 2), flush_ms=round(med["flush"], 4), calls=len(calls),
                       bi_share=round(float((plans["mode"] >= 3).sum() / max(1, (plans["mode"] != 0).sum())), 2),
                       mbytes=round(nbytes / 1e6, 2), hbm_share=round(nbytes / (med["faceN"] * 1e-3) / HBM_PEAK, 4))
            rows.append(row)
            print(json.dumps(row), flush=True)
    print("| case | face 1/launch ms | face 16/launch ms/pic | record ms (of which ctypes) | flush ms | calls | bi share | MB | share of HBM peak (whole call) |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %.4f | %.4f | %.2f (%.2f) | %.4f | %d | %.2f | %.2f | %.4f |" % (
            r["case"], r["face_ms_1"], r["face_ms_16"], r["record_ms"], r["null_ms"], r["flush_ms"], r["calls"], r["bi_share"], r["mbytes"],
            r["hbm_share"]))


if __name__ == "__main__":
    main()
