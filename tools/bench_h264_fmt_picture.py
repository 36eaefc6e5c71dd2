#!/usr/bin/env python3
"""tools/bench_h264_fmt_picture.py — the _fmt faces of the H.264 whole-picture inter prediction and residual
(ffhip_h264_inter_pictures_fmt_dev, ffhip_h264_residual_pictures_fmt_dev) at 4:2:2 and 4:4:4 against what a caller had for these
formats before, on the same commit, and their own 4:2:0 path as a sanity line in the same process.

Content: the test generators' pictures (tests/h264_fmt_picture_gen.py; at 4:2:0 tests/h264_inter_picture_gen.py /
h264_res_picture_gen.py) at 1080p (120 x 68 macroblocks), 8 and 10 bits, mixed positions: P and B slices, every partition shape, 4
slices, 3 references, weights of every kind, 10 % intra macroblocks.  Before timing, the planes of the two paths are compared and
must be identical.  Then, in one process, alternating, after warm-up, medians of --reps (>= 20):
  inter     face_ms_1 / face_ms_16: the face with 1 and 16 pictures per launch, ms per picture (HIP events); record_ms: the host's
            wall clock to put the same prediction's records into the picture object made for the format (one thread, through ctypes);
            flush_ms: ffhip_h264_picture_flush of those records (HIP events).  At 4:2:0 old_ms_16 is ffhip_h264_inter_pictures_dev.
  residual  face_ms_1 / face_ms_16 as above; calls_ms: the per-call batch face on host-built lists, ffhip_h264_idct_mb_batch_dev_hbd
            with which 0 and 1 per plane and 4 (idct_add8_422) on an image whose chroma DCs are already transformed, so one launch
            fewer than a caller needs (HIP events; the coefficient images, which the batch face consumes, are rewritten outside the timed
            region).  At 4:2:0 old_ms_16 is ffhip_h264_residual_pictures_dev.
One JSON line per case, then a table."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import h264_fmt_picture_gen as F  # noqa: E402
import h264_inter_picture_gen as GI  # noqa: E402
import h264_res_picture_gen as GR  # noqa: E402
from ffmpeg_amd import _lib, h264  # noqa: E402

NPICS = 16
FMT = {1: "4:2:0", 2: "4:2:2", 3: "4:4:4"}


def events(fn, before=None):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if before:
        before()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def typed(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def med(v):
    return round(float(np.median(v)), 4)


def inter_case(mb_w, mb_h, bd, fmt, reps):
    L = _lib.lib()
    rng = np.random.default_rng(mb_w + bd + fmt)
    kw = dict(nslices=4, nrefs=3, p_intra=0.1, p_far=0.02)
    pic = GI.InterPicture(rng, mb_w, mb_h, bd, **kw) if fmt == 1 else F.InterPicture(rng, mb_w, mb_h, fmt, bd, **kw)
    cover = (GI.model(pic, oracle=False) if fmt == 1 else F.inter_model(pic, oracle=False))[2]
    strides = [r.strides[0] for r in pic.refs[0]]
    step = [r.nbytes for r in pic.refs[0]]
    refs = [dev(np.concatenate([r[p] for r in pic.refs])) for p in range(3)]
    ins = [dev(pic.mb), dev(pic.mvf), dev(pic.slices)]
    dsts = [[torch.full((step[p],), GI.POISON, dtype=torch.uint8, device="cuda") for p in range(3)] for _ in range(NPICS + 1)]
    arg = lambda d: dict(dst=d, dst_stride=strides, mb=ins[0], mvf=ins[1], slices=ins[2], mvf_stride=pic.w4, nslices=pic.nslices,
                         refs=[dict(base=[refs[p].data_ptr() + k * step[p] for p in range(3)], stride=strides) for k in range(pic.nrefs)])
    face_args = [arg(d) for d in dsts[:NPICS]]
    face = lambda n: h264.inter_pictures_fmt(face_args[:n], mb_w, mb_h, bd, fmt)
    old = lambda n: h264.inter_pictures(face_args[:n], mb_w, mb_h, bd, fmt)
    obj = h264.Picture(mb_w, mb_h, bit_depth=bd, chroma_format=fmt)
    records = GI.picture_records(pic, cover["calls"], strides, step) if fmt == 1 else F.picture_records(pic, cover["calls"], strides, step)
    fns = {"mc_luma": L.ffhip_h264_picture_mc_luma, "mc_luma_plane": L.ffhip_h264_picture_mc_luma_plane,
           "mc_chroma": L.ffhip_h264_picture_mc_chroma, "weight": L.ffhip_h264_picture_weight}
    recs = [(fns[name], lead, r.ctypes.data) for name, lead, r in records]

    def record():
        obj.begin()
        p = obj._p
        for fn, lead, at in recs:
            fn(p, *lead, at)

    flush = lambda: obj.flush(dsts[NPICS], strides, refs)
    record(); flush(); face(NPICS)
    torch.cuda.synchronize()
    for p in range(3):
        assert torch.equal(dsts[NPICS][p], dsts[0][p]) and torch.equal(dsts[NPICS][p], dsts[NPICS - 1][p]), (fmt, bd, p)
        assert (dsts[0][p] != GI.POISON).float().mean() > 0.85
    t = {k: [] for k in ("face1", "faceN", "oldN", "record", "flush")}
    for _ in range(2):
        record(); flush(); face(1); face(NPICS)
        if fmt == 1:
            old(NPICS)
    torch.cuda.synchronize()
    for _ in range(reps):
        t0 = time.perf_counter(); record(); t["record"].append((time.perf_counter() - t0) * 1e3)
        t["flush"].append(events(flush))
        t["face1"].append(events(lambda: face(1)))
        t["faceN"].append(events(lambda: face(NPICS)) / NPICS)
        if fmt == 1:
            t["oldN"].append(events(lambda: old(NPICS)) / NPICS)
    assert L.ffhip_stream_synchronize(None) == 0, L.ffhip_last_error()
    obj.close()
    return dict(face="inter", case="%dx%d %s %d bits" % (16 * mb_w, 16 * mb_h, FMT[fmt], bd), face_ms_1=med(t["face1"]), face_ms_16=med(t["faceN"]),
                old_ms_16=med(t["oldN"]) if fmt == 1 else None, record_ms=med(t["record"]), flush_ms=med(t["flush"]), calls=len(recs))


def res_case(mb_w, mb_h, bd, fmt, reps):
    L = _lib.lib()
    rng = np.random.default_rng(mb_w + bd + fmt + 7)
    pic = GR.ResPicture(rng, mb_w, mb_h, bd, p_intra=0.1) if fmt == 1 else F.ResPicture(rng, mb_w, mb_h, fmt, bd, p_intra=0.1)
    lists = []
    want = (GR.model(pic, lists=lists) if fmt == 1 else F.res_model(pic, lists=lists))[0]
    ps, cdt = (2 if bd > 8 else 1), GR.coef_dtype(bd)
    strides = [b.strides[0] for b in pic.before]
    d_mb, d_res, d_co = dev(pic.mb), dev(pic.res), dev(pic.coeffs)
    start = [dev(b) for b in pic.before]
    pics = [dict(dst=[s.clone() for s in start], dst_stride=strides, mb=d_mb, res=d_res, coeffs=d_co, ncoeffs=pic.ncoeffs) for _ in range(NPICS)]
    face = lambda n: h264.residual_pictures_fmt(pics[:n], mb_w, mb_h, bd, fmt)
    old = lambda n: h264.residual_pictures(pics[:n], mb_w, mb_h, bd, fmt)

    def reset():
        for p in pics:
            for a, b in zip(p["dst"], start):
                a.copy_(b)
    # ---- the per-call batch face on the model's lists (4:2:2 / 4:4:4) ----
    launches = []
    if fmt != 1:
        planes = [s.clone() for s in start]
        for pl in range(3 if fmt == 3 else 1):
            bo = np.zeros(48, np.int32)
            bo[:16] = [4 * F.Y4[i] * strides[pl] + 4 * F.X4[i] * ps for i in range(16)]
            for t8 in (0, 1):
                sel = [e for e in lists if e["t8"] == t8 and len(e["planes"]) > pl]
                if sel:
                    launches.append((t8, planes[pl], None, strides[pl],
                                     typed(np.array([(e["m"] // mb_w) * 16 * strides[pl] + (e["m"] % mb_w) * 16 * ps for e in sel], np.int32)), typed(bo),
                                     typed(np.array([e["planes"][pl][0] for e in sel], cdt)), typed(np.array([e["planes"][pl][1] for e in sel], np.uint8)), len(sel)))
        if fmt == 2:
            sel = [e for e in lists if "chroma" in e]
            bo = np.zeros(48, np.int32)
            for j in (1, 2):
                for k in range(4):
                    bo[16 * j + k] = (k >> 1) * 4 * strides[1] + (k & 1) * 4 * ps
                    bo[16 * j + 8 + k] = (2 + (k >> 1)) * 4 * strides[1] + (k & 1) * 4 * ps
            launches.append((4, planes[1], planes[2], strides[1],
                             typed(np.array([(e["m"] // mb_w) * 16 * strides[1] + (e["m"] % mb_w) * 8 * ps for e in sel], np.int32)), typed(bo),
                             typed(np.array([e["chroma"][0] for e in sel], cdt)), typed(np.array([e["chroma"][1] for e in sel], np.uint8)), len(sel)))
        images = [l[6].clone() for l in launches]

    def restore():
        for l, im in zip(launches, images):
            l[6].copy_(im)
        for a, b in zip(planes, start):
            a.copy_(b)

    def calls():
        for which, d0, d1, s, off, bo, blocks, nnzc, n in launches:
            _lib.check(L.ffhip_h264_idct_mb_batch_dev_hbd(bd, which, d0.data_ptr(), d1.data_ptr() if d1 is not None else None, s, off.data_ptr(),
                                                          bo.data_ptr(), blocks.data_ptr(), nnzc.data_ptr(), n, None), "idct_mb")
    face(NPICS)
    torch.cuda.synchronize()
    for p, w in enumerate(want):
        exp = dev(w)
        assert torch.equal(pics[0]["dst"][p], exp) and torch.equal(pics[NPICS - 1]["dst"][p], exp), (fmt, bd, p)
    if fmt != 1:
        calls()
        assert L.ffhip_stream_synchronize(None) == 0
        torch.cuda.synchronize()
        for p, w in enumerate(want):
            assert torch.equal(planes[p], dev(w)), (fmt, bd, p)
    t = {k: [] for k in ("face1", "faceN", "oldN", "calls")}
    for _ in range(2):
        face(1); face(NPICS)
    torch.cuda.synchronize()
    for _ in range(reps):
        t["face1"].append(events(lambda: face(1), reset))
        t["faceN"].append(events(lambda: face(NPICS), reset) / NPICS)
        if fmt == 1:
            t["oldN"].append(events(lambda: old(NPICS), reset) / NPICS)
        else:
            t["calls"].append(events(lambda: (calls(), L.ffhip_stream_synchronize(None)), restore))
    return dict(face="residual", case="%dx%d %s %d bits" % (16 * mb_w, 16 * mb_h, FMT[fmt], bd), face_ms_1=med(t["face1"]), face_ms_16=med(t["faceN"]),
                old_ms_16=med(t["oldN"]) if fmt == 1 else None, calls_ms=med(t["calls"]) if fmt != 1 else None, launches=len(launches))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--size", default="120x68")
    ap.add_argument("--depths", default="8,10")
    ap.add_argument("--formats", default="1,2,3")
    ap.add_argument("--faces", default="inter,residual")
    args = ap.parse_args()
    reps = max(20, args.reps)
    mb_w, mb_h = map(int, args.size.split("x"))
    rows = []
    for which in args.faces.split(","):
        for bd in map(int, args.depths.split(",")):
            for fmt in map(int, args.formats.split(",")):
                rows.append((inter_case if which == "inter" else res_case)(mb_w, mb_h, bd, fmt, reps))
                print(json.dumps(rows[-1]), flush=True)
    f = lambda v: "-" if v is None else "%.4f" % v
    print("| face | case | face 1/launch ms | face 16/launch ms/pic | existing 4:2:0 face ms/pic | record ms | flush ms | per-call launches ms |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %s | %s | %s | %s | %s | %s | %s |" % (r["face"], r["case"], f(r["face_ms_1"]), f(r["face_ms_16"]), f(r.get("old_ms_16")),
                                                          f(r.get("record_ms")), f(r.get("flush_ms")), f(r.get("calls_ms"))))


if __name__ == "__main__":
    main()
