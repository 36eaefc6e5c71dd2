#!/usr/bin/env python3
"""tools/bench_h264_res_picture.py — H.264 residuals of whole pictures (ffhip_h264_residual_pictures_dev) against the path it
replaces on the same commit: the four per-call launches (ffhip_h264_idct_add_mb_batch_dev with which 0 and 1,
ffhip_h264_chroma_dc_dequant_idct_batch_dev, ffhip_h264_idct_add8_batch_dev; the _hbd twins at 10 bits) on lists a caller builds on
the host.

Inputs: seeded pictures at 1080p (120 x 68 macroblocks) and 2160p (240 x 135), 4:2:0, 8 and 10 bits, 10 % intra macroblocks, a quarter
of the others with the 8x8 transform, at three coded densities: "sparse P" (15 % of the macroblocks coded, 20 % of their blocks),
"typical" (60 %, 40 %) and "all coded".  A coded block has about half of its coefficients non-zero.  Before timing, the planes of
the two paths are compared on the same content and must be identical.  Then, in one process, alternating, after warm-up, medians of
--reps (>= 20):
  face_ms_1 / face_ms_16   the face with 1 and 16 pictures per launch (16 pictures with coefficients and planes of their own), ms per
                           picture (HIP events);
  chain_ms                 the four launches for one picture, HIP events; they clear what they consume, so the coefficient image is
                           restored by a device copy before every run, outside the timed window.  That copy leaves the chain's
                           coefficients in the last-level cache, so the face's coefficients are rewritten by a device copy before
                           its runs as well (16 pictures' worth do not fit there: face_ms_16 reads from HBM);
  lists_ms                 the host's wall clock (numpy, one thread) to build the chain's lists from what the face takes: the
                           mb_offset list per transform size, the 40- and 120-byte nnzc caches, the dense 256 / 768 coefficients per
                           macroblock, the chroma DC's block_offset and qmul lists.  Their upload is not timed.
Algorithmic bytes per picture, from the shapes: the coefficients of every coded block read once, its samples read and written once,
24 bytes of records per macroblock; hbm_share is those bytes over face_ms_16 as a share of the 8 TB/s HBM peak: a figure of the whole
call.  One JSON line per case, then a table."""
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
import h264_res_picture_gen as G  # noqa: E402
import test_gpu_h264_res_picture as T  # noqa: E402
from h264_intra_gen import SCAN8, scan8_chroma  # noqa: E402
from ffmpeg_amd import _lib, h264  # noqa: E402

HBM_PEAK = 8.0e12
NPICS = h264.RES_PICS_PER_LAUNCH
DENSITIES = {"sparse P": (0.15, 0.2), "typical": (0.6, 0.4), "all coded": (1.0, 1.0)}
POS = np.array([G.X4[i] + 4 * G.Y4[i] for i in range(16)])
CH = np.concatenate([256 + np.arange(64), 512 + np.arange(64)])      # the coefficients of the eight chroma blocks in sl->mb
SCAN8C = np.array([scan8_chroma(1 + c, j) for c in range(2) for j in range(4)])


def events(fn, before=None):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if before:
        before()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def content(rng, mb_w, mb_h, bd, p_mb, p_blk):
    """(mb, res, coeffs) as the face takes them, vectorised: the generator of the tests draws macroblock by macroblock"""
    n, cdt = mb_w * mb_h, G.coef_dtype(bd)
    intra, t8 = rng.random(n) < 0.1, rng.random(n) < 0.25
    coded = (rng.random(n) < p_mb) & ~intra
    blk = (rng.random((n, 16)) < p_blk) & coded[:, None]
    blk = np.where(t8[:, None], np.repeat(blk[:, ::4], 4, axis=1), blk)
    with_c = coded & (rng.random(n) < max(p_blk, 0.5))
    cblk = (rng.random((n, 8)) < p_blk) & with_c[:, None]
    cdc = (rng.random((n, 2)) < 0.7) & with_c[:, None]
    lim = 300 << (bd - 8)
    dense = rng.integers(-lim, lim + 1, (n, 768), dtype=np.int16 if bd == 8 else np.int32)
    dense[rng.random((n, 768)) < 0.5] = 0
    dense[:, :256] *= np.repeat(blk, 16, axis=1)
    chroma = dense[:, CH] * np.repeat(cblk, 16, axis=1)
    chroma[:, ::16] = np.where(np.repeat(cdc, 4, axis=1) | cblk, dense[:, CH[::16]], 0)
    dense[:, 256:] = 0
    dense[:, CH] = chroma
    mb, res = np.zeros(n, G.MB), np.zeros(n, G.RES)
    mb["flags"] = intra | (t8 << 1)
    mb["nnz"] = (blk.astype(np.int64) << POS).sum(1)
    mb["qp"] = 30 + 6 * (bd - 8)
    res["chroma"] = (cblk.astype(np.int64) << np.arange(8)).sum(1)
    res["chroma_dc"] = cdc[:, 0] | (cdc[:, 1] << 1)
    res["qmul"] = rng.integers(16, 1 << 10, (n, 2))
    need = np.where(with_c & ((res["chroma"] | res["chroma_dc"]) != 0), 768, np.where(mb["nnz"] != 0, 256, 0))
    res["coeff_offset"] = np.cumsum(need) - need
    coeffs = np.concatenate([dense[m, :need[m]] for m in np.nonzero(need)[0]] + [np.zeros(16, cdt)]).astype(cdt)
    nblk = int(blk[~t8].sum() + cblk.sum() + (np.repeat(cdc, 4, axis=1) & ~cblk).sum()) + 4 * int(blk[t8][:, ::4].sum())
    return mb, res, coeffs, int(need.sum()), nblk


def build_lists(mb_w, bd, mb, res, coeffs, strides):
    """the lists of the four per-call launches from the face's inputs: what tests/test_gpu_h264_res_picture.py's batch_lists() builds
    from the model, here in numpy over whole pictures"""
    ps = 2 if bd > 8 else 1
    n = len(mb)
    inter = (mb["flags"] & 1) == 0
    t8 = (mb["flags"] >> 1) & 1
    chroma = inter & ((res["chroma"] | res["chroma_dc"]) != 0)
    bits = (mb["nnz"][:, None].astype(np.int64) >> POS) & 1
    bits = np.where(t8[:, None] == 1, np.repeat(bits[:, ::4], 4, axis=1), bits).astype(bool)
    off = res["coeff_offset"].astype(np.int64)
    m = np.arange(n)
    bo = np.zeros(48, np.int32)
    for i in range(16):
        bo[i] = 4 * G.Y4[i] * strides[0] + 4 * G.X4[i] * ps
    for j in (1, 2):
        for k in range(4):
            bo[16 * j + k] = (k >> 1) * 4 * strides[1] + (k & 1) * 4 * ps
    out = dict(bo=bo)
    for which in (0, 1):
        sel = np.nonzero(inter & (t8 == which) & (mb["nnz"] != 0))[0]
        blocks = coeffs[off[sel][:, None] + np.arange(256)] * np.repeat(bits[sel], 16, axis=1)
        per = 64 if which else 16
        cnt = np.maximum((blocks.reshape(len(sel), 256 // per, per) != 0).sum(2), 1)
        nnzc = np.zeros((len(sel), 40), np.uint8)
        nnzc[:, SCAN8] = np.minimum(np.repeat(cnt, per // 16, axis=1), 64) * bits[sel]
        out["luma%d" % which] = dict(mb_off=((m[sel] // mb_w) * 16 * strides[0] + (m[sel] % mb_w) * 16 * ps).astype(np.int32),
                                     blocks=np.ascontiguousarray(blocks), nnzc=nnzc)
    sel = np.nonzero(chroma)[0]
    cb = ((res["chroma"][sel][:, None] >> np.arange(8)) & 1).astype(bool)
    cdc = ((res["chroma_dc"][sel][:, None] >> np.arange(2)) & 1).astype(bool)
    blocks = np.zeros((len(sel), 768), coeffs.dtype)
    raw = coeffs[off[sel][:, None] + CH]
    blocks[:, CH] = raw * np.repeat(cb, 16, axis=1)
    blocks[:, CH[::16]] = np.where(cb | np.repeat(cdc, 4, axis=1), raw[:, ::16], 0)
    nnzc = np.zeros((len(sel), 120), np.uint8)
    ac = raw.reshape(len(sel), 8, 16)[:, :, 1:]
    nnzc[:, SCAN8C] = np.maximum((ac != 0).sum(2), 1) * cb
    k, c = np.nonzero(cdc)
    out["chroma"] = dict(mb_off=((m[sel] // mb_w) * 8 * strides[1] + (m[sel] % mb_w) * 8 * ps).astype(np.int32), blocks=blocks, nnzc=nnzc,
                         dc_off=(k * 768 + 256 * (1 + c)).astype(np.int32), dc_qmul=res["qmul"][sel][k, c].astype(np.int32))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="120x68,240x135")
    ap.add_argument("--depths", default="8,10")
    args = ap.parse_args()
    reps = max(20, args.reps)
    L = _lib.lib()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    rows = []
    for size in args.sizes.split(","):
        mb_w, mb_h = map(int, size.split("x"))
        for bd in map(int, args.depths.split(",")):
            ps = 2 if bd > 8 else 1
            for name, (p_mb, p_blk) in DENSITIES.items():
                rng = np.random.default_rng(mb_w + bd + len(name))
                mb, res, coeffs, ncoeffs, nblk = content(rng, mb_w, mb_h, bd, p_mb, p_blk)
                shapes = ((16 * mb_h, 16 * mb_w), (8 * mb_h, 8 * mb_w), (8 * mb_h, 8 * mb_w))
                strides = [w * ps for _, w in shapes]
                start = [(rng.integers(100, 156, s) << (bd - 8)).astype(G.sample_dtype(bd)) for s in shapes]
                d_mb, d_res = dev(mb), dev(res)
                pics = [dict(dst=[dev(p) for p in start], dst_stride=strides, mb=d_mb, res=d_res, coeffs=dev(coeffs), ncoeffs=ncoeffs)
                        for _ in range(NPICS)]
                lists = build_lists(mb_w, bd, mb, res, coeffs, strides)
                d = T.to_device(torch, lists)
                image = {k: d[k]["blocks"].clone() for k in ("luma0", "luma1", "chroma")}
                chain_planes = [dev(p) for p in start]

                def restore():
                    for k, t in image.items():
                        d[k]["blocks"].copy_(t)

                coeff_image = dev(coeffs)

                def rewrite(n):                                   # the face's coefficients as freshly written as the chain's
                    for k in range(n):
                        pics[k]["coeffs"].copy_(coeff_image)

                face = lambda n: h264.residual_pictures(pics[:n], mb_w, mb_h, bd, 1)
                chain = lambda: T.launch_batch_chain(torch, bd, chain_planes, strides, d)
                # ---- the two paths give identical planes ----
                face(NPICS)
                chain()
                torch.cuda.synchronize()
                for p in range(3):
                    assert torch.equal(chain_planes[p], pics[0]["dst"][p]) and torch.equal(chain_planes[p], pics[NPICS - 1]["dst"][p]), (size, bd, name, p)
                assert not torch.equal(chain_planes[0], dev(start[0]))
                # ---- timing ----
                t = {k: [] for k in ("face1", "faceN", "chain", "lists")}
                for _ in range(2):
                    face(1); face(NPICS); restore(); chain()
                torch.cuda.synchronize()
                for i in range(reps):
                    t["chain"].append(events(chain, restore))
                    t["face1"].append(events(lambda: face(1), lambda: rewrite(1)))
                    t["faceN"].append(events(lambda: face(NPICS), lambda: rewrite(NPICS)) / NPICS)
                    if i < 5:
                        t0 = time.perf_counter(); build_lists(mb_w, bd, mb, res, coeffs, strides); t["lists"].append((time.perf_counter() - t0) * 1e3)
                assert L.ffhip_stream_synchronize(None) == 0, L.ffhip_last_error()
                med = {k: float(np.median(v)) for k, v in t.items()}
                cs = 2 * ps
                nbytes = nblk * (16 * cs + 2 * 16 * ps) + 24 * mb_w * mb_h
                row = dict(case="%dx%d %d-bit %s" % (16 * mb_w, 16 * mb_h, bd, name), face_ms_1=round(med["face1"], 4),
                           face_ms_16=round(med["faceN"], 4), chain_ms=round(med["chain"], 4), lists_ms=round(med["lists"], 2),
                           blocks=nblk, coeff_mbytes=round(ncoeffs * cs / 1e6, 2), dense_mbytes=round(mb_w * mb_h * 768 * cs / 1e6, 2),
                           mbytes=round(nbytes / 1e6, 2), hbm_share=round(nbytes / (med["faceN"] * 1e-3) / HBM_PEAK, 4))
                rows.append(row)
                print(json.dumps(row), flush=True)
                del pics, d, image, chain_planes
                torch.cuda.empty_cache()
    print("| case | face 1/launch ms | face 16/launch ms/pic | chain (4 launches) ms | host list-building ms | 4x4 blocks | coeffs MB (dense MB) | "
          "algorithmic MB | share of HBM peak (whole call) |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %.4f | %.4f | %.4f | %.2f | %d | %.2f (%.2f) | %.2f | %.4f |" % (
            r["case"], r["face_ms_1"], r["face_ms_16"], r["chain_ms"], r["lists_ms"], r["blocks"], r["coeff_mbytes"], r["dense_mbytes"], r["mbytes"],
            r["hbm_share"]))


if __name__ == "__main__":
    main()
