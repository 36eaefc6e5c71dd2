#!/usr/bin/env python3
"""tools/bench_h264_bs_fmt.py — H.264 edge parameters and frame-order deblocking of whole pictures at chroma_format_idc 0 .. 3
(ffhip_h264_edge_params_pictures_fmt_dev, ffhip_h264_deblock_pictures_fmt_dev).

16 pictures of 120 x 68 macroblocks (--mb, --pics) at 8 and 10 bits, two different pictures of the test generators alternating.  Per
format, each a median over --reps calls (HIP events around the call, one warm-up call before), repeated --runs times; the table
gives the median of the runs and their spread (min .. max):
  edge_ms     ffhip_h264_edge_params_pictures_fmt_dev, all pictures in one call;
  deblock_ms  ffhip_h264_deblock_pictures_fmt_dev on the tables of that call;
  chain_ms    inter_pictures_fmt -> residual_pictures_fmt -> edge_params_pictures_fmt -> deblock_pictures_fmt on one stream;
and at 4:2:2 / 4:4:4 what a caller did before these faces:
  host_ms     ffhip_h264_edge_params_pictures_fmt_host for all pictures on one CPU thread (wall clock);
  upload_ms   the copy of their tables from pinned host memory to the device;
  flush_ms    h264.Picture.flush() of the pictures one after another from deblock_mb() records alone (wall clock around the flushes and
              a device synchronise; the deblock_mb() calls themselves are not timed).
With --parent-lib PATH (a libffhip.so built from the parent commit) the format-1 edge-parameter launch and the format-1 deblock face
are timed against that library's ffhip_h264_edge_params_pictures_dev and frame faces (three calls: luma, Cb, Cr, the pictures as
frames at a constant pitch) in the same process, alternating new and parent inside every run.  Every timed call goes straight to the
library with record arrays built beforehand.  One JSON line per row, then a table."""
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
import h264_bs_fmt_gen as F  # noqa: E402
import h264_fmt_picture_gen as FP  # noqa: E402
import h264_inter_picture_gen as GI  # noqa: E402
import h264_res_picture_gen as GR  # noqa: E402
from ffmpeg_amd import _lib, h264  # noqa: E402

TABLES = ("luma", "cb", "cr")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def timed(fn, reps):
    """median ms of `reps` calls, HIP events around each"""
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


def wall(fn, reps):
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms))


def content(fmt, bd, mb_w, mb_h, seed):
    """one picture's host records for the four faces: the inter and residual generators' pictures on one macroblock array"""
    rng = np.random.default_rng(seed)
    sh = bd - 8
    shapes = [(16 * mb_h, 16 * mb_w)] + ([FP.chroma_shape(fmt, mb_w, mb_h)] * 2 if fmt else [])
    smooth = lambda s: (rng.integers(118, 138, s) << sh).astype(GI.sample_dtype(bd))
    refs = [[smooth(s) for s in shapes] + [None] * (3 - len(shapes)) for _ in range(3)]
    kw = dict(nslices=4, nrefs=3, p_intra=0.15, weights="none")
    if fmt >= 2:
        ip = FP.InterPicture(rng, mb_w, mb_h, fmt, bd, **kw)
        rp = FP.ResPicture(rng, mb_w, mb_h, fmt, bd, density=0.3, wild=0.0)
    else:
        ip = GI.InterPicture(rng, mb_w, mb_h, bd, chroma=fmt == 1, refs=refs, **kw)
        rp = GR.ResPicture(rng, mb_w, mb_h, bd, chroma=fmt == 1, density=0.3, wild=0.0)
    ip.refs = refs
    rp.mb["flags"] = (rp.mb["flags"] & 0xFE) | (ip.mb["flags"] & 1)
    rp.mb["slice"] = ip.mb["slice"]
    rp.mb["qp"] = rng.integers(28, 46, mb_w * mb_h) + 6 * sh
    rp.layout()
    bs = np.zeros(ip.nslices, h264.BS_SLICE_DTYPE)
    bs["ref"], bs["num_ref"], bs["flags"] = ip.slices["ref"], ip.slices["num_ref"], ip.is_b
    cqp = np.stack([F.G.chroma_qp_table(2, 6 * sh), F.G.chroma_qp_table(-3, 6 * sh)])
    return dict(ip=ip, rp=rp, mb=rp.mb, bs_slices=bs, chroma_qp=cqp, before=[smooth(s) for s in shapes], shapes=shapes)


class Case:
    """npics pictures of one format and depth on the device: the inputs of two generated pictures, shared; planes and tables per picture"""

    def __init__(self, fmt, bd, mb_w, mb_h, npics):
        self.fmt, self.bd, self.mb_w, self.mb_h, self.npics = fmt, bd, mb_w, mb_h, npics
        self.host = [content(fmt, bd, mb_w, mb_h, 100 * fmt + bd + k) for k in range(2)]
        n, per = mb_w * mb_h, F.PER[fmt]
        self.ins = []
        for c in self.host:
            ip, rp = c["ip"], c["rp"]
            self.ins.append(dict(mb=dev(c["mb"]), mvf=dev(ip.mvf), slices=dev(ip.slices), bs_slices=dev(c["bs_slices"]), chroma_qp=dev(c["chroma_qp"]),
                                 res=dev(rp.res), coeffs=dev(rp.coeffs), refs=[[dev(p) for p in r if p is not None] for r in ip.refs]))
        # plane p of every picture in one tensor at a constant pitch, and table t likewise: what the frame faces take as nframes frames
        before = self.host[0]["before"]
        self.plane_all = [torch.stack([dev(self.host[k % 2]["before"][p]) for k in range(npics)]) for p in range(len(before))]
        self.edge_all = [torch.zeros((npics, n * q * 12), dtype=torch.uint8, device="cuda") for q in (8, per, per)]
        self.planes = [[t[k] for t in self.plane_all] for k in range(npics)]
        self.edges = [[t[k] for t in self.edge_all] for k in range(npics)]
        self.strides = [b.strides[0] for b in self.host[0]["before"]] + [0] * (3 - len(self.host[0]["before"]))
        pad3 = lambda l: list(l) + [None] * (3 - len(l))
        self.inter_args, self.res_args, self.bs_args, self.lf_args = [], [], [], []
        for k in range(npics):
            i, c = self.ins[k % 2], self.host[k % 2]
            ip, dst = c["ip"], pad3(self.planes[k])
            self.inter_args.append(dict(dst=dst, dst_stride=self.strides, mb=i["mb"], mvf=i["mvf"], slices=i["slices"], mvf_stride=ip.w4,
                                        nslices=ip.nslices, refs=[dict(base=pad3(r), stride=self.strides) for r in i["refs"]]))
            self.res_args.append(dict(dst=dst, dst_stride=self.strides, mb=i["mb"], res=i["res"], coeffs=i["coeffs"], ncoeffs=c["rp"].ncoeffs))
            self.bs_args.append(dict(mb=i["mb"], mvf=i["mvf"], slices=i["bs_slices"], chroma_qp=i["chroma_qp"], luma=self.edges[k][0],
                                     cb=self.edges[k][1], cr=self.edges[k][2], mvf_stride=ip.w4, nslices=ip.nslices))
            self.lf_args.append(dict(planes=self.planes[k], edges=self.edges[k][:len(self.planes[k])]))
        # the record arrays once, outside the timed calls: the events time the library, not the marshalling
        ptr = lambda t: t.data_ptr()
        vp = lambda a: C.cast(a, C.c_void_p)
        self.keep = [h264.inter_pics(self.inter_args), h264.res_pics(self.res_args, ptr), h264._bs_pics(self.bs_args, ptr), h264.lf_pics(self.lf_args)]
        self.inter_arr, self.res_arr, self.bs_arr, self.lf_arr = (vp(a) for a in self.keep)
        self.L = _lib.lib()

    def edge(self):
        assert self.L.ffhip_h264_edge_params_pictures_fmt_dev(self.fmt, self.mb_w, self.mb_h, 0, 6 * (self.bd - 8), self.npics, self.bs_arr, None) == 0

    def deblock(self):
        assert self.L.ffhip_h264_deblock_pictures_fmt_dev(self.bd, self.fmt, self.mb_w, self.mb_h, self.strides[0], self.strides[1], self.npics,
                                                          self.lf_arr, None) == 0

    def chain(self):
        assert self.L.ffhip_h264_inter_pictures_fmt_dev(self.bd, self.fmt, self.mb_w, self.mb_h, self.npics, self.inter_arr, None) == 0
        assert self.L.ffhip_h264_residual_pictures_fmt_dev(self.bd, self.fmt, self.mb_w, self.mb_h, self.npics, self.res_arr, None) == 0
        self.edge()
        self.deblock()

    # ---- what a caller did before: tables on the host, an upload, the picture object's flush
    def host_tables(self):
        n, per = self.mb_w * self.mb_h, F.PER[self.fmt]
        maps = []
        for k in range(self.npics):
            c = self.host[k % 2]
            t = {name: np.zeros(n * q, h264.EDGE_DTYPE) for name, q in (("luma", 8), ("cb", per), ("cr", per))}
            maps.append(dict(mb=c["mb"], mvf=c["ip"].mvf, slices=c["bs_slices"], chroma_qp=c["chroma_qp"], mvf_stride=c["ip"].w4,
                             nslices=c["ip"].nslices, **t))
        return maps

    def host_path(self, reps):
        maps = self.host_tables()
        face = lambda: h264.edge_params_pictures_fmt_host(maps, self.mb_w, self.mb_h, 0, 6 * (self.bd - 8), self.fmt)
        host_ms = wall(face, max(3, reps // 4))
        pinned = [[torch.from_numpy(m[t].view(np.uint8)).pin_memory() for t in TABLES] for m in maps]
        upload_ms = timed(lambda: [e.copy_(p, non_blocking=True) for es, ps in zip(self.edges, pinned) for e, p in zip(es, ps)], reps)
        per = F.PER[self.fmt]
        objs = []
        for k, m in enumerate(maps):
            pic = h264.Picture(self.mb_w, self.mb_h, bit_depth=self.bd, chroma_format=self.fmt)
            objs.append(pic)

        def record():
            for pic, m in zip(objs, maps):
                pic.begin()
                for mb in range(self.mb_w * self.mb_h):
                    mx, my = mb % self.mb_w, mb // self.mb_w
                    pic.deblock_mb(0, mx, my, m["luma"][8 * mb:8 * mb + 8])
                    pic.deblock_mb(1, mx, my, m["cb"][per * mb:per * mb + per])
                    pic.deblock_mb(2, mx, my, m["cr"][per * mb:per * mb + per])

        ms = []
        for _ in range(max(3, reps // 4) + 1):
            record()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for pic, pl in zip(objs, self.planes):
                pic.flush(pl, self.strides, pl)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        for pic in objs:
            pic.close()
        return host_ms, upload_ms, float(np.median(ms[1:]))


class Parent:
    """the parent commit's library: its edge-parameter face and frame faces on a Case of format 1"""

    def __init__(self, path, case):
        self.L = C.CDLL(path)
        vp = C.c_void_p
        self.L.ffhip_h264_edge_params_pictures_dev.argtypes = [C.c_int] * 5 + [vp, vp]
        self.L.ffhip_h264_deblock_frames_dev_hbd.argtypes = [C.c_int, C.c_int, vp, C.c_size_t, C.c_int, C.c_ssize_t, C.c_int, C.c_int, vp, vp]
        self.c = case
        self.arr = h264._bs_pics(case.bs_args, lambda t: t.data_ptr())

    def edge(self):
        c = self.c
        assert self.L.ffhip_h264_edge_params_pictures_dev(c.mb_w, c.mb_h, 0, 6 * (c.bd - 8), c.npics, C.cast(self.arr, C.c_void_p), None) == 0

    def deblock(self):
        """the same pictures through the parent's frame faces: one call per plane kind, the pictures as frames at a constant pitch"""
        c = self.c
        for p, (pl, e) in enumerate(zip(c.plane_all, c.edge_all)):
            assert self.L.ffhip_h264_deblock_frames_dev_hbd(c.bd, int(p > 0), pl.data_ptr(), pl.stride(0), c.npics, c.strides[min(p, 1)], c.mb_w,
                                                            c.mb_h, e.data_ptr(), None) == 0


def spread(v):
    return dict(median=round(float(np.median(v)), 4), min=round(min(v), 4), max=round(max(v), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--mb", default="120x68")
    ap.add_argument("--pics", type=int, default=16)
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    mb_w, mb_h = (int(v) for v in args.mb.split("x"))
    rows = []
    for bd in (8, 10):
        for fmt in range(4):
            case = Case(fmt, bd, mb_w, mb_h, args.pics)
            parent = Parent(args.parent_lib, case) if args.parent_lib and fmt == 1 else None
            m = {k: [] for k in ("edge_ms", "deblock_ms", "chain_ms", "parent_edge_ms", "parent_deblock_ms")}
            for _ in range(args.runs):
                m["edge_ms"].append(timed(case.edge, args.reps))
                if parent:
                    m["parent_edge_ms"].append(timed(parent.edge, args.reps))
                m["deblock_ms"].append(timed(case.deblock, args.reps))
                if parent:
                    m["parent_deblock_ms"].append(timed(parent.deblock, args.reps))
                m["chain_ms"].append(timed(case.chain, args.reps))
            row = dict(bit_depth=bd, chroma_format_idc=fmt, pictures=args.pics, mb="%dx%d" % (mb_w, mb_h), reps=args.reps, runs=args.runs)
            row.update({k: spread(v) for k, v in m.items() if v})
            if fmt >= 2:
                host_ms, upload_ms, flush_ms = case.host_path(args.reps)
                row.update(host_ms=round(host_ms, 3), upload_ms=round(upload_ms, 4), flush_ms=round(flush_ms, 3))
            rows.append(row)
            print(json.dumps(row), flush=True)
            del case, parent
            torch.cuda.empty_cache()
    cell = lambda r, k: "%.3f (%.3f .. %.3f)" % (r[k]["median"], r[k]["min"], r[k]["max"]) if k in r else "-"
    num = lambda r, k: "%.3f" % r[k] if k in r else "-"
    print("| bits | format | edge ms | deblock ms | chain ms | parent edge ms | parent frame faces ms | _fmt_host ms | upload ms | object flush ms |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %d | %d | %s | %s | %s | %s | %s | %s | %s | %s |" % (
            r["bit_depth"], r["chroma_format_idc"], cell(r, "edge_ms"), cell(r, "deblock_ms"), cell(r, "chain_ms"), cell(r, "parent_edge_ms"),
            cell(r, "parent_deblock_ms"), num(r, "host_ms"), num(r, "upload_ms"), num(r, "flush_ms")))


if __name__ == "__main__":
    main()
