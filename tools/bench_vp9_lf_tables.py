#!/usr/bin/env python3
"""tools/bench_vp9_lf_tables.py — VP9 loop-filter tables of whole frames (ffhip_vp9_lf_tables_pictures_dev) against the path it
replaces, on a 4K 4:2:0 picture: 60 x 34 superblocks (480 x 272 8x8 blocks) with the test generator's mixed partition
(tests/vp9_lf_tab_gen.py), 1 and 8 pictures.
Runs, after warm-up, median of --reps (>= 20), ms for all pictures of the row:
  dev_ms        the device path: the copy of the records and sb_first from pinned host memory + the launch (HIP events);
  launch_ms     the launch alone, records resident;
  sb_tables_ms  the path at the parent commit, host part: ffhip_vp9_lf_sb_tables() per superblock from the decoder's VP9Filter, one CPU
                thread, called through ctypes (wall clock; the call overhead of the binding is in it);
  host_face_ms  for scale, one C call: ffhip_vp9_lf_tables_pictures_host(), which builds the VP9Filter from the records as well;
  upload_ms     the copy of the finished tables from pinned host memory to the device (HIP events);
  replaced_ms   sb_tables_ms + upload_ms.
One JSON line per row, then a table."""
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
import vp9_lf_tab_gen as G  # noqa: E402
from ffmpeg_amd import _lib, vp9  # noqa: E402

COLS, ROWS, SS = 480, 272, (1, 1)


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


def wall(fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    reps = max(20, args.reps)
    L = _lib.lib()
    pics = [G.TabPicture.random(4000 + k, COLS, ROWS, SS) for k in range(8)]
    nsb = pics[0].nsb
    ms = [p.maps() for p in pics]
    vp9.lf_tables_pictures_host(ms, COLS, ROWS, SS)          # the VP9Filter a decoder would hold, and the tables to upload
    rows = []
    for n in (1, 8):
        pinned = [{k: torch.from_numpy(m[k].copy()).pin_memory() for k in G.INPUTS + ("tables",)} for m in ms[:n]]
        ds = []
        for m, p in zip(ms[:n], pinned):
            d = dict(m)
            d.update(blocks=torch.empty_like(p["blocks"], device="cuda"), sb_first=torch.empty_like(p["sb_first"], device="cuda"),
                     tables=torch.empty(nsb * 1280, dtype=torch.uint8, device="cuda"), filters=None)
            ds.append(d)

        def dev(copy=True):
            if copy:
                for d, p in zip(ds, pinned):
                    d["blocks"].copy_(p["blocks"], non_blocking=True)
                    d["sb_first"].copy_(p["sb_first"], non_blocking=True)
            vp9.lf_tables_pictures(ds, COLS, ROWS, SS)
        dev_ms, launch_ms = timed(dev, reps), timed(lambda: dev(False), reps)
        for d, m in zip(ds, ms):
            assert np.array_equal(d["tables"].cpu().numpy(), m["tables"])
        out = np.zeros((nsb, 320), np.uint32)

        def parent():
            for m, p in zip(ms[:n], pics):
                f, lim, mblim = m["filters"].ctypes.data, p.lim.ctypes.data, p.mblim.ctypes.data
                for i in range(nsb):
                    L.ffhip_vp9_lf_sb_tables(out[i].ctypes.data, f + 192 * i, 8 * (i // p.sb_cols), 8 * (i % p.sb_cols), 1, 1, lim, mblim)
        sb_ms = wall(parent, reps)
        assert np.array_equal(out.view(np.uint8).reshape(-1), ms[n - 1]["tables"])
        host_ms = wall(lambda: vp9.lf_tables_pictures_host(ms[:n], COLS, ROWS, SS), reps)
        upload = timed(lambda: [d["tables"].copy_(p["tables"], non_blocking=True) for d, p in zip(ds, pinned)], reps)
        row = dict(case="%dx%d sb, %d pictures" % (pics[0].sb_cols, pics[0].sb_rows, n), dev_ms=round(dev_ms, 4), launch_ms=round(launch_ms, 4),
                   sb_tables_ms=round(sb_ms, 3), host_face_ms=round(host_ms, 3), upload_ms=round(upload, 4), replaced_ms=round(sb_ms + upload, 3),
                   record_kbytes=round(sum(p["blocks"].numel() + p["sb_first"].numel() for p in pinned) / 1e3, 1),
                   table_mbytes=round(n * nsb * 1280 / 1e6, 2))
        rows.append(row)
        print(json.dumps(row), flush=True)
    print("| case | records + launch ms | launch ms | sb_tables per superblock ms | host face ms | upload of tables ms | replaced ms | records KB | tables MB |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %.4f | %.4f | %.3f | %.3f | %.4f | %.3f | %.1f | %.2f |" % (r["case"], r["dev_ms"], r["launch_ms"], r["sb_tables_ms"],
                                                                              r["host_face_ms"], r["upload_ms"], r["replaced_ms"],
                                                                              r["record_kbytes"], r["table_mbytes"]))


if __name__ == "__main__":
    main()
