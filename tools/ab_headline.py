"""A/B of two builds of libffhip.so on the headline conversion (nv12 1080p -> 4K bicubic, 256 frames) and a few neighbours.

  python tools/ab_headline.py tools/ab/libffhip_old.so ffmpeg_amd/libffhip.so
      alternating in subprocesses of one run: every subprocess allocates its own frame batches, so the placement of the buffers (which
      moves these kernels by several per cent) differs from line to line
  python tools/ab_headline.py --same-buffers [--passes N] tools/ab/libffhip_old.so ffmpeg_amd/libffhip.so
      both libraries loaded into ONE process and alternated on the same frame batches: what is left between the lines is the code"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = (("nv12 1080p->4K", 23, 1920, 1080, 23, 3840, 2160, 256), ("yuv420p 1080p->4K", 0, 1920, 1080, 0, 3840, 2160, 128),
         ("nv12 4K->1080p", 23, 3840, 2160, 23, 1920, 1080, 64))
if len(sys.argv) > 2 and sys.argv[1] not in ("--child", "--same-buffers"):
    for p in range(3):
        for so in sys.argv[1:]:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", os.path.abspath(so)], capture_output=True, text=True)
            print(out.stdout.strip() or out.stderr[-400:], flush=True)
    sys.exit(0)
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from ffmpeg_amd import _lib  # noqa: E402

dev = torch.device("cuda:0")


def timed(c, src, dst, warm=20, k=60):
    for _ in range(warm):
        c.scale_batch(src, dst)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(k):
        c.scale_batch(src, dst)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / k


if sys.argv[1] == "--same-buffers":
    args = sys.argv[2:]
    passes = 5
    if args[0] == "--passes":
        passes, args = int(args[1]), args[2:]
    # the two builds take the places of the product and the measure library of the binding: select() switches between them call by call
    _lib.SO, _lib.SO_MEASURE = os.path.abspath(args[0]), os.path.abspath(args[1])
    from ffmpeg_amd import swscale as S  # noqa: E402
    which = ("product", "measure")
    for name, sf, sw, sh, df, dw, dh, n in CASES:
        src = [torch.randint(0, 256, (n, r, c), dtype=torch.uint8, device=dev) for r, c in S.plane_shapes(sf, sw, sh)]
        dst = [torch.zeros((n, r, c), dtype=torch.uint8, device=dev) for r, c in S.plane_shapes(df, dw, dh)]
        ctx = []
        for w in which:
            _lib.select(w)
            ctx.append(S.SwsContext(sw, sh, sf, dw, dh, df, 4))
        ms = ([], [])
        for p in range(passes):
            for i, w in enumerate(which):
                _lib.select(w)
                ms[i].append(round(timed(ctx[i], src, dst), 4))
        for i, w in enumerate(which):
            _lib.select(w)
            ctx[i].close()
            print(json.dumps({"case": name, "so": os.path.basename(args[i]), "ms": ms[i], "min": min(ms[i]), "median": sorted(ms[i])[len(ms[i]) // 2],
                              "max": max(ms[i])}), flush=True)
        del src, dst
    sys.exit(0)

_lib.SO = sys.argv[2]
from ffmpeg_amd import swscale as S  # noqa: E402

res = {"so": os.path.basename(sys.argv[2])}
for name, sf, sw, sh, df, dw, dh, n in CASES:
    src = [torch.randint(0, 256, (n, r, c), dtype=torch.uint8, device=dev) for r, c in S.plane_shapes(sf, sw, sh)]
    dst = [torch.zeros((n, r, c), dtype=torch.uint8, device=dev) for r, c in S.plane_shapes(df, dw, dh)]
    byt = n * (S.frame_bytes(sf, sw, sh) + S.frame_bytes(df, dw, dh))
    c = S.SwsContext(sw, sh, sf, dw, dh, df, 4)
    ms = timed(c, src, dst)
    res[name] = [round(ms, 4), round(byt / ms / 1e6 / 8000, 4)]
    c.close()
    del src, dst
print(json.dumps(res))
