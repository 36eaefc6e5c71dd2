"""GPU parity of the exact-2x kernel's edge layout (sws_up2.hip; the geometry itself: tests/test_up2_plan.py) vs the oracle, byte for byte.
Rows of ngroups % 64 = 0, 32 or 16 put their two ends, cut off at 32, 16 or 8 groups, side by side with the ends of other frames in one wave
of 1, 2 or 4 frames; the smallest widths that reach each cut, with and without whole blocks between the ends, and two widths that keep the
shared ragged end; batches that end inside an edge wave; several strips; both depths of the row buffer; every instantiation of the kernel.
FFHIP_UP2_EDGE=0 (measure build) is the ragged-end layout on the same pictures: both must equal the oracle, hence each other."""
import ctypes as C

import numpy as np
import pytest

import ffi
from ffi import PIX
from test_gpu_sws_fast import _run
from test_gpu_sws_hbd import _run as _run_hbd

pytestmark = pytest.mark.gpu

# luma width -> (groups per row of the luma plane and of an interleaved chroma pair, edge lanes per frame)
WIDTHS = {64: (16, 16), 128: (32, 32), 256: (64, 64), 320: (80, 16), 384: (96, 32), 512: (128, 64), 448: (112, 0), 136: (34, 0)}
BATCHES = (1, 2, 3, 5)
BASE = {"yuvj420p": "yuv420p"}


def _edge_envs(eligible):
    return [{}, {"FFHIP_UP2_EDGE": "0"}] if eligible else [{}]


def _go(case, env, monkeypatch, n, seed):
    monkeypatch.delenv("FFHIP_UP2_EDGE", raising=False)
    _run(*case, env=env, monkeypatch=monkeypatch, n=n, seed=seed, need="up2")


@pytest.mark.parametrize("w", sorted(WIDTHS))
def test_edges_product_library(w, monkeypatch):
    """no knob: the library FFmpeg links"""
    for h in (22, 40):
        for n in BATCHES:
            _go(("nv12", w, h, "nv12", 2 * w, 2 * h, ffi.SWS_BICUBIC), {}, monkeypatch, n, w + n)


@pytest.mark.parametrize("depth", ["3", "6"])
@pytest.mark.parametrize("strip", ["6", "12"])
@pytest.mark.parametrize("h", [22, 40])
@pytest.mark.parametrize("w", sorted(WIDTHS))
def test_edges_strips_depths_batches(w, h, strip, depth, monkeypatch):
    for n in BATCHES:
        for e in _edge_envs(WIDTHS[w][1]):
            _go(("nv12", w, h, "nv12", 2 * w, 2 * h, ffi.SWS_BICUBIC), dict(e, FFHIP_UP2_STRIP=strip, FFHIP_UP2_DEPTH=depth), monkeypatch, n, w + h + n)


FORMATS = [
    ("nv21", 320, "nv12", ffi.SWS_BICUBIC),        # the channels swap
    ("nv21", 128, "nv12", ffi.SWS_BICUBIC),
    ("yuv420p", 384, "yuv420p", ffi.SWS_BICUBIC),  # luma 96 groups: edge waves of 2 frames; chroma 48: the ragged end, in one launch
    ("yuv420p", 256, "yuv420p", ffi.SWS_BICUBIC),  # luma 64 groups, chroma 32: 1 and 2 frames per edge wave in one launch
    ("yuv420p", 128, "yuv420p", ffi.SWS_BICUBIC),  # 2 and 4 frames per edge wave
    ("nv12", 384, "nv12", ffi.SWS_BILINEAR),
    ("nv12", 320, "nv12", ffi.SWS_POINT),
    ("nv12", 512, "nv12", ffi.SWS_BILINEAR),
]


@pytest.mark.parametrize("sf,w,df,flags", FORMATS, ids=lambda v: str(v))
def test_edges_formats(sf, w, df, flags, monkeypatch):
    for h, strip in ((22, "6"), (40, "12")):
        for n in BATCHES:
            for e in _edge_envs(True):
                _go((sf, w, h, df, 2 * w, 2 * h, flags), dict(e, FFHIP_UP2_STRIP=strip), monkeypatch, n, w + n)
    _go((sf, w, 22, df, 2 * w, 44, flags), {}, monkeypatch, 3, w)   # the product library


HBD = [
    ("p010le", 64, "p010le"),            # 16 groups, luma and (u, v) pair: 4 frames per edge wave
    ("p010le", 384, "p010le"),           # 96 groups: 2 frames per edge wave and a whole block
    ("p010le", 512, "p010le"),
    ("yuv420p10le", 256, "yuv420p10le"),  # luma 64 groups, chroma 32
    ("yuv420p10le", 384, "yuv420p10le"),  # luma 96: edge layout; chroma 48: the ragged end
    ("yuv420p10le", 640, "yuv420p10le"),  # luma 160 groups (32 + 2 blocks), chroma 80 (16 + 1 block)
]


@pytest.mark.parametrize("edge", ["edge", "ragged"])
@pytest.mark.parametrize("sf,w,df", HBD, ids=lambda v: str(v))
def test_edges_above_8_bits(sf, w, df, edge, monkeypatch):
    """the 16-bit twins (k_sws_up2<., ., 1>): plane and pair"""
    if edge == "ragged":
        monkeypatch.setenv("FFHIP_UP2_EDGE", "0")
    for h, n in ((22, 1), (40, 2), (22, 3), (40, 5)):
        _run_hbd((sf, w, h, df, 2 * w, 2 * h, ffi.SWS_BICUBIC), nframes=n)


def _convert(sf, df, sw, sh, frames, monkeypatch, env):
    """frames: lists of planes of the source's base format -> the oracle's bytes, from the exact-2x kernel"""
    import torch
    from ffmpeg_amd import swscale as S
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    for k in ("FFHIP_UP2_EDGE", "FFHIP_UP2_STRIP", "FFHIP_UP2_DEPTH", "FFHIP_UP2_FSHIFT", "FFHIP_SWS_UP2"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    bs, bd = BASE.get(sf, sf), BASE.get(df, df)
    dw, dh = 2 * sw, 2 * sh
    flags = ffi.SWS_BICUBIC
    ht = S.HostTables(sw, sh, PIX[sf], dw, dh, PIX[df], flags)
    ranges = (int(sf in BASE), int(df in BASE))
    t = ffi.make_otables(sw, sh, PIX[bs], dw, dh, PIX[bd], flags, ht.banks(), ht.coeffs(), ranges=ranges)
    ctx = S.SwsContext(sw, sh, PIX[sf], dw, dh, PIX[df], flags)
    assert ctx.up2_path, "case does not reach the exact-2x kernel"
    n = len(frames)
    dsrc = [torch.from_numpy(np.stack([f[p] for f in frames])).to("cuda:0") for p in range(len(frames[0]))]
    shapes = [a.shape for a in ffi.alloc_frame(PIX[bd], dw, dh)]
    ddst = [torch.full((n,) + s, 0xA5, dtype=torch.uint8, device="cuda:0") for s in shapes]
    ctx.scale_batch(dsrc, ddst)
    torch.cuda.synchronize()
    for f in range(n):
        want = ffi.alloc_frame(PIX[bd], dw, dh)
        sp, ss = ffi.planes([np.ascontiguousarray(p) for p in frames[f]])
        dp, ds = ffi.planes(want)
        assert ffi.oracle().ffo_sws_scale_frame(C.byref(t), sp, ss, dp, ds) == dh
        for p, a in enumerate(want):
            got = ddst[p][f].cpu().numpy()
            assert np.array_equal(got, a), "frame %d plane %d: %d mismatches" % (f, p, (got != a).sum())
    ctx.close()


@pytest.mark.parametrize("w", [384, 256])
def test_edges_range_stage(w, monkeypatch):
    """yuvj420p -> yuv420p: the range stage between the passes (k_sws_up2<., ., 0, 1>), extreme samples at the row ends"""
    rng = np.random.default_rng(w)
    for h, n in ((22, 2), (40, 5)):
        frames = [ffi.alloc_frame(PIX["yuv420p"], w, h, rng) for _ in range(n)]
        for f in frames:
            for pl in f:
                pl[::5, :12] = 255
                pl[::5, -12:] = 255
                pl[3::7, :9] = 0
                pl[3::7, -9:] = 0
        for env in ({}, {"FFHIP_UP2_STRIP": "12"}, {"FFHIP_UP2_STRIP": "12", "FFHIP_UP2_EDGE": "0"}):
            _convert("yuvj420p", "yuv420p", w, h, frames, monkeypatch, env)


@pytest.mark.parametrize("w", [64, 320, 384, 512])
def test_edges_saturating_content(w, monkeypatch):
    """samples alternating 0 and 255 at both ends of every row (and runs of them between): the end columns' own coefficients and the int16
    saturation of the horizontal sums (min(., 32767) in hScale8To15_c) inside the edge waves"""
    rng = np.random.default_rng(w + 1)
    h = 22
    frames = []
    for f in range(3):
        y = np.where(rng.integers(0, 2, (h, w)) > 0, 255, 0).astype(np.uint8)
        uv = np.where(rng.integers(0, 2, (h // 2, w)) > 0, 255, 0).astype(np.uint8)
        for pl, step in ((y, 1), (uv, 2)):            # a chroma pair alternates per channel: every other (u, v) column
            alt = ((np.arange(24) // step + f) & 1) * 255
            pl[:, :24] = alt
            pl[:, -24:] = alt[::-1]
            pl[1::2, :24] = 255 - alt                 # ... and down the columns
            pl[1::2, -24:] = 255 - alt[::-1]
        frames.append([y, uv])
    for env in ({}, {"FFHIP_UP2_STRIP": "6"}, {"FFHIP_UP2_STRIP": "6", "FFHIP_UP2_EDGE": "0"}):
        _convert("nv12", "nv12", w, h, frames, monkeypatch, env)
