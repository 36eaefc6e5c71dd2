"""GPU: the batch kernels that renumber their workgroups (sws_block_numbering, sws_kernels.h) run every workgroup of every launch.

A workgroup the numbering skips writes nothing, so every case fills its destination with a sentinel before EVERY call (a buffer that
still holds the previous call's right bytes would hide it), pads the pitch past the row, converts distinct frames and compares each
frame with the oracle.  The launch counts are the point: ragged grids (gridDim.x % 8 != 0), grids below 8, the tails of the chunked
numberings and batches that end inside a pack of frames.  tests/test_sws_numbering_cpu.py pins the numbering itself."""
import numpy as np
import pytest

import ffi
from ffi import PIX

import test_gpu_sws as T
import test_gpu_sws_fast as F
import test_gpu_sws_hbd as H

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
COUNTS = list(range(1, 10)) + [17]


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _table_grid(w, h, n):
    """gridDim.x of k_yuv420p_rgb24_t (ffhip_launch_yuv420p_rgb24, rows not flattened): 4 waves per workgroup, one wave per 64
    16-pixel chunks of a row pair"""
    chunks = ((w & ~1) + 15) // 16
    return ((chunks + 63) // 64 * (h // 2) * n + 3) // 4


def _stale(got, bw):
    """(frame, first row, last row) of every run of rows left wholly at the sentinel"""
    runs = []
    for f, r in (got[:, :, :bw] == SENTINEL).all(dim=2).nonzero().tolist():
        if runs and runs[-1][0] == f and runs[-1][2] == r - 1:
            runs[-1][2] = r
        else:
            runs.append([f, r, r])
    return [tuple(x) for x in runs]


def _table_case(w, h, n, dst, seed):
    """a context, n distinct frames on the device, the oracle's frames on the device and a padded destination"""
    from ffmpeg_amd import swscale as S
    torch = _torch()
    rng = np.random.default_rng(seed)
    first = ffi.alloc_frame(PIX["yuv420p"], w, h, rng)
    dsrc, hsrc = F._upload_aligned(first, n, rng)
    want = np.stack([T._oracle_unscaled([np.ascontiguousarray(p[f, :, :a.shape[1]]) for p, a in zip(hsrc, first)], w, h, dst == "bgr24")
                     for f in range(n)])
    bw = 3 * w
    ddst = torch.empty((n, h, (bw + 63) // 64 * 64 + 64), dtype=torch.uint8, device="cuda:0")
    ctx = S.SwsContext(w, h, PIX["yuv420p"], w, h, PIX[dst], S.SWS_BICUBIC)
    return ctx, dsrc, torch.from_numpy(want).to("cuda:0"), ddst


def _table_call(ctx, dsrc, want, ddst):
    """one call into a destination refilled with the sentinel; None when every frame is the oracle's and the padding untouched"""
    torch = _torch()
    bw = want.shape[2]
    ddst.fill_(SENTINEL)
    ctx.scale_batch(dsrc, [ddst])
    torch.cuda.synchronize()
    if torch.equal(ddst[:, :, :bw], want) and bool((ddst[:, :, bw:] == SENTINEL).all()):
        return None
    bad = (ddst[:, :, :bw] != want).any(dim=2)
    return "%d rows differ, stale (frame, rows): %s, padding written: %s" % (
        int(bad.sum()), _stale(ddst, bw), not bool((ddst[:, :, bw:] == SENTINEL).all()))


# (a) the product path: launches of 64 MiB and more go through the launch tuner, which runs calls 1, 2, 5, 6 (and, once decided, every
#     call on a box where it wins) in the eighth-per-XCD numbering.  These batches launch 2970, 4500 and 3780 workgroups.
@pytest.mark.parametrize("dst", ["rgb24", "bgr24"])
@pytest.mark.parametrize("w,h,n", [(1920, 1080, 11), (1280, 720, 25), (2560, 1440, 7)])
def test_table_converter_tuner_on_ragged_grids(w, h, n, dst):
    assert _table_grid(w, h, n) % 8 and w * h * 3 * n >= 64 << 20
    ctx, dsrc, want, ddst = _table_case(w, h, n, dst, seed=w + n)
    assert ctx.tuned_numbering == -1
    seen, failed = [], []
    for call in range(11):
        err = _table_call(ctx, dsrc, want, ddst)
        if err:
            failed.append("call %d (numbering %s): %s" % (call, "tuning" if call < 8 else ctx.tuned_numbering, err))
        seen.append(ctx.tuned_numbering)
    ctx.close()
    assert not failed, "grid %d:\n%s" % (_table_grid(w, h, n), "\n".join(failed))
    assert seen[:8] == [-1] * 8 and seen[8] in (0, 1) and seen[8:] == [seen[8]] * 3, seen


# (b) every numbering, forced by name (the measure build), on small batches whose grids are below 8, take every residue mod 8, and sit
#     just below, on and above the 8 * 2^k workgroups a chunked numbering deals round-robin (xcd2: chunks of 4, xcd4: chunks of 16)
TABLE_SHAPES = [(1000, 6, n) for n in range(1, 25)] + [(1000, 62, 4), (1000, 64, 4), (1000, 6, 43), (1000, 64, 5), (1000, 64, 9),
                                                        (1000, 254, 4), (1000, 256, 4), (1000, 258, 4), (1000, 64, 17)]


def test_table_shapes_cover_the_grids_they_are_meant_to():
    grids = [_table_grid(*s) for s in TABLE_SHAPES]
    assert set(range(1, 19)) <= set(grids)                          # below 8, and every residue above it
    assert {g % 8 for g in grids if g > 8} == set(range(8))
    for span in (32, 128):                                          # xcd2, xcd4: all remapped, a part and a tail, all tail
        assert {span - 1, span, span + 1, span + 8} <= set(grids), span
    assert 72 in grids and 136 in grids


@pytest.mark.parametrize("dst", ["rgb24", "bgr24"])
@pytest.mark.parametrize("variant", ["", "xcd", "xcd2", "xcd4", "st+xcd"])
def test_table_converter_forced_numberings(variant, dst, monkeypatch):
    if variant:
        monkeypatch.setenv("FFHIP_YUV2RGB_VARIANT", variant)
    else:
        monkeypatch.delenv("FFHIP_YUV2RGB_VARIANT", raising=False)
    failed = []
    for w, h, n in TABLE_SHAPES:
        ctx, dsrc, want, ddst = _table_case(w, h, n, dst, seed=w + h + n)
        err = _table_call(ctx, dsrc, want, ddst)
        ctx.close()
        if err:
            failed.append("%dx%d x %d (grid %d): %s" % (w, h, n, _table_grid(w, h, n), err))
    assert not failed, "\n".join(failed)


# (c) the other kernels that renumber workgroups or pack frames into waves, at every batch count up to 9 and at 17
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("fshift", [None, "0", "1", "2"], ids=lambda v: "fshift_" + (v or "default"))
@pytest.mark.parametrize("xcd", [None, "0", "2", "3"], ids=lambda v: "xcd_" + (v or "default"))
def test_up2_batch_counts(xcd, fshift, n, monkeypatch):
    env = {k: v for k, v in (("FFHIP_UP2_XCD", xcd), ("FFHIP_UP2_FSHIFT", fshift)) if v is not None}
    F._run("nv12", 192, 108, "nv12", 384, 216, ffi.SWS_BICUBIC, env=env, monkeypatch=monkeypatch, n=n, seed=n, need="up2")


@pytest.mark.parametrize("n", COUNTS)
def test_up2_above_8_bits_batch_counts(n):
    """k_sws_up2's 16-bit twin (a fresh zeroed destination per call, padded past the row: test_gpu_sws_hbd._run)"""
    from ffmpeg_amd import swscale as S
    _torch()
    ctx = S.SwsContext(64, 36, H.FMT["yuv420p10le"][0], 128, 72, H.FMT["yuv420p10le"][0], ffi.SWS_BICUBIC)
    assert ctx.up2_path
    ctx.close()
    H._run(("yuv420p10le", 64, 36, "yuv420p10le", 128, 72, ffi.SWS_BICUBIC), nframes=n)


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("xcd", [None, "0"], ids=lambda v: "xcd_" + (v or "default"))
def test_down2_batch_counts(xcd, n, monkeypatch):
    env = {"FFHIP_DN2_XCD": xcd} if xcd else None
    F._run("nv12", 384, 216, "nv12", 192, 108, ffi.SWS_BICUBIC, env=env, monkeypatch=monkeypatch, n=n, seed=n, need="down2")


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("sf,df,dw,dh", [("yuv420p", "rgb24", 200, 108), ("yuv420p", "bgra", 1288, 48), ("yuv420p", "abgr", 12, 8),
                                         ("yuv420p", "bgr24", 1032, 20), ("yuv420p", "rgba", 260, 16), ("yuv420p", "argb", 2048, 12)])
def test_down2_rgb_batch_counts(sf, df, dw, dh, n, monkeypatch):
    """k_sws_down2_rgb, the fused exact-half path (test_rgb_exact_half_fused_planar's shapes)"""
    F._run(sf, 2 * dw, 2 * dh, df, dw, dh, ffi.SWS_BICUBIC, env={"FFHIP_SWS_DOWN2": "1"}, monkeypatch=monkeypatch, n=n, seed=dw + n,
           need="any")


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("fpp", ["1", "2", "4"])
def test_up2rgb_batch_counts(fpp, n, monkeypatch):
    F._run("yuv420p", 128, 72, "rgb24", 256, 144, ffi.SWS_BICUBIC, env={"FFHIP_UP2RGB_FPP": fpp}, monkeypatch=monkeypatch, n=n, seed=n,
           need="up2rgb")


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("fpp", ["1", "2", "4"])
def test_eqrgb_batch_counts(fpp, n, monkeypatch):
    from ffmpeg_amd import swscale as S
    ctx = S.SwsContext(192, 108, PIX["nv12"], 192, 108, PIX["rgb24"], ffi.SWS_BICUBIC)
    assert ctx.paths & 128, "case does not reach the equal-size kernel"
    ctx.close()
    F._run("nv12", 192, 108, "rgb24", 192, 108, ffi.SWS_BICUBIC, env={"FFHIP_EQRGB_FPP": fpp}, monkeypatch=monkeypatch, n=n, seed=n,
           need="any")
