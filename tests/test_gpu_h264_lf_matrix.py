"""GPU tier of the H.264 in-loop filter matrix (tests/h264_lf_matrix.py): every route the kernels branch on x every decision cell of
the filter arithmetic, byte for byte against the oracle.  The batch faces over the batch launches, compared over the WHOLE buffer
(guards, stride padding and the bytes in front of an unaligned base included); the frame faces over the cell pictures, the `waves`
pictures and the mixed picture on each of the three frame kernels, stride padding included; the host faces of ff_h264dsp_init_hip
over the cell records with the pointer on every residue.  Every test asserts that its launches changed something and names, on a
mismatch, the first bad cell with its label, route and line."""
import ctypes as C

import numpy as np
import pytest

import ffi
import h264_lf_matrix as M
from ffi import u8p, i8p

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _dev(torch, a):
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    assert t.data_ptr() % 16 == 0                     # what h264_lf_matrix.kernel_route / frame_kernel assume of the device base
    return t


# ---------------------------------------------------------------------------------------------------------------------------
# the batch faces
# ---------------------------------------------------------------------------------------------------------------------------
def _run_batch(torch, L):
    from ffmpeg_amd import h264, _lib
    n = len(L.segs)
    want = L.want_oracle()
    assert (want != L.buf).any(), L.name
    for i, s in enumerate(L.segs):
        assert M.kernel_route(L, i) == s.route
    d_buf = _dev(torch, L.buf)
    d_ed = torch.from_numpy(L.edge_records().view(np.uint8).reshape(n, 12).copy()).cuda()
    if L.face == "b8":
        h264.loop_filter_batch(d_buf[L.k * L.ps:], L.stride, d_ed, n)
    else:
        assert _lib.lib().ffhip_h264_loop_filter_batch_dev_hbd(L.bd, C.c_void_p(d_buf.data_ptr() + L.k * L.ps), C.c_ssize_t(L.stride),
                                                               C.c_void_p(d_ed.data_ptr()), n, None) == 0
    torch.cuda.synchronize()
    bad = L.first_bad(d_buf.cpu().numpy(), want)
    assert bad is None, bad


@pytest.mark.parametrize("group", M.BATCH_GROUPS)
@pytest.mark.parametrize("bd", M.DEPTHS)
def test_batch_routes(bd, group):
    """8 bits: ffhip_h264_loop_filter_batch_dev (k_h264_loop_filter: lf_line behind the dword, the sample-wise and the row path);
    10 / 14 bits: the same launches through ..._dev_hbd (k_h264_loop_filter_hbd has one column path: there the groups differ in
    alignment alone)"""
    torch = _torch()
    launches = M.batch_launches(bd, group)
    if group == "counts":
        assert [len(L.segs) for L in launches] == M.COUNTS
    else:
        for route in [r for r in M.BATCH_ROUTES if r.startswith(group)]:
            assert M.batch_missing(launches, route) == [], route
    for L in launches:
        _run_batch(torch, L)


@pytest.mark.parametrize("bd", M.MEMBER_DEPTHS)
def test_batch_hbd_members(bd):
    """the 14 members of k_h264_loop_filter_hbd (plain, MBAFF, 4:2:2: FFHipH264Edge.pad = lines per tc0 entry), each over every cell
    of its class"""
    torch = _torch()
    launches = M.member_launches(bd)
    assert [(L.kind(0), L.segs[0].rec.inner) for L in launches] == M.MEMBERS
    for L in launches:
        assert M.batch_missing([L], "any", [L.segs[0].rec.cls]) == [], L.name
        _run_batch(torch, L)


# ---------------------------------------------------------------------------------------------------------------------------
# the frame faces
# ---------------------------------------------------------------------------------------------------------------------------
#: face -> (kernel, stride padding in samples, FFHIP_DEBLOCK_OLD, pictures per launch)
FACES = {"skew": ("skew", 0, None, 1), "skew-pad": ("skew", 16, None, 1), "skew-frames": ("skew", 0, None, 3), "band": ("band", 4, None, 1),
         "band-frames": ("band", 4, None, 3), "band-old2": ("band", 0, "2", 1), "row": ("row", 3, None, 1), "row-old1": ("row", 0, "1", 3)}
FRAME_CASES = [(f, c, bd) for f in FACES for c in (0, 1) for bd in M.DEPTHS
               if (bd == 8 or FACES[f][0] == "skew") and not (c and FACES[f][0] == "row")]


def _launch_frames(torch, bd, chroma, pics, pad, per_launch):
    """the pictures (one geometry) in launches of up to per_launch pictures at a pitch; returns the planes read back"""
    from ffmpeg_amd import h264
    P = pics[0]
    planes = [X.embed(pad) for X in pics]
    stride = planes[0].strides[0]
    gap = 48 * stride if pad != 3 else 5 * stride + 1                   # between the pictures of a launch: a pitch beyond the plane
    size = planes[0].nbytes
    pitch = size + gap
    got = []
    for at in range(0, len(pics), per_launch):
        grp = list(range(at, min(at + per_launch, len(pics))))
        rng = np.random.default_rng(at + pad)
        buf = rng.integers(0, 256, pitch * len(grp), dtype=np.uint8)
        for j, i in enumerate(grp):
            buf[j * pitch:j * pitch + size] = planes[i].view(np.uint8).reshape(-1)
        d = _dev(torch, buf)
        ed = np.concatenate([pics[i].edges for i in grp])
        d_ed = torch.from_numpy(ed.view(np.uint8).reshape(-1, 12).copy()).cuda()
        assert d_ed.data_ptr() % 16 == 0
        if bd > 8:
            h264.deblock_frames_hbd(bd, d, pitch, len(grp), stride, P.mb_w, P.mb_h, d_ed, chroma=bool(chroma))
        elif chroma:
            h264.deblock_frames_chroma(d, pitch, len(grp), stride, P.mb_w, P.mb_h, d_ed)
        elif len(grp) == 1:
            h264.deblock_frame(d, stride, P.mb_w, P.mb_h, d_ed)
        else:
            h264.deblock_frames(d, pitch, len(grp), stride, P.mb_w, P.mb_h, d_ed)
        torch.cuda.synchronize()
        back = d.cpu().numpy()
        for j, i in enumerate(grp):
            assert np.array_equal(back[j * pitch + size:(j + 1) * pitch], buf[j * pitch + size:(j + 1) * pitch]), "%s: bytes between the pictures changed" % pics[i].name
            got.append(back[j * pitch:j * pitch + size].view(planes[i].dtype).reshape(planes[i].shape))
    return got, stride, pitch


@pytest.mark.parametrize("face,chroma,bd", FRAME_CASES)
def test_frame_faces(face, chroma, bd, monkeypatch):
    """one kernel x plane class x depth: the four cell pictures (vertical / horizontal edges, k == 0 / k > 0: every cell of the plane's
    classes on each, every hand-off class of the kernel on the k == 0 horizontal one), the two waves pictures and the mixed picture"""
    from ffmpeg_amd import _lib
    torch = _torch()
    kernel, pad, old, per_launch = FACES[face]
    if old:
        monkeypatch.setenv("FFHIP_DEBLOCK_OLD", old)
    cellp = list(M.frame_pics(bd, chroma))
    for dk in M.FRAME_DK:
        assert M.frame_missing(cellp, dk, cellp[0].classes) == [], dk
    assert M.handoff_missing(cellp, kernel, per_launch) == []
    for X in M.waves_pics(bd, chroma):
        assert set(M.COMPOSITIONS) <= M.compositions(X)
    for pics in (cellp, list(M.waves_pics(bd, chroma)), [M.mixed_pic(bd, chroma)]):
        got, stride, pitch = _launch_frames(torch, bd, chroma, pics, pad, per_launch)
        assert M.frame_kernel(bd, chroma, 0, stride, pitch if per_launch > 1 and len(pics) > 1 else 0, 0, int(old or 0)) == kernel
        assert _lib.lib().ffhip_stream_synchronize(None) == 0
        for X, g in zip(pics, got):
            want = X.want_oracle(pad)
            assert (want != X.embed(pad)).sum() > 300, X.name
            if not np.array_equal(g, want):
                raise AssertionError(X.first_bad(g, want, kernel) if X.places else "%s (%s): %d mismatches, first at %s" % (
                    X.name, kernel, (g != want).sum(), np.argwhere(g != want)[0].tolist()))


# ---------------------------------------------------------------------------------------------------------------------------
# the object route of 4:2:2 chroma
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", [8, 10])
def test_c422_object(bd):
    """k_h264_deblock_c422 (lf_line) through h264.Picture(chroma_format=2).deblock_mb() and flush() on planes 1 and 2: the four cell
    pictures and a mixed one per plane, Cb and Cr holding different ones, against ffo_h264_deblock_frame_c422_bd; luma carries no
    record and must not change"""
    from ffmpeg_amd import h264
    torch = _torch()
    cb, cr = M.c422_pics(bd, 1), M.c422_pics(bd, 2)
    for dk in M.FRAME_DK:
        assert M.frame_missing(cb[:-1], dk, (1, 3)) == [] and M.frame_missing(cr[:-1], dk, (1, 3)) == [], dk
    pad = 8
    for j in range(len(cb)):
        pair = (cb[j], cr[(j + 1) % 4] if j < 4 else cr[j])                  # Cr: another (direction, k class) than Cb
        P = pair[0]
        assert (pair[1].mb_w, pair[1].mb_h) == (P.mb_w, P.mb_h)
        luma = np.random.default_rng(j).integers(0, 1 << bd, (P.mb_h * 16, P.mb_w * 16 + pad)).astype(P.before.dtype)
        planes = [luma] + [X.embed(pad) for X in pair]
        strides = [a.strides[0] for a in planes]
        pic = h264.Picture(P.mb_w, P.mb_h, bit_depth=bd, chroma_format=2)
        pic.begin()
        for pl, X in ((1, pair[0]), (2, pair[1])):
            for mb in range(X.mb_w * X.mb_h):
                pic.deblock_mb(pl, mb % X.mb_w, mb // X.mb_w, X.edges[6 * mb:6 * mb + 6].copy())
        d = [_dev(torch, a) for a in planes]
        pic.flush(d, strides, d)
        torch.cuda.synchronize()
        pic.close()
        assert np.array_equal(d[0].cpu().numpy().view(luma.dtype).reshape(luma.shape), luma)
        for pl, X in ((1, pair[0]), (2, pair[1])):
            want = X.want_oracle(pad)
            assert (want != planes[pl]).sum() > 100, X.name
            g = d[pl].cpu().numpy().view(want.dtype).reshape(want.shape)
            if not np.array_equal(g, want):
                raise AssertionError("plane %d: %s" % (pl, X.first_bad(g, want, "c422") if X.places else "%s: %d mismatches, first at %s" % (
                    X.name, (g != want).sum(), np.argwhere(g != want)[0].tolist())))


# ---------------------------------------------------------------------------------------------------------------------------
# the MBAFF object route
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", [8, 10])
def test_mbaff_object(bd):
    """k_h264_mbaff_deblock (lf_line at the depth) through ffhip_h264_mbaff_filter_call() / ffhip_h264_mbaff_flush(): one call per live
    macroblock pair and plane in disjoint tiles - the ordinary members at the frame's and at twice the line size
    (FFHIP_H264_LF_CALL_FIELD), the 8 / 4-line _mbaff members likewise - against ffo_h264_loop_filter_bd call by call"""
    from ffmpeg_amd import _lib
    torch = _torch()
    L = _lib.lib()
    P = M.mbaff_pic(bd)
    assert all(P.in_tile(c) for c in P.calls)
    pad = 8
    planes = P.embed(pad)
    strides = [a.strides[0] for a in planes]
    m = C.c_void_p()
    assert L.ffhip_h264_mbaff_create_fmt(C.byref(m), P.mb_w, P.mb_h, bd) == 0 and m
    try:
        L.ffhip_h264_mbaff_begin(m)
        for c in sorted(P.calls, key=lambda c: (c.mb_y // 2, c.mb_x, c.plane)):       # pair by pair in decoding order
            e = P.edge(c, strides[c.plane])
            assert L.ffhip_h264_mbaff_filter_call(m, c.plane, c.mb_x, c.mb_y, C.c_void_p(e.ctypes.data)) == 0, (c[:7], L.ffhip_last_error())
        d = [_dev(torch, a) for a in planes]
        assert L.ffhip_h264_mbaff_flush(m, (C.c_void_p * 3)(*[t.data_ptr() for t in d]), (C.c_int * 3)(*strides), None) == 0, L.ffhip_last_error()
        torch.cuda.synchronize()
        assert L.ffhip_stream_synchronize(None) == 0
    finally:
        L.ffhip_h264_mbaff_free(C.byref(m))
    want = P.want_oracle(pad)
    got = [t.cpu().numpy().view(w.dtype).reshape(w.shape) for t, w in zip(d, want)]
    assert all((w != a).sum() > 100 for w, a in zip(want, planes))
    bad = P.first_bad(got, want)
    assert bad is None, bad


# ---------------------------------------------------------------------------------------------------------------------------
# the host faces
# ---------------------------------------------------------------------------------------------------------------------------
def _aligned(nbytes, mod):
    raw = np.zeros(nbytes + 8, np.uint8)
    at = (mod - raw.ctypes.data) % 4
    a = raw[at:at + nbytes]
    assert a.ctypes.data % 4 == mod
    return a


@pytest.mark.parametrize("bd", [8, 10])
def test_host_faces(bd):
    """the eight loop-filter members of the table ff_h264dsp_init_hip fills, over every cell record of the member's class; column
    edges with the host pointer on every residue modulo 4 (16 bits: the even ones)"""
    from ffmpeg_amd import _lib
    from test_gpu_shims import H264DSP
    _torch()
    L = _lib.lib()
    O = M.oracle()
    c = H264DSP()
    assert L.ff_h264dsp_init_hip(C.byref(c), bd, 1) == 0
    names = ["v_loop_filter_luma", "h_loop_filter_luma", "v_loop_filter_chroma", "h_loop_filter_chroma",
             "v_loop_filter_luma_intra", "h_loop_filter_luma_intra", "v_loop_filter_chroma_intra", "h_loop_filter_chroma_intra"]
    ps = 1 if bd == 8 else 2
    dt = np.uint8 if bd == 8 else np.uint16
    rng = np.random.default_rng(1950 + bd)
    H, W = 32, 40                                                          # samples; the stride is a multiple of 4 bytes
    seen = {}
    n = 0
    for kind, name in enumerate(names):
        cls, col = (kind >> 1 & 1) | (kind >> 2 & 1) << 1, kind & 1
        for r0 in M.records(bd, cls):
            for rep in range(2 if col else 1):                             # column edges: every record at two residues
                n += 1
                r = M.rot(r0, n)
                mod = (n * ps) % 4 if col else 0
                a = _aligned(H * W * ps + 4, mod)
                pa = a[:H * W * ps].view(dt).reshape(H, W)
                pa[:] = rng.integers(0, 1 << bd, (H, W))
                y, x = (8, 16) if col else (16, 8)
                M.BatchLaunch._put(pa, col, y, x, M.rec_lines(r))
                before = a.copy()
                b = a.copy()
                off = (y * W + x) * ps
                assert (a.ctypes.data + off) % 4 == mod
                tc0 = np.array(r.tc0, np.int8)
                pix = C.cast(a.ctypes.data + off, u8p)
                if kind < 4:
                    getattr(c, name)(pix, W * ps, r.alpha, r.beta, ffi.ptr(tc0, i8p))
                else:
                    getattr(c, name)(pix, W * ps, r.alpha, r.beta)
                O.ffo_h264_loop_filter_bd(bd, kind, r.inner, C.cast(b.ctypes.data + off, u8p), W * ps, r.alpha, r.beta, ffi.ptr(tc0, i8p))
                if not np.array_equal(a, b):
                    ga, gb = a[:H * W * ps].view(dt).reshape(H, W), b[:H * W * ps].view(dt).reshape(H, W)
                    yy, xx = (int(v) for v in np.argwhere(ga != gb)[0])
                    line = yy - y if col else xx - x
                    cell = r.cells[line] if 0 <= line < len(r.cells) else None
                    raise AssertionError("%s (residue %d, alpha %d beta %d tc0 %s): line %d, cell %s, label %s: got %d, want %d at %s" % (
                        name, mod, r.alpha, r.beta, list(r.tc0), line, cell.name if cell else "(guard)", cell.label if cell else "-",
                        int(ga[yy, xx]), int(gb[yy, xx]), (yy, xx)))
                s = seen.setdefault(name, {"mods": set(), "cells": set(), "changed": 0})
                s["mods"].add(mod)
                s["cells"] |= {x.name for x in r.cells}
                s["changed"] += int((b != before).sum())
    assert len(seen) == 8
    for kind, name in enumerate(names):
        cls = (kind >> 1 & 1) | (kind >> 2 & 1) << 1
        assert seen[name]["mods"] == (set(range(0, 4, ps)) if kind & 1 else {0}), name
        assert seen[name]["cells"] - {"fill"} == {x.name for x in M.cells(bd) if x.cls == cls}, name
        assert seen[name]["changed"] > 0, name
