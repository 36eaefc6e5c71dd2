"""GPU tier of the VP9 loop-filter matrix (tests/vp9_lf_matrix.py): every route the kernels branch on x every decision cell of the
filter arithmetic, byte for byte against the oracle.  vp9.loop_filter_batch over the batch launches, compared over the WHOLE buffer
(guards, stride padding and the bytes in front of an unaligned base included); the frame faces over the cell pictures, the `waves`
pictures and the mixed picture, against run_tables / run_ctables superblock by superblock in raster order; the host faces of
ff_vp9dsp_loopfilter_init_hip with one segment per label class and the pointer on every residue."""
import ctypes as C

import numpy as np
import pytest

import ffi
import vp9_lf_matrix as M
from ffi import u8p
from test_gpu_vp9_lf_frame import compare

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _dev(torch, a):
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    assert t.data_ptr() % 16 == 0                     # what vp9_lf_matrix.kernel_route assumes of the device base
    return t


# ---------------------------------------------------------------------------------------------------------------------------
# the batch face
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", M.BATCH_GROUPS)
@pytest.mark.parametrize("bd", M.DEPTHS)
def test_batch_routes(bd, group):
    from ffmpeg_amd import vp9
    torch = _torch()
    launches = M.batch_launches(bd, group)
    if group == "counts":
        assert [len(L.segs) for L in launches] == M.COUNTS
    else:
        for route in [r for r in M.BATCH_ROUTES if r.startswith(group)]:
            assert M.batch_missing(launches, route) == [], route
    for L in launches:
        n = len(L.segs)
        want = L.want_oracle()
        for i, s in enumerate(L.segs):
            assert M.kernel_route(L, i) == s.route
            a, b = L.lines(L.buf, i), L.lines(want, i)
            for line, c in enumerate(s.rec.cells):                      # the oracle changed exactly the designed samples
                assert set(np.flatnonzero(a[line] != b[line]).tolist()) == set(c.changed), (L.name, i, line, c.name)
        rec = L.edge_records(vp9.EDGE_DTYPE)
        d_buf = _dev(torch, L.buf)
        vp9.loop_filter_batch(d_buf[L.k * L.ps:], L.stride, torch.from_numpy(rec.view(np.uint8).reshape(n, 12).copy()).cuda(), n, bit_depth=bd)
        torch.cuda.synchronize()
        bad = L.first_bad(d_buf.cpu().numpy(), want)
        assert bad is None, bad


# ---------------------------------------------------------------------------------------------------------------------------
# the frame faces
# ---------------------------------------------------------------------------------------------------------------------------
FACES = {"default": ("420", {}), "1-row-workgroups": ("420", {"FFHIP_VP9_LF_WPB": "1"}), "2-row-workgroups": ("420", {"FFHIP_VP9_LF_WPB": "2"}),
         "3-row-workgroups": ("420", {"FFHIP_VP9_LF_WPB": "3"}), "row-kernel": ("420", {"FFHIP_VP9_LF_OLD": "1"}), "444": ("444", {}),
         "422": ("422", {}), "440": ("440", {}), "frames": ("420", {}), "frames-444": ("444", {}), "frames-422": ("422", {}), "frames-440": ("440", {})}


def _first_bad(P, dev, wants):
    """the first wrong line of a cell picture with its route, cell and label, for the failure message"""
    for pl in P.places:
        w = wants[pl.plane]
        got = dev[pl.plane].cpu().numpy().view(w.dtype).reshape(w.shape)
        a = got[pl.y - 8:pl.y + 8, pl.x:pl.x + 8].T if pl.d else got[pl.y:pl.y + 8, pl.x - 8:pl.x + 8]
        b = P.lines(wants, pl)
        rows = np.flatnonzero((a != b).any(axis=1))
        if len(rows):
            line = int(rows[0])
            c = pl.rec.cells[line]
            return "%s: route %s, entry at (%d, %d), width %d E %d I %d H %d valid %d, line %d: cell %s, label %s: got %s, want %s" % (
                P.name, P.route(pl), pl.y, pl.x, pl.rec.wd, pl.rec.E, pl.rec.I, pl.rec.H, pl.valid, line, c.name, c.label, a[line].tolist(), b[line].tolist())
    return "%s: outside every entry" % P.name


@pytest.mark.parametrize("face", list(FACES))
@pytest.mark.parametrize("bd", M.DEPTHS)
def test_frame_faces(bd, face, monkeypatch):
    from ffmpeg_amd import vp9, _lib
    torch = _torch()
    fmt, knobs = FACES[face]
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    pics = list(M.frame_pics(bd, fmt)) + [M.mixed_pic(bd, fmt)]
    for route in M.FRAME_ROUTES:
        if route.startswith(fmt):
            assert M.frame_missing(pics[:-1], route) == [], route
    for d in (0, 1):
        assert M.compositions_missing(pics, d) == [], d
    ss = M.FORMATS[fmt]
    ssc = fmt in ("422", "440")
    dev = [[_dev(torch, b) for b in P.before] for P in pics]
    tabs = [torch.from_numpy(P.tables.view(np.int32)).cuda() for P in pics]
    ctabs = [torch.from_numpy(P.ctables.view(np.int32)).cuda() for P in pics]
    stride = lambda P: (P.before[0].strides[0], P.before[1].strides[0])
    if face.startswith("frames"):                                         # the pictures of one geometry as the pictures of one launch
        for shape in sorted({(P.sbc, P.sbr) for P in pics}):
            idx = [i for i, P in enumerate(pics) if (P.sbc, P.sbr) == shape]
            assert len(idx) >= 2
            P = pics[idx[0]]
            if ssc:
                vp9.loopfilter_frames_ssc([(*dev[i], tabs[i], ctabs[i]) for i in idx], *stride(P), P.cols, P.rows, ss, bit_depth=bd)
            else:
                vp9.loopfilter_frames([(*dev[i], tabs[i]) for i in idx], *stride(P), P.cols, P.rows, bit_depth=bd, ss=ss)
    else:
        for i, P in enumerate(pics):
            if ssc:
                vp9.loopfilter_frame_ssc(*dev[i], *stride(P), P.cols, P.rows, tabs[i], ctabs[i], ss, bit_depth=bd)
            else:
                vp9.loopfilter_frame(*dev[i], *stride(P), P.cols, P.rows, tabs[i], bit_depth=bd, ss=ss)
    torch.cuda.synchronize()
    assert _lib.lib().ffhip_stream_synchronize(None) == 0
    for i, P in enumerate(pics):
        wants = P.want_oracle()
        assert sum(int((w != b).sum()) for w, b in zip(wants, P.before)) > 500, P.name
        try:
            compare(dev[i], wants, P.before, P.cols, P.rows, ss)          # the planes, and nothing written beyond the picture
        except AssertionError as e:
            raise AssertionError("%s\n%s" % (_first_bad(P, dev[i], wants), e)) from None


# ---------------------------------------------------------------------------------------------------------------------------
# the host faces
# ---------------------------------------------------------------------------------------------------------------------------
def _aligned(nbytes, mod):
    raw = np.zeros(nbytes + 8, np.uint8)
    at = (mod - raw.ctypes.data) % 4
    a = raw[at:at + nbytes]
    assert a.ctypes.data % 4 == mod
    return a


@pytest.mark.parametrize("bd", M.DEPTHS)
def test_host_faces(bd):
    """loop_filter_8[w][d], loop_filter_16[d], loop_filter_mix2[w1][w2][d]: every record (so every label class of the width), the host
    pointer on every residue modulo 4 (16 bits: the even ones); the two halves of _16 and mix2 from different records in both orders"""
    from ffmpeg_amd import vp9
    _torch()
    c = vp9.lf_init(bd)
    O = ffi.oracle()
    ps = 1 if bd == 8 else 2
    dt = np.uint8 if bd == 8 else np.uint16
    rng = np.random.default_rng(950 + bd)
    recs = M.records(bd)
    by_wd = {wd: [r for r in recs if r.wd == wd] for wd in M.WD}
    H, W = 40, 48                                                          # samples; the stride is a multiple of 4 bytes
    label = lambda r: {M.lf_model(x.px, r.wd, r.E, r.I, r.H, bd)[1] for x in r.cells}
    calls = []                                                             # (face name, function, [records], packed limits)
    for w, wd in enumerate(M.WD):
        for d in (0, 1):
            calls += [("loop_filter_8[%d][%d]" % (w, d), c.loop_filter_8[w][d], d, [r], (r.E, r.I, r.H)) for r in by_wd[wd]]
    same16 = [r for r in by_wd[16] if (r.E, r.I, r.H) == (255, 255, 255)]
    for d in (0, 1):
        for a, b in zip(same16, same16[1:] + same16[:1]):
            for pair in ((a, b), (b, a)):
                calls.append(("loop_filter_16[%d]" % d, c.loop_filter_16[d], d, list(pair), (255, 255, 255)))
        for w1 in (0, 1):
            for w2 in (0, 1):
                A, B = by_wd[M.WD[w1]], by_wd[M.WD[w2]]
                for n in range(max(len(A), len(B))):
                    for a, b in [(A[n % len(A)], B[(n + 1) % len(B)])] + ([(B[(n + 1) % len(B)], A[n % len(A)])] if w1 == w2 else []):
                        calls.append(("loop_filter_mix2[%d][%d][%d]" % (w1, w2, d), c.loop_filter_mix2[w1][w2][d], d, [a, b],
                                      (a.E | b.E << 8, a.I | b.I << 8, a.H | b.H << 8)))
    of_width = {wd: set().union(*(label(r) for r in by_wd[wd])) for wd in M.WD}           # the label classes a width's records reach
    assert of_width[4] == {"none", "tap_hev", "tap_soft"} and of_width[8] == {"tap_soft", "flat8"} and of_width[16] == {"none", "tap_soft", "flat8", "flat16"}
    seen = {}
    for n, (name, fn, d, rs, lim) in enumerate(calls):
        mod = (n * ps) % 4
        a = _aligned(H * W * ps + 4, mod)
        pa = a[:H * W * ps].view(dt).reshape(H, W)
        pa[:] = rng.integers(0, 1 << bd, (H, W))
        y, x = 12, 16
        for k, r in enumerate(rs):
            M.BatchLaunch._put(pa, d, y + (0 if d else 8 * k), x + (8 * k if d else 0), M.rec_lines(r))
        b = a.copy()
        off = (y * W + x) * ps
        assert (a.ctypes.data + off) % 4 == mod
        fn(a.ctypes.data + off, W * ps, *lim)
        for k, r in enumerate(rs):
            O.ffo_vp9_loop_filter_bd(bd, r.wd, d, C.cast(b.ctypes.data + off + 8 * k * (ps if d else W * ps), u8p), W * ps, r.E, r.I, r.H)
        assert np.array_equal(a, b), (name, mod, [(r.wd, r.E, r.I, r.H, [x.name for x in r.cells]) for r in rs])
        s = seen.setdefault(name, {"mods": set(), "labels": set(), "pairs": set()})
        s["mods"].add(mod)
        s["labels"] |= set().union(*(label(r) for r in rs))
        if len(rs) == 2:
            s["pairs"] |= {(la, lb) for la in label(rs[0]) for lb in label(rs[1])}
    assert len(seen) == 6 + 2 + 8
    for name, s in seen.items():
        assert s["mods"] == set(range(0, 4, ps)), (name, s["mods"])
        widths = {"loop_filter_8[0]": [4], "loop_filter_8[1]": [8], "loop_filter_8[2]": [16], "loop_filter_16": [16], "loop_filter_mix2[0][0]": [4],
                  "loop_filter_mix2[0][1]": [4, 8], "loop_filter_mix2[1][0]": [4, 8], "loop_filter_mix2[1][1]": [8]}[name[:name.rindex("[")]]
        want = set().union(*(of_width[wd] for wd in widths)) - ({"none"} if name.startswith("loop_filter_16") else set())
        assert s["labels"] >= want, (name, s["labels"])
        if s["pairs"]:                                                    # halves of different labels in both orders
            mixed = {(la, lb) for la, lb in s["pairs"] if la != lb}
            assert mixed, name
            if "mix2[0][1]" not in name and "mix2[1][0]" not in name:    # (those two faces are each other's reverse order)
                assert all((lb, la) in mixed for la, lb in mixed), (name, mixed)
