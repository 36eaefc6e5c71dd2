"""vp8dsp on the GPU, byte for byte against the NumPy model of vp8dsp_model.py: every member of VP8DSPContext through the host-pointer
table (ff_vp78dsp_init_hip / ff_vp8dsp_init_hip), the three batch device faces over ragged counts, and the whole-frame loop filter
(ffhip_vp8_loopfilter_frames_dev), destinations, stride padding and consumed coefficients included."""
import ctypes as C

import numpy as np
import pytest

import vp8dsp_model as M
from ffmpeg_amd import _lib, vp8

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _sync():
    assert _lib.lib().ffhip_stream_synchronize(None) == 0


@pytest.fixture(scope="module")
def dsp():
    c = vp8.dsp_init()
    assert all(getattr(c, k) for k, _ in vp8.VP8DSPContext._fields_[:16])
    return c


def _p(a, y=0, x=0):
    return a.ctypes.data + y * a.strides[0] + x


# ---------------------------------------------------------------- the host-pointer table
def test_transforms_per_call(dsp):
    rng = np.random.default_rng(10)
    fb0 = _lib.lib().ffhip_shim_fallbacks()
    for it in range(60):
        big = it % 3 == 0
        dc = rng.integers(-32768 if big else -3000, 32768 if big else 3000, 16).astype(np.int16)
        blk = rng.integers(-500, 500, (16, 16)).astype(np.int16)
        for fn, ref in ((dsp.vp8_luma_dc_wht, M.luma_dc_wht), (dsp.vp8_luma_dc_wht_dc, M.luma_dc_wht_dc)):
            d1, b1, d2, b2 = dc.copy(), blk.copy(), dc.copy(), blk.copy()
            fn(b1.ctypes.data, d1.ctypes.data)
            ref(b2, d2)
            assert np.array_equal(b1, b2) and np.array_equal(d1, d2), it
        plane = rng.integers(0, 256, (12, 24)).astype(np.uint8)
        co = rng.integers(-2048 if it % 2 else -300, 2048 if it % 2 else 300, (4, 16)).astype(np.int16)
        for fn, ref, n in ((dsp.vp8_idct_add, M.idct_add, 1), (dsp.vp8_idct_dc_add, M.idct_dc_add, 1),
                           (dsp.vp8_idct_dc_add4y, M.idct_dc_add4y, 4), (dsp.vp8_idct_dc_add4uv, M.idct_dc_add4uv, 4)):
            a, b = plane.copy(), plane.copy()
            ca, cb = co[:n].copy(), co[:n].copy()
            fn(_p(a, 2, 3), ca.ctypes.data, a.strides[0])
            ref(b, 2, 3, cb[0] if n == 1 else cb)
            assert np.array_equal(a, b) and np.array_equal(ca, cb), (it, n)
    assert _lib.lib().ffhip_shim_fallbacks() == fb0


def _lf_lines(rng, n):
    """n lines of 8 samples (p3 .. q3): mostly small steps, some edges, some flat"""
    base = rng.integers(20, 236, n)[:, None]
    steps = rng.integers(-6, 7, (n, 8))
    steps[:, 4] += rng.choice([0, 0, 5, -5, 20, -20, 60], n)
    return np.clip(base + np.cumsum(steps, axis=1), 0, 255)


def _near(L):
    """(E, I, H) at the line's own thresholds: simple limit, largest inner difference, largest |p1 - p0| / |q1 - q0|"""
    p3, p2, p1, p0, q0, q1, q2, q3 = (int(v) for v in L)
    e = 2 * abs(p0 - q0) + (abs(p1 - q1) >> 1)
    i = max(abs(p3 - p2), abs(p2 - p1), abs(p1 - p0), abs(q3 - q2), abs(q2 - q1), abs(q1 - q0))
    h = max(abs(p1 - p0), abs(q1 - q0))
    return e, i, h


def test_loop_filters_per_call(dsp):
    rng = np.random.default_rng(11)
    fb0 = _lib.lib().ffhip_shim_fallbacks()
    members = [("vp8_v_loop_filter16y", True, 16, M.MBEDGE, 1), ("vp8_h_loop_filter16y", False, 16, M.MBEDGE, 1),
               ("vp8_v_loop_filter8uv", True, 8, M.MBEDGE, 2), ("vp8_h_loop_filter8uv", False, 8, M.MBEDGE, 2),
               ("vp8_v_loop_filter16y_inner", True, 16, M.INNER, 1), ("vp8_h_loop_filter16y_inner", False, 16, M.INNER, 1),
               ("vp8_v_loop_filter8uv_inner", True, 8, M.INNER, 2), ("vp8_h_loop_filter8uv_inner", False, 8, M.INNER, 2),
               ("vp8_v_loop_filter_simple", True, 16, M.SIMPLE, 1), ("vp8_h_loop_filter_simple", False, 16, M.SIMPLE, 1)]
    for name, vertical, n, kind, nplanes in members:
        fn = getattr(dsp, name)
        for it in range(40):
            planes = []
            for _ in range(nplanes):
                p = rng.integers(0, 256, (24, 24)).astype(np.uint8)
                L = _lf_lines(rng, n).T                                  # [8, n]
                if vertical:
                    p[4:12, 8:8 + n] = L
                else:
                    p[8:8 + n, 4:12] = L.T
                planes.append(p)
            line = (planes[0][4:12, 8 + it % n] if vertical else planes[0][8 + it % n, 4:12])
            e, i, h = _near(line)
            d = (it % 3) - 1                                             # the thresholds at, one below, one above the line's values
            if it < 30:
                E, I, H = e + d, i + d * (it % 2), h - d * ((it >> 1) % 2)
            else:
                E, I, H = rng.integers(0, 200), rng.integers(0, 64), rng.integers(0, 4)
            E, I, H = int(max(E, 0)), int(max(I, 0)), int(max(H, 0))
            want = [p.copy() for p in planes]
            for w in want:
                M.loop_filter(w, 8, 8, vertical, n, kind, E, I, H)
            got = [p.copy() for p in planes]
            if kind == M.SIMPLE:
                fn(_p(got[0], 8, 8), got[0].strides[0], E)
            elif nplanes == 2:
                fn(_p(got[0], 8, 8), _p(got[1], 8, 8), got[0].strides[0], E, I, H)
            else:
                fn(_p(got[0], 8, 8), got[0].strides[0], E, I, H)
            for g, w in zip(got, want):
                assert np.array_equal(g, w), (name, it, E, I, H)
    assert _lib.lib().ffhip_shim_fallbacks() == fb0


def test_mc_per_call_every_slot(dsp):
    rng = np.random.default_rng(12)
    fb0 = _lib.lib().ffhip_shim_fallbacks()
    src = rng.integers(0, 256, (48, 40)).astype(np.uint8)
    for bil, tab in ((False, dsp.put_vp8_epel_pixels_tab), (True, dsp.put_vp8_bilinear_pixels_tab)):
        for idx, w in enumerate((16, 8, 4)):
            for v in range(3):
                for hs in range(3):
                    fn = tab[idx][v][hs]
                    lo = 0 if bil else 1
                    cases = [(mx, my, int(rng.integers(1, 2 * w + 1))) for mx in range(lo, 8) for my in range(lo, 8)
                             if (hs or mx == lo) and (v or my == lo)]
                    cases += [(int(rng.integers(lo, 8)), int(rng.integers(lo, 8)), h) for h in range(1, 2 * w + 1)]
                    for mx, my, h in cases:
                        sy, sx = int(rng.integers(2, 48 - h - 3 + 1)), int(rng.integers(2, 40 - w - 3 + 1))
                        dst = rng.integers(0, 256, (33, 20)).astype(np.uint8)
                        want = dst.copy()
                        want[1:1 + h, 2:2 + w] = M.put(src, sy, sx, w, h, mx, my, v, hs, bil)
                        fn(_p(dst, 1, 2), dst.strides[0], _p(src, sy, sx), src.strides[0], h, mx, my)
                        assert np.array_equal(dst, want), (bil, w, v, hs, mx, my, h)
    assert _lib.lib().ffhip_shim_fallbacks() == fb0


# ---------------------------------------------------------------- batch faces
COUNTS = [1, 63, 64, 65, 100000]


def _check_ids(n, rng):
    """every record for small counts; for the large one the first and last 200 and 2000 more"""
    if n <= 1000:
        return range(n)
    return sorted(set(range(200)) | set(range(n - 200, n)) | set(rng.integers(0, n, 2000).tolist()))


@pytest.mark.parametrize("n", COUNTS)
def test_wht_batch(n):
    torch = _torch()
    rng = np.random.default_rng(20 + n)
    per = 16 + 256                                                   # dc[16] then block[4][4][16], int16
    co = rng.integers(-3000, 3000, (n, per)).astype(np.int16)
    co[::7, :16] = rng.integers(-32768, 32768, (len(co[::7]), 16))    # wrapping sums
    recs = np.zeros(n, vp8.WHT_DTYPE)
    recs["dc_offset"] = np.arange(n) * per * 2
    recs["block_offset"] = recs["dc_offset"] + 32
    recs["dc_only"] = rng.integers(0, 2, n)
    d_co = torch.from_numpy(co.copy()).cuda()
    vp8.luma_dc_wht_batch(d_co, torch.from_numpy(recs.view(np.uint8).copy()).cuda(), n)
    _sync()
    got = d_co.cpu().numpy()
    for i in _check_ids(n, rng):
        dc, blk = co[i, :16].copy(), co[i, 16:].reshape(16, 16).copy()
        (M.luma_dc_wht_dc if recs["dc_only"][i] else M.luma_dc_wht)(blk, dc)
        assert np.array_equal(got[i, :16], dc) and np.array_equal(got[i, 16:].reshape(16, 16), blk), i


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("odd", [False, True])
def test_idct_batch(n, odd):
    """blocks on a grid 64 blocks wide; odd: a stride and origin that are not multiples of 4 (the byte path)"""
    if odd and n == 100000:
        n = 4097
    torch = _torch()
    rng = np.random.default_rng(30 + n + odd)
    rows = (n + 63) // 64
    stride, x0 = (259, 1) if odd else (260, 0)
    plane = rng.integers(0, 256, (rows * 4 + 1, stride)).astype(np.uint8)
    co = rng.integers(-300, 300, (n, 16)).astype(np.int16)
    co[::5] = rng.integers(-4000, 4000, (len(co[::5]), 16))
    order = rng.permutation(n)                                       # records in any order
    recs = np.zeros(n, vp8.IDCT_DTYPE)
    recs["dst_offset"] = (order // 64) * 4 * stride + (order % 64) * 4 + x0
    recs["coeff_offset"] = np.arange(n) * 32
    recs["dc_only"] = rng.integers(0, 2, n)
    d_pl, d_co = torch.from_numpy(plane.copy()).cuda(), torch.from_numpy(co.copy()).cuda()
    vp8.idct_add_batch(d_pl, stride, d_co, torch.from_numpy(recs.view(np.uint8).copy()).cuda(), n)
    _sync()
    gp, gc = d_pl.cpu().numpy(), d_co.cpu().numpy()
    want = plane.copy()
    for i in _check_ids(n, rng):
        off = int(recs["dst_offset"][i])
        y, x = off // stride, off % stride
        c = co[i].copy()
        (M.idct_dc_add if recs["dc_only"][i] else M.idct_add)(want, y, x, c)
        assert np.array_equal(gp[y:y + 4, x:x + 4], want[y:y + 4, x:x + 4]) and np.array_equal(gc[i], c), i
    if n <= 1000:                                                    # nothing outside the blocks moved
        assert np.array_equal(gp, want)


@pytest.mark.parametrize("n", COUNTS)
def test_mc_batch(n):
    torch = _torch()
    rng = np.random.default_rng(40 + n)
    SW, SH = 256, 128
    src = rng.integers(0, 256, (SH, SW)).astype(np.uint8)
    recs = np.zeros(n, vp8.MC_DTYPE)
    w = rng.choice([16, 8, 4], n)
    h = np.array([rng.integers(1, 2 * x + 1) for x in w]) if n <= 1000 else (rng.random(n) * 2 * w).astype(int) + 1
    bil = rng.integers(0, 2, n)
    ht, vt = rng.integers(0, 3, n), rng.integers(0, 3, n)
    mx = np.where(bil == 1, rng.integers(0, 8, n), rng.integers(1, 8, n))
    my = np.where(bil == 1, rng.integers(0, 8, n), rng.integers(1, 8, n))
    sy = (rng.random(n) * (SH - 5 - h)).astype(int) + 2
    sx = (rng.random(n) * (SW - 5 - w)).astype(int) + 2
    DW = 20                                                          # a 16 x 32 destination slot per record, 4 padding columns
    recs["dst_offset"] = np.arange(n) * 32 * DW
    recs["src_offset"] = sy * SW + sx
    recs["width"], recs["h"], recs["mx"], recs["my"] = w, h, mx, my
    recs["htaps"], recs["vtaps"], recs["bilinear"] = ht, vt, bil
    dst = rng.integers(0, 256, (n * 32, DW)).astype(np.uint8)
    d_dst = torch.from_numpy(dst.copy()).cuda()
    vp8.mc_batch(d_dst, DW, torch.from_numpy(src).cuda(), SW, torch.from_numpy(recs.view(np.uint8).copy()).cuda(), n)
    _sync()
    got = d_dst.cpu().numpy()
    for i in _check_ids(n, rng):
        want = dst[32 * i:32 * i + 32].copy()
        want[:h[i], :w[i]] = M.put(src, int(sy[i]), int(sx[i]), int(w[i]), int(h[i]), int(mx[i]), int(my[i]), int(vt[i]), int(ht[i]),
                                   bool(bil[i]))
        assert np.array_equal(got[32 * i:32 * i + 32], want), (i, recs[i])


def test_mc_batch_skips_malformed_records():
    torch = _torch()
    rng = np.random.default_rng(49)
    src = rng.integers(0, 256, (64, 64)).astype(np.uint8)
    bad = [dict(width=12), dict(h=0), dict(h=33), dict(htaps=3), dict(vtaps=3), dict(bilinear=2), dict(mx=0), dict(my=8, vtaps=1),
           dict(bilinear=1, mx=8)]
    recs = np.zeros(len(bad), vp8.MC_DTYPE)
    for i, b in enumerate(bad):
        recs[i] = (i * 32 * 16, 20 * 64 + 20, 16, 8, 3, 3, 2, 2, 0, 0)
        for k, v_ in b.items():
            recs[k][i] = v_
    dst = rng.integers(0, 256, (len(bad) * 32, 16)).astype(np.uint8)
    d_dst = torch.from_numpy(dst.copy()).cuda()
    vp8.mc_batch(d_dst, 16, torch.from_numpy(src).cuda(), 64, torch.from_numpy(recs.view(np.uint8).copy()).cuda(), len(bad))
    _sync()
    assert np.array_equal(d_dst.cpu().numpy(), dst)


# ---------------------------------------------------------------- the whole-frame loop filter
def _content(rng, h, w):
    """smooth gradients with blocky steps and small noise: what a reconstructed frame looks like to the filters"""
    yy, xx = np.mgrid[0:h, 0:w]
    a = 128 + 60 * np.sin(yy / (7 + rng.random() * 20) + rng.random() * 6) * np.cos(xx / (9 + rng.random() * 20))
    a += rng.integers(-12, 13, (h // 4 + 1, w // 4 + 1)).repeat(4, 0).repeat(4, 1)[:h, :w]
    a += rng.integers(-3, 4, (h, w))
    return np.clip(a, 0, 255).astype(np.uint8)


def _strengths(rng, mb_h, mb_w):
    st = np.zeros((mb_h, mb_w), vp8.STRENGTH_DTYPE)
    level = rng.integers(0, 64, (mb_h, mb_w))
    level[rng.random((mb_h, mb_w)) < 0.15] = 0
    sharp = rng.integers(0, 8)
    il = level.copy()
    if sharp:                                                        # filter_level_for_mb's interior limit
        il = np.minimum(il >> ((sharp + 3) >> 2), 9 - sharp)
    st["filter_level"], st["inner_limit"] = level, np.maximum(il, 1)
    st["inner_filter"] = rng.random((mb_h, mb_w)) < 0.7
    bad = rng.random((mb_h, mb_w)) < 0.05                            # malformed records: the face reads them as level 0
    st["filter_level"][bad & (rng.random((mb_h, mb_w)) < 0.3)] = 64 + rng.integers(0, 100)
    st["inner_limit"][bad & (rng.random((mb_h, mb_w)) < 0.5)] = 64
    st["inner_filter"][bad & (rng.random((mb_h, mb_w)) < 0.5)] = 2
    return st


def _frame_host(rng, npics, mb_w, mb_h, filter_type, keyframe):
    """(per frame the buffers (Y, U, V, strengths), per frame the model's buffers, the strides) on the host"""
    sy, suv = 16 * mb_w + 4 * int(rng.integers(1, 9)), 8 * mb_w + 4 * int(rng.integers(1, 9))
    frames, wants = [], []
    for _ in range(npics):
        Y = rng.integers(0, 256, (16 * mb_h + 3, sy)).astype(np.uint8)  # stride padding and rows below: garbage that must stay
        U = rng.integers(0, 256, (8 * mb_h + 3, suv)).astype(np.uint8)
        V = rng.integers(0, 256, (8 * mb_h + 3, suv)).astype(np.uint8)
        Y[:16 * mb_h, :16 * mb_w] = _content(rng, 16 * mb_h, 16 * mb_w)
        U[:8 * mb_h, :8 * mb_w] = _content(rng, 8 * mb_h, 8 * mb_w)
        V[:8 * mb_h, :8 * mb_w] = _content(rng, 8 * mb_h, 8 * mb_w)
        st = _strengths(rng, mb_h, mb_w)
        w = [Y.copy(), U.copy(), V.copy()]
        M.loop_filter_frame(w[0], w[1], w[2], st, filter_type, keyframe)
        frames.append((Y, U, V, st))
        wants.append(w)
    return frames, wants, sy, suv


def _frames_to_device(torch, frames):
    """_frame_host()'s frames on the device: (the face's pictures, per frame the device planes, tensors to keep alive)"""
    hosts, pics, keep = [], [], []
    for Y, U, V, st in frames:
        d = [torch.from_numpy(a.copy()).cuda() for a in (Y, U, V)]
        ds = torch.from_numpy(st.view(np.uint8).reshape(-1).copy()).cuda()
        keep += d + [ds]
        pics.append((d[0], d[1], d[2], ds))
        hosts.append(d)
    return pics, hosts, keep


def _frame_upload(torch, rng, npics, mb_w, mb_h, filter_type, keyframe):
    """(the face's pictures, per frame the device planes, per frame the model's buffers, the strides, tensors to keep alive)"""
    frames, wants, sy, suv = _frame_host(rng, npics, mb_w, mb_h, filter_type, keyframe)
    pics, hosts, keep = _frames_to_device(torch, frames)
    return pics, hosts, wants, sy, suv, keep


def _frame_compare(hosts, wants):
    """whole buffers, stride padding and the rows below included"""
    for i, (d, w) in enumerate(zip(hosts, wants)):
        for p in range(3):
            g = d[p].cpu().numpy()
            if not np.array_equal(g, w[p]):
                bad = np.argwhere(g != w[p])
                raise AssertionError("frame %d plane %d: %d samples differ, first at %s" % (i, p, len(bad), bad[0]))


def _frame_case(torch, rng, npics, mb_w, mb_h, filter_type, keyframe, stream=None):
    pics, hosts, wants, sy, suv, keep = _frame_upload(torch, rng, npics, mb_w, mb_h, filter_type, keyframe)
    vp8.loopfilter_frames(pics, filter_type, keyframe, mb_w, mb_h, sy, suv, stream=stream)
    assert _lib.lib().ffhip_stream_synchronize(stream) == 0
    _frame_compare(hosts, wants)


@pytest.mark.parametrize("mb_w,mb_h", [(1, 1), (1, 23), (37, 1), (17, 9)])
@pytest.mark.parametrize("filter_type", [0, 1])
@pytest.mark.parametrize("keyframe", [0, 1])
def test_frame_filter_sizes(mb_w, mb_h, filter_type, keyframe):
    _frame_case(_torch(), np.random.default_rng(mb_w * 100 + mb_h + 7 * filter_type + 3 * keyframe), 1, mb_w, mb_h, filter_type, keyframe)


@pytest.mark.parametrize("filter_type,keyframe", [(0, 1), (1, 0)])
def test_frame_filter_1080p(filter_type, keyframe):
    _frame_case(_torch(), np.random.default_rng(1080 + filter_type), 1, 120, 68, filter_type, keyframe)


@pytest.mark.parametrize("npics", [3, 16, 17])
@pytest.mark.parametrize("filter_type", [0, 1])
def test_frame_filter_batches(npics, filter_type):
    _frame_case(_torch(), np.random.default_rng(500 + npics + filter_type), npics, 9, 5, filter_type, npics & 1)


def test_frame_filter_chains_the_members(dsp):
    """the frame face equals the per-call table run in filter_mb's order over the same frame (the decoder's C loop with our members)"""
    torch = _torch()
    rng = np.random.default_rng(77)
    mb_w, mb_h = 5, 4
    Y, U, V = _content(rng, 64, 80), _content(rng, 32, 40), _content(rng, 32, 40)
    st = _strengths(rng, mb_h, mb_w)
    y, u, v = Y.copy(), U.copy(), V.copy()
    for my in range(mb_h):
        for mx in range(mb_w):
            lv, il, inner = (int(st[k][my, mx]) for k in ("filter_level", "inner_limit", "inner_filter"))
            if not M.strength_ok(lv, il, inner):
                continue
            bE, H = 2 * lv + il, int(M.HEV_LUT[0][lv])
            pY, pU, pV = _p(y, 16 * my, 16 * mx), _p(u, 8 * my, 8 * mx), _p(v, 8 * my, 8 * mx)
            if mx:
                dsp.vp8_h_loop_filter16y(pY, 80, bE + 4, il, H)
                dsp.vp8_h_loop_filter8uv(pU, pV, 40, bE + 4, il, H)
            if inner:
                for k in (4, 8, 12):
                    dsp.vp8_h_loop_filter16y_inner(pY + k, 80, bE, il, H)
                dsp.vp8_h_loop_filter8uv_inner(pU + 4, pV + 4, 40, bE, il, H)
            if my:
                dsp.vp8_v_loop_filter16y(pY, 80, bE + 4, il, H)
                dsp.vp8_v_loop_filter8uv(pU, pV, 40, bE + 4, il, H)
            if inner:
                for k in (4, 8, 12):
                    dsp.vp8_v_loop_filter16y_inner(pY + 80 * k, 80, bE, il, H)
                dsp.vp8_v_loop_filter8uv_inner(pU + 160, pV + 160, 40, bE, il, H)
    d = [torch.from_numpy(a.copy()).cuda() for a in (Y, U, V)]
    vp8.loopfilter_frames([(d[0], d[1], d[2], torch.from_numpy(st.view(np.uint8).reshape(-1).copy()).cuda())], 0, 0, mb_w, mb_h, 80, 40)
    _sync()
    for g, w in zip(d, (y, u, v)):
        assert np.array_equal(g.cpu().numpy(), w)
