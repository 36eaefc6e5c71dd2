"""GPU tier of the HEVC in-loop filter matrix: hevc.loop_filter_batch, hevc.sao_batch and hevc.sao_restore_batch over the launches
of tests/hevc_lf_matrix.py — every route the batch kernels branch on x every decision cell — byte for byte against the oracle applied
record by record, over the WHOLE buffer (guards, stride padding and the bytes in front of an unaligned base included: a store that
leaves its footprint is a mismatch).  A failure names the first wrong segment or block with its route and labels.  The host faces
of ff_hevc_dsp_init_hip run one case per decision class with their pointers on every residue."""
import ctypes as C

import numpy as np
import pytest

import ffi
import hevc_lf_matrix as M
from ffi import i16p, i32p, ptr, u8p

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _dev(torch, a):
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    assert t.data_ptr() % 16 == 0                     # what hevc_lf_matrix.kernel_route assumes of the device base
    return t


def _back(t, like):
    return t.cpu().numpy().view(like.dtype).reshape(like.shape)


# ---------------------------------------------------------------------------------------------------------------------------
# deblocking
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", M.LF_GROUPS)
@pytest.mark.parametrize("bd", M.DEPTHS)
def test_lf_routes(bd, group):
    from ffmpeg_amd import hevc
    torch = _torch()
    launches = M.lf_launches(bd, group)
    # coverage, from the generator's tables
    luma_routes, chroma_routes = M.LF_GROUP_ROUTES[group]
    for route in luma_routes:
        assert M.lf_missing(launches, route, 0) == [], route
    for route in chroma_routes:
        assert M.lf_missing(launches, route, 1) == [], route
    if group == "counts":
        assert sorted({len(L.segs) for L in launches}) == M.COUNTS and len(launches) == 4 * len(M.COUNTS)
    for L in launches:
        n = len(L.segs)
        want = L.want_oracle()
        # the oracle moved every group that should move and left alone none, tc == 0 and no_p && no_q
        p0, p1 = L.plane(L.buf), L.plane(want)
        for i, s in enumerate(L.segs):
            assert M.kernel_route(L, i) == s.route
            for j, lab in enumerate(s.labels):
                r = L.group_region(i, j)
                if M.should_change(lab) is not None:
                    assert bool((p0[r] != p1[r]).any()) == M.should_change(lab), (L.name, i, j, lab)
        rec = np.zeros(n, hevc.EDGE_DTYPE)
        for i, s in enumerate(L.segs):
            rec[i]["offset"], rec[i]["kind"], rec[i]["beta"] = s.offset, (2 if s.spec.chroma else 0) + int(s.vertical), s.spec.beta8
            rec[i]["tc"], rec[i]["no_p"], rec[i]["no_q"] = s.spec.tc8, s.spec.no_p, s.spec.no_q
        d_buf = _dev(torch, L.buf)
        hevc.loop_filter_batch(d_buf[L.k * L.ps:], L.stride, torch.from_numpy(rec.view(np.uint8).reshape(n, 16).copy()).cuda(), n, bit_depth=bd)
        torch.cuda.synchronize()
        bad = L.first_bad(_back(d_buf, L.buf), want)
        assert bad is None, bad


def _aligned(nbytes, mod, align=8):
    """a zeroed byte array whose address is `mod` modulo `align`"""
    raw = np.zeros(nbytes + 2 * align, np.uint8)
    at = (mod - raw.ctypes.data) % align
    a = raw[at:at + nbytes]
    assert a.ctypes.data % align == mod
    return a


@pytest.mark.parametrize("bd", M.DEPTHS)
def test_lf_host_faces(bd):
    """hevc_{h,v}_loop_filter_{luma,chroma}: one segment per decision class, the host pix on every address modulo 8"""
    from ffmpeg_amd import hevc
    _torch()
    c = hevc.dsp_init(bd)
    O = ffi.oracle()
    ps = 1 if bd == 8 else 2
    dt = np.uint8 if bd == 8 else np.uint16
    rng = np.random.default_rng(900 + bd)
    names = ["hevc_h_loop_filter_luma", "hevc_v_loop_filter_luma", "hevc_h_loop_filter_chroma", "hevc_v_loop_filter_chroma"]
    luma = [s for s in M.luma_specs()[:10]] + M.luma_specs()[18:26:3]
    chroma = M.chroma_specs()[:5] + M.chroma_specs()[-10:]
    H, W = 24, 32                                                          # samples; the stride is a multiple of 8 bytes
    for which, name in enumerate(names):
        is_chroma, vertical = which >> 1, which & 1
        mods, modes = set(), set()
        for idx, spec in enumerate(chroma if is_chroma else luma):
            mod = (idx * ps) % 8
            lines = M.seg_lines(spec, bd, rng)
            _, labels = M.lf_model(lines, spec.chroma, bd, spec.beta8, spec.tc8, spec.no_p, spec.no_q)
            modes |= {(l.mode, l.skip, l.clip0, l.clipmax) for l in labels}
            a = _aligned(H * W * ps, 0)
            pa = a.view(dt).reshape(H, W)
            pa[:] = rng.integers(0, 1 << bd, (H, W))
            y, x = (8, 16 + mod // ps) if vertical else (12, 8 + mod // ps)
            M.LfLaunch._put(pa, vertical, y, x, lines)
            b = a.copy()
            off = (y * W + x) * ps
            assert (a.ctypes.data + off) % 8 == mod
            mods.add(mod)
            tc, no_p, no_q = np.array(spec.tc8, np.int32), np.array(spec.no_p, np.uint8), np.array(spec.no_q, np.uint8)
            fn = getattr(c, name + ("_c" if idx & 1 else ""))
            if is_chroma:
                fn(a.ctypes.data + off, W * ps, tc.ctypes.data, no_p.ctypes.data, no_q.ctypes.data)
            else:
                fn(a.ctypes.data + off, W * ps, spec.beta8, tc.ctypes.data, no_p.ctypes.data, no_q.ctypes.data)
            O.ffo_hevc_loop_filter_bd(bd, is_chroma, vertical, C.cast(b.ctypes.data + off, u8p), W * ps, spec.beta8, ptr(tc, i32p), ptr(no_p), ptr(no_q))
            assert np.array_equal(a, b), (name, idx, spec, labels)
        assert mods == set(range(0, 8, ps)), name
        if is_chroma:
            assert {m[2] for m in modes} == {False, True} and {m[3] for m in modes} == {False, True}
        else:
            assert {m[0] for m in modes} == set(M.LUMA_MODES) and {m[1] for m in modes} >= {"", "part"}
            assert any(m[2] for m in modes) and any(m[3] for m in modes)


# ---------------------------------------------------------------------------------------------------------------------------
# SAO
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bytewise", [0, 1], ids=["packed", "bytewise"])
@pytest.mark.parametrize("edge", [0, 1], ids=["band", "edge"])
@pytest.mark.parametrize("bd", M.DEPTHS)
def test_sao(bd, edge, bytewise):
    from ffmpeg_amd import hevc
    torch = _torch()
    launches = M.sao_launches(bd, edge, bytewise)
    assert M.sao_missing(launches[:2], bd, edge, bytewise) == []
    assert [len(L.blocks) for L in launches[2:]] == M.SAO_COUNTS
    for L in launches:
        n = len(L.blocks)
        want = L.want_oracle()
        ins = L.inside()
        assert (want[ins] != L.dst0[ins]).mean() > .5 and np.array_equal(want[~ins], L.dst0[~ins])
        rec = np.zeros(n, hevc.SAO_DTYPE)
        for i, b in enumerate(L.blocks):
            rec[i] = (L.dst_offset(i), L.src_offset(i), b.off, b.edge, b.cls, b.w, b.h, (0, 0))
        d_dst = _dev(torch, L.dst0)
        hevc.sao_batch(d_dst, L.sd * L.ps, _dev(torch, L.src), L.ss * L.ps, torch.from_numpy(rec.view(np.uint8).reshape(n, 24).copy()).cuda(), n,
                       bit_depth=bd)
        torch.cuda.synchronize()
        bad = L.first_bad(_back(d_dst, L.dst0), want)
        assert bad is None, bad


@pytest.mark.parametrize("bd", M.DEPTHS)
def test_sao_host_faces(bd):
    """sao_band_filter / sao_edge_filter with the host destination and source on every address modulo 4 (16 bits: every even one)"""
    from ffmpeg_amd import hevc
    _torch()
    c = hevc.dsp_init(bd)
    O = ffi.oracle()
    ps = 1 if bd == 8 else 2
    dt = np.uint8 if bd == 8 else np.uint16
    SS, SD = 192, 160                                                      # bytes; the edge filter's source stride is fixed
    for edge in (0, 1):
        L = M.sao_launches(bd, edge, 0)[0]
        picks = list(range(len(L.blocks) - 16, len(L.blocks)))             # the blocks whose content is built: classes and clips
        seen = set()
        for n, i in enumerate(picks):
            b = L.blocks[i]
            dm, sm = (n % 4, n // 4 % 4) if bd == 8 else (2 * (n % 2), 2 * (n // 2 % 2))
            seen.add((dm, sm))
            src = _aligned((b.h + 2) * SS + 8, sm, 4)
            (y, x) = L.spos[i]
            rows = src[:(b.h + 2) * SS].reshape(b.h + 2, SS)
            rows[:, :(b.w + 2) * ps] = np.ascontiguousarray(L.src[y - 1:y + b.h + 1, x - 1:x + b.w + 1]).view(np.uint8).reshape(b.h + 2, -1)
            sp = src.ctypes.data + SS + ps
            assert sp % 4 == (sm + ps) % 4
            a = _aligned(b.h * SD + 8, dm, 4)
            a[:] = np.arange(a.size) % 251
            w = a.copy()
            off = np.array(b.off, np.int16)
            idx = [0, 1, 2, 2, 3, 3, 4, 4][((b.w + 7) >> 3) - 1]
            if edge:
                c.sao_edge_filter[idx](a.ctypes.data, sp, SD, off.ctypes.data, b.cls, b.w, b.h)
                O.ffo_hevc_sao_edge_bd(bd, ptr(w), C.cast(sp, u8p), SD, SS, ptr(off, i16p), b.cls, b.w, b.h)
            else:
                c.sao_band_filter[idx](a.ctypes.data, sp, SD, SS, off.ctypes.data, b.cls, b.w, b.h)
                O.ffo_hevc_sao_band_bd(bd, ptr(w), C.cast(sp, u8p), SD, SS, ptr(off, i16p), b.cls, b.w, b.h)
            got = np.ascontiguousarray(a[:b.h * SD].reshape(b.h, SD)[:, :b.w * ps]).view(dt)
            assert np.array_equal(a, w), (edge, b, dm, sm)
            assert np.array_equal(got, L.model[i][0].astype(dt)), (edge, b)
        assert len(seen) == (16 if bd == 8 else 4)


# ---------------------------------------------------------------------------------------------------------------------------
# SAO restore
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", M.DEPTHS)
def test_sao_restore(bd):
    """launches of 1 and 5 records and of all, on 2 x 2, 2 x 64 and 64 x 2 blocks: the candidate columns and rows coincide"""
    from ffmpeg_amd import hevc
    torch = _torch()
    O = ffi.oracle()
    cases = M.restore_cases(bd)
    ps = 1 if bd == 8 else 2
    dt = np.uint8 if bd == 8 else np.uint16
    rng = np.random.default_rng(800 + bd)
    S, per_row = 80, 6
    W, H = per_row * S + 3, (len(cases) + per_row - 1) // per_row * S
    src = rng.integers(0, 1 << bd, (H, W)).astype(dt)
    dst0 = rng.integers(0, 1 << bd, (H, W + 2)).astype(dt)
    rec = np.zeros(len(cases), hevc.RESTORE_DTYPE)
    bits = lambda a: int(sum(int(bool(v)) << k for k, v in enumerate(a)))
    for i, (var, eo, off0, borders, w, h, ve, he, de) in enumerate(cases):
        y, x = i // per_row * S + 8, i % per_row * S + 8 + i % 4
        rec[i] = ((y * (W + 2) + x) * ps, (y * W + x) * ps, off0, w, h, eo, var, bits(borders), bits(ve), bits(he), bits(de), (0, 0))
    d_src = _dev(torch, src)
    changed = 0
    for lo, hi in [(0, 1), (1, 2), (2, 3), (3, 8), (8, 13), (0, len(cases))]:
        want = dst0.copy()
        for i in range(lo, hi):
            var, eo, off0, borders, w, h, ve, he, de = cases[i]
            O.ffo_hevc_sao_edge_restore_bd(bd, var, C.cast(want.ctypes.data + int(rec[i]["dst_offset"]), u8p),
                                           C.cast(src.ctypes.data + int(rec[i]["src_offset"]), u8p), (W + 2) * ps, W * ps, eo, off0, ptr(borders, i32p), w, h,
                                           ptr(ve), ptr(he), ptr(de))
        changed += int((want != dst0).sum())
        d_dst = _dev(torch, dst0)
        n = hi - lo
        hevc.sao_restore_batch(d_dst, (W + 2) * ps, d_src, W * ps, torch.from_numpy(rec[lo:hi].view(np.uint8).reshape(n, 20).copy()).cuda(), n,
                               bit_depth=bd)
        torch.cuda.synchronize()
        got = _back(d_dst, dst0)
        assert np.array_equal(got, want), (lo, hi, np.argwhere(got != want)[:5])
    assert changed > 100
