"""GPU tier of the bilateral motion search: ffhip_me_search_bilat_batch_dev and ffhip_me_search_bilat_sequence_dev == their host faces ==
the model, byte for byte, on the inputs of tests/test_me_bilat_search_cpu.py.  The kernels are the predictive searches' (one wave per
block row, hand-off between rows and pairs) with the bilateral cost as their cost policy; so beside the shapes there are runs with the
number of workgroups fixed, calls split into launches by pairs, a call continued by another on the same stream, and 1920 x 1080."""
import functools

import numpy as np
import pytest

import me_bilat_model as M
import test_me_bilat_search_cpu as B
from test_gpu_me_search import Guarded

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _sync(torch):
    from ffmpeg_amd import _lib
    assert _lib.lib().ffhip_stream_synchronize(None) == 0, _lib.lib().ffhip_last_error()
    torch.cuda.synchronize()


def pairs_dev(torch, method, A, Bp, w, h, mb, R, p1, p2):
    """the pair face on guarded buffers -> mv, cost; nothing outside the outputs may change, no hand-off may be lost"""
    from ffmpeg_amd import me
    nf, _, stride = A.shape
    per = (w // mb) * (h // mb)
    ga, gb = Guarded(torch, A), Guarded(torch, Bp)
    g1, g2 = (None if p is None else Guarded(torch, p) for p in (p1, p2))
    gm, gk = Guarded(torch, np.full((nf, per * 2), 0x5A5A, np.int16)), Guarded(torch, np.full((nf, per), 0x5A5A5A5A, np.uint32))
    me.search_bilat_batch(method, ga.t, gb.t, w, h, stride, h * stride, nf, mb, R, g1 and g1.t, g2 and g2.t, gm.t, gk.t)
    _sync(torch)
    assert ga.unchanged() and gb.unchanged() and gm.guards_intact() and gk.guards_intact()
    assert all(g is None or g.unchanged() for g in (g1, g2))
    return gm.host(), gk.host()


def sequence_dev(torch, method, pics, w, h, mb, R, i1, i2):
    """the sequence face on guarded buffers -> mv (np, nseq, b * 2), cost (np, nseq, b)"""
    from ffmpeg_amd import me
    nseq, nfr, _, stride = pics.shape
    per = (w // mb) * (h // mb)
    gp = Guarded(torch, pics)
    g1, g2 = (None if p is None else Guarded(torch, p) for p in (i1, i2))
    gm, gk = Guarded(torch, np.full((nfr - 1, nseq, per * 2), 0x5A5A, np.int16)), Guarded(torch, np.full((nfr - 1, nseq, per), 0x5A5A5A5A, np.uint32))
    me.search_bilat_sequence(method, gp.t, w, h, stride, h * stride, nfr, nfr * h * stride, nseq, mb, R, g1 and g1.t, g2 and g2.t, gm.t, gk.t)
    _sync(torch)
    assert gp.unchanged() and gm.guards_intact() and gk.guards_intact() and all(g is None or g.unchanged() for g in (g1, g2))
    return gm.host(), gk.host()


@pytest.mark.parametrize("big_r", (False, True), ids=["R=mb", "R=32"])
@pytest.mark.parametrize("shape", B.SHAPES, ids=["2x2", "6x5", "4x3+3"])
@pytest.mark.parametrize("mb", (8, 16))
def test_pair_face_equals_host_equals_model(mb, shape, big_r):
    torch = _torch()
    R = B.search_params(mb)[big_r]
    pics, fields = B.sequences(*shape, mb)
    w, h, _ = B.geometry(*shape, mb)
    A, Bp = np.ascontiguousarray(pics[:, 0]), np.ascontiguousarray(pics[:, 1])
    for method in B.METHODS:
        for prev in B.PREVS:
            wmv, wcost, _ = B.pair_reference(method, shape, mb, R, prev)
            hmv, hcost, _ = B.host_pairs(method, A, Bp, w, h, mb, R, *fields[prev])
            mv, cost = pairs_dev(torch, method, A, Bp, w, h, mb, R, *fields[prev])
            what = (M.NAMES[method], prev)
            assert np.array_equal(cost, hcost) and np.array_equal(mv, hmv), what
            assert np.array_equal(cost, wcost) and np.array_equal(mv, wmv), what


@pytest.mark.parametrize("nseq", (1, 3))
@pytest.mark.parametrize("mb,shape", [(8, B.SHAPES[2]), (16, B.SHAPES[1]), (16, B.SHAPES[0])], ids=["mb8-4x3+3", "mb16-6x5", "mb16-2x2"])
def test_sequence_face_equals_host_equals_model(mb, shape, nseq):
    torch = _torch()
    pics, fields = B.sequences(*shape, mb)
    w, h, _ = B.geometry(*shape, mb)
    sub = np.ascontiguousarray(pics[:nseq])
    for method in B.METHODS:
        for prev in ("none", "any"):
            i1, i2 = (None if f is None else f[:nseq] for f in fields[prev])
            wmv, wcost, _ = B.sequence_reference(method, shape, mb, 32, prev)
            mv, cost = sequence_dev(torch, method, sub, w, h, mb, 32, i1, i2)
            assert np.array_equal(cost, wcost[:, :nseq]) and np.array_equal(mv, wmv[:, :nseq]), (M.NAMES[method], prev)


@pytest.mark.parametrize("v", [(1, 0), (2, 1), (-3, 2)])
def test_found_motion(v):
    torch = _torch()
    A, Bp, _ = B.found_pictures(v)
    w, h = B.BW * B.MB, B.BH * B.MB
    for method in B.METHODS:
        hmv, hcost, _ = B.host_pairs(method, A[None], Bp[None], w, h, B.MB, B.RR, None, None)
        mv, cost = pairs_dev(torch, method, A[None], Bp[None], w, h, B.MB, B.RR, None, None)
        assert np.array_equal(mv, hmv) and np.array_equal(cost, hcost)
        field = mv.reshape(B.BH, B.BW, 2)
        for by in range(1, B.BH - 1):
            for bx in range(1, B.BW - 1):
                X, Y = int(field[by, bx, 0]), int(field[by, bx, 1])
                assert (X - bx * B.MB, Y - by * B.MB) == v
                assert M.sbad(A, Bp, w, h, B.MB, B.RR, bx * B.MB, by * B.MB, X, Y) == 0


@pytest.mark.parametrize("wgs", ["1", "3"])
@pytest.mark.parametrize("mb,shape", [(16, B.SHAPES[1]), (8, B.SHAPES[2])], ids=["mb16-6x5", "mb8-4x3+3"])
def test_ticket_rounds(mb, shape, wgs, monkeypatch):
    """on one wave every awaited unit is finished before the next begins; three waves leave the units they await to each other"""
    torch = _torch()
    monkeypatch.setenv("FFHIP_ME_PRED_WGS", wgs)
    pics, fields = B.sequences(*shape, mb)
    w, h, _ = B.geometry(*shape, mb)
    for method in B.METHODS:
        wmv, wcost, _ = B.pair_reference(method, shape, mb, 32, "made")
        mv, cost = pairs_dev(torch, method, np.ascontiguousarray(pics[:, 0]), np.ascontiguousarray(pics[:, 1]), w, h, mb, 32, *fields["made"])
        assert np.array_equal(cost, wcost) and np.array_equal(mv, wmv)
        smv, scost, _ = B.sequence_reference(method, shape, mb, 32, "made")
        mv, cost = sequence_dev(torch, method, pics, w, h, mb, 32, *fields["made"])
        assert np.array_equal(cost, scost) and np.array_equal(mv, smv)


@pytest.mark.parametrize("mb,shape", [(16, B.SHAPES[1]), (8, B.SHAPES[2])], ids=["mb16-6x5", "mb8-4x3+3"])
def test_the_variant_without_the_early_pass_gives_the_same_bytes(mb, shape, monkeypatch):
    """the measurement build's FFHIP_ME_BILAT_NO_EARLY runs EPZS's predictor list in order behind the wait (docs/EXPERIMENTS.md)"""
    torch = _torch()
    monkeypatch.setenv("FFHIP_ME_BILAT_NO_EARLY", "1")
    pics, fields = B.sequences(*shape, mb)
    w, h, _ = B.geometry(*shape, mb)
    for prev in ("made", "any"):
        smv, scost, _ = B.sequence_reference(M.EPZS, shape, mb, 32, prev)
        mv, cost = sequence_dev(torch, M.EPZS, pics, w, h, mb, 32, *fields[prev])
        assert np.array_equal(cost, scost) and np.array_equal(mv, smv), prev


@functools.lru_cache(maxsize=None)
def _long(nseq, n):
    """n pictures of 16 x 16 per sequence (2 x 2 blocks of 8): a noise patch that shifts from picture to picture"""
    rng = np.random.default_rng(4100 + nseq)
    base = rng.integers(0, 256, (nseq, 32, 32), dtype=np.uint8)
    pics = np.zeros((nseq, n, 16, 16), np.uint8)
    for s in range(nseq):
        x = y = 8
        for p in range(n):
            x, y = min(max(x + int(rng.integers(-2, 3)), 0), 16), min(max(y + int(rng.integers(-2, 3)), 0), 16)
            pics[s, p] = base[s, y:y + 16, x:x + 16]
    pics.setflags(write=False)
    return pics


def test_a_pair_call_split_into_launches():
    """2 x 2 blocks have 2 block rows: 4095 pairs fill a progress-pool slot, so 4100 pairs are two launches"""
    torch = _torch()
    pics = _long(1, 4101)[0]
    A, Bp = np.ascontiguousarray(pics[:-1]), np.ascontiguousarray(pics[1:])
    for method in B.METHODS:
        hmv, hcost, _ = B.host_pairs(method, A, Bp, 16, 16, 8, 8, None, None)
        mv, cost = pairs_dev(torch, method, A, Bp, 16, 16, 8, 8, None, None)
        assert np.array_equal(cost, hcost) and np.array_equal(mv, hmv)


@pytest.mark.parametrize("nseq,n", [(1, 4101), (3, 1400)])
def test_a_sequence_call_split_at_a_pair_boundary(nseq, n):
    """one sequence: 4095 pairs per launch, the second launch reads the first's fields plainly; three: 1365 pairs per launch"""
    torch = _torch()
    pics = _long(nseq, n)
    for method in B.METHODS:
        hmv, hcost, _ = B.host_sequence(method, pics, 16, 16, 8, 8, None, None)
        mv, cost = sequence_dev(torch, method, pics, 16, 16, 8, 8, None, None)
        assert np.array_equal(cost, hcost) and np.array_equal(mv, hmv)


@pytest.mark.parametrize("method", B.METHODS, ids=B.IDS)
def test_a_call_continues_the_one_before_on_one_stream(method):
    """3 + 2 pictures queued on one stream without a synchronisation in between, the second call's starting fields the first call's two
    steps where it wrote them, == one call of 4"""
    from ffmpeg_amd import me
    torch = _torch()
    shape, mb, R = B.SHAPES[1], 16, 32
    pics, fields = B.sequences(*shape, mb)
    w, h, stride = B.geometry(*shape, mb)
    per, plane = shape[0] * shape[1], h * stride
    i1, i2 = fields["made"]
    wmv, wcost, _ = B.sequence_reference(method, shape, mb, R, "made")
    gp, g1, g2 = Guarded(torch, pics), Guarded(torch, i1), Guarded(torch, i2)
    gm = Guarded(torch, np.full((B.NFRAMES - 1, B.NSEQ, per * 2), 0x5A5A, np.int16))
    gk = Guarded(torch, np.full((B.NFRAMES - 1, B.NSEQ, per), 0x5A5A5A5A, np.uint32))
    step = lambda g, k: g.t[k * B.NSEQ * per * 4:]
    me.search_bilat_sequence(method, gp.t, w, h, stride, plane, 3, B.NFRAMES * plane, B.NSEQ, mb, R, g1.t, g2.t, gm.t, gk.t)
    me.search_bilat_sequence(method, gp.t[2 * plane:], w, h, stride, plane, 2, B.NFRAMES * plane, B.NSEQ, mb, R, step(gm, 1), step(gm, 0), step(gm, 2),
                             step(gk, 2))
    _sync(torch)
    assert gp.unchanged() and g1.unchanged() and g2.unchanged() and gm.guards_intact() and gk.guards_intact()
    assert np.array_equal(gk.host(), wcost) and np.array_equal(gm.host(), wmv)


@functools.lru_cache(maxsize=None)
def _hd_pair():
    rng = np.random.default_rng(1080)
    big = B.texture(rng, 1080 + 32, 1920 + 32)
    A, Bp = B.moved(big, 16, 1920, 1080, 1920, (3, -2))
    noise = rng.integers(-2, 3, (2, 1080, 1920))
    A, Bp = (np.clip(p.astype(np.int64) + n, 0, 255).astype(np.uint8) for p, n in zip((A, Bp), noise))
    return A[None], Bp[None]


@pytest.mark.parametrize("method", B.METHODS, ids=B.IDS)
def test_1080p_against_the_host_face(method):
    """120 x 67 blocks: 67 waves in flight, each two blocks behind the row above"""
    torch = _torch()
    A, Bp = _hd_pair()
    hmv, hcost, _ = B.host_pairs(method, A, Bp, 1920, 1080, 16, 16, None, None)
    mv, cost = pairs_dev(torch, method, A, Bp, 1920, 1080, 16, 16, None, None)
    assert np.array_equal(cost, hcost) and np.array_equal(mv, hmv)
