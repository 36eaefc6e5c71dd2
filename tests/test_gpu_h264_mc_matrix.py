"""GPU tier of H.264's motion-compensation matrix: h264.qpel_batch and h264.chroma_mc_batch (and their _hbd faces) over the cell
lists of tests/h264_mc_matrix.py — every size, position, put / avg, source alignment modulo 16, destination alignment modulo 4, the
groups of four that do and do not leave as a tile, the picture-edge ladders — byte for byte against the oracle over the WHOLE
destination buffer (a store that leaves its block is a mismatch), on every kernel ffhip_launch_h264_qpel can pick, and once more
on a source whose samples outside the probed footprints (edge lists: outside the picture) are complemented.  A failure names the
first wrong cell (H264Batch.first_bad).

A list's samples, records and oracle output are made once per (list, stride, depth) and shared by the routes that run on it."""
import functools

import numpy as np
import pytest

import h264_mc_matrix as H

pytestmark = pytest.mark.gpu

S16, S4, SODD = 2048, 2052, 2051       # luma strides: whole 16 bytes; whole dwords, 4 modulo 16; odd
C4, CODD = 1024, 1021                  # chroma strides

#: route -> (stride, records: None = the whole list of 16397, knobs).  What ffhip_launch_h264_qpel (kernels/h264_qpel.hip) picks:
#:   first branch   stride % 16 == 0 and none of FFHIP_QPEL_M=0, _OLD=1, _W=0: k_h264_qpel_mp if _PIPE=1, else k_h264_qpel_m<NG>
#:                  (FFHIP_QPEL_NG, 1 without the knob); FFHIP_QPEL_XCD=0 numbers the workgroups in launch order
#:   second         stride % 16 == 0, n >= 1024, neither _OLD=1 nor _W=0: k_h264_qpel_t (reached with FFHIP_QPEL_M=0)
#:   third          stride % 4 == 0, not _OLD=1: k_h264_qpel_l<4> if n >= 16384, <2> if n >= 8192, else <1>
#:   else           k_h264_qpel
ROUTES = {
    "m1":              (S16, None, {}),                            # no knob, 2048: first branch, k_h264_qpel_m<1>
    "m2":              (S16, None, {"FFHIP_QPEL_NG": "2"}),        # first branch, k_h264_qpel_m<2>
    "m4":              (S16, None, {"FFHIP_QPEL_NG": "4"}),        # first branch, k_h264_qpel_m<4>
    "mp":              (S16, None, {"FFHIP_QPEL_PIPE": "1"}),      # first branch, k_h264_qpel_mp
    "m1-launch-order": (S16, None, {"FFHIP_QPEL_XCD": "0"}),       # k_h264_qpel_m<1>, per_xcd = 0
    "t":               (S16, None, {"FFHIP_QPEL_M": "0"}),         # first branch refused, 16397 >= 1024: k_h264_qpel_t
    "l1-below-t":      (S16, 1023, {"FFHIP_QPEL_M": "0"}),         # 1023 < 1024: falls through to k_h264_qpel_l<1>
    "l4-nowindow":     (S16, None, {"FFHIP_QPEL_W": "0"}),         # first and second refused, 16397 >= 16384: k_h264_qpel_l<4>
    "regs-old":        (S16, None, {"FFHIP_QPEL_OLD": "1"}),       # every branch but the last refused: k_h264_qpel
    "l4":              (S4, None, {}),                             # no knob, 2052 = 4 mod 16, 16397 >= 16384: k_h264_qpel_l<4>
    "l2":              (S4, 8193, {}),                             # 8192 <= 8193 < 16384: k_h264_qpel_l<2>, the last wave holds one record
    "l1":              (S4, 1023, {}),                             # 1023 < 8192: k_h264_qpel_l<1>
    "regs":            (SODD, None, {}),                           # no knob, odd stride: k_h264_qpel
}
TAILS = [1, 2, 3, 5, 63, 65, 1025]
#: the edge lists (13500 records): the same branches; at 2052, 8192 <= 13500 < 16384 picks k_h264_qpel_l<2>
EDGE_ROUTES = {"m1": ROUTES["m1"], "mp": ROUTES["mp"], "t": ROUTES["t"], "l2": ROUTES["l4"], "regs": ROUTES["regs"]}


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _back(t, like):
    return t.cpu().numpy().view(like.dtype).reshape(like.shape)


class _Case:
    """one list laid out, its sample planes, records and the oracle's output (read-only: shared between tests)"""


@functools.lru_cache(maxsize=4)
def _case(kind, stride, bd):
    c = _Case()
    c.b = b = H.lay_out(kind, stride)
    seed = 1000 * bd + stride + len(kind)
    c.bd, c.src, c.dst0 = bd, b.source(bd, seed), b.destination(bd, seed + 1)
    c.want = b.want(bd, c.src, c.dst0)
    rec = b.records(c.src.itemsize)
    c.rec = rec.view(np.uint8).reshape(len(rec), rec.itemsize).copy()
    for a in (c.src, c.dst0, c.want, c.rec):
        a.setflags(write=False)
    # not vacuous: the oracle changed most samples of the blocks and nothing else; both clips fire
    ins = b.inside()
    assert (c.want[ins] != c.dst0[ins]).mean() > .5
    assert np.array_equal(c.want[~ins], c.dst0[~ins])
    assert (c.want[ins] == 0).any() and (c.want[ins] == (1 << bd) - 1).any()
    return c


@functools.lru_cache(maxsize=1)
def _poisoned(kind, stride, bd):
    c = _case(kind, stride, bd)
    p = c.b.poisoned(c.src, bd)
    p.setflags(write=False)
    return p


def _run(c, src, first=0, n=None):
    """records first .. first + n - 1 through the batch face of the case's depth: 8 bits the product faces, above the _hbd ones
    (offsets and strides in bytes); edge lists through the _pic forms"""
    from ffmpeg_amd import _lib, h264
    torch = _torch()
    b, ps = c.b, c.src.itemsize
    n = len(b.cells) - first if n is None else n
    d_dst, d_src, d_rec = _dev(torch, c.dst0), _dev(torch, src), torch.from_numpy(c.rec[first:first + n].copy()).cuda()
    pic = b.pic if isinstance(b, H.EdgeBatch) else None
    if c.bd == 8:
        (h264.chroma_mc_batch if b.chroma else h264.qpel_batch)(d_dst, d_src, b.stride, d_rec, n, pic=pic)
    else:
        L = _lib.lib()
        name = "ffhip_h264_%s_batch_dev_hbd" % ("chroma_mc" if b.chroma else "qpel")
        if pic:
            r = getattr(L, name + "_pic")(c.bd, d_dst.data_ptr(), d_src.data_ptr(), b.stride * ps, pic[0], pic[1], d_rec.data_ptr(), n, None)
        else:
            r = getattr(L, name)(c.bd, d_dst.data_ptr(), d_src.data_ptr(), b.stride * ps, d_rec.data_ptr(), n, None)
        _lib.check(r, name)
    torch.cuda.synchronize()
    return _back(d_dst, c.dst0)


def _knobs(monkeypatch, knobs):
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)      # tests/conftest.py: the first FFHIP_* knob switches to the measure build


# ---------------------------------------------------------------------------------------------------------------------------
# luma
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", list(ROUTES))
def test_luma_matrix(route, monkeypatch):
    """the whole list (16397 records: the cross product, the group family, one last record), or a prefix of it, on every kernel of
    ffhip_launch_h264_qpel: ROUTES states each case's stride, n and knob and the branch they select.  16397 = 4 * 4099 + 1 =
    16 * 1024 + 13: the last group of four holds one record (min(b0 + k, n - 1) in every kernel that takes several per wave), the
    last workgroup is not full, and the XCD renumbering (8 * ceil(1025 / 8) = 1032 workgroups) leaves seven empty"""
    stride, n, knobs = ROUTES[route]
    _knobs(monkeypatch, knobs)
    c = _case("luma", stride, 8)
    want = c.want if n is None else c.b.want(8, c.src, c.dst0, 0, n)
    bad = c.b.first_bad(_run(c, c.src, 0, n), want)
    assert bad is None, bad


@pytest.mark.parametrize("n", TAILS)
@pytest.mark.parametrize("route", ["m1", "m2", "m4", "mp", "t"])
def test_luma_tails(route, n, monkeypatch):
    """prefixes of the GROUP family (records 6144 .. 6144 + n - 1; its first groups are all tile candidates) that cut the group of
    four and the workgroup: tile must turn false for the cut group, and records past n must not be stored (min(b0 + k, n - 1) reads
    the last record again).  stride 2048: k_h264_qpel_m<1>, <2>, <4>, _mp by the knobs of ROUTES; n = 1: eight workgroups launched,
    seven empty; 1025: 72 launched, 65 used.  With FFHIP_QPEL_M=0 only 1025 >= 1024 reaches k_h264_qpel_t (n % 4 == 1 there); the
    shorter prefixes run k_h264_qpel_l<1>, as the launcher has it"""
    stride, whole, knobs = ROUTES[route]
    assert whole is None
    _knobs(monkeypatch, knobs)
    c = _case("luma", stride, 8)
    assert H.tile_candidate(c.b.cells[H.N_CROSS + n - n % 4:H.N_CROSS + n - n % 4 + 4])
    want = c.b.want(8, c.src, c.dst0, H.N_CROSS, n)
    bad = c.b.first_bad(_run(c, c.src, H.N_CROSS, n), want)
    assert bad is None, bad


@pytest.mark.parametrize("route", ["m1", "t", "l4"])
def test_luma_poison(route, monkeypatch):
    """k_h264_qpel_m<1> (which since round 6 leaves out the chunks and rows a position does not read), k_h264_qpel_t and
    k_h264_qpel_l<4> (which load the whole 21 x 21 window whatever the position): nothing outside a position's probed footprint —
    for H + V a cross — reaches its samples.  The documented over-reads (aligned 16-byte chunks, whole dwords) land in the slack"""
    stride, n, knobs = ROUTES[route]
    _knobs(monkeypatch, knobs)
    c = _case("luma", stride, 8)
    poisoned = _poisoned("luma", stride, 8)
    assert (poisoned != c.src).mean() > .3
    first, second = _run(c, c.src), _run(c, poisoned)
    bad = c.b.first_bad(first, c.want)
    assert bad is None, bad
    bad = c.b.first_bad(second, first)
    assert bad is None, "poisoned source: " + bad


@pytest.mark.parametrize("route", list(EDGE_ROUTES))
def test_luma_edges(route, monkeypatch):
    """FFHIP_MC_EMU through qpel_batch(..., pic=(48, 32)): every size x mcxy x rung pair of the two ladders, unflagged interior
    records in between, on the clamped-load path of k_h264_qpel_m<1>, _mp, _t, _l<2> (13500 records at stride 2052) and k_h264_qpel;
    then again with everything outside the picture complemented: include/ffhip.h promises that flagged records touch only samples
    inside the picture, and the unflagged ones' windows lie inside it"""
    stride, n, knobs = EDGE_ROUTES[route]
    _knobs(monkeypatch, knobs)
    c = _case("luma_edge", stride, 8)
    assert 8192 <= len(c.b.cells) < 16384
    first = _run(c, c.src)
    bad = c.b.first_bad(first, c.want)
    assert bad is None, bad
    bad = c.b.first_bad(_run(c, c.b.poisoned(c.src, 8)), first)
    assert bad is None, "surroundings of the picture complemented: " + bad


# ---------------------------------------------------------------------------------------------------------------------------
# chroma
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [C4, CODD])
def test_chroma_matrix(stride):
    """k_h264_chroma_mc: every width x height x class x source address modulo 4 x destination address modulo 4 x put / avg and every
    (x, y); on a dword stride a block's rows keep its alignment (the dword-store branch on every row, or on none), on an odd one
    they take all four in turn.  Then the poisoned source: cm_row's dwords bring bytes the reference does not read, no more"""
    c = _case("chroma", stride, 8)
    first = _run(c, c.src)
    bad = c.b.first_bad(first, c.want)
    assert bad is None, bad
    poisoned = c.b.poisoned(c.src, 8)
    assert (poisoned != c.src).mean() > .3
    bad = c.b.first_bad(_run(c, poisoned), first)
    assert bad is None, "poisoned source: " + bad


@pytest.mark.parametrize("stride", [C4, CODD])
def test_chroma_edges(stride):
    """FFHIP_MC_EMU through chroma_mc_batch(..., pic=(24, 16)): cm_row_emu on the ladders, and the surroundings complemented"""
    c = _case("chroma_edge", stride, 8)
    first = _run(c, c.src)
    bad = c.b.first_bad(first, c.want)
    assert bad is None, bad
    bad = c.b.first_bad(_run(c, c.b.poisoned(c.src, 8)), first)
    assert bad is None, "surroundings of the picture complemented: " + bad


# ---------------------------------------------------------------------------------------------------------------------------
# above 8 bits: one sample per lane (k_h264_qpel_hbd, k_h264_chroma_mc_hbd), one route each
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", [10, 14])
@pytest.mark.parametrize("kind,stride", [("luma", SODD), ("chroma", CODD), ("luma_edge", SODD), ("chroma_edge", CODD)])
def test_hbd(kind, stride, bd):
    """the same lists on 16-bit samples through the _hbd faces (edge lists: _hbd_pic) against the _bd oracle: offsets and strides in
    bytes, the content classes at the depth's maximum"""
    c = _case(kind, stride, bd)
    assert c.src.dtype == np.uint16 and c.src.max() == (1 << bd) - 1
    bad = c.b.first_bad(_run(c, c.src), c.want)
    assert bad is None, bad
