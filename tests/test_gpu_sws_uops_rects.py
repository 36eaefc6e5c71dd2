"""SwsOpBackend `hip` (csrc/sws_uops.hip) on the paths of the generated kernel that production runs on every frame and whole-picture
calls from line 0 never reach: rectangles that start off a thread's vector (`body<FULL, false>`: the scalar dither columns, filter
weights and offsets taken from an `xabs` that is no vector multiple), slices that start below line 0 (`yabs`: the dither row, the
vertical filter's weight row, `rowtab` built from `in_bump_y[y_start + r]`), several lines per thread (the `rr` loop recomputing
plane pointers, `skip` and `yabs`), device planes at any naturally aligned address, and more tables on one handle than it keeps.

The expectation is backend_c's committed whole-picture output (tests/golden/sws_uops.npz), reached rectangle by rectangle — which
tests/test_sws_uops_rects_cpu.py shows the oracle to reproduce byte for byte with the same SwsOpExecs — and the oracle itself for
random pictures and for the hand-built 4-bit / 1-bit lists.  Every comparison is byte-exact (floats bit for bit, NaNs one value);
destinations hold 0x5A beforehand and everything no rectangle covers, line padding and the bytes around the planes included, must
still hold it."""
import ctypes as C
import os

import numpy as np
import pytest

import ffi
import swsops as S

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "sws_uops.npz")


def _oracle():
    return S.declare(ffi.oracle(), "ffo_sws_uops_")


class Hip:
    """libffhip's two faces on Bufs: device copies for ffhip_sws_uops_run_dev, the Bufs themselves for ffhip_sws_uops_func"""

    def __init__(self):
        from ffmpeg_amd import _lib as m
        self.L = m.lib()
        self.g = S.declare(self.L, "ffhip_sws_uops_")

    def compile(self, lst):
        h = C.c_void_p()
        r = self.g("compile")(lst.uops, lst.n, C.byref(h))
        assert r == 0, (r, self.L.ffhip_last_error())
        return h, self.g("block_size")(h)

    def free(self, h):
        self.g("free")(C.byref(h))

    def upload(self, bufs):
        import torch
        ts = [torch.from_numpy(b.flat.copy()).cuda() for b in bufs]
        return ts, [t.data_ptr() + b.off for t, b in zip(ts, bufs)]

    def download(self, ts):
        assert self.L.ffhip_stream_synchronize(None) == 0
        return [t.cpu().numpy() for t in ts]

    def run_dev(self, h, e, r, sb, db, nframes=1):
        ip = (C.c_ssize_t * 4)(*([b.fpitch for b in sb] + [0] * (4 - len(sb))))
        op = (C.c_ssize_t * 4)(*([b.fpitch for b in db] + [0] * (4 - len(db))))
        rc = self.L.ffhip_sws_uops_run_dev(h, C.byref(e), r[0], r[1], r[2], r[3], nframes, ip, op, None)
        assert rc == 0, (rc, self.L.ffhip_last_error())

    def func(self, h, e, r):
        self.g("func")(C.byref(e), h, *r)

    def fallbacks(self):
        return self.L.ffhip_shim_fallbacks()


def _hip():
    return Hip()


def _cases():
    return S.rect_cases(GOLDEN, _oracle())


_batches = {}


def _batch(case):
    """3 pictures of a case's source (the fixture's, two random ones) and the destination planes they must give; built once"""
    if case.name not in _batches:
        sb, _ = case.bufs(frames=3)
        case.randomise(np.random.default_rng(len(_batches) + 50), sb, (1, 2))
        want = S.oracle_pictures(_oracle(), case, sb, (1, 2))
        want[0] = case.want
        for b in sb:
            b.flat.setflags(write=False)
        _batches[case.name] = (sb, want)
    return _batches[case.name]


def check_planes(errs, case, db, flats, want, what):
    """`want`: {picture: planes}; the pictures of `db` that are not in it were in no call"""
    for i, (b, f) in enumerate(zip(db, flats)):
        for pic, planes in want.items():
            if not S.same_bytes(b.payload(pic, f), planes[i], case.f32):
                errs.append((case.name, what, "picture %d plane %d: %d bytes differ" % (pic, i, int((b.payload(pic, f) != planes[i]).sum()))))
        idle = np.zeros((b.frames, b.lines, b.rows), bool)
        idle[[p for p in range(b.frames) if p not in want]] = True
        if not b.outside_kept(f, but=idle):
            errs.append((case.name, what, "plane %d: bytes outside the rectangles were written" % i))


@pytest.mark.parametrize("nframes", (1, 3))
@pytest.mark.parametrize("tiling", (0, 1))
def test_device_face_by_rectangles(tiling, nframes):
    """a. one ffhip_sws_uops_run_dev per rectangle on device-resident planes: x cuts off the vector (columns 1 and 3, an odd middle
    block; 2 and 6 for the 4-bit lists), y cuts {0, 1, 3, H} / {0, 2, H - 1, H}; with 3 pictures per call (frame pitches) the second
    and third are random and the oracle's"""
    dev = _hip()
    errs = []
    for case in _cases():
        h, bs = dev.compile(case.lst)
        sb, want = _batch(case)
        want = {f: want[f] for f in range(nframes)}
        _, db = case.bufs(frames=3)
        ts, sa = dev.upload(sb)
        td, da = dev.upload(db)
        S.run_rects(lambda e, *r: dev.run_dev(h, e, r, sb, db, nframes), case, bs, sb, sa, db, da, S.tilings(case.w, case.h, bs)[tiling])
        check_planes(errs, case, db, dev.download(td), want, "tiling %d, %d pictures" % (tiling, nframes))
        if not all(np.array_equal(a, b.flat) for a, b in zip(dev.download(ts), sb)):
            errs.append((case.name, "the source was written"))
        dev.free(h)
    assert not errs, errs


@pytest.mark.parametrize("tiling", (0, 1))
def test_host_face_by_rectangles(tiling):
    """b. the same rectangles through ffhip_sws_uops_func on host arrays, as the slices of a threaded sws_scale_frame arrive; every
    call is answered by the device"""
    dev = _hip()
    before = dev.fallbacks()
    errs = []
    for case in _cases():
        h, bs = dev.compile(case.lst)
        sb, db = case.bufs()
        S.run_rects(lambda e, *r: dev.func(h, e, r), case, bs, sb, [b.flat.ctypes.data + b.off for b in sb], db,
                    [b.flat.ctypes.data + b.off for b in db], S.tilings(case.w, case.h, bs)[tiling])
        check_planes(errs, case, db, [b.flat for b in db], {0: case.want}, "tiling %d" % tiling)
        dev.free(h)
    assert not errs, errs
    assert dev.fallbacks() == before, "the host face answered through its fallback"


@pytest.mark.parametrize("k", (1, 3))
def test_device_planes_at_any_address(k):
    """c. whole pictures on device planes whose bases are k elements of their own type past an aligned address (u8: 1 and 3 bytes,
    u16: 2 and 6, f32: 4 and 12 — natural alignment is what the C backend itself needs, no more is assumed), line pitches of row
    bytes + 7 rounded up to the element: the committed output, and the bytes before, between and after the lines still the fill"""
    dev = _hip()
    errs = []
    for case in _cases():
        h, bs = dev.compile(case.lst)
        sb, db = case.bufs(src_off=k, dst_off=k, tight=True)
        ts, sa = dev.upload(sb)
        td, da = dev.upload(db)
        es, ed = S.SIZE[case.lst.read.type], S.SIZE[case.lst.write.type]
        assert all(a % es == 0 and a % (4 * es) for a in sa) and all(a % ed == 0 and a % (4 * ed) for a in da)
        S.run_rects(lambda e, *r: dev.run_dev(h, e, r, sb, db), case, bs, sb, sa, db, da, [(0, case.w, 0, case.h)])
        check_planes(errs, case, db, dev.download(td), {0: case.want}, "planes moved by %d elements" % k)
        dev.free(h)
    assert not errs, errs


def _frames_for(V, npx, ny, rows):
    """the smallest number of pictures with which the launch walks `rows` lines per thread"""
    from test_sws_uops_rects_cpu import shape
    nf = 1
    while shape(V, npx, ny, nf)[3] != rows:
        nf += 1
        assert nf <= 1 << 16, "no picture count gives %d lines per thread" % rows
    return nf


def _many_pictures(dev, case, rows, seed):
    """`case` on as many distinct random pictures as make the launch walk `rows` lines per thread: every picture and all padding
    against the oracle, called once per picture"""
    nf = _frames_for(4, case.w, case.h, rows)
    from test_sws_uops_rects_cpu import shape
    gx, gy, gz, got = shape(4, case.w, case.h, nf)
    assert got == rows and gz == nf and (rows == 1 or case.h > 4 * gy), (nf, gx, gy, gz, got)     # the line loop runs again
    sb, db = case.bufs(frames=nf)
    case.randomise(np.random.default_rng(seed), sb, range(nf))
    want = [S.Buf(b.rows, b.lines, nf, fill=S.FILL) for b in db]
    S.oracle_into(_oracle(), case, sb, want, range(nf))
    h, bs = dev.compile(case.lst)
    assert bs == 1
    ts, sa = dev.upload(sb)
    td, da = dev.upload(db)
    S.run_rects(lambda e, *r: dev.run_dev(h, e, r, sb, db, nf), case, bs, sb, sa, db, da, [(0, case.w, 0, case.h)])
    flats = dev.download(td)
    dev.free(h)
    for i, (f, w) in enumerate(zip(flats, want)):
        bad = np.flatnonzero(f != w.flat)
        assert not bad.size, (case.name, "%d lines per thread, %d pictures, plane %d: %d bytes differ, the first in picture %d, line %d"
                              % (rows, nf, i, bad.size, (bad[0] - w.off) // w.fpitch, (bad[0] - w.off) % w.fpitch // w.pitch))


def _named(name):
    return [c for c in _cases() if c.name == name][0]


@pytest.mark.parametrize("rows", (8, 4, 2, 1))
def test_several_lines_per_thread_dither(rows):
    """d. yuv444p -> rgb24 (dither: the matrix row must follow the line of each iteration) on 64 x 33 pictures, as many as make the
    launch walk 8, 4, 2 and 1 lines per thread; 33 lines: the last iteration is ragged (some threadIdx.y run one line more)"""
    c = _named("yuv444p rgb24 70x9-70x9")
    assert any(c.lst.uops[i].uop == S.DITHER for i in range(c.lst.n))
    w, hgt = 64, 33
    case = S.RectCase("yuv444p rgb24 64x33", c.lst, w, hgt, [np.zeros((hgt, w), np.uint8)] * 3, [np.zeros((hgt, 3 * w), np.uint8)])
    _many_pictures(_hip(), case, rows, 60 + rows)


def test_several_lines_per_thread_vertical_filter():
    """d. yuv444p 64x12 -> 64x24 (READ_PLANAR_FV: the skipped source lines, the tap rows and the weight row of each iteration) at
    8 lines per thread"""
    c = _named("yuv444p yuv444p 64x12-64x24")
    assert c.lst.read.uop == S.READ_PLANAR_FV
    _many_pictures(_hip(), c, 8, 70)


def test_more_tables_than_a_handle_keeps():
    """e. gray 40 -> 96 (READ_PLANAR_FH) on one handle, the columns [0, k) for k = 1 ... 40: 40 distinct in_offset_x tables, past the
    32 a handle keeps before it drains the device and starts over.  After each call its columns are right and the later ones still
    hold the fill; then the whole picture"""
    dev = _hip()
    case = _named("gray gray 40x8-96x8")
    assert case.lst.read.uop == S.READ_PLANAR_FH
    h, bs = dev.compile(case.lst)
    assert bs == 1
    sb, db = case.bufs()
    ts, sa = dev.upload(sb)
    td, da = dev.upload(db)
    b, want = db[0], case.want[0]
    for k in list(range(1, 41)) + [case.w]:
        S.run_rects(lambda e, *r: dev.run_dev(h, e, r, sb, db), case, bs, sb, sa, db, da, [(0, k, 0, case.h)])
        f = dev.download(td)[0]
        assert np.array_equal(b.payload(0, f)[:, :k], want[:, :k]), "columns [0, %d)" % k
        later = np.zeros((1, b.lines, b.rows), bool)
        later[:, :, k:] = True
        assert b.outside_kept(f, but=later), "columns [0, %d): bytes outside them were written" % k
    dev.free(h)
