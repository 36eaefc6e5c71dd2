"""SwsOpBackend `hip`, the anchor of tests/test_gpu_sws_uops_rects.py, without a GPU: the oracle (oracle/ffo_sws_uops.c) run
rectangle by rectangle — each rectangle with an SwsOpExec of its own (swsops.rect_exec: what a threaded sws_scale_frame and a caller
with column ranges hand a backend) — reproduces backend_c's committed whole-picture outputs (tests/golden/sws_uops.npz) byte for
byte, so "the committed output, reached rectangle by rectangle" is what the generated kernels are held to; and the launch shape
of those kernels (ffhip_sws_uops_launch_shape_host), which the GPU tests ask for the frame counts they need."""
import ctypes as C
import os

import numpy as np
import pytest

import ffi
import swsops as S

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "sws_uops.npz")


def _oracle():
    return S.declare(ffi.oracle(), "ffo_sws_uops_")


def _cases():
    return S.rect_cases(GOLDEN, _oracle())


def test_fixture_holds_the_paths_the_rectangles_are_for():
    """the lists the GPU tests lean on are there: dither, both filtered reads, a matrix, packed and planar I/O, a 1-bit write"""
    cases = _cases()
    assert len(cases) == 11 + 3
    ops = {c.lst.uops[i].uop for c in cases for i in range(c.lst.n)}
    for op in (S.DITHER, S.READ_PLANAR_FH, S.READ_PLANAR_FV, S.LINEAR, S.READ_PACKED, S.WRITE_PACKED, S.READ_PLANAR, S.WRITE_PLANAR,
               S.WRITE_BIT, S.READ_NIBBLE, S.WRITE_NIBBLE, S.READ_BIT):
        assert op in ops, op


@pytest.mark.parametrize("tiling", (0, 1))
def test_oracle_by_rectangles_is_the_committed_output(tiling):
    """every list, x cuts {0, bs, 3 bs, an odd middle block, W} (the 1-bit lists have 8-pixel blocks: their x cuts are multiples
    of 8), y cuts {0, 1, 3, H} / {0, 2, H - 1, H}, into one destination that held 0x5A: the committed output (hand-built 4-bit and
    1-bit lists: the oracle's own whole-picture output, which must not be all zero), and the line padding untouched"""
    g = _oracle()
    for case in _cases():
        h = C.c_void_p()
        assert g("compile")(case.lst.uops, case.lst.n, C.byref(h)) == 0, case.name
        bs = g("block_size")(h)
        if any(case.lst.uops[i].uop in (S.READ_BIT, S.WRITE_BIT) for i in range(case.lst.n)):
            assert bs == 8
        rects = S.tilings(case.w, case.h, bs)[tiling]
        assert all(x0 % bs == 0 and x1 % bs == 0 for x0, x1, _, _ in rects)
        assert sum((x1 - x0) * (y1 - y0) for x0, x1, y0, y1 in rects) == case.w * case.h
        sb, db = case.bufs()
        S.run_rects(lambda e, *r: g("func")(C.byref(e), h, *r), case, bs, sb, [b.flat.ctypes.data + b.off for b in sb],
                    db, [b.flat.ctypes.data + b.off for b in db], rects)
        g("free")(C.byref(h))
        for i, (b, want) in enumerate(zip(db, case.want)):
            assert S.same_bytes(b.payload(0), want, case.f32), (case.name, "plane %d" % i, int((b.payload(0) != want).sum()))
            assert b.outside_kept(), (case.name, "plane %d: bytes outside the lines were written" % i)
        if case.name.startswith("hand"):
            assert case.want[0].any() and (case.want[0] != S.FILL).any(), case.name


def test_hand_built_lists_are_what_they_say():
    """4-bit read, 4-bit write, 1-bit read against numpy (oracle/ffo_sws_uops.c:287-310 are the bodies under test)"""
    cases = {c.name: c for c in _cases()}
    c = cases["hand nibble-read"]
    assert np.array_equal(c.want[0], np.stack([c.src[0] >> 4, c.src[0] & 15], -1).reshape(c.h, c.w))
    c = cases["hand nibble-write"]
    assert c.src[0].max() == 15 and np.array_equal(c.want[0], c.src[0][:, 0::2] << 4 | c.src[0][:, 1::2])
    c = cases["hand bit-read"]
    assert np.array_equal(c.want[0], np.unpackbits(c.src[0], axis=1))


# ---- the launch shape ---------------------------------------------------------------------------------------------------------------
def shape(V, npx, ny, nframes):
    from ffmpeg_amd import _lib
    out = (C.c_int32 * 4)()
    assert _lib.lib().ffhip_sws_uops_launch_shape_host(V, npx, ny, nframes, out) == 0
    return tuple(out)


def cdiv(a, b):
    return -(-a // b)


def test_launch_shape():
    """lines per thread: a power of two in 1..8, the largest that still leaves 2048 workgroups (else 1); grid x = 64 threads of V
    pixels, grid y = workgroups of 4 lines x lines per thread, capped at 16384 (the kernel's line loop takes the rest), grid z the
    pictures"""
    seen = set()
    for V in (4, 8):
        for npx in (1, 7, 64, 255, 256, 257, 1920, 3840, 7680):
            for ny in (1, 3, 4, 5, 24, 33, 1080, 2160, 70000, 600000):
                for nf in (1, 2, 3, 16, 410, 683, 1024, 2048, 5000):
                    gx, gy, gz, rows = shape(V, npx, ny, nf)
                    assert rows in (1, 2, 4, 8)
                    assert gx == cdiv(cdiv(npx, V), 64) and gz == nf
                    assert gy == min(cdiv(ny, 4 * rows), 16384)
                    work = lambda r: gx * cdiv(ny, 4 * r) * nf      # noqa: E731
                    assert rows == 1 or work(rows) >= 2048
                    assert rows == 8 or work(2 * rows) < 2048
                    seen.add(rows)
    assert seen == {1, 2, 4, 8}
    assert shape(4, 3840, 2160, 1)[3] >= 2
    assert shape(4, 1920, 1080, 1)[3] == 1
    assert shape(4, 64, 600000, 1)[1] == 16384           # the cap: 600000 lines / (4 x 8) would be 18750


def test_launch_shape_rejects_bad_arguments():
    from ffmpeg_amd import _lib
    L = _lib.lib()
    out = (C.c_int32 * 4)()
    for args in ((0, 64, 8, 1), (4, 0, 8, 1), (4, 64, 0, 1), (4, 64, 8, 0)):
        assert L.ffhip_sws_uops_launch_shape_host(*args, out) == _lib.EINVAL
    assert L.ffhip_sws_uops_launch_shape_host(4, 64, 8, 1, None) == _lib.EINVAL
