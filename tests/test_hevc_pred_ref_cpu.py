"""CPU tier of HEVC intra prediction: the restatement in hevc_pred_ref.py anchored by properties it does not share code with, and the
ABI of the new faces that needs no device (record size; the refusals of a box without one)."""
import ctypes as C

import numpy as np
import pytest

import hevc_pred_ref as R
from ffmpeg_amd import _lib, hevc

SIZES = (4, 8, 16, 32)
DEPTHS = (8, 10, 12)


@pytest.mark.parametrize("bd", DEPTHS)
def test_constant_line_predicts_the_constant(bd):
    for N in SIZES:
        for v in (0, 1, (1 << bd) // 3, (1 << bd) - 1):
            line = [v] * (4 * N + 1)
            for c_idx in (0, 1):
                for mode in range(35):
                    out = R.predict(R.filter_line(line, N, mode, c_idx, bd, strong=True), N, mode, c_idx, bd)
                    assert (out == v).all(), (N, v, c_idx, mode)


def test_pure_vertical_and_horizontal_copy_their_side():
    rng = np.random.default_rng(1)
    for N in SIZES:
        left, top = rng.integers(0, 256, 2 * N), rng.integers(0, 256, 2 * N)
        line = R.join(left, 77, top)
        assert (R.predict(line, N, 26, 1, 8) == np.tile(top[:N], (N, 1))).all()
        assert (R.predict(line, N, 10, 1, 8) == np.tile(left[:N, None], (1, N))).all()


def test_modes_2_and_34_are_the_45_degree_copies():
    rng = np.random.default_rng(2)
    for N in SIZES:
        left, top = rng.integers(0, 1024, 2 * N), rng.integers(0, 1024, 2 * N)
        line = R.join(left, 5, top)
        y, x = np.mgrid[0:N, 0:N]
        for c_idx in (0, 1):
            assert (R.predict(line, N, 34, c_idx, 10) == top[x + y + 1]).all()
            assert (R.predict(line, N, 2, c_idx, 10) == left[x + y + 1]).all()


def test_planar_reproduces_a_unit_ramp():
    """line[k] = a + s (k - 2N) is the plane a + s (x - y) sampled at the reference positions; planar rebuilds it exactly for s = +-1"""
    for N in SIZES:
        y, x = np.mgrid[0:N, 0:N]
        for a, s in ((128, 1), (128, -1), (500, 1)):
            line = [a + s * (k - 2 * N) for k in range(4 * N + 1)]
            assert (R.predict(line, N, 0, 0, 10) == a + s * (x - y)).all(), (N, a, s)


def test_transposed_line_and_mirrored_mode_transpose_the_block():
    rng = np.random.default_rng(3)
    for bd in (8, 12):
        for N in SIZES:
            left, top, c = rng.integers(0, 1 << bd, 2 * N), rng.integers(0, 1 << bd, 2 * N), int(rng.integers(0, 1 << bd))
            line, tline = R.join(left, c, top), R.join(top, c, left)
            for c_idx in (0, 1):
                for mode in range(35):
                    m2 = mode if mode < 2 else 36 - mode
                    a = R.predict(R.filter_line(line, N, mode, c_idx, bd), N, mode, c_idx, bd)
                    b = R.predict(R.filter_line(tline, N, m2, c_idx, bd), N, m2, c_idx, bd)
                    assert (a == b.T).all(), (bd, N, c_idx, mode)


@pytest.mark.parametrize("bd", DEPTHS)
def test_substitution(bd):
    for N in SIZES:
        L = 4 * N + 1
        line = list(range(10, 10 + L))
        assert R.substitute(line, [False] * L, bd) == [1 << (bd - 1)] * L
        # only the last unit of the top (4 samples) available: everything before it takes its first sample
        av = [False] * (L - 4) + [True] * 4
        assert R.substitute(line, av, bd) == [line[L - 4]] * (L - 4) + line[L - 4:]
        # one gap in the middle takes the sample below it
        av = [True] * L
        av[N:N + 3] = [False] * 3
        assert R.substitute(line, av, bd) == line[:N] + [line[N - 1]] * 3 + line[N + 3:]
        # the record's unit masks: avail_left counts left units from the top, avail_top from the left
        av = R.availability(N, 1, 1 << ((2 * N >> 2) - 1), False, 2, 2)
        assert av[2 * N - 4:2 * N] == [True] * 4 and not any(av[:2 * N - 4]) and not av[2 * N]
        assert av[L - 4:] == [True] * 4 and not any(av[2 * N + 1:L - 4])


@pytest.mark.parametrize("bd", DEPTHS)
def test_strong_smoothing_threshold(bd):
    N, thr = 32, 1 << (bd - 5)
    c = 1 << (bd - 1)
    for side in ("top", "left"):
        for dev, want in ((thr - 1, True), (thr, False), (-(thr - 1), True), (-thr, False)):
            # a flat line whose far end on one side moves by `dev`: |c + end - 2 * mid| == |dev|
            left, top = [c] * 64, [c] * 64
            (top if side == "top" else left)[63] = c + dev
            line = R.join(left, c, top)
            assert R.strong_applies(line, N, 0, bd, True) == want, (side, dev)
            assert not R.strong_applies(line, N, 1, bd, True) and not R.strong_applies(line, N, 0, bd, False)
            out = R.filter_line(line, N, 2, 0, bd, strong=True)
            l2, c2, t2 = R.split(out)
            if want:   # bi-linear between the corner and the far ends; the ends and the corner stay
                assert c2 == c and t2[63] == top[63] and l2[63] == left[63]
                assert t2[0] == (63 * c + top[63] + 32) >> 6 and l2[0] == (63 * c + left[63] + 32) >> 6
            else:      # the [1 2 1] filter
                assert c2 == (left[0] + 2 * c + top[0] + 2) >> 2 and t2[31] == (top[30] + 2 * top[31] + top[32] + 2) >> 2


def test_intra_record_matches_the_c_struct():
    assert hevc.INTRA_DTYPE.itemsize == _lib.lib().ffhip_hevc_intra_record_size() == 16
    assert hevc.intra_c_idx_unit(2, 1, 2) == 2 | 1 << 2 | 2 << 4
    assert C.sizeof(hevc.HEVCPredContext) == 13 * C.sizeof(C.c_void_p)


@pytest.mark.skipif(_lib.lib().ffhip_device_count() > 0, reason="a HIP device is present: the refusal path is not reachable")
def test_no_device_refusals():
    L = _lib.lib()
    buf = (C.c_uint8 * 256)()
    p = C.cast(buf, C.c_void_p)
    assert L.ff_hevc_pred_init_hip(p, 8) == _lib.ENOSYS and not any(buf)
    assert L.ff_hevc_pred_init_hip(p, 9) == _lib.EINVAL and not any(buf)
    assert L.ffhip_hevc_intra_batch_dev(8, p, 64, p, p, 1, None) == _lib.ENOSYS
    assert L.ffhip_hevc_intra_batch_dev(9, p, 64, p, p, 1, None) == _lib.EINVAL
    assert L.ffhip_hevc_intra_batch_dev(10, p, 63, p, p, 1, None) == _lib.EINVAL
    assert L.ffhip_hevc_intra_batch_dev(8, p, 64, p, p, -1, None) == _lib.EINVAL
