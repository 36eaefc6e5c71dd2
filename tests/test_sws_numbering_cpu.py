"""CPU check of the workgroup numbering of the swscale batch kernels (sws_block_numbering, sws_kernels.h; the host copy is
ffhip_sws_block_numbering_host, the same inline function).  k_sws_up2, k_sws_down2, k_sws_down2_rgb and k_yuv420p_rgb24_t run workgroup b
on the units of workgroup numbering(b): a number that never comes out is a workgroup whose rows are never written.  So every mode must be
a permutation of [0, nb) at every grid, not only at multiples of 8 — and keep the property it is there for."""
import numpy as np
import pytest

from ffmpeg_amd import _lib

# every small grid, and the grids the batch faces launch for 1080p / 720p / 1440p / 4K at 1..64 frames (the table converter's: 270,
# 180, 540 and 1080 workgroups a frame) and the ragged batches 1920x1080 x 11, 1280x720 x 25, 2560x1440 x 7
GRIDS = sorted(set(range(1, 4097)) | {k * n for k in (270, 180, 540, 1080) for n in range(1, 65)} | {2970, 4500, 3780})


def numbering(mode, nb):
    out = np.empty(nb, np.uint32)
    assert _lib.lib().ffhip_sws_block_numbering_host(mode, nb, out.ctypes.data) == 0
    return out.astype(np.int64)


def check(mode, nb):
    m = numbering(mode, nb)
    assert np.array_equal(np.sort(m), np.arange(nb)), "mode %d, %d workgroups: not a permutation (missing %s)" % (
        mode, nb, np.setdiff1d(np.arange(nb), m)[:8].tolist())
    if mode == 0:
        assert np.array_equal(m, np.arange(nb))
    elif mode == 1:
        # the workgroups of XCD x (b % 8 == x) take one contiguous ascending run; the runs follow in XCD order, lengths within one
        start, lengths = 0, []
        for x in range(min(8, nb)):
            run = m[x::8]
            assert np.array_equal(run, start + np.arange(len(run))), "mode 1, %d workgroups: XCD %d" % (nb, x)
            start += len(run)
            lengths.append(len(run))
        assert max(lengths) - min(lengths) <= 1
    else:
        # chunks of C = 2^k: each chunk an XCD receives is C contiguous numbers, and its j-th chunk is one of the j-th eight, so the
        # XCDs' fronts stay within eight chunks of each other; the workgroups past the last whole round keep their own number
        C = 1 << (mode - 1)
        full = nb & ~(8 * C - 1)
        assert np.array_equal(m[full:], np.arange(full, nb)), "mode %d, %d workgroups: tail" % (mode, nb)
        for x in range(8):
            chunks = m[x:full:8].reshape(-1, C)
            assert (chunks == chunks[:, :1] + np.arange(C)).all(), "mode %d, %d workgroups: XCD %d" % (mode, nb, x)
            assert (chunks[:, 0] % C == 0).all() and (chunks[:, 0] // (8 * C) == np.arange(len(chunks))).all()


@pytest.mark.parametrize("mode", range(6))
def test_numbering_is_a_permutation_with_its_property(mode):
    for nb in GRIDS:
        check(mode, nb)


def test_grids_that_are_a_multiple_of_8_keep_the_numbering_they_had():
    """at nb % 8 == 0 an eighth per XCD is (b % 8) * nb / 8 + b / 8 — the form every kernel used, the table converter included: the
    bench's launches (the 4K table converter: 1080 * 64 workgroups) keep their workgroups and their order"""
    for nb in (8, 64, 1080 * 64, 4320):
        b = np.arange(nb)
        assert np.array_equal(numbering(1, nb), (b & 7) * (nb >> 3) + (b >> 3))

