"""CPU check of the exact-2x kernel's geometry (sws_up2.hip): which (frame, strip, group) every lane of every wave of a launch owns.
ffhip_sws_up2_walk_host plans a one-job launch the way the scaler does and walks sws_up2_unit / sws_up2_lane (sws_kernels.h), the
inline functions k_sws_up2 itself calls.  Rows of n groups with n % 64 in {0, 16, 32} take the edge layout: the two ends of a row, cut
off at e / 2 groups, sit side by side with the ends of other frames in one wave of 64 / e frames, and the rest of the row is whole
64-lane blocks that never see a row end.  Every other n keeps the whole blocks and the shared ragged end."""
import ctypes as C

import numpy as np
import pytest

from ffmpeg_amd import _lib

GROUPS = [16, 32, 34, 64, 80, 96, 112, 128, 240, 480]
SRC_H = 40      # 41 steps: strips of 6 -> 7 strips, of 12 -> 4, of 60 -> 1


def edge_lanes(n):
    """the rule of the layout: e lanes of a wave per frame, 0 = whole blocks and a shared ragged end"""
    return {0: 64, 32: 32, 16: 16}.get(n % 64, 0) if n >= 16 else 0


def walk(n, frames, want, fshift=-1):
    L = _lib.lib()
    info = (C.c_int32 * 4)()
    waves = L.ffhip_sws_up2_walk_host(n, SRC_H, frames, want, fshift, None, 0, info)
    assert waves > 0
    out = np.zeros((waves, 64, 4), np.int32)
    assert L.ffhip_sws_up2_walk_host(n, SRC_H, frames, want, fshift, out.ctypes.data, out.size, info) == waves
    return out, dict(e=info[0], fshift=info[1], upj=info[2], nstrips=info[3])


def check_cover(rec, info, n, frames):
    """every (frame, strip, group) has exactly one active lane; the waves flagged interior hold no row end and read inside the row"""
    frame, strip, group, edge = (rec[..., i] for i in range(4))
    act = frame >= 0
    key = (frame[act].astype(np.int64) * info["nstrips"] + strip[act]) * n + group[act]
    assert (group[act] >= 0).all() and (group[act] < n).all() and (strip[act] < info["nstrips"]).all() and (frame[act] < frames).all()
    counts = np.bincount(key, minlength=frames * info["nstrips"] * n)
    assert counts.size == frames * info["nstrips"] * n and (counts == 1).all(), "owned %d..%d times" % (counts.min(), counts.max())
    assert (edge.min(axis=1) == edge.max(axis=1)).all()           # wave-uniform
    inner = edge[:, 0] == 0
    gi = group[inner]                                             # every lane of an interior wave, idle ones too
    assert (gi >= 1).all() and (gi <= n - 2).all()
    # source bytes a lane reads per row: 8 bits [4g - 4, 4g + 8) of 4n; above 8 bits a plane [8g - 4, 8g + 12), a pair [8g - 8, 8g + 16) of 8n
    for lo, hi, row in ((4 * gi - 4, 4 * gi + 8, 4 * n), (8 * gi - 4, 8 * gi + 12, 8 * n), (8 * gi - 8, 8 * gi + 16, 8 * n)):
        assert (lo >= 0).all() and (hi <= row).all()
    return inner


@pytest.mark.parametrize("want", [6, 12, 60])
@pytest.mark.parametrize("frames", [1, 2, 3, 5])
@pytest.mark.parametrize("n", GROUPS)
def test_every_group_has_one_owner(n, frames, want):
    rec, info = walk(n, frames, want)
    assert info["nstrips"] == {6: 7, 12: 4, 60: 1}[want]
    inner = check_cover(rec, info, n, frames)
    e = edge_lanes(n)
    assert info["e"] == e                                         # the edge layout exactly where the rule says (34, 112, 240: not)
    assert 64 >> info["fshift"] <= (e or 64)                      # the pack holds at least one edge wave's frames
    if not e:
        return
    group, frame = rec[..., 2], rec[..., 0]
    # interior waves: whole blocks of one frame from e / 2 on; edge waves: 64 / e frames, e / 2 groups from either end of the row
    # (a wave whose first frame lies beyond the batch ends at once: all its lanes idle)
    live = (frame >= 0).any(axis=1)
    assert (inner & live).sum() == (n - e) // 64 * frames * info["nstrips"]
    for w in np.nonzero(inner & live)[0]:
        assert (frame[w] == frame[w, 0]).all() and (group[w] == group[w, 0] + np.arange(64)).all() and (group[w, 0] - e // 2) % 64 == 0
    lane = np.arange(64) % e
    want_g = np.where(lane < e // 2, lane, n - e + lane)
    for w in np.nonzero(~inner)[0]:
        assert (group[w] == want_g).all()
        on = frame[w] >= 0
        f = frame[w][on]
        if f.size:
            assert (f == f[0] + (np.nonzero(on)[0] // e)).all()
    assert (~inner & live).sum() == -(-frames * e // 64) * info["nstrips"]
    # of a pack's 15 units at 480 groups and 2 frames, one is an edge wave
    if n == 480 and frames == 2:
        assert info["upj"] == 15 and (~inner).sum() == info["nstrips"]


@pytest.mark.parametrize("fshift", [0, 1, 2])
@pytest.mark.parametrize("n", GROUPS)
def test_a_forced_pack_keeps_the_shared_ragged_end(n, fshift):
    """FFHIP_UP2_FSHIFT (measure build): the whole blocks and the ragged end shared by 1 << fshift frames, at every n"""
    for frames in (1, 3, 5):
        rec, info = walk(n, frames, 12, fshift)
        assert info["e"] == 0 and info["fshift"] == fshift
        check_cover(rec, info, n, frames)


def test_walk_rejects_bad_arguments():
    L = _lib.lib()
    info = (C.c_int32 * 4)()
    assert L.ffhip_sws_up2_walk_host(0, SRC_H, 1, 60, -1, None, 0, info) == _lib.EINVAL
    assert L.ffhip_sws_up2_walk_host(64, SRC_H, 0, 60, -1, None, 0, info) == _lib.EINVAL
    assert L.ffhip_sws_up2_walk_host(64, SRC_H, 1, 60, 3, None, 0, info) == _lib.EINVAL
    out = np.zeros(4, np.int32)
    assert L.ffhip_sws_up2_walk_host(64, SRC_H, 1, 60, -1, out.ctypes.data, out.size, info) == _lib.ENOMEM
