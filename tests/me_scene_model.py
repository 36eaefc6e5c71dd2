"""The scene-change rule of ffhip_me_scene_sequence_dev() / _host(), written from the rule text of include/ffhip.h: numpy int64 sums,
Python floats (IEEE doubles) for mafd and the carry, np.float32 for the score.  And the scene actions of
ffhip_me_interp_sequence_scd_dev(): what a flagged MCI job writes."""
import struct

import numpy as np

SCENE_BLEND, SCENE_DUP = 1, 2


def sad(a, b):
    """the exact sum of |a - b| over two 2-D sample arrays (uint8, or uint16 holding the full 16-bit value)"""
    return int(np.abs(a.astype(np.int64) - b.astype(np.int64)).sum())


def mafd(s, width, height, depth):
    return float(s) * 100.0 / (height * width) / (1 << depth)


def score(m, prev):
    v = np.float32(min(m, abs(m - prev)))
    return np.float32(min(max(v, np.float32(0.0)), np.float32(100.0)))


def step(s, prev, width, height, depth, threshold):
    """(score as np.float32, flag, the new carry) of one pair whose sum is s"""
    m = mafd(s, width, height, depth)
    sc = score(m, prev)
    return sc, int(float(sc) >= threshold), m


def sequence(pics, depth, threshold, mafd_in=None):
    """pics[s][p]: 2-D arrays.  Pair-major (sad, score, flag) lists and the carries after the last pair."""
    nseq, nframes = len(pics), len(pics[0]) if pics else 0
    steps = max(nframes - 1, 0)
    sads, scores, flags = [0] * (steps * nseq), [np.float32(0)] * (steps * nseq), [0] * (steps * nseq)
    out = []
    for s in range(nseq):
        prev = 0.0 if mafd_in is None else float(mafd_in[s])
        h, w = pics[s][0].shape
        for k in range(steps):
            sads[k * nseq + s] = sad(pics[s][k], pics[s][k + 1])
            scores[k * nseq + s], flags[k * nseq + s], prev = step(sads[k * nseq + s], prev, w, h, depth, threshold)
        out.append(prev)
    return sads, scores, flags, out


def bits32(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def bits64(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def scene_picture(A, B, alpha, action):
    """what a flagged MCI job writes: planes A and B (lists of 2-D uint8 arrays) at instant alpha"""
    if action == SCENE_DUP:
        return [p.copy() for p in (A if alpha <= 512 else B)]
    return [((alpha * b.astype(np.int64) + (1024 - alpha) * a.astype(np.int64) + 512) >> 10).astype(np.uint8) for a, b in zip(A, B)]
