"""A restatement of HEVC intra sample prediction (H.265 8.4.4.2) in plain Python integers, any bit depth: the pin the GPU kernels of
HEVCPredContext are checked against.  It is written from the standard's text, not from the device code.

A reference line of a block of size N holds 4N + 1 samples from bottom-left to top-right:
    line[k] = left[2N-1-k] for k < 2N,   line[2N] = the corner,   line[2N+1+x] = top[x]."""
import numpy as np

ANGLE = [32, 26, 21, 17, 13, 9, 5, 2, 0, -2, -5, -9, -13, -17, -21, -26, -32, -26, -21, -17, -13, -9, -5, -2, 0, 2, 5, 9, 13, 17, 21, 26, 32]
INV_ANGLE = [-4096, -1638, -910, -630, -482, -390, -315, -256, -315, -390, -482, -630, -910, -1638, -4096]


def split(line):
    """(left, corner, top) of a line: left[y] and top[x] for y, x in 0..2N-1"""
    line = [int(v) for v in line]
    n2 = (len(line) - 1) // 2
    return line[:n2][::-1], line[n2], line[n2 + 1:]


def join(left, corner, top):
    return [int(v) for v in left][::-1] + [int(corner)] + [int(v) for v in top]


def availability(N, avail_left, avail_top, corner, log2_uh, log2_uv):
    """per-sample availability along the line from the record's unit masks (bit i of avail_left = left units counted from the top)"""
    left = [bool(avail_left >> (y >> log2_uv) & 1) for y in range(2 * N)]
    top = [bool(avail_top >> (x >> log2_uh) & 1) for x in range(2 * N)]
    return join(left, bool(corner), top)


def substitute(line, avail, bd):
    """8.4.4.2.2"""
    line = [int(v) for v in line]
    if not any(avail):
        return [1 << (bd - 1)] * len(line)
    out = list(line)
    if not avail[0]:
        out[0] = line[next(k for k, a in enumerate(avail) if a)]
    for k in range(1, len(line)):
        if not avail[k]:
            out[k] = out[k - 1]
    return out


def filter_applies(N, mode, c_idx, smoothing_disabled=False, chroma444=False):
    if smoothing_disabled or not (c_idx == 0 or chroma444) or mode == 1 or N == 4:
        return False
    return min(abs(mode - 26), abs(mode - 10)) > {8: 7, 16: 1, 32: 0}[N]


def strong_applies(line, N, c_idx, bd, strong):
    left, c, top = split(line)
    thr = 1 << (bd - 5)
    return bool(strong and c_idx == 0 and N == 32 and abs(c + top[63] - 2 * top[31]) < thr and abs(c + left[63] - 2 * left[31]) < thr)


def filter_line(line, N, mode, c_idx, bd, strong=False, smoothing_disabled=False, chroma444=False):
    """8.4.4.2.3"""
    line = [int(v) for v in line]
    if not filter_applies(N, mode, c_idx, smoothing_disabled, chroma444):
        return line
    left, c, top = split(line)
    if strong_applies(line, N, c_idx, bd, strong):
        nt = [((63 - i) * c + (i + 1) * top[63] + 32) >> 6 for i in range(63)] + [top[63]]
        nl = [((63 - i) * c + (i + 1) * left[63] + 32) >> 6 for i in range(63)] + [left[63]]
        return join(nl, c, nt)
    out = list(line)
    for k in range(1, len(line) - 1):
        out[k] = (line[k - 1] + 2 * line[k] + line[k + 1] + 2) >> 2
    return out


def predict(line, N, mode, c_idx, bd):
    """8.4.4.2.4 - 8.4.4.2.6 on a prepared line: an N x N int64 array indexed [y, x]"""
    left, c, top = split(line)
    log2 = N.bit_length() - 1
    maxv = (1 << bd) - 1
    clip = lambda v: min(max(v, 0), maxv)  # noqa: E731
    out = np.zeros((N, N), np.int64)
    if mode == 0:
        for y in range(N):
            for x in range(N):
                out[y, x] = ((N - 1 - x) * left[y] + (x + 1) * top[N] + (N - 1 - y) * top[x] + (y + 1) * left[N] + N) >> (log2 + 1)
        return out
    if mode == 1:
        dc = (sum(top[:N]) + sum(left[:N]) + N) >> (log2 + 1)
        out[:, :] = dc
        if c_idx == 0 and N < 32:
            out[0, 0] = (left[0] + 2 * dc + top[0] + 2) >> 2
            for x in range(1, N):
                out[0, x] = (top[x] + 3 * dc + 2) >> 2
            for y in range(1, N):
                out[y, 0] = (left[y] + 3 * dc + 2) >> 2
        return out
    angle = ANGLE[mode - 2]
    main, side = ([c] + top, [c] + left) if mode >= 18 else ([c] + left, [c] + top)   # main[x] = top[x - 1] from the top
    ref = {x: main[x] for x in range(2 * N + 1)}
    last = (N * angle) >> 5
    if angle < 0 and last < -1:
        inv = INV_ANGLE[mode - 11]
        for x in range(last, 0):
            ref[x] = side[(x * inv + 128) >> 8]                                          # side[i] = left[i - 1]
    for v in range(N):
        i, f = ((v + 1) * angle) >> 5, ((v + 1) * angle) & 31
        for u in range(N):
            s = ref[u + i + 1] if f == 0 else ((32 - f) * ref[u + i + 1] + f * ref[u + i + 2] + 16) >> 5
            if mode >= 18:
                out[v, u] = s
            else:
                out[u, v] = s
    if c_idx == 0 and N < 32:
        if mode == 26:
            for y in range(N):
                out[y, 0] = clip(top[0] + ((left[y] - c) >> 1))
        elif mode == 10:
            for x in range(N):
                out[0, x] = clip(left[0] + ((top[x] - c) >> 1))
    return out


def predict_raw(line, N, mode, c_idx, bd, avail, strong=False, smoothing_disabled=False, chroma444=False):
    """the whole path of a raw line: substitution, filtering, prediction"""
    line = substitute(line, avail, bd)
    line = filter_line(line, N, mode, c_idx, bd, strong, smoothing_disabled, chroma444)
    return predict(line, N, mode, c_idx, bd)
