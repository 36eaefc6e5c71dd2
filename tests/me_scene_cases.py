"""The calls that tests/test_me_scene_cpu.py and tests/test_gpu_me_scene.py share: sequences of pictures for
ffhip_me_scene_sequence_dev() / _host() in one buffer with strides above the width, pitches above the picture, a base misaligned by
1..15 bytes and row padding of different random bytes in every picture; outputs between guard elements; the model's results
(tests/me_scene_model.py) and the host face's, each computed once per call.

The buffer starts on a 16-byte boundary and is uploaded whole, so the device sees the same misalignment.  frame_pitch rotates through
the picture's own size, a multiple of 16 (the rows of a pair then agree modulo 16: the kernel's wide loads, behind a head the
misalignment decides) and a pitch that is none."""
import functools

import numpy as np

import me_scene_model as M

GUARD = 96              # bytes before and after the pictures; a multiple of 16
WIDTHS = (1, 3, 15, 16, 17, 63, 64, 65, 255, 257, 1000)
HEIGHTS = (1, 2, 5, 37)
PADS = (0, 1, 13)       # samples a row is longer than the width
DEPTHS = (8, 10, 16)
THRESHOLDS = (10.0, 0.0, 0.5, 100.0, 33.0)
SENT64, SENT32, SENT8 = 0xA5A5A5A5A5A5A5A5, 0xA5A5A5A5, 0xA5


def aligned_bytes(n, fill=None, rng=None):
    """n bytes that start on a 16-byte boundary"""
    raw = np.zeros(n + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    a = raw[off:off + n]
    a[:] = rng.integers(0, 256, n, dtype=np.uint8) if fill is None else fill
    return a


class Case:
    def __init__(self, width, height, pad, depth, k):
        self.width, self.height, self.depth = width, height, depth
        self.px = 2 if depth > 8 else 1
        self.mis = (1 + k % 15) if depth == 8 else 2 * (1 + k % 7)
        self.nseq = (1, 3)[k % 2]
        self.nframes = 2 + (k // 2) % 5
        self.threshold = THRESHOLDS[k % 5]
        self.stride = (width + pad) * self.px
        pic = self.stride * height
        self.frame_pitch = (pic, (pic + 31) // 16 * 16, pic + 6 * self.px + (16 if (pic + 6 * self.px) % 16 == 0 else 0))[(k // 3) % 3]
        self.seq_pitch = (self.nframes - 1) * self.frame_pitch + pic + (0, 10 * self.px)[(k // 5) % 2]
        self.size = (self.nseq - 1) * self.seq_pitch + (self.nframes - 1) * self.frame_pitch + (height - 1) * self.stride + width * self.px
        rng = np.random.default_rng(7000 + k)
        self.buf = aligned_bytes(2 * GUARD + self.mis + self.size, rng=rng)
        self.off = GUARD + self.mis
        self.name = "%dx%d+%d-d%d-k%d" % (width, height, pad, depth, k)
        # some pictures darker than others, so that mafd moves from pair to pair
        for s in range(self.nseq):
            for p in range(self.nframes):
                sh = int(rng.integers(0, 4))
                v = self.picture(s, p, writeable=True)
                v[:] = v >> sh
        self.buf0 = self.buf.copy()
        self.mafd_in = None if k % 4 == 0 else rng.random(self.nseq) * 60.0
        self.npairs = (self.nframes - 1) * self.nseq

    def picture(self, s, p, writeable=False):
        o = self.off + s * self.seq_pitch + p * self.frame_pitch
        a = self.buf[o:o + (self.height - 1) * self.stride + self.width * self.px]
        if self.px == 2:
            a = a.view(np.uint16)
        return np.lib.stride_tricks.as_strided(a, (self.height, self.width), (self.stride, self.px), writeable=writeable)

    def args(self, frames_addr):
        return (frames_addr + self.off, self.depth, self.width, self.height, self.stride, self.frame_pitch, self.nframes, self.seq_pitch, self.nseq,
                self.threshold)

    def model(self):
        return _model(self)

    def host(self):
        return _host(self)


class Outputs:
    """sad, score, flags and mafd_out between guard elements, every element holding a sentinel before the call"""

    def __init__(self, npairs, nseq):
        self.npairs, self.nseq = npairs, nseq
        self.sad = np.full(npairs + 2, SENT64, np.uint64)
        self.score = np.full(npairs + 2, SENT32, np.uint32)
        self.flags = np.full(npairs + 2, SENT8, np.uint8)
        self.mafd = np.full(nseq + 2, SENT64, np.uint64)

    def arrays(self):
        return self.sad, self.score, self.flags, self.mafd

    def addresses(self, base=None):
        """the addresses of element 1 of each array (on the host, or in device copies at the addresses `base`)"""
        b = base or [a.ctypes.data for a in self.arrays()]
        return b[0] + 8, b[1] + 4, b[2] + 1, b[3] + 8

    def results(self, arrays=None):
        """(sad ints, score bit patterns, flags, mafd bit patterns) after the guards were checked"""
        sad, score, flags, mafd = arrays or self.arrays()
        for a, sent in ((sad, SENT64), (score, SENT32), (flags, SENT8), (mafd, SENT64)):
            assert int(a[0]) == sent and int(a[-1]) == sent, "a guard element was written"
        return [int(v) for v in sad[1:-1]], [int(v) for v in score[1:-1]], [int(v) for v in flags[1:-1]], [int(v) for v in mafd[1:-1]]


def model_results(pics, depth, threshold, mafd_in):
    sads, scores, flags, out = M.sequence(pics, depth, threshold, mafd_in)
    return sads, [M.bits32(v) for v in scores], flags, [M.bits64(v) for v in out]


@functools.lru_cache(maxsize=None)
def _model(c):
    pics = [[c.picture(s, p) for p in range(c.nframes)] for s in range(c.nseq)]
    return model_results(pics, c.depth, c.threshold, c.mafd_in)


@functools.lru_cache(maxsize=None)
def _host(c):
    from ffmpeg_amd import me
    o = Outputs(c.npairs, c.nseq)
    sad, score, flags, mafd = o.addresses()
    me.scene_sequence_host(*c.args(c.buf.ctypes.data), mafd_in=c.mafd_in, mafd_out=mafd, sad_out=sad, score_out=score, flags_out=flags)
    assert np.array_equal(c.buf, c.buf0), "%s: an input changed" % c.name
    return o.results()


@functools.lru_cache(maxsize=None)
def cases(depth):
    """every width x height x row padding at one depth; misalignment, sequence and picture counts, threshold, pitches and mafd_in rotate"""
    out, k = [], DEPTHS.index(depth)
    for w in WIDTHS:
        for h in HEIGHTS:
            for pad in PADS:
                out.append(Case(w, h, pad, depth, k))
                k += 1
    return out
