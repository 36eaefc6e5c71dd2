"""The calls that tests/test_me_interp_cpu.py and tests/test_gpu_me_interp.py share: pictures, fields, windows and jobs of
ffhip_me_interp_sequence_dev() / _host(), laid out in buffers with guard bytes round every plane, field and output, strides above the
width and pitches above the picture; the host face's bytes and the model's (tests/me_interp_model.py), each computed once per call."""
import functools

import numpy as np

import me_interp_model as M

GUARD = 96
FILL = 0xA5             # what an output buffer holds before a call
ALPHAS = (0, 1, 341, 512, 1023, 1024)


# ---- windows ----------------------------------------------------------------------------------------------------------------------------
def window(kind, mb, seed=0):
    n = 2 * mb
    rng = np.random.default_rng(1000 + seed)
    if kind == "ramp":          # separable and linear: h(i) = 1, 3, .. up to the middle and down again; zero in the corners at mb 16
        h = np.array([2 * min(i, n - 1 - i) + 1 for i in range(n)])
        return ((h[:, None] * h[None, :]) >> (2 if mb == 16 else 0)).astype(np.uint8).reshape(-1)
    if kind == "random":
        return rng.integers(0, 256, n * n, dtype=np.uint8)
    if kind == "holes":         # zero rows and columns
        w = rng.integers(1, 256, (n, n), dtype=np.uint8)
        w[[0, 5, n - 1], :] = 0
        w[:, [1, 6, n - 2]] = 0
        return w.reshape(-1)
    assert kind == "full"
    return np.full(n * n, 255, np.uint8)


# ---- fields: [pairs, nseq, b_h, b_w, 2] absolute positions ------------------------------------------------------------------------------
def field(kind, W, H, mb, R, pairs, nseq, seed, at=None):
    lg = {16: 4, 8: 3}[mb]
    bw, bh = W >> lg, H >> lg
    rng = np.random.default_rng(2000 + seed)
    org = np.zeros((bh, bw, 2), np.int64)
    org[..., 0] = np.arange(bw)[None, :] << lg
    org[..., 1] = np.arange(bh)[:, None] << lg
    shape = (pairs, nseq, bh, bw, 2)
    if kind == "zero":
        v = np.zeros(shape, np.int64)
    elif kind == "random":
        v = rng.integers(-R, R + 1, shape)
    elif kind == "plus":
        v = np.full(shape, R, np.int64)
    elif kind == "minus":
        v = np.full(shape, -R, np.int64)
    elif kind == "int16":       # any int16 content is legal: most of it malformed, some not
        f = rng.integers(-32768, 32768, shape)
        ok = rng.random(shape[:-1]) < 0.3
        f[ok] = (org + rng.integers(-R, R + 1, shape))[ok]
        return f.astype(np.int16)
    else:
        assert kind == "pileup"   # every block within R of pixel `at` puts its window centre (alpha 0, dir 0: sx + mb) on it
        v = np.zeros(shape, np.int64)
        want = np.array(at)[None, None, :] - mb // 2 - org
        near = (np.abs(want) <= R).all(axis=-1)
        v[:, :, near] = want[near]
    return (org + v).astype(np.int16)


class Buffer:
    """`count` items of `size` bytes, `pitch` apart, between two guards"""

    def __init__(self, count, size, pitch, fill=None, rng=None):
        self.n = 2 * GUARD + (max(count, 1) - 1) * pitch + size
        self.a = rng.integers(0, 256, self.n, dtype=np.uint8) if fill is None else np.full(self.n, fill, np.uint8)
        self.pitch = pitch

    def item(self, k, size):
        return self.a[GUARD + k * self.pitch:GUARD + k * self.pitch + size]


class Call:
    """One call of the face and everything it reads and writes"""

    def __init__(self, name, W, H, mb, chroma, fkind, wkind, jobs, R=32, nseq=1, nframes=2, seed=0, at=None, pad=(5, 3, 7), gap=(37, 11, 23)):
        self.name, self.W, self.H, self.mb, self.R, self.nseq, self.nframes, self.jobs = name, W, H, mb, R, nseq, nframes, list(jobs)
        self.nplanes = 1 if chroma is None else 3
        self.sw, self.sh = chroma or (0, 0)
        rng = np.random.default_rng(3000 + seed)
        self.window = window(wkind, mb, seed)
        self.pw = [W if i == 0 else (W + (1 << self.sw) - 1) >> self.sw for i in range(self.nplanes)]
        self.ph = [H if i == 0 else (H + (1 << self.sh) - 1) >> self.sh for i in range(self.nplanes)]
        self.stride = [self.pw[i] + pad[i] for i in range(self.nplanes)]
        self.fpitch = [self.stride[i] * self.ph[i] + gap[i] for i in range(self.nplanes)]
        self.spitch = [nframes * self.fpitch[i] + gap[i] + 1 for i in range(self.nplanes)]
        self.dpitch = [self.stride[i] * self.ph[i] + 2 * gap[i] for i in range(self.nplanes)]
        size = [(self.ph[i] - 1) * self.stride[i] + self.pw[i] for i in range(self.nplanes)]
        self.src = [Buffer(1, (nseq - 1) * self.spitch[i] + (nframes - 1) * self.fpitch[i] + size[i], 0, rng=rng) for i in range(self.nplanes)]
        self.dst = [Buffer(len(jobs), size[i], self.dpitch[i], fill=FILL) for i in range(self.nplanes)]
        lg = {16: 4, 8: 3}[mb]
        self.per = (W >> lg) * (H >> lg)
        self.fields = []
        for d in range(2):
            f = field(fkind, W, H, mb, R, nframes - 1, nseq, seed + 17 * d, at)
            b = Buffer(1, f.size * 2, 0, rng=rng)
            b.a[GUARD:GUARD + f.size * 2] = f.reshape(-1).view(np.uint8)
            self.fields.append(b)
        self.src0 = [b.a.copy() for b in self.src]
        self.fields0 = [b.a.copy() for b in self.fields]

    # -- views --
    def plane(self, whole, off, i):
        """the 2-D view of plane i at `off` behind the guard of the buffer `whole`"""
        a = whole[GUARD + off:GUARD + off + (self.ph[i] - 1) * self.stride[i] + self.pw[i]]
        return np.lib.stride_tricks.as_strided(a, (self.ph[i], self.pw[i]), (self.stride[i], 1), writeable=False)

    def picture(self, s, p):
        return [self.plane(self.src[i].a, s * self.spitch[i] + p * self.fpitch[i], i) for i in range(self.nplanes)]

    def output(self, j, bufs):
        """output picture j's planes in the output buffers `bufs`"""
        return [self.plane(bufs[i], j * self.dpitch[i], i) for i in range(self.nplanes)]

    def field_array(self, d):
        lg = {16: 4, 8: 3}[self.mb]
        n = (self.nframes - 1) * self.nseq * self.per * 2
        return self.fields[d].a[GUARD:GUARD + 2 * n].view(np.int16).reshape(self.nframes - 1, self.nseq, self.H >> lg, self.W >> lg, 2)

    # -- the face's arguments, for buffers at the given addresses --
    def args(self, me, src_addr, dst_addr, field_addr):
        src = me.planes([a + GUARD for a in src_addr], self.stride, self.fpitch, self.spitch)
        dst = me.planes([a + GUARD for a in dst_addr], self.stride, self.dpitch)
        return (src, dst, self.nplanes, self.sw, self.sh, self.W, self.H, self.nframes, self.nseq, self.mb, self.R, self.window,
                field_addr[0] + GUARD, field_addr[1] + GUARD, self.jobs)

    def check_guards(self, dst_bufs):
        """only the samples of the output pictures may differ from the fill; the inputs are what they were"""
        for i in range(self.nplanes):
            mask = np.ones(self.dst[i].n, bool)
            for j in range(len(self.jobs)):
                for y in range(self.ph[i]):
                    o = GUARD + j * self.dpitch[i] + y * self.stride[i]
                    mask[o:o + self.pw[i]] = False
            assert (dst_bufs[i][mask] == FILL).all(), "%s: plane %d written outside its samples" % (self.name, i)
        for b, b0 in zip(self.src + self.fields, self.src0 + self.fields0):
            assert np.array_equal(b.a, b0), "%s: an input changed" % self.name

    def host(self):
        """(the output buffers after the host face, its counts)"""
        return _host(self)

    def model(self):
        """([job j's planes], counts) of the model"""
        return _model(self)


@functools.lru_cache(maxsize=None)
def _host(c):
    from ffmpeg_amd import me
    counts = me.interp_sequence_host(*c.args(me, [b.a.ctypes.data for b in c.src], [b.a.ctypes.data for b in c.dst],
                                             [b.a.ctypes.data for b in c.fields]))
    bufs = [b.a.copy() for b in c.dst]
    for b in c.dst:
        b.a[:] = FILL
    c.check_guards(bufs)
    return bufs, counts


@functools.lru_cache(maxsize=None)
def _model(c):
    pics = [[c.picture(s, p) for p in range(c.nframes)] for s in range(c.nseq)]
    return M.interp_sequence(pics, c.W, c.H, c.sw, c.sh, c.mb, c.R, c.window, c.field_array(0), c.field_array(1), c.jobs)


# ---- the calls --------------------------------------------------------------------------------------------------------------------------
SHAPES = ((48, 32), (52, 38), (53, 37), (12, 12))
CHROMA = ((0, 0), (1, 0), (1, 1), None)
FIELDS = ("zero", "random", "plus", "minus", "int16")
WINDOWS = ("ramp", "random", "holes", "full")
PILE_AT = (50, 41)


@functools.lru_cache(maxsize=None)
def calls():
    """name -> Call.  Every shape x block size x field; chroma, window, mv_range and alpha rotate so that every value of each meets
    every shape and every field."""
    out = {}
    k = 0
    for si, (W, H) in enumerate(SHAPES):
        for mb in (16, 8):
            for fi, fk in enumerate(FIELDS):
                chroma, wk = CHROMA[(k + si) % 4], WINDOWS[(k // 4 + fi) % 4]
                R = (32, 7)[k % 2]
                a = [ALPHAS[(k + t) % 6] for t in (0, 3)]
                jobs = [(0, 0, a[0], M.MCI), (0, 0, ALPHAS[(k + 1) % 6], M.BLEND), (0, 0, a[1], M.MCI)]
                name = "%dx%d-mb%d-%s-%s-%s-r%d" % (W, H, mb, fk, wk, "y" if chroma is None else "c%d%d" % chroma, R)
                out[name] = Call(name, W, H, mb, chroma, fk, wk, jobs, R=R, seed=k)
                k += 1
    # the cap: about 8 x 8 windows stacked on one pixel against a cap of 16
    out["pileup"] = Call("pileup", 96, 80, 8, (1, 1), "pileup", "full", [(0, 0, 0, M.MCI)], R=32, seed=90, at=PILE_AT)
    # several jobs on one pair, jobs across 3 sequences x 4 pictures, BLEND mixed in
    jobs = [(s, p, ALPHAS[(2 * s + p + t) % 6], M.BLEND if (s + p + t) % 4 == 3 else M.MCI) for s in range(3) for p in range(3) for t in range(2)]
    out["sequences"] = Call("sequences", 48, 32, 16, (1, 1), "random", "ramp", jobs, R=16, nseq=3, nframes=4, seed=91)
    out["sequences-mb8"] = Call("sequences-mb8", 52, 38, 8, (1, 0), "random", "random", jobs[::2], R=9, nseq=3, nframes=4, seed=92)
    return out


NAMES = tuple(calls())
