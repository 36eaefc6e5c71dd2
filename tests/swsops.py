"""ctypes mirrors of the SwsOpBackend boundary (include/ffhip.h: FFHipSwsUOp, FFHipSwsOpExec ...) and the test shapes of
tests/checkasm/sw_ops.c: one micro-op between a planar read and a planar write, 64 pixels x 16 lines, value ranges per micro-op.
Test infrastructure."""
import ctypes as C

import numpy as np

from ffmpeg_amd.swsops import *  # noqa: F401,F403  (the boundary's structs and constants)

def declare(L, prefix):
    """argtypes of the five entry points, `ffhip_sws_uops_` (libffhip) or `ffo_sws_uops_` (oracle)"""
    g = lambda n: getattr(L, prefix + n)   # noqa: E731
    g("compile").argtypes = [C.POINTER(UOp), C.c_int, C.POINTER(C.c_void_p)]
    g("free").argtypes = [C.POINTER(C.c_void_p)]
    g("free").restype = None
    g("block_size").argtypes = [C.c_void_p]
    g("func").argtypes = [C.POINTER(Exec), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    g("func").restype = None
    g("set_fallback").argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    g("set_fallback").restype = None
    return g


def declare_ref(R):
    R.ffref_sws_hip_bind.argtypes = [C.c_void_p] * 5
    R.ffref_sws_hip_count.argtypes = [C.c_int]
    R.ffref_sws_hip_count.restype = C.c_long
    R.ffref_sws_frame_convert.argtypes = [C.c_int] * 8 + [C.POINTER(C.c_void_p), C.POINTER(C.c_int)] + [C.c_int] * 3 + \
        [C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
    R.ffref_sws_uops_run_c.argtypes = [C.POINTER(UOp), C.c_int, C.POINTER(Exec), C.c_int, C.c_int, C.c_int, C.c_int]
    R.ffref_sws_filter_generate.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]
    R.ffref_sws_uop_instance.argtypes = [C.c_int, C.POINTER(UOp), C.c_char_p, C.c_int]
    R.ffref_pix_fmt.argtypes = [C.c_char_p]
    R.ffref_image_layout.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_int), C.POINTER(C.c_int)]
    R.ffref_sws_describe_uops.argtypes = [C.c_int] * 8 + [C.c_char_p, C.c_int]
    return R


def bind(R, L, prefix):
    """make backend_hip of the reference build call the five entry points of L"""
    f = lambda n: C.cast(getattr(L, prefix + n), C.c_void_p)   # noqa: E731
    R.ffref_sws_hip_bind(f("compile"), f("free"), f("block_size"), f("func"), f("set_fallback"))


def unbind(R):
    R.ffref_sws_hip_bind(None, None, None, None, None)


# ---------------------------------------------------------------------------------------------------------------------------------
def synthetic_kernel(rng, dst_size, src_size, filter_size):
    """weights summing to SWS_FILTER_SCALE with negative lobes; what ff_sws_filter_generate produces has this shape (filters.c)"""
    fs = min(filter_size, src_size)
    w = np.zeros((dst_size, fs), np.int32)
    for i in range(dst_size):
        g = rng.dirichlet(np.ones(fs)) * 1.3 - 0.3 / fs
        w[i] = np.round(g * 16384)
        w[i, -1] += 16384 - w[i].sum()
    off = np.clip(np.round((np.arange(dst_size) + 0.5) * src_size / dst_size - fs / 2), 0, src_size - fs).astype(np.int32)
    return Kernel(w, off, fs, src_size)


def ref_kernel(R, scaler, src_size, dst_size):
    fs = C.c_int()
    w = np.zeros(dst_size * 256, np.int32)
    o = np.zeros(dst_size, np.int32)
    assert R.ffref_sws_filter_generate(scaler, src_size, dst_size, C.byref(fs), w.ctypes.data_as(C.POINTER(C.c_int)), w.size,
                                       o.ctypes.data_as(C.POINTER(C.c_int))) == 0
    return Kernel(w[:dst_size * fs.value].reshape(dst_size, fs.value), o, fs.value, src_size)


def rnd_normal_f32(rng, n):
    """checkasm's rndf(): uniformly random bits that are a normal float"""
    out = np.empty(n, np.uint32)
    k = 0
    while k < n:
        b = rng.integers(0, 1 << 32, n - k, dtype=np.uint64).astype(np.uint32)
        e = (b >> 23) & 0xFF
        b = b[(e != 0) & (e != 255)]
        out[k:k + b.size] = b
        k += b.size
    return out.view(np.float32)


def fill(rng, typ, nbytes, rng_max):
    """checkasm's fill8/16/32/32f: `rng_max` 0 = every bit pattern (floats: every normal number)"""
    n = nbytes // SIZE[typ]
    if typ == F32:
        return (rnd_normal_f32(rng, n) if not rng_max else (rng.random(n) * rng_max).astype(np.float32)).view(np.uint8)
    hi = (1 << (8 * SIZE[typ])) - 1
    return rng.integers(0, (rng_max if rng_max and rng_max < hi else hi) + 1, n, dtype=np.uint64).astype(NP[typ]).view(np.uint8)


def rndpx(rng, typ):
    p = Pixel()
    if typ == F32:
        p.f32 = float(rnd_normal_f32(rng, 1)[0])
    else:
        p.u32 = int(rng.integers(0, 1 << (8 * SIZE[typ])))
    return p


class Case:
    """one list + the planes it runs on, checkasm-shaped (sw_ops.c:291-380: read, micro-op, write)"""

    def __init__(self, name, uops, keep, type_in, type_out, planes_in, planes_out, bits_in, bits_out, ranges):
        self.name, self.keep = name, keep
        self.uops = (UOp * len(uops))(*uops)
        self.type_in, self.type_out, self.planes_in, self.planes_out = type_in, type_out, planes_in, planes_out
        self.bits_in, self.bits_out, self.ranges = bits_in, bits_out, ranges

    def planes(self, rng):
        src = np.zeros((4, LINES, STRIDE), np.uint8)
        for p in range(4):
            if self.planes_in >> p & 1:
                src[p] = fill(rng, self.type_in, LINES * STRIDE, self.ranges[p]).reshape(LINES, STRIDE)
        return src

    def execute(self, src, dst, pixels=PIXELS, lines=LINES, x0=0, block=1, off=0):
        """the SwsOpExec of sw_ops.c:196-236 over src / dst ((4, LINES, STRIDE) uint8 arrays); `off` shifts the planes by bytes"""
        e = Exec(width=PIXELS, height=LINES, slice_h=LINES)
        rd = self.uops[0]
        read_size, write_size = pixels * self.bits_in >> 3, pixels * self.bits_out >> 3
        for i in range(4):
            e.in_[i] = src[i].ctypes.data + off + (x0 * self.bits_in >> 3 if rd.uop != READ_PLANAR_FH else 0)
            e.out[i] = dst[i].ctypes.data + off + (x0 * self.bits_out >> 3)
            e.in_stride[i] = e.out_stride[i] = STRIDE
            e.in_bump[i], e.out_bump[i] = STRIDE - read_size, STRIDE - write_size
            e.block_size_in[i], e.block_size_out[i] = block * self.bits_in >> 3, block * self.bits_out >> 3
        if rd.uop == READ_PALETTE:
            e.in_[1] = src[1].ctypes.data + off
            e.in_bump[1] = e.in_stride[1] = 0
        self._tabs = []
        if rd.uop == READ_PLANAR_FV:
            o = np.ctypeslib.as_array(rd.data.kernel.contents.offsets, (LINES,))
            b = np.zeros(LINES, np.int32)
            b[:-1] = o[1:] - o[:-1] - 1
            self._tabs.append(b)
            e.in_bump_y = b.ctypes.data_as(C.POINTER(C.c_int32))
        if rd.uop == READ_PLANAR_FH:
            o = np.ctypeslib.as_array(rd.data.kernel.contents.offsets, (PIXELS,))
            b = (o * self.bits_in >> 3).astype(np.int32)
            self._tabs.append(b)
            e.in_offset_x = b.ctypes.data_as(C.POINTER(C.c_int32))
        return e

    def compare(self, a, b):
        """the planes a list writes, as its output type; NaNs of any payload are one value (IEEE leaves the payload open)"""
        n = PIXELS * self.bits_out >> 3
        for p in range(4):
            if not self.planes_out >> p & 1:
                continue
            x, y = a[p][:, :n], b[p][:, :n]
            if self.type_out == F32:
                xf, yf = x.copy().view(np.float32), y.copy().view(np.float32)
                same = (x.copy().view(np.uint32) == y.copy().view(np.uint32)) | (np.isnan(xf) & np.isnan(yf))
                if not same.all():
                    return "plane %d: %d floats differ" % (p, (~same).sum())
            elif not np.array_equal(x, y):
                return "plane %d: %d bytes differ" % (p, (x != y).sum())
            if not np.array_equal(a[p][:, n:], b[p][:, n:]):
                return "plane %d: bytes outside the line were written" % p
        return None


def _mk(typ, uop, mask=0xF, **kw):
    u = UOp(type=typ, uop=uop, mask=mask)
    for k, v in kw.items():
        setattr(u, k, v)
    return u


def case_of(rng, name, u, R=None, scaler_kernels=True):
    """the checkasm test of one micro-op instance (sw_ops.c:291-640): the data it needs, the read / write around it, the ranges.
    Returns a list of Cases (filters: several kernels) — empty for instances the hip backend declines (LUT_3D)."""
    typ, op, keep = u.type, u.uop, []
    t_in = t_out = typ
    if TO_U8 <= op <= TO_F32:
        t_out = U8 + (op - TO_U8)
    elif op == EXPAND_PAIR:
        t_out = U16
    elif op == EXPAND_QUAD:
        t_out = U32
    elif op in (READ_PLANAR_FH, READ_PLANAR_FV):
        t_out = u.par.filter.type
    bits_in, bits_out = 8 * SIZE[t_in], 8 * SIZE[t_out]
    planes_in = planes_out = 0
    ranges = [0, 0, 0, 0]
    if op in (READ_PLANAR, READ_PLANAR_FH, READ_PLANAR_FV):
        planes_in = u.mask
    elif op == WRITE_PLANAR:
        planes_out = u.mask
    elif op == READ_PACKED:
        planes_in, bits_in = 1, bits_in * bin(u.mask).count("1")
    elif op == WRITE_PACKED:
        planes_out, bits_out = 1, bits_out * bin(u.mask).count("1")
    elif op == READ_NIBBLE:
        planes_in, bits_in = 1, 4
    elif op == WRITE_NIBBLE:
        planes_out, bits_out = 1, 4
    elif op == READ_BIT:
        planes_in, bits_in = 1, 1
    elif op == WRITE_BIT:
        planes_out, bits_out = 1, 1
    elif op == READ_PALETTE:
        planes_in, bits_in = 3, 8
    mask_in = mask_out = 0xF
    # the per-micro-op ranges and data of check_* (sw_ops.c:470-640)
    if op in READS:
        mask_in = mask_out = u.mask
    elif op in WRITES:
        mask_in = mask_out = u.mask
        ranges = [1 if op == WRITE_BIT else 15 if op == WRITE_NIBBLE else 255] * 4      # check_write, sw_ops.c:494-502
    elif op in (PERMUTE, COPY):
        mask_out = u.mask
    elif op == EXPAND_BIT:
        ranges = [1] * 4
    elif TO_U8 <= op <= TO_F32 or op in (EXPAND_PAIR, EXPAND_QUAD):
        mask_in = mask_out = u.mask
        isz, osz = SIZE[t_in], SIZE[t_out]
        r = (1 << (8 * osz)) - 1
        if isz < osz or t_out == F32:
            r = 0
        ranges = [r] * 4
    elif op == SCALE:
        u.data.scalar = rndpx(rng, typ)
        if typ != F32:
            s = u.data.scalar.u32 & ((1 << (8 * SIZE[typ])) - 1)
            ranges = [((1 << (8 * SIZE[typ])) - 1) // (s if s else 1)] * 4
    elif op == ADD:
        u.data.scalar = rndpx(rng, typ)      # check_scalar: only element 0 is random, the rest of the vec4 stays 0
    elif op in (MIN, MAX, CLEAR):
        for i in range(4):
            u.data.vec4[i] = rndpx(rng, typ)
    elif op == UNPACK:
        total = sum(u.par.pack.pattern)
        ranges = [(1 << total) - 1] * 4
        mask_in, mask_out = 1, u.mask
    elif op == PACK:
        ranges = [(1 << b) - 1 for b in u.par.pack.pattern]
        mask_in, mask_out = u.mask, 1
    elif op == LINEAR:
        for i in range(4):
            for j in range(5):
                bit = 1 << (5 * i + j)
                if u.par.lin.zero & bit:
                    u.data.mat4[i][j].u32 = 0
                elif u.par.lin.one & bit:
                    if typ == F32:
                        u.data.mat4[i][j].f32 = 1.0
                    else:
                        u.data.mat4[i][j].u32 = 1
                else:
                    u.data.mat4[i][j] = rndpx(rng, typ)
    elif op == DITHER:
        size = 1 << u.par.dither.size_log2
        mo = max(u.par.dither.y_offset[c] for c in range(4))
        m = np.zeros((size + mo) * size, np.uint32)
        m[:size * size] = rnd_normal_f32(rng, size * size).view(np.uint32) if typ == F32 else \
            rng.integers(0, 1 << (8 * SIZE[typ]), size * size, dtype=np.uint64).astype(np.uint32)
        m[size * size:] = m[:size * mo]
        keep.append(m)
        u.data.ptr = m.ctypes.data_as(C.POINTER(Pixel))
    elif op == LUT_3D:
        return []

    def wrap(u, kern=None, nm=name):
        uops = []
        pin, pout, bi, bo = planes_in, planes_out, bits_in, bits_out
        if not pin:
            pin, bi = mask_in, 8 * SIZE[t_in]
            uops.append(_mk(INT_OF[SIZE[t_in]], READ_PLANAR))
        uops.append(u)
        if not pout:
            pout, bo = mask_out, 8 * SIZE[t_out]
            uops.append(_mk(INT_OF[SIZE[t_out]], WRITE_PLANAR))
        return Case(nm, uops, keep + [kern], t_in, t_out, pin, pout, bi, bo, ranges)

    if op in (READ_PLANAR_FH, READ_PLANAR_FV):
        out = []
        dst = LINES if op == READ_PLANAR_FV else PIXELS
        src = 1
        while src <= dst:
            kerns = [synthetic_kernel(rng, dst, src, 4)]
            if R is not None and scaler_kernels:
                kerns += [ref_kernel(R, 3, src, dst), ref_kernel(R, 6, src, dst)]   # SWS_SCALE_POINT, SWS_SCALE_SINC (sw_ops.c:511-514)
            for ki, k in enumerate(kerns):
                v = UOp.from_buffer_copy(u)
                v.data.kernel = C.pointer(k.c)
                out.append(wrap(v, k, "%s_%d_%d" % (name, src, ki)))
            src <<= 1
        return out
    return [wrap(u)]


def instances(R):
    """(name, UOp) of every instance backend_c implements"""
    u, nm = UOp(), C.create_string_buffer(64)
    n = R.ffref_sws_uop_instance(-1, C.byref(u), nm, 64)
    out = []
    for i in range(n):
        u = UOp()
        R.ffref_sws_uop_instance(i, C.byref(u), nm, 64)
        out.append((nm.value.decode(), u))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
class Picture:
    """planes of a w x h picture in any pixel format the reference knows (av_image_fill_linesizes / _plane_sizes)"""

    def __init__(self, R, fmt_name, w, h, rng=None, align=64, pad=0, slack=0):
        """`slack`: bytes added to every line (room for a dispatcher to run whole blocks without its padded-copy tail path)"""
        self.fmt = R.ffref_pix_fmt(fmt_name.encode())
        assert self.fmt >= 0, fmt_name
        ls, ln = (C.c_int * 4)(), (C.c_int * 4)()
        assert R.ffref_image_layout(self.fmt, w, h, 1, ls, ln) > 0
        ls = [(v + slack + align - 1) // align * align if v else 0 for v in ls]
        self.w, self.h, self.linesize, self.lines = w, h, list(ls), list(ln)
        self.planes = []
        for i in range(4):
            n = self.linesize[i] * self.lines[i]
            self.planes.append((rng.integers(0, 256, n + pad, dtype=np.uint8) if rng is not None else np.zeros(n + pad, np.uint8)) if n else None)
        if fmt_name == "pal8":                   # plane 1 is the 256-entry palette (linesize 0)
            self.planes[1] = rng.integers(0, 256, 1024, dtype=np.uint8) if rng is not None else np.zeros(1024, np.uint8)
        self.data = (C.c_void_p * 4)(*[p.ctypes.data if p is not None else None for p in self.planes])
        self.strides = (C.c_int * 4)(*self.linesize)

    def payload(self, R):
        """the bytes of every line that belong to the picture (the padding of a line is nobody's)"""
        ls, ln = (C.c_int * 4)(), (C.c_int * 4)()
        R.ffref_image_layout(self.fmt, self.w, self.h, 1, ls, ln)
        return [self.planes[i][:self.linesize[i] * self.lines[i]].reshape(self.lines[i], self.linesize[i])[:, :ls[i]] for i in range(4)
                if self.planes[i] is not None and self.linesize[i]]


def convert(R, backends, src, dst, flags=0, scaler=-1, dither=-1, threads=1):
    return R.ffref_sws_frame_convert(backends, flags, scaler, dither, threads, src.w, src.h, src.fmt, src.data, src.strides,
                                     dst.w, dst.h, dst.fmt, dst.data, dst.strides)


BACKEND_C, BACKEND_MEMCPY, BACKEND_HIP = 2, 4, 64



# ---------------------------------------------------------------------------------------------------------------------------------
# micro-op lists of real conversions, captured from the reference's graph and stored as fixtures (tests/golden/sws_uops_*.npz)
# ---------------------------------------------------------------------------------------------------------------------------------
COMPILE_CB = C.CFUNCTYPE(C.c_int, C.POINTER(UOp), C.c_int, C.POINTER(C.c_void_p))


def capture_lists(R, O, sf, df, size, **kw):
    """the lists the reference's dispatch compiles for a conversion, in order (those the oracle backend accepts; a declined list is
    split by the reference and its parts come back).  Returns [(uops bytes (n, 112), {index: side arrays})]"""
    declare(O, "ffo_sws_uops_")
    got = []

    def compile_cb(uops, n, out):
        r = O.ffo_sws_uops_compile(uops, n, out)
        if r == 0:
            raw = np.frombuffer(C.string_at(uops, n * C.sizeof(UOp)), np.uint8).reshape(n, C.sizeof(UOp)).copy()
            side = {}
            for i in range(n):
                u = uops[i]
                if u.uop in (READ_PLANAR_FH, READ_PLANAR_FV):
                    k = u.data.kernel.contents
                    side[i] = ("kernel", np.ctypeslib.as_array(k.weights, (k.dst_size * k.filter_size,)).copy(),
                               np.ctypeslib.as_array(k.offsets, (k.dst_size,)).copy(), np.array([k.filter_size, k.src_size], np.int32))
                elif u.uop == DITHER:
                    size_ = 1 << u.par.dither.size_log2
                    rows = size_ + max(u.par.dither.y_offset[c] for c in range(4))
                    side[i] = ("dither", np.ctypeslib.as_array(C.cast(u.data.ptr, C.POINTER(C.c_uint32)), (rows * size_,)).copy())
            got.append((raw, side))
        return r
    cb = COMPILE_CB(compile_cb)
    f = lambda n: C.cast(getattr(O, "ffo_sws_uops_" + n), C.c_void_p)   # noqa: E731
    R.ffref_sws_hip_bind(C.cast(cb, C.c_void_p), f("free"), f("block_size"), f("func"), f("set_fallback"))
    try:
        sw, sh, dw, dh = size
        src, dst = Picture(R, sf, sw, sh), Picture(R, df, dw, dh)
        assert convert(R, BACKEND_HIP | BACKEND_MEMCPY, src, dst, **kw) >= 0
    finally:
        unbind(R)
    return got


def pack_lists(lists):
    """-> dict of arrays for np.savez"""
    out = {"count": np.array([len(lists)], np.int32)}
    for k, (raw, side) in enumerate(lists):
        out["l%d" % k] = raw
        for i, s in side.items():
            if s[0] == "kernel":
                out["l%d_k%d_w" % (k, i)], out["l%d_k%d_o" % (k, i)], out["l%d_k%d_m" % (k, i)] = s[1], s[2], s[3]
            else:
                out["l%d_d%d" % (k, i)] = s[1]
    return out


def golden_cases(path):
    """tests/golden/sws_uops.npz -> [(name, size, UOpList, [src planes], [dst planes])]"""
    z = np.load(path)
    out = []
    for j in range(int(z["ncases"][0])):
        p = "c%d_" % j
        src = [z[p + "src%d" % i] for i in range(4) if p + "src%d" % i in z]
        dst = [z[p + "dst%d" % i] for i in range(4) if p + "dst%d" % i in z]
        out.append((bytes(z[p + "name"]).decode(), tuple(int(v) for v in z[p + "size"]), load_lists(z, p)[0], src, dst))
    return out


def run_golden(func, handle, block, lst, size, src, dst_shapes, pad=64):
    """one whole picture through `func` (an SwsOpFunc on host memory); returns the destination planes"""
    sw, sh, dw, dh = size
    sp = [np.zeros((a.shape[0], a.shape[1] + pad), np.uint8) for a in src]
    for a, b in zip(sp, src):
        a[:, :b.shape[1]] = b
    dp = [np.zeros((s[0], s[1] + pad), np.uint8) for s in dst_shapes]
    e = plain_exec(lst, [a.ctypes.data for a in sp], [a.shape[1] for a in sp], [a.ctypes.data for a in dp], [a.shape[1] for a in dp],
                   dw, dh, block)
    func(C.byref(e), handle, 0, 0, (dw + block - 1) // block, dh)
    return [a[:, :s[1]] for a, s in zip(dp, dst_shapes)], dp


# ---------------------------------------------------------------------------------------------------------------------------------
# a picture reached rectangle by rectangle: what a threaded sws_scale_frame (slices) and a caller with column ranges hand a backend
# ---------------------------------------------------------------------------------------------------------------------------------
FILL = 0x5A        # what destinations hold before a call; whatever no rectangle covers must still hold it afterwards


def rect_exec(lst, src_addrs, src_strides, dst_addrs, dst_strides, w, h, block, x0, x1, y0):
    """the SwsOpExec of the columns [x0, x1) from line y0 on, of a w x h picture: plain_exec() of the whole picture with the
    pointers and bumps moved the way op_pass_setup and the dispatcher move them for a slice (ops_dispatch.c:207-290, 403-436).
    The call is then func(e, handle, x0 // block, y0, x1 // block, y1); x0 and x1 are whole blocks."""
    assert x0 % block == 0 and x1 % block == 0 and 0 <= x0 < x1, (x0, x1, block)
    e = plain_exec(lst, src_addrs, src_strides, dst_addrs, dst_strides, w, h, block)
    rd = lst.read
    _, bi = rw_geometry(rd)
    _, bo = rw_geometry(lst.write)
    npx = x1 - x0
    dy = y0
    if rd.uop == READ_PLANAR_FV:                 # in_bump_y stays the whole picture's: it is indexed by the absolute line
        o = np.ctypeslib.as_array(rd.data.kernel.contents.offsets, (rd.data.kernel.contents.dst_size,))
        dy = int(o[y0]) - int(o[0])
    for i in range(4):
        if e.in_[i] and not (rd.uop == READ_PALETTE and i == 1):
            if rd.uop == READ_PLANAR_FH:         # in_offset_x stays the whole picture's: it is indexed by the absolute column
                e.in_[i] += y0 * e.in_stride[i]
                e.in_bump[i] = e.in_stride[i]
            else:
                e.in_[i] += dy * e.in_stride[i] + (x0 * bi >> 3)
                e.in_bump[i] = e.in_stride[i] - (npx * bi >> 3)
        if e.out[i]:
            e.out[i] += y0 * e.out_stride[i] + (x0 * bo >> 3)
            e.out_bump[i] = e.out_stride[i] - (npx * bo >> 3)
    return e


def tilings(w, h, block):
    """two tilings of a w x h picture, as lists of (x0, x1, y0, y1): x cuts {0, block, 3 blocks, an odd block near the middle, w},
    y cuts {0, 1, 3, h} and {0, 2, h - 1, h}.  With 1-pixel blocks the columns 1, 3 and the odd middle one start a rectangle off
    the 4-pixel vector of a thread; with 2-pixel blocks (4-bit lists) the columns 2 and 6 do; with 8-pixel blocks (1-bit lists: the
    x cuts are multiples of 8) the block IS the vector and no rectangle can."""
    assert w % block == 0
    nb = w // block
    xs = sorted({0, block, 3 * block, (nb // 2 | 1) * block, w})
    assert xs[-1] == w and len(xs) == 5, (w, block)
    out = []
    for ys in ((0, 1, 3, h), (0, 2, h - 1, h)):
        ys = sorted({y for y in ys if 0 <= y <= h})
        out.append([(x0, x1, y0, y1) for y0, y1 in zip(ys, ys[1:]) for x0, x1 in zip(xs, xs[1:])])
    return out


class HandList:
    """a list put together in the test (UOpList's face)"""

    def __init__(self, uops):
        self.n = len(uops)
        self.uops = (UOp * self.n)(*uops)

    read = UOpList.read
    write = UOpList.write


class Buf:
    """`frames` pictures of one plane behind one another in one flat byte buffer: `lines` lines of `rows` payload bytes, `pitch`
    apart, the first `off` bytes into the buffer, `tail` bytes after the last.  Flat so that it can live on the host or, copied,
    on the device, and so that every byte that is not payload can be checked."""

    def __init__(self, rows, lines, frames=1, off=0, pitch=None, fill=0, tail=64):
        self.rows, self.lines, self.frames, self.off, self.fill = rows, lines, frames, off, fill
        self.pitch = pitch if pitch is not None else rows + 64
        assert self.pitch >= rows
        self.fpitch = lines * self.pitch
        self.flat = np.full(off + frames * self.fpitch + tail, fill, np.uint8)

    def view(self, flat=None):
        f = self.flat if flat is None else flat
        return f[self.off:self.off + self.frames * self.fpitch].reshape(self.frames, self.lines, self.pitch)

    def payload(self, frame=0, flat=None):
        return self.view(flat)[frame][:, :self.rows]

    def outside_kept(self, flat=None, but=None):
        """every byte that is not payload still holds the fill.  `but`: a (frames, lines, rows) mask of payload bytes that must
        hold it as well (what no call has covered yet)"""
        f = self.flat if flat is None else flat
        m = np.ones(f.size, bool)
        self.view(m)[:, :, :self.rows] = False if but is None else but
        return bool((f[m] == self.fill).all())


def same_bytes(a, b, f32):
    """byte-exact; floats bit for bit with the NaNs as one value (as Case.compare)"""
    if not f32:
        return np.array_equal(a, b)
    x, y = np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)
    return a.shape == b.shape and bool(((x == y) | (np.isnan(x.view(np.float32)) & np.isnan(y.view(np.float32)))).all())


def random_rows(rng, lst, shape, rng_max=0):
    """source bytes of a plane: every bit pattern for integer planes (below `rng_max` + 1 where the list wants a range), numbers
    in [0, 1) for float planes"""
    if lst.read.type == F32:
        return rng.random((shape[0], shape[1] // 4)).astype(np.float32).view(np.uint8)
    return rng.integers(0, (rng_max or 255) + 1, shape, dtype=np.uint8)


class RectCase:
    """a list, the size of its destination picture, its source planes and the destination planes it must produce"""

    def __init__(self, name, lst, w, h, src, want, rng_max=0):
        self.name, self.lst, self.w, self.h, self.src, self.want, self.rng_max = name, lst, w, h, src, want, rng_max
        self.f32 = lst.write.type == F32

    def bufs(self, frames=1, dst_fill=FILL, src_off=0, dst_off=0, tight=False):
        """(source Bufs with picture 0 filled in, destination Bufs holding the fill).  `tight`: line pitches of row bytes + 7 rounded
        up to the element, the least a caller may choose"""
        es, ed = SIZE[self.lst.read.type], SIZE[self.lst.write.type]
        tp = lambda rows, el: (rows + 7 + el - 1) // el * el if tight else None      # noqa: E731
        sb = [Buf(a.shape[1], a.shape[0], frames, src_off * es, tp(a.shape[1], es)) for a in self.src]
        db = [Buf(a.shape[1], a.shape[0], frames, dst_off * ed, tp(a.shape[1], ed), fill=dst_fill) for a in self.want]
        for b, a in zip(sb, self.src):
            b.payload(0)[:] = a
        return sb, db

    def randomise(self, rng, sb, frames):
        for b in sb:
            for f in frames:
                b.payload(f)[:] = random_rows(rng, self.lst, (b.lines, b.rows), self.rng_max)


def run_rects(call, case, block, sb, s_addrs, db, d_addrs, rects):
    """one call per rectangle: call(exec, bx_start, y_start, bx_end, y_end)"""
    for x0, x1, y0, y1 in rects:
        e = rect_exec(case.lst, s_addrs, [b.pitch for b in sb], d_addrs, [b.pitch for b in db], case.w, case.h, block, x0, x1, y0)
        call(e, x0 // block, y0, x1 // block, y1)


def oracle_into(g, case, sb, db, frames):
    """the oracle's whole-picture answer for pictures `frames` of the source Bufs, written into the same pictures of `db`"""
    h = C.c_void_p()
    assert g("compile")(case.lst.uops, case.lst.n, C.byref(h)) == 0, case.name
    bs = g("block_size")(h)
    for f in frames:
        e = plain_exec(case.lst, [b.flat.ctypes.data + b.off + f * b.fpitch for b in sb], [b.pitch for b in sb],
                       [b.flat.ctypes.data + b.off + f * b.fpitch for b in db], [b.pitch for b in db], case.w, case.h, bs)
        g("func")(C.byref(e), h, 0, 0, (case.w + bs - 1) // bs, case.h)
    g("free")(C.byref(h))


def oracle_pictures(g, case, sb, frames):
    """-> {frame: [destination planes]}"""
    db = [Buf(a.shape[1], a.shape[0], sb[0].frames) for a in case.want]
    oracle_into(g, case, sb, db, frames)
    assert all(b.outside_kept() for b in db), case.name
    return {f: [b.payload(f).copy() for b in db] for f in frames}


HAND_W, HAND_H = 88, 9      # whole 8-pixel blocks; 44 2-pixel blocks, so that the tiling's columns 2, 6 and 46 are off a thread's 4 pixels

_rect_cases = {}


def rect_cases(path, g):
    """the committed lists of real conversions (expectation: backend_c's committed output) and three hand-built lists for the 4-bit
    and 1-bit accesses the fixture lacks (expectation: the oracle `g` on the whole picture).  Built once; nobody writes into them.
    Pixel values are 0..15 / 0..15 / 0..1 as in checkasm's check_write: for the packed reads that is every byte pattern."""
    if path in _rect_cases:
        return _rect_cases[path]
    out = [RectCase("%s %dx%d-%dx%d" % ((name,) + size), lst, size[2], size[3], src, dst) for name, size, lst, src, dst in golden_cases(path)]
    rng = np.random.default_rng(4100)
    w, h = HAND_W, HAND_H
    for name, uops, rows_in, rows_out, rng_max in (
            ("hand nibble-read", [_mk(U8, READ_NIBBLE, 1), _mk(U8, WRITE_PLANAR, 1)], w // 2, w, 0),
            ("hand nibble-write", [_mk(U8, READ_PLANAR, 1), _mk(U8, WRITE_NIBBLE, 1)], w, w // 2, 15),
            ("hand bit-read", [_mk(U8, READ_BIT, 1), _mk(U8, WRITE_PLANAR, 1)], w // 8, w, 0)):
        lst = HandList(uops)
        case = RectCase(name, lst, w, h, [random_rows(rng, lst, (h, rows_in), rng_max)], [np.zeros((h, rows_out), np.uint8)], rng_max)
        sb, _ = case.bufs()
        case.want = oracle_pictures(g, case, sb, [0])[0]
        out.append(case)
    for c in out:
        for a in c.src + c.want:
            a.setflags(write=False)
    _rect_cases[path] = out
    return out


