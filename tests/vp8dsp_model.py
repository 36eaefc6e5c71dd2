"""A NumPy restatement of VP8DSPContext (libavcodec/vp8dsp.c, the VP8 members and the MC tables ff_vp78dsp_init fills) and of the frame
loop filter of libavcodec/vp8.c (filter_mb / filter_mb_simple over every macroblock in raster order), written as sequential calls of
the member model.  It is what the GPU faces are checked against byte for byte.  Each function names the reference function it
restates; roundings are spelled out where they happen.

Conventions: planes are 2-D uint8 arrays changed in place, a position is (y, x) of the sample the reference's dst points at;
coefficients are int16 arrays changed in place (the reference consumes them).  Intermediates the reference keeps in int16 (dc[] after
the WHT's first pass, the IDCT's tmp[]) wrap to 16 bits here too."""
import numpy as np

# subpel_filters[mx - 1] (vp8dsp.c): taps F0..F5 for the samples at -2..3
SUBPEL = np.array([[0, 6, 123, 12, 1, 0], [2, 11, 108, 36, 8, 1], [0, 9, 93, 50, 6, 0], [3, 16, 77, 77, 16, 3],
                   [0, 6, 50, 93, 9, 0], [1, 8, 36, 108, 11, 2], [0, 1, 12, 123, 6, 0]], np.int64)

# hev_thresh_lut[keyframe][filter_level] (vp8.c filter_mb): inter frames 1 from 15, 2 from 20, 3 from 40; key frames 1 from 15, 2 from 40
HEV_LUT = np.array([[0] * 15 + [1] * 5 + [2] * 20 + [3] * 24, [0] * 15 + [1] * 25 + [2] * 24], np.int64)


def s16(v):
    """the value an int16_t store keeps"""
    return ((np.asarray(v, np.int64) + 32768) & 0xFFFF) - 32768


# ---------------------------------------------------------------- transforms
def luma_dc_wht(block, dc):
    """vp8_luma_dc_wht_c: block = int16 [16, 16] (block[i][j] is row 16 * (4 i + j)), dc = int16 [16].  Columns first, the results
    stored back into dc[] (int16); then rows, +3 on the t0 / t3 paths, >> 3, into block[4 i + j][0]; dc[] zeroed."""
    d = dc.astype(np.int64)
    for i in range(4):
        t0, t1 = d[i] + d[12 + i], d[4 + i] + d[8 + i]
        t2, t3 = d[4 + i] - d[8 + i], d[i] - d[12 + i]
        d[i], d[4 + i], d[8 + i], d[12 + i] = s16(t0 + t1), s16(t3 + t2), s16(t0 - t1), s16(t3 - t2)
    for i in range(4):
        t0, t1 = d[4 * i] + d[4 * i + 3] + 3, d[4 * i + 1] + d[4 * i + 2]
        t2, t3 = d[4 * i + 1] - d[4 * i + 2], d[4 * i] - d[4 * i + 3] + 3
        block[4 * i + 0, 0] = s16((t0 + t1) >> 3)
        block[4 * i + 1, 0] = s16((t3 + t2) >> 3)
        block[4 * i + 2, 0] = s16((t0 - t1) >> 3)
        block[4 * i + 3, 0] = s16((t3 - t2) >> 3)
    dc[:] = 0


def luma_dc_wht_dc(block, dc):
    """vp8_luma_dc_wht_dc_c: (dc[0] + 3) >> 3 into all 16 block[..][0]; dc[0] zeroed"""
    val = (int(dc[0]) + 3) >> 3
    dc[0] = 0
    block[:, 0] = s16(val)


def _mul20091(a):
    return ((a * 20091) >> 16) + a


def _mul35468(a):
    return (a * 35468) >> 16


def idct_residual(block):
    """the 4 x 4 values vp8_idct_add_c adds (rows), the first pass (down the columns) kept in an int16 tmp[]; (x + 4) >> 3 at the end"""
    b = block.astype(np.int64).reshape(4, 4)   # b[r, c] = block[4 r + c]
    t0, t1 = b[0] + b[2], b[0] - b[2]
    t2 = _mul35468(b[1]) - _mul20091(b[3])
    t3 = _mul20091(b[1]) + _mul35468(b[3])
    tmp = s16(np.stack([t0 + t3, t1 + t2, t1 - t2, t0 - t3]))   # tmp[k, c]: column c's k-th output (the reference's tmp[4 c + k])
    t0, t1 = tmp[:, 0] + tmp[:, 2], tmp[:, 0] - tmp[:, 2]       # indexed by row k
    t2 = _mul35468(tmp[:, 1]) - _mul20091(tmp[:, 3])
    t3 = _mul20091(tmp[:, 1]) + _mul35468(tmp[:, 3])
    return np.stack([(t0 + t3 + 4) >> 3, (t1 + t2 + 4) >> 3, (t1 - t2 + 4) >> 3, (t0 - t3 + 4) >> 3], axis=1)


def _add(plane, y, x, res):
    h, w = res.shape
    plane[y:y + h, x:x + w] = np.clip(plane[y:y + h, x:x + w].astype(np.int64) + res, 0, 255)


def idct_add(plane, y, x, block):
    """vp8_idct_add_c: adds the inverse transform, all 16 coefficients zeroed"""
    _add(plane, y, x, idct_residual(block))
    block[:] = 0


def idct_dc_add(plane, y, x, block):
    """vp8_idct_dc_add_c: adds (block[0] + 4) >> 3, block[0] zeroed"""
    dc = (int(block[0]) + 4) >> 3
    block[0] = 0
    _add(plane, y, x, np.full((4, 4), dc, np.int64))


def idct_dc_add4y(plane, y, x, blocks):
    """vp8_idct_dc_add4y_c: blocks [4, 16] at +0, +4, +8, +12 samples"""
    for i in range(4):
        idct_dc_add(plane, y, x + 4 * i, blocks[i])


def idct_dc_add4uv(plane, y, x, blocks):
    """vp8_idct_dc_add4uv_c: blocks [4, 16] at (0, 0), (0, 4), (4, 0), (4, 4)"""
    for i in range(4):
        idct_dc_add(plane, y + 4 * (i >> 1), x + 4 * (i & 1), blocks[i])


# ---------------------------------------------------------------- loop filters
MBEDGE, INNER, SIMPLE = 0, 1, 2


def filter_lines(L, kind, E, I, H):
    """the lines L = int64 [8, n] (rows p3 p2 p1 p0 q0 q1 q2 q3, a line per column) after one member's per-line rule:
       simple_limit: 2|p0 - q0| + (|p1 - q1| >> 1) <= E; normal_limit adds |p3-p2|, |p2-p1|, |p1-p0|, |q3-q2|, |q2-q1|, |q1-q0| <= I;
       hev: |p1 - p0| > H or |q1 - q0| > H;
       filter_common(is4tap): a = clip_int8(3 (q0 - p0) [+ clip_int8(p1 - q1)]), f1 = min(a + 4, 127) >> 3, f2 = min(a + 3, 127) >> 3,
         p0 + f2, q0 - f1 clamped to 0..255 (cm[]); not is4tap: also p1 + (f1 + 1) >> 1, q1 - the same;
       filter_mbedge: w = clip_int8(clip_int8(p1 - q1) + 3 (q0 - p0)), (27 w + 63) >> 7, (18 w + 63) >> 7, (9 w + 63) >> 7 on p0 / q0,
         p1 / q1, p2 / q2.
     MB-edge members (vp8_{v,h}_loop_filter16y / 8uv): hev ? common(4-tap) : mbedge; inner members: common(is4tap = hev); simple
     members: simple_limit only, then common(4-tap)."""
    p3, p2, p1, p0, q0, q1, q2, q3 = L
    c8 = lambda v: np.clip(v, -128, 127)   # noqa: E731  clip_int8
    u8 = lambda v: np.clip(v, 0, 255)      # noqa: E731  cm[]
    on = 2 * np.abs(p0 - q0) + (np.abs(p1 - q1) >> 1) <= E
    if kind != SIMPLE:
        for a, b in ((p3, p2), (p2, p1), (p1, p0), (q3, q2), (q2, q1), (q1, q0)):
            on &= np.abs(a - b) <= I
        hv = (np.abs(p1 - p0) > H) | (np.abs(q1 - q0) > H)
    else:
        hv = np.ones_like(on)
    out = L.copy()
    # filter_common, 4-tap where hv, 2-tap (p1 / q1 too) elsewhere
    a = c8(3 * (q0 - p0) + np.where(hv, c8(p1 - q1), 0))
    f1, f2 = np.minimum(a + 4, 127) >> 3, np.minimum(a + 3, 127) >> 3
    cp0, cq0 = u8(p0 + f2), u8(q0 - f1)
    b = (f1 + 1) >> 1
    cp1, cq1 = np.where(hv, p1, u8(p1 + b)), np.where(hv, q1, u8(q1 - b))
    if kind == MBEDGE:
        w = c8(c8(p1 - q1) + 3 * (q0 - p0))
        a0, a1, a2 = (27 * w + 63) >> 7, (18 * w + 63) >> 7, (9 * w + 63) >> 7
        m = on & ~hv
        c = on & hv
        out[1] = np.where(m, u8(p2 + a2), p2)
        out[2] = np.where(m, u8(p1 + a1), p1)
        out[3] = np.where(m, u8(p0 + a0), np.where(c, cp0, p0))
        out[4] = np.where(m, u8(q0 - a0), np.where(c, cq0, q0))
        out[5] = np.where(m, u8(q1 - a1), q1)
        out[6] = np.where(m, u8(q2 - a2), q2)
    else:
        out[2] = np.where(on, cp1, p1)
        out[3] = np.where(on, cp0, p0)
        out[4] = np.where(on, cq0, q0)
        out[5] = np.where(on, cq1, q1)
    return out


def loop_filter(plane, y, x, vertical, n, kind, E, I=0, H=0):
    """one loop-filter member on `n` lines at (y, x): vertical (the v_ members, strideb = stride) filters the row edge above (y, x)
    for columns x .. x + n - 1; otherwise (h_) the column edge left of (y, x) for rows y .. y + n - 1"""
    if vertical:
        view = plane[y - 4:y + 4, x:x + n]
        view[:] = filter_lines(view.astype(np.int64), kind, E, I, H)
    else:
        view = plane[y:y + n, x - 4:x + 4]
        view[:] = filter_lines(view.astype(np.int64).T, kind, E, I, H).T


def v_loop_filter16y(p, y, x, E, I, H): loop_filter(p, y, x, True, 16, MBEDGE, E, I, H)          # noqa: E704
def h_loop_filter16y(p, y, x, E, I, H): loop_filter(p, y, x, False, 16, MBEDGE, E, I, H)         # noqa: E704
def v_loop_filter16y_inner(p, y, x, E, I, H): loop_filter(p, y, x, True, 16, INNER, E, I, H)     # noqa: E704
def h_loop_filter16y_inner(p, y, x, E, I, H): loop_filter(p, y, x, False, 16, INNER, E, I, H)    # noqa: E704
def v_loop_filter_simple(p, y, x, E): loop_filter(p, y, x, True, 16, SIMPLE, E)                  # noqa: E704
def h_loop_filter_simple(p, y, x, E): loop_filter(p, y, x, False, 16, SIMPLE, E)                 # noqa: E704


def v_loop_filter8uv(u, v, y, x, E, I, H):
    loop_filter(u, y, x, True, 8, MBEDGE, E, I, H)
    loop_filter(v, y, x, True, 8, MBEDGE, E, I, H)


def h_loop_filter8uv(u, v, y, x, E, I, H):
    loop_filter(u, y, x, False, 8, MBEDGE, E, I, H)
    loop_filter(v, y, x, False, 8, MBEDGE, E, I, H)


def v_loop_filter8uv_inner(u, v, y, x, E, I, H):
    loop_filter(u, y, x, True, 8, INNER, E, I, H)
    loop_filter(v, y, x, True, 8, INNER, E, I, H)


def h_loop_filter8uv_inner(u, v, y, x, E, I, H):
    loop_filter(u, y, x, False, 8, INNER, E, I, H)
    loop_filter(v, y, x, False, 8, INNER, E, I, H)


# ---------------------------------------------------------------- MC
def put(src, sy, sx, w, h, mx, my, vsel, hsel, bilinear):
    """put_vp8_epel_pixels_tab / put_vp8_bilinear_pixels_tab[.][vsel][hsel](dst, ., src + sy * stride + sx, ., h, mx, my): the h x w
    block it writes (uint8).  Epel: FILTER_6TAP = cm[(F2 s0 - F1 s-1 + F0 s-2 + F3 s1 - F4 s2 + F5 s3 + 64) >> 7], FILTER_4TAP drops F0 and
    F5; a 2-D call filters h + 5 (6-tap vertical, from 2 rows up) or h + 3 (4-tap, from 1 row up) rows into a uint8 temporary first.
    Bilinear: ((8 - m) a + m b + 4) >> 3, 2-D through h + 1 temporary rows.  Slot 0 along both axes: a copy."""
    s = src.astype(np.int64)
    if not vsel and not hsel:
        return src[sy:sy + h, sx:sx + w].copy()
    if bilinear:
        def hpass(y0, rows):
            a = s[y0:y0 + rows, sx:sx + w]
            b = s[y0:y0 + rows, sx + 1:sx + w + 1]
            return ((8 - mx) * a + mx * b + 4) >> 3

        def vpass(t):
            return ((8 - my) * t[:-1] + my * t[1:] + 4) >> 3
        if hsel and vsel:
            return vpass(hpass(sy, h + 1)).astype(np.uint8)
        if hsel:
            return hpass(sy, h).astype(np.uint8)
        return vpass(s[sy:sy + h + 1, sx:sx + w]).astype(np.uint8)

    def taps(F, six, get):
        acc = F[2] * get(0) - F[1] * get(-1) + F[3] * get(1) - F[4] * get(2)
        if six:
            acc = acc + F[0] * get(-2) + F[5] * get(3)
        return np.clip((acc + 64) >> 7, 0, 255)

    def hpass(y0, rows):
        return taps(SUBPEL[mx - 1], hsel == 2, lambda k: s[y0:y0 + rows, sx + k:sx + k + w])

    if hsel and vsel:
        before = 2 if vsel == 2 else 1
        t = hpass(sy - before, h + (5 if vsel == 2 else 3))
        return taps(SUBPEL[my - 1], vsel == 2, lambda k: t[before + k:before + k + h]).astype(np.uint8)
    if hsel:
        return hpass(sy, h).astype(np.uint8)
    return taps(SUBPEL[my - 1], vsel == 2, lambda k: s[sy + k:sy + k + h, sx:sx + w]).astype(np.uint8)


# ---------------------------------------------------------------- the frame loop filter (vp8.c)
def strength_ok(level, inner_limit, inner_filter):
    """the face's reading of a record: anything filter_level_for_mb() cannot leave counts as level 0"""
    return 0 < level <= 63 and inner_limit <= 63 and inner_filter <= 1


def filter_mb(Y, U, V, mb_x, mb_y, level, inner_limit, inner_filter, keyframe):
    """filter_mb (vp8.c, VP8): the left MB edge, the inner column edges, the top MB edge, the inner row edges"""
    if not level:
        return
    bedge = 2 * level + inner_limit
    mbedge = bedge + 4
    H = int(HEV_LUT[keyframe][level])
    y, x, cy, cx = 16 * mb_y, 16 * mb_x, 8 * mb_y, 8 * mb_x
    if mb_x:
        h_loop_filter16y(Y, y, x, mbedge, inner_limit, H)
        h_loop_filter8uv(U, V, cy, cx, mbedge, inner_limit, H)
    if inner_filter:
        for k in (4, 8, 12):
            h_loop_filter16y_inner(Y, y, x + k, bedge, inner_limit, H)
        h_loop_filter8uv_inner(U, V, cy, cx + 4, bedge, inner_limit, H)
    if mb_y:
        v_loop_filter16y(Y, y, x, mbedge, inner_limit, H)
        v_loop_filter8uv(U, V, cy, cx, mbedge, inner_limit, H)
    if inner_filter:
        for k in (4, 8, 12):
            v_loop_filter16y_inner(Y, y + k, x, bedge, inner_limit, H)
        v_loop_filter8uv_inner(U, V, cy + 4, cx, bedge, inner_limit, H)


def filter_mb_simple(Y, mb_x, mb_y, level, inner_limit, inner_filter):
    """filter_mb_simple (vp8.c): luma only, mbedge_lim on the MB edges, bedge_lim inside"""
    if not level:
        return
    bedge = 2 * level + inner_limit
    mbedge = bedge + 4
    y, x = 16 * mb_y, 16 * mb_x
    if mb_x:
        h_loop_filter_simple(Y, y, x, mbedge)
    if inner_filter:
        for k in (4, 8, 12):
            h_loop_filter_simple(Y, y, x + k, bedge)
    if mb_y:
        v_loop_filter_simple(Y, y, x, mbedge)
    if inner_filter:
        for k in (4, 8, 12):
            v_loop_filter_simple(Y, y + k, x, bedge)


def loop_filter_frame(Y, U, V, strength, filter_type, keyframe):
    """every macroblock in raster order (filter_mb_row over every row); strength = STRENGTH records [mb_h, mb_w] (structured array or
    an int array [..., 3]); planes of mb_w * 16 x mb_h * 16 (chroma * 8) samples, changed in place"""
    st = np.asarray(strength)
    if st.dtype.names:
        st = np.stack([st["filter_level"], st["inner_limit"], st["inner_filter"]], axis=-1)
    mb_h, mb_w = st.shape[:2]
    for mb_y in range(mb_h):
        for mb_x in range(mb_w):
            level, il, inner = (int(v) for v in st[mb_y, mb_x])
            if not strength_ok(level, il, inner):
                continue
            if filter_type == 0:
                filter_mb(Y, U, V, mb_x, mb_y, level, il, inner, keyframe)
            else:
                filter_mb_simple(Y, mb_x, mb_y, level, il, inner)
