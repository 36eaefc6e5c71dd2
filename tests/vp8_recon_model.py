"""A NumPy model of VP8 macroblock reconstruction (libavcodec/vp8.c: inter_predict / intra_predict / idct_mb over the records of
ffhip_vp8_recon_frames_dev, include/ffhip.h), on top of vp8dsp_model's put / idct_add / idct_dc_add / luma_dc_wht*.  Two statements of
the same frame:

 (a) recon_frame(): the plane rule.  Reference coordinates are clamped to the plane; intra prediction sees a virtual border (127 above,
     (-1, -1) included, 129 to the left) and always evaluates the mode the record names.
 (b) recon_frame_ptr(): the route the reference takes with pointers.  Inter: an edge-replicated padded copy of the reference is read
     directly where the block with its subpel_idx margins lies inside the plane, and through an emulated_edge_mc buffer otherwise.
     Intra: the mode substitutions of check_intra_pred8x8_mode_emuedge / check_intra_pred4x4_mode_emuedge, the 5 x 8 copy_dst buffer
     and tr_right; the frame sits in a margin of 0xEE bytes, so a read the substitutions should have avoided shows.

The VP8 prediction forms (h264pred.c / h264pred_template.c as ff_h264_pred_init installs them for VP8) are restated here."""
import numpy as np

import vp8dsp_model as M

PRED_DC, PRED_HOR, PRED_VERT, PRED_TM, MODE_I4x4 = 0, 1, 2, 3, 4
PRED_LEFT_DC, PRED_TOP_DC, PRED_DC_128, PRED_DC_127, PRED_DC_129 = 4, 5, 6, 7, 8
PRED_NONE = 255   # no pred16x16[] slot: an I4x4 macroblock (4 is LEFT_DC's slot)
B_VERT, B_HOR, B_DC, B_DDL, B_DDR, B_VR, B_HD, B_VL, B_HU, B_TM = range(10)
B_VERT_PLAIN, B_DC_127, B_DC_129, B_HOR_PLAIN = 10, 12, 13, 14
PART_NONE, PART_16x8, PART_8x16, PART_8x8, PART_4x4 = range(5)
MB_COEFFS = 400
SUBPEL_IDX = [[0, 1, 2, 1, 2, 1, 2, 1], [0, 3, 5, 3, 5, 3, 5, 3], [0, 2, 3, 2, 3, 2, 3, 2]]   # vp8.c subpel_idx


def code(mb, b):
    return (int(mb["block_code"][b >> 2]) >> (2 * (b & 3))) & 3


def coded(mb):
    return bool(mb["y2"]) or any(int(c) for c in mb["block_code"])


def well_formed(mb, refs, coeff_count):
    if mb["ref_frame"] > 3 or mb["y2"] > 2:
        return False
    if mb["ref_frame"]:
        r = refs[mb["ref_frame"] - 1] if mb["ref_frame"] - 1 < len(refs) else None
        if r is None or mb["partitioning"] > 4:
            return False
    else:
        if mb["mode"] > 4 or mb["chroma_mode"] > 3 or (mb["mode"] == 4 and (mb["sub_mode"] > 9).any()):
            return False
    if any(code(mb, b) == 3 for b in range(24)):
        return False
    co = int(mb["coeff_offset"])
    if coded(mb) and (co < 0 or co % 16 or co + MB_COEFFS > coeff_count):
        return False
    return True


# ---------------------------------------------------------------- inter: the calls
def _luma_call(mb_x, mb_y, x, y, w, h, mv):
    mvx, mvy = int(mv[0]), int(mv[1])
    mx, my = (mvx * 2) & 7, (mvy * 2) & 7
    return dict(plane=0, x=x, y=y, w=w, h=h, mx=mx, my=my, vslot=SUBPEL_IDX[0][my], hslot=SUBPEL_IDX[0][mx],
                sx=16 * mb_x + x + (mvx >> 2), sy=16 * mb_y + y + (mvy >> 2))


def _chroma_calls(mb_x, mb_y, x, y, w, h, mvx, mvy, fullpel):
    if fullpel:
        mvx, mvy = mvx & ~7, mvy & ~7
    mx, my = mvx & 7, mvy & 7
    return [dict(plane=p, x=x, y=y, w=w, h=h, mx=mx, my=my, vslot=SUBPEL_IDX[0][my], hslot=SUBPEL_IDX[0][mx],
                 sx=8 * mb_x + x + (mvx >> 3), sy=8 * mb_y + y + (mvy >> 3)) for p in (1, 2)]


def mb_preds(mb, mb_x, mb_y, fullpel):
    """inter_predict(): the vp8_mc_luma / vp8_mc_chroma calls in its order"""
    mv, part, out = mb["mv"], int(mb["partitioning"]), []
    if part == PART_4x4:
        for i in range(16):
            out.append(_luma_call(mb_x, mb_y, 4 * (i & 3), 4 * (i >> 2), 4, 4, mv[i]))
        for cy in range(2):
            for cx in range(2):
                s = []
                for k in range(2):
                    t = sum(int(mv[(2 * cy + dy) * 4 + 2 * cx + dx][k]) for dy in range(2) for dx in range(2))
                    s.append((t + 2 + (-1 if t < 0 else 0)) >> 2)   # FF_SIGNBIT
                out += _chroma_calls(mb_x, mb_y, 4 * cx, 4 * cy, 4, 4, s[0], s[1], fullpel)
        return out
    parts = {PART_NONE: [(0, 0, 16, 16)], PART_16x8: [(0, 0, 16, 8), (0, 8, 16, 8)], PART_8x16: [(0, 0, 8, 16), (8, 0, 8, 16)],
             PART_8x8: [(0, 0, 8, 8), (8, 0, 8, 8), (0, 8, 8, 8), (8, 8, 8, 8)]}[part]
    for i, (x, y, w, h) in enumerate(parts):   # vp8_mc_part
        out.append(_luma_call(mb_x, mb_y, x, y, w, h, mv[i]))
        out += _chroma_calls(mb_x, mb_y, x // 2, y // 2, w // 2, h // 2, int(mv[i][0]), int(mv[i][1]), fullpel)
    return out


def _mc_clamped(ref, c, bilinear):
    """(a): every coordinate clamped to the plane"""
    H, W = ref.shape
    ys = np.clip(np.arange(c["sy"] - 2, c["sy"] + c["h"] + 3), 0, H - 1)
    xs = np.clip(np.arange(c["sx"] - 2, c["sx"] + c["w"] + 3), 0, W - 1)
    return M.put(ref[np.ix_(ys, xs)], 2, 2, c["w"], c["h"], c["mx"], c["my"], c["vslot"], c["hslot"], bilinear)


PAD = 32


def _mc_ptr(ref, padded, c, bilinear):
    """(b): vp8_mc_luma / vp8_mc_chroma: the padded reference read in place unless the block with its margins leaves the plane"""
    H, W = ref.shape
    sx, sy, w, h, mx, my = c["sx"], c["sy"], c["w"], c["h"], c["mx"], c["my"]
    if not (mx or my) and not _moved(c):
        return padded[PAD + sy:PAD + sy + h, PAD + sx:PAD + sx + w].copy()
    if (sx < SUBPEL_IDX[0][mx] or sx >= W - w - SUBPEL_IDX[2][mx] or sy < SUBPEL_IDX[0][my] or sy >= H - h - SUBPEL_IDX[2][my]):
        # emulated_edge_mc(buf, src - my_idx * stride - mx_idx, ., block_w + subpel_idx[1][mx], block_h + subpel_idx[1][my], ...)
        x0, y0 = sx - SUBPEL_IDX[0][mx], sy - SUBPEL_IDX[0][my]
        bw, bh = w + SUBPEL_IDX[1][mx], h + SUBPEL_IDX[1][my]
        buf = ref[np.ix_(np.clip(np.arange(y0, y0 + bh), 0, H - 1), np.clip(np.arange(x0, x0 + bw), 0, W - 1))]
        buf = np.pad(buf, ((0, 3), (0, 3)), constant_values=0xEE)   # what the call must not read
        return M.put(buf, SUBPEL_IDX[0][my], SUBPEL_IDX[0][mx], w, h, mx, my, c["vslot"], c["hslot"], bilinear)
    return M.put(padded, PAD + sy, PAD + sx, w, h, mx, my, c["vslot"], c["hslot"], bilinear)


def _moved(c):
    return c.get("moved", True)


# ---------------------------------------------------------------- residuals
def _add_residuals(planes, mb, mb_x, mb_y, coeffs, only=None):
    """idct_mb(): the WHT per y2 into the luma DCs, then each block per its code (`only`: one luma block, for I4x4)"""
    if not coded(mb):
        return
    co = coeffs[int(mb["coeff_offset"]):int(mb["coeff_offset"]) + MB_COEFFS].astype(np.int16).copy()
    blocks, dc = co[:384].reshape(24, 16), co[384:400]
    if mb["y2"] == 1:
        M.luma_dc_wht_dc(blocks[:16], dc)
    elif mb["y2"] == 2:
        M.luma_dc_wht(blocks[:16], dc)
    for b in range(24) if only is None else [only]:
        c = code(mb, b)
        if not c:
            continue
        if b < 16:
            P, y, x = planes[0], 16 * mb_y + 4 * (b >> 2), 16 * mb_x + 4 * (b & 3)
        else:
            q = (b - 16) & 3
            P, y, x = planes[1 + ((b - 16) >> 2)], 8 * mb_y + 4 * (q >> 1), 8 * mb_x + 4 * (q & 1)
        (M.idct_dc_add if c == 1 else M.idct_add)(P, y, x, blocks[b])


# ---------------------------------------------------------------- intra: the forms
def _a3(a, b, c):
    return (a + 2 * b + c + 2) >> 2


def _a2(a, b):
    return (a + b + 1) >> 1


def pred4x4(slot, t, l, lt):
    """pred4x4[slot] of VP8: t = the row above and the top-right (8), l = the left column (4), lt = the corner; out[y][x]"""
    t, l, lt = [int(v) for v in t], [int(v) for v in l], int(lt)
    o = np.zeros((4, 4), np.int64)
    if slot == B_DC_127:
        o[:] = 127
    elif slot == B_DC_129:
        o[:] = 129
    elif slot == B_VERT:          # pred4x4_vertical_vp8_c
        o[:] = [_a3(lt, t[0], t[1]), _a3(t[0], t[1], t[2]), _a3(t[1], t[2], t[3]), _a3(t[2], t[3], t[4])]
    elif slot == B_HOR:           # pred4x4_horizontal_vp8_c
        o[0], o[1], o[2], o[3] = _a3(lt, l[0], l[1]), _a3(l[0], l[1], l[2]), _a3(l[1], l[2], l[3]), _a3(l[2], l[3], l[3])
    elif slot == B_VERT_PLAIN:
        o[:] = t[:4]
    elif slot == B_HOR_PLAIN:
        o[:] = np.array(l)[:, None]
    elif slot == B_DC:
        o[:] = (sum(t[:4]) + sum(l) + 4) >> 3
    elif slot == B_TM:            # pred4x4_tm_vp8_c
        o[:] = np.clip(np.array(l)[:, None] + np.array(t[:4])[None, :] - lt, 0, 255)
    elif slot == B_DDL:
        for y in range(4):
            for x in range(4):
                i = x + y
                o[y, x] = _a3(t[i], t[i + 1], t[i + 2]) if i < 6 else _a3(t[6], t[7], t[7])
    elif slot == B_DDR:
        e = [l[3], l[2], l[1], l[0], lt] + t[:4]
        for y in range(4):
            for x in range(4):
                i = 3 - y + x
                o[y, x] = _a3(e[i], e[i + 1], e[i + 2])
    elif slot == B_VR:            # o[y][x] below is written src(x, y) in h264pred_template.c
        o[0, 0] = o[2, 1] = _a2(lt, t[0]); o[1, 0] = o[3, 1] = _a3(l[0], lt, t[0])
        o[0, 1] = o[2, 2] = _a2(t[0], t[1]); o[1, 1] = o[3, 2] = _a3(lt, t[0], t[1])
        o[0, 2] = o[2, 3] = _a2(t[1], t[2]); o[1, 2] = o[3, 3] = _a3(t[0], t[1], t[2])
        o[0, 3] = _a2(t[2], t[3]); o[1, 3] = _a3(t[1], t[2], t[3])
        o[2, 0] = _a3(lt, l[0], l[1]); o[3, 0] = _a3(l[0], l[1], l[2])
    elif slot == B_HD:
        o[0, 0] = o[1, 2] = _a2(lt, l[0]); o[0, 1] = o[1, 3] = _a3(l[0], lt, t[0])
        o[0, 2] = _a3(lt, t[0], t[1]); o[0, 3] = _a3(t[0], t[1], t[2])
        o[1, 0] = o[2, 2] = _a2(l[0], l[1]); o[1, 1] = o[2, 3] = _a3(lt, l[0], l[1])
        o[2, 0] = o[3, 2] = _a2(l[1], l[2]); o[2, 1] = o[3, 3] = _a3(l[0], l[1], l[2])
        o[3, 0] = _a2(l[2], l[3]); o[3, 1] = _a3(l[1], l[2], l[3])
    elif slot == B_VL:            # pred4x4_vertical_left_vp8_c
        o[0, 0] = _a2(t[0], t[1]); o[0, 1] = o[2, 0] = _a2(t[1], t[2]); o[0, 2] = o[2, 1] = _a2(t[2], t[3]); o[0, 3] = o[2, 2] = _a2(t[3], t[4])
        o[1, 0] = _a3(t[0], t[1], t[2]); o[1, 1] = o[3, 0] = _a3(t[1], t[2], t[3]); o[1, 2] = o[3, 1] = _a3(t[2], t[3], t[4])
        o[1, 3] = o[3, 2] = _a3(t[3], t[4], t[5])
        o[2, 3] = _a3(t[4], t[5], t[6]); o[3, 3] = _a3(t[5], t[6], t[7])
    elif slot == B_HU:
        o[0, 0] = _a2(l[0], l[1]); o[0, 1] = _a3(l[0], l[1], l[2]); o[0, 2] = o[1, 0] = _a2(l[1], l[2]); o[0, 3] = o[1, 1] = _a3(l[1], l[2], l[3])
        o[1, 2] = o[2, 0] = _a2(l[2], l[3]); o[1, 3] = o[2, 1] = _a3(l[2], l[3], l[3])
        o[2, 2] = o[2, 3] = o[3, 0] = o[3, 1] = o[3, 2] = o[3, 3] = l[3]
    else:
        raise ValueError(slot)
    return o.astype(np.uint8)


def pred_blk(N, slot, t, l, lt):
    """pred16x16[slot] (H.264's DC forms) / pred8x8[slot] (the RV40 DC forms) of VP8: t, l = N samples each"""
    t, l = np.asarray(t, np.int64), np.asarray(l, np.int64)
    o = np.zeros((N, N), np.int64)
    sh = 4 if N == 16 else 3
    if slot == PRED_DC:
        o[:] = (t.sum() + l.sum() + N) >> (sh + 1)
    elif slot == PRED_LEFT_DC:
        o[:] = (l.sum() + N // 2) >> sh
    elif slot == PRED_TOP_DC:
        o[:] = (t.sum() + N // 2) >> sh
    elif slot in (PRED_DC_128, PRED_DC_127, PRED_DC_129):
        o[:] = {PRED_DC_128: 128, PRED_DC_127: 127, PRED_DC_129: 129}[slot]
    elif slot == PRED_VERT:
        o[:] = t[None, :]
    elif slot == PRED_HOR:
        o[:] = l[:, None]
    elif slot == PRED_TM:
        o[:] = np.clip(l[:, None] + t[None, :] - int(lt), 0, 255)
    else:
        raise ValueError(slot)
    return o.astype(np.uint8)


# ---------------------------------------------------------------- intra: the substitutions (vp8.c check_*_mode*)
def blk_slot(mode, mb_x, mb_y):
    if mode == PRED_DC:
        return (PRED_TOP_DC if mb_y else PRED_DC_128) if not mb_x else (mode if mb_y else PRED_LEFT_DC)
    if mode == PRED_VERT:
        return mode if mb_y else PRED_DC_127
    if mode == PRED_HOR:
        return mode if mb_x else PRED_DC_129
    if mode == PRED_TM:
        return (PRED_VERT if mb_y else PRED_DC_129) if not mb_x else (mode if mb_y else PRED_HOR)
    raise ValueError(mode)


def sub_slot(mode, bx, by):
    """(slot, copy) for a sub-block in column bx / row by of the frame's sub-blocks"""
    if mode == B_VERT and not bx and by:
        return mode, 1
    if mode in (B_VERT, B_DDL, B_VL):
        return (mode if by else B_DC_127), 0
    if mode == B_HOR and not by:
        return mode, 1
    if mode in (B_HOR, B_HU):
        return (mode if bx else B_DC_129), 0
    if mode == B_TM:
        return ((B_VERT_PLAIN if by else B_DC_129) if not bx else (mode if by else B_HOR_PLAIN)), 0
    return mode, int(not by or not bx)


def intra_modes(mb, mb_x, mb_y):
    i4 = mb["mode"] == MODE_I4x4
    subs = [sub_slot(int(mb["sub_mode"][i]), 4 * mb_x + (i & 3), 4 * mb_y + (i >> 2)) if i4 else (0, 0) for i in range(16)]
    return dict(mode16=PRED_NONE if i4 else blk_slot(int(mb["mode"]), mb_x, mb_y), chroma=blk_slot(int(mb["chroma_mode"]), mb_x, mb_y),
                sub=[s for s, _ in subs], copy=[c for _, c in subs])


# ---------------------------------------------------------------- (a) the plane rule
def _border(P, y, x):
    """sample (y, x) of a plane with the virtual border"""
    if y < 0:
        return 127
    if x < 0:
        return 129
    return int(P[y, x])


def _intra_plane(planes, mb, mb_x, mb_y, mb_w, coeffs):
    for p, N, mode in ((1, 8, int(mb["chroma_mode"])), (2, 8, int(mb["chroma_mode"])), (0, 16, int(mb["mode"]))):
        P, y0, x0 = planes[p], N * mb_y, N * mb_x
        if mode == MODE_I4x4:
            continue
        t = [_border(P, y0 - 1, x0 + i) for i in range(N)]
        l = [_border(P, y0 + i, x0 - 1) for i in range(N)]
        if mode == PRED_DC:   # only the sides that exist
            slot = (PRED_TOP_DC if mb_y else PRED_DC_128) if not mb_x else (PRED_DC if mb_y else PRED_LEFT_DC)
        else:
            slot = mode
        P[y0:y0 + N, x0:x0 + N] = pred_blk(N, slot, t, l, _border(P, y0 - 1, x0 - 1))
    if mb["mode"] != MODE_I4x4:
        _add_residuals(planes, mb, mb_x, mb_y, coeffs)
        return
    Y, y0, x0 = planes[0], 16 * mb_y, 16 * mb_x
    # the four samples above-right of the macroblock
    if mb_y == 0:
        tr = [127] * 4
    elif mb_x == mb_w - 1:
        tr = [int(Y[y0 - 1, x0 + 15])] * 4
    else:
        tr = [int(v) for v in Y[y0 - 1, x0 + 16:x0 + 20]]
    for b in range(16):
        bx, by = b & 3, b >> 2
        y, x = y0 + 4 * by, x0 + 4 * bx
        t = [_border(Y, y - 1, x + i) for i in range(4)] + (tr if bx == 3 else [_border(Y, y - 1, x + 4 + i) for i in range(4)])
        l = [_border(Y, y + i, x - 1) for i in range(4)]
        Y[y:y + 4, x:x + 4] = pred4x4(int(mb["sub_mode"][b]), t, l, _border(Y, y - 1, x - 1))
        _add_residuals(planes, mb, mb_x, mb_y, coeffs, only=b)
    for b in range(16, 24):
        _add_residuals(planes, mb, mb_x, mb_y, coeffs, only=b)


def recon_frame(planes, mbs, coeffs, refs, mb_w, mb_h, bilinear=0, fullpel=0):
    """(a).  planes = [Y, U, V] uint8 arrays of the frame's size, changed in place (a malformed record leaves its bytes); mbs = MB
    records [mb_h * mb_w]; refs = up to three [Y, U, V] lists (or None)"""
    for m in range(mb_w * mb_h):
        mb, mb_x, mb_y = mbs[m], m % mb_w, m // mb_w
        if not well_formed(mb, refs, len(coeffs)):
            continue
        if mb["ref_frame"]:
            ref = refs[mb["ref_frame"] - 1]
            for c in mb_preds(mb, mb_x, mb_y, fullpel):
                N = 8 if c["plane"] else 16
                planes[c["plane"]][N * mb_y + c["y"]:N * mb_y + c["y"] + c["h"], N * mb_x + c["x"]:N * mb_x + c["x"] + c["w"]] = \
                    _mc_clamped(ref[c["plane"]], c, bilinear)
            _add_residuals(planes, mb, mb_x, mb_y, coeffs)
        else:
            _intra_plane(planes, mb, mb_x, mb_y, mb_w, coeffs)
    return planes


# ---------------------------------------------------------------- (b) the pointer route
MARGIN = 8


def _intra_ptr(G, mb, mb_x, mb_y, mb_w, planes, coeffs):
    """intra_predict(): G = the planes inside a margin of 0xEE bytes; planes = views of their frames"""
    o = MARGIN
    for p, N, mode in ((0, 16, int(mb["mode"])), (1, 8, int(mb["chroma_mode"])), (2, 8, int(mb["chroma_mode"]))):
        if mode == MODE_I4x4:
            continue
        A, y0, x0 = G[p], o + N * mb_y, o + N * mb_x
        slot = blk_slot(mode, mb_x, mb_y)
        A[y0:y0 + N, x0:x0 + N] = pred_blk(N, slot, A[y0 - 1, x0:x0 + N], A[y0:y0 + N, x0 - 1], A[y0 - 1, x0 - 1])
    if mb["mode"] == MODE_I4x4:
        A, y0, x0 = G[0], o + 16 * mb_y, o + 16 * mb_x
        lo, hi = 127, 129
        tr_top = [lo] * 4
        tr_right = [int(v) for v in A[y0 - 1, x0 + 16:x0 + 20]]
        if mb_y and mb_x == mb_w - 1:
            tr_right = [int(A[y0 - 1, x0 + 15])] * 4
        for by in range(4):
            for bx in range(4):
                y, x = y0 + 4 * by, x0 + 4 * bx
                topright = [int(v) for v in A[y - 1, x + 4:x + 8]]
                if (by == 0 or bx == 3) and mb_y == 0:
                    topright = tr_top
                elif bx == 3:
                    topright = tr_right
                slot, copy = sub_slot(int(mb["sub_mode"][4 * by + bx]), 4 * mb_x + bx, 4 * mb_y + by)
                if copy:
                    cd = np.full(40, 0xEE, np.int64)   # copy_dst[5 * 8], the block at 12
                    if not (4 * mb_y + by):
                        cd[3] = lo
                        cd[4:8] = lo
                    else:
                        cd[4:8] = A[y - 1, x:x + 4]
                        cd[3] = hi if not (4 * mb_x + bx) else A[y - 1, x - 1]
                    if not (4 * mb_x + bx):
                        cd[[11, 19, 27, 35]] = hi
                    else:
                        cd[[11, 19, 27, 35]] = A[y:y + 4, x - 1]
                    t, l, lt = list(cd[4:8]) + topright, cd[[11, 19, 27, 35]], cd[3]
                else:
                    t, l, lt = [int(v) for v in A[y - 1, x:x + 4]] + topright, A[y:y + 4, x - 1], A[y - 1, x - 1]
                A[y:y + 4, x:x + 4] = pred4x4(slot, t, l, lt)
                _add_residuals(planes, mb, mb_x, mb_y, coeffs, only=4 * by + bx)
        for b in range(16, 24):
            _add_residuals(planes, mb, mb_x, mb_y, coeffs, only=b)
    else:
        _add_residuals(planes, mb, mb_x, mb_y, coeffs)


def recon_frame_ptr(planes, mbs, coeffs, refs, mb_w, mb_h, bilinear=0, fullpel=0):
    """(b).  Same arguments and result as recon_frame()."""
    G = [np.full((P.shape[0] + 2 * MARGIN, P.shape[1] + 2 * MARGIN + 16), 0xEE, np.uint8) for P in planes]
    V = [g[MARGIN:MARGIN + P.shape[0], MARGIN:MARGIN + P.shape[1]] for g, P in zip(G, planes)]
    for v, P in zip(V, planes):
        v[:] = P
    padded = [None if r is None else [np.pad(q, PAD, mode="edge") for q in r] for r in refs]
    for m in range(mb_w * mb_h):
        mb, mb_x, mb_y = mbs[m], m % mb_w, m // mb_w
        if not well_formed(mb, refs, len(coeffs)):
            continue
        if mb["ref_frame"]:
            r = mb["ref_frame"] - 1
            calls = mb_preds(mb, mb_x, mb_y, fullpel)
            for c in calls:
                N = 8 if c["plane"] else 16
                # AV_RN32A(mv): a zero MV is put_pixels_tab[.][0][0] on the reference in place
                c["moved"] = (c["sx"], c["sy"]) != (N * mb_x + c["x"], N * mb_y + c["y"]) or bool(c["mx"] or c["my"])
                V[c["plane"]][N * mb_y + c["y"]:N * mb_y + c["y"] + c["h"], N * mb_x + c["x"]:N * mb_x + c["x"] + c["w"]] = \
                    _mc_ptr(refs[r][c["plane"]], padded[r][c["plane"]], c, bilinear)
            _add_residuals(V, mb, mb_x, mb_y, coeffs)
        else:
            _intra_ptr(G, mb, mb_x, mb_y, mb_w, V, coeffs)
    for v, P in zip(V, planes):
        P[:] = v
    return planes
