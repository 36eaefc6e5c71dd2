"""Synthetic H.264 pictures for the whole-picture inter prediction face (ffhip_h264_inter_pictures_dev) and its plan face
(ffhip_h264_inter_plan_pictures_host), and the model both are checked against.

The generator builds what a decoder holds after parsing a picture: P and B slices (contiguous in raster order) with their own
reference lists over the picture's slots and their own prediction weights (none, explicit, implicit); per macroblock intra or one of
the partition shapes 16x16 / 16x8 / 8x16 / 8x8 with the sub-partitions 8x8 / 8x4 / 4x8 / 4x4 per quadrant; a reference (or two) per
partition, per quadrant in an 8x8 macroblock; a vector per (sub-)partition and list.  free=True drops the partition structure: every
4x4 block has lists, references and vectors of its own, which no stream can hold but the face defines.

The model knows partitions; the face does not.  model() expands a picture into the decoder-order calls of mc_part(): per partition
and plane the put of the first list, then the put of the second list into a scratch array and biweight, or its avg, or weight on the
one list, each run by the oracle (ffo_h264_qpel_bd, ffo_h264_chroma_mc_bd, ffo_h264_weight_bd, ffo_h264_biweight_bd) on a source window
gathered with numpy index clipping (what emulated_edge_mc gives).  Its decisions (decide()) are written from the rules of
include/ffhip.h on their own, not from kernels/h264_inter_rules.h, and its samples are the oracle's, not kernels/h264_mc_rules.h's.  It
also returns the plan of every 4x4 block and what it covered: the (size, mcxy) pairs, chroma fractions, modes, partition shapes and
picture sides crossed."""
import ctypes as C
import functools

import numpy as np

import ffi
from ffmpeg_amd import h264

POISON = 0xA7                    # what a destination holds before the call: samples no rule writes keep it
PLAN = h264.INTER_PLAN_DTYPE

MB_SHAPES = {"16x16": [(0, 0, 16, 16)], "16x8": [(0, 0, 16, 8), (0, 8, 16, 8)], "8x16": [(0, 0, 8, 16), (8, 0, 8, 16)]}
SUB_SHAPES = {"8x8": [(0, 0, 8, 8)], "8x4": [(0, 0, 8, 4), (0, 4, 8, 4)], "4x8": [(0, 0, 4, 8), (4, 0, 4, 8)],
              "4x4": [(0, 0, 4, 4), (4, 0, 4, 4), (0, 4, 4, 4), (4, 4, 4, 4)]}
FREE = [(4 * (i & 3), 4 * (i >> 2), 4, 4) for i in range(16)]
FAR = (-32768, -32767, -8001, -2000, -333, 333, 2000, 8001, 32767)


@functools.lru_cache(None)
def _oracle():
    O = ffi.oracle()
    u8p = ffi.u8p
    O.ffo_h264_qpel_bd.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, u8p, u8p, C.c_ssize_t]
    O.ffo_h264_chroma_mc_bd.argtypes = [C.c_int, C.c_int, C.c_int, u8p, u8p, C.c_ssize_t, C.c_int, C.c_int, C.c_int]
    O.ffo_h264_weight_bd.argtypes = [C.c_int, C.c_int, u8p, C.c_ssize_t, C.c_int, C.c_int, C.c_int, C.c_int]
    O.ffo_h264_biweight_bd.argtypes = [C.c_int, C.c_int, u8p, u8p, C.c_ssize_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    return O


def sample_dtype(bd):
    return np.uint8 if bd == 8 else np.uint16


def random_slice(rng, s, nrefs, b, use_weight):
    """one INTER_SLICE_DTYPE record filled in place: lists over the slots, weights of every kind"""
    for l in range(2 if b else 1):
        k = int(rng.integers(1, 5))
        s["num_ref"][l] = k
        s["ref"][l][:k] = rng.integers(0, nrefs, k)
        s["ref"][l][k:] = 250                                    # never read by a well-formed block
    s["use_weight"] = use_weight
    s["use_weight_chroma"] = int(rng.integers(0, 2)) if use_weight == 1 else 0
    s["luma_log2_denom"], s["chroma_log2_denom"] = rng.integers(0, 8, 2)
    lw = s["luma_weight"]
    lw[..., 0] = rng.choice([1 << int(s["luma_log2_denom"]), -128, 127, 3, -17, 64], lw[..., 0].shape)
    lw[..., 1] = rng.choice([0, -128, 127, 5, -9], lw[..., 1].shape)
    cw = s["chroma_weight"]
    cw[..., 0] = rng.choice([1 << int(s["chroma_log2_denom"]), -128, 127, 7, -3, 40], cw[..., 0].shape)
    cw[..., 1] = rng.choice([0, -128, 127, 2, -30], cw[..., 1].shape)
    s["implicit_weight"] = rng.choice([32, 32, 33, 21, 43, -64, 128, 0, 64], (32, 32))


class InterPicture:
    """One picture.  mb: (mb_h * mb_w,) of h264.BS_MB_DTYPE; mvf: (4 mb_h, 4 mb_w) of h264.BS_MVF_DTYPE; slices:
    h264.INTER_SLICE_DTYPE; refs[slot]: [Y, Cb, Cr] sample arrays (Cb / Cr None without chroma), chroma_dy[slot]; parts[mb]: the
    (x, y, w, h, name) of the macroblock's partitions in decoder order (None: intra)."""

    def __init__(self, rng, mb_w, mb_h, bd=8, chroma=True, nrefs=3, nslices=2, p_intra=0.15, free=False, types="any", weights="any",
                 p_far=0.08, mv_range=40, refs=None, chroma_dy=None, p_bi=0.5):
        self.mb_w, self.mb_h, self.bd, self.chroma, self.nrefs = mb_w, mb_h, bd, chroma, nrefs
        self.w4, self.h4 = 4 * mb_w, 4 * mb_h
        n = mb_w * mb_h
        W, H, top = 16 * mb_w, 16 * mb_h, 1 << bd
        dt = sample_dtype(bd)
        self.refs = refs if refs is not None else [
            [rng.integers(0, top, (H, W)).astype(dt)] + ([rng.integers(0, top, (H // 2, W // 2)).astype(dt) for _ in range(2)] if chroma else [None, None])
            for _ in range(nrefs)]
        self.chroma_dy = list(chroma_dy) if chroma_dy is not None else [0] * nrefs
        nslices = self.nslices = max(1, min(nslices, n))
        S = self.slices = np.zeros(nslices, h264.INTER_SLICE_DTYPE)
        self.is_b = np.array([{"P": False, "B": True}.get(types, bool((i + (types == "any")) & 1)) for i in range(nslices)])
        for i, s in enumerate(S):
            b = bool(self.is_b[i])
            uw = {"none": 0, "explicit": 1, "implicit": 2 if b else 0}.get(weights)
            if uw is None:
                uw = int(rng.choice([0, 1, 2] if b else [0, 1]))
            random_slice(rng, s, nrefs, b, uw)
        cuts = np.sort(rng.choice(np.arange(1, n), nslices - 1, replace=False)) if nslices > 1 else np.zeros(0, int)
        mb = self.mb = np.zeros(n, h264.BS_MB_DTYPE)
        mb["slice"] = np.searchsorted(cuts, np.arange(n), side="right")
        mb["flags"] = (rng.random(n) < p_intra) * h264.BS_MB_INTRA
        mb["qp"] = 30
        mvf = self.mvf = np.zeros((self.h4, self.w4), h264.BS_MVF_DTYPE)
        mvf["ref_idx"] = -1
        mvf["mv"] = rng.integers(-99, 100, mvf["mv"].shape)      # stale vectors behind unused lists and intra macroblocks
        self.parts = [None] * n
        draw_mv = lambda: [int(rng.choice(FAR)) if rng.random() < p_far else int(rng.integers(-mv_range, mv_range + 1)) for _ in range(2)]
        for i in range(n):
            if mb["flags"][i] & 1:
                continue
            my, mx = divmod(i, mb_w)
            s = S[mb["slice"][i]]
            b = bool(self.is_b[mb["slice"][i]])
            if free:
                groups = [[p + ("4x4",)] for p in FREE]
            else:
                kind = str(rng.choice(["16x16", "16x8", "8x16", "8x8"], p=[0.3, 0.15, 0.15, 0.4]))
                if kind != "8x8":
                    groups = [[p + (kind,)] for p in MB_SHAPES[kind]]
                else:
                    groups = []
                    for qd in range(4):
                        sub = str(rng.choice(list(SUB_SHAPES)))
                        groups.append([(x + 8 * (qd & 1), y + 8 * (qd >> 1), w, h, sub) for x, y, w, h in SUB_SHAPES[sub]])
            self.parts[i] = [p for g in groups for p in g]
            for g in groups:                                     # one choice of lists and references per group
                use = [True, False] if not b else [True, True] if rng.random() < p_bi else [[True, False], [False, True]][int(rng.integers(0, 2))]
                ri = [int(rng.integers(0, s["num_ref"][l])) if use[l] else -1 for l in range(2)]
                for x, y, w, h, _ in g:
                    blk = mvf[my * 4 + y // 4:my * 4 + (y + h) // 4, mx * 4 + x // 4:mx * 4 + (x + w) // 4]
                    blk["ref_idx"] = ri
                    for l in range(2):
                        if use[l]:
                            blk["mv"][..., l, :] = draw_mv()
                        elif rng.random() < 0.5:
                            blk["mv"][..., l, :] = 0

    def free_parts(self):
        """every inter macroblock as sixteen 4x4 partitions (for pictures edited by hand)"""
        self.parts = [None if f & 1 else [p + ("4x4",) for p in FREE] for f in self.mb["flags"]]
        return self


def blank(mb_w, mb_h, bd=8, chroma=True, nrefs=2, b=True, seed=1):
    """an all-inter picture of 4x4 partitions predicting from list 0, ref_idx 0, vector (0, 0): one slice without weights whose lists
    are the slots in order"""
    pic = InterPicture(np.random.default_rng(seed), mb_w, mb_h, bd, chroma, nrefs, 1, 0.0, free=True, types="B" if b else "P", weights="none")
    s = pic.slices[0]
    s["num_ref"] = [nrefs, nrefs if b else 0]
    s["ref"][:] = 250
    for l in range(2 if b else 1):
        s["ref"][l][:nrefs] = np.arange(nrefs)
    s["implicit_weight"] = 32
    pic.mvf["mv"] = 0
    pic.mvf["ref_idx"] = [0, -1]
    return pic


# --------------------------------------------------------------------------------------------------------------------- the model
def decide(pic, m, f):
    """the plan of a 4x4 block (a PLAN record) from its macroblock record m and its motion record f: rules 1, 2 and 5 to 8"""
    p = np.zeros((), PLAN)
    if m["flags"] & 1 or m["slice"] >= pic.nslices:
        return p
    S = pic.slices[m["slice"]]
    r = [int(f["ref_idx"][0]), int(f["ref_idx"][1])]
    used = [l for l in range(2) if r[l] >= 0]
    if not used or S["luma_log2_denom"] > 7 or S["chroma_log2_denom"] > 7 or S["use_weight"] > 2:
        return p
    for l in used:
        if r[l] >= 32 or S["num_ref"][l] > 32 or r[l] >= S["num_ref"][l] or S["ref"][l][r[l]] >= pic.nrefs:
            return p
    uw = int(S["use_weight"])
    if len(used) == 2:
        p["slot"] = [S["ref"][0][r[0]], S["ref"][1][r[1]]]
        iw = int(S["implicit_weight"][r[0]][r[1]])
        if uw == 2 and iw != 32:
            p["mode"], p["chroma_weighted"] = h264.INTER_BI_W, 1
            p["luma_log2_denom"] = p["chroma_log2_denom"] = 5
            p["luma_weight"] = [iw, 64 - iw]
            p["chroma_weight"] = [[iw, 64 - iw]] * 2
        elif uw == 1:
            p["mode"], p["chroma_weighted"] = h264.INTER_BI_W, 1
            p["luma_log2_denom"], p["chroma_log2_denom"] = S["luma_log2_denom"], S["chroma_log2_denom"]
            p["luma_weight"] = [S["luma_weight"][r[0]][0][0], S["luma_weight"][r[1]][1][0]]
            p["luma_offset"] = int(S["luma_weight"][r[0]][0][1]) + int(S["luma_weight"][r[1]][1][1])
            for c in range(2):
                p["chroma_weight"][c] = [S["chroma_weight"][r[0]][0][c][0], S["chroma_weight"][r[1]][1][c][0]]
                p["chroma_offset"][c] = int(S["chroma_weight"][r[0]][0][c][1]) + int(S["chroma_weight"][r[1]][1][c][1])
        else:
            p["mode"] = h264.INTER_BI_AVG
        return p
    L = used[0]
    p["list"], p["slot"][0] = L, S["ref"][L][r[L]]
    if uw != 1:
        p["mode"] = h264.INTER_UNI
        return p
    p["mode"] = h264.INTER_UNI_W
    p["luma_log2_denom"] = S["luma_log2_denom"]
    p["luma_weight"][0], p["luma_offset"] = S["luma_weight"][r[L]][L]
    if S["use_weight_chroma"]:
        p["chroma_weighted"], p["chroma_log2_denom"] = 1, S["chroma_log2_denom"]
        for c in range(2):
            p["chroma_weight"][c][0], p["chroma_offset"][c] = S["chroma_weight"][r[L]][L][c]
    return p


PITCH = 32                       # samples per row of the model's scratch arrays


def _window(plane, x0, y0, w, h):
    """rows y0 .. y0 + h - 1, columns x0 .. x0 + w - 1 of the plane at clipped coordinates, in a PITCH-wide array"""
    ys = np.clip(np.arange(y0, y0 + h), 0, plane.shape[0] - 1)
    xs = np.clip(np.arange(x0, x0 + w), 0, plane.shape[1] - 1)
    a = np.zeros((h, PITCH), plane.dtype)
    a[:, :w] = plane[np.ix_(ys, xs)]
    return a


def _at(a, y, x):
    return C.cast(a.ctypes.data + y * a.strides[0] + x * a.itemsize, ffi.u8p)


def model(pic, fill=POISON, oracle=True):
    """(want planes [Y, Cb, Cr] that hold `fill` bytes where nothing is predicted, plans (h4, w4) of PLAN, cover): the decoder-order
    calls of every partition through the oracle.  oracle=False lists the calls (cover["calls"]) without making them: the planes are
    not valid then."""
    O = _oracle()
    bd, W, H = pic.bd, 16 * pic.mb_w, 16 * pic.mb_h
    dt = sample_dtype(bd)
    fillv = np.frombuffer(bytes([fill]) * 2, dt)[0]
    want = [np.full((H, W), fillv, dt)] + ([np.full((H // 2, W // 2), fillv, dt) for _ in range(2)] if pic.chroma else [None, None])
    plans = np.zeros((pic.h4, pic.w4), PLAN)
    cover = {"mcxy": set(), "cfrac": set(), "modes": set(), "parts": set(), "sides": set(), "calls": []}
    calls = cover["calls"]       # the calls in decoder order, for picture_records()
    stride = PITCH * np.dtype(dt).itemsize
    for i, parts in enumerate(pic.parts):
        my, mx = divmod(i, pic.mb_w)
        m = pic.mb[i]
        for by in range(4):
            for bx in range(4):
                plans[my * 4 + by, mx * 4 + bx] = decide(pic, m, pic.mvf[my * 4 + by, mx * 4 + bx])
        if parts is None:
            continue
        for x, y, w, h, name in parts:
            f = pic.mvf[my * 4 + y // 4, mx * 4 + x // 4]
            p = plans[my * 4 + y // 4, mx * 4 + x // 4]
            mode = int(p["mode"])
            if mode == h264.INTER_SKIP:
                continue
            cover["modes"].add(mode)
            cover["parts"].add(name)
            bi = mode >= h264.INTER_BI_AVG
            lists = [0, 1] if bi else [int(p["list"])]
            px, py = mx * 16 + x, my * 16 + y
            for pl in range(3 if pic.chroma else 1):
                dst = np.zeros((16, PITCH), dt)
                tmp = np.zeros((16, PITCH), dt)
                pw, phh = (w, h) if pl == 0 else (w // 2, h // 2)
                for n, L in enumerate(lists):
                    slot = int(p["slot"][n])
                    ref = pic.refs[slot][pl]
                    mvx, mvy = int(f["mv"][L][0]), int(f["mv"][L][1])
                    weighted = mode == h264.INTER_BI_W
                    tgt, avg = (dst, 0) if n == 0 else (tmp, 0) if weighted else (dst, 1)
                    if pl == 0:
                        sq = min(w, h)                           # the qpel members are square: a 16x8 partition is two 8x8 calls
                        mcxy = (mvx & 3) + ((mvy & 3) << 2)
                        cover["mcxy"].add((sq, mcxy))
                        sx, sy = px + (mvx >> 2), py + (mvy >> 2)
                        if sx - 2 < 0: cover["sides"].add("left")
                        if sy - 2 < 0: cover["sides"].add("top")
                        if sx + w + 3 > W: cover["sides"].add("right")
                        if sy + h + 3 > H: cover["sides"].add("bottom")
                        for oy in range(0, h, sq):
                            for ox in range(0, w, sq):
                                src = _window(ref, sx + ox - 2, sy + oy - 2, sq + 5, sq + 5) if oracle else dst
                                oracle and O.ffo_h264_qpel_bd(bd, avg, {16: 0, 8: 1, 4: 2}[sq], mcxy, _at(tgt, oy, ox), _at(src, 2, 2), stride)
                                calls.append(("mc", 0, 2 if avg else int(tgt is tmp), px + ox, py + oy, sq, sq, mcxy & 3, mcxy >> 2, slot,
                                              sx + ox, sy + oy))
                    else:
                        cx, cy = mvx, mvy + pic.chroma_dy[slot]
                        cover["cfrac"].add((cx & 7, cy & 7))
                        src = _window(ref, px // 2 + (cx >> 3), py // 2 + (cy >> 3), pw + 1, phh + 1) if oracle else dst
                        oracle and O.ffo_h264_chroma_mc_bd(bd, avg, pw, _at(tgt, 0, 0), _at(src, 0, 0), stride, phh, cx & 7, cy & 7)
                        calls.append(("mc", pl, 2 if avg else int(tgt is tmp), px // 2, py // 2, pw, phh, cx & 7, cy & 7, slot,
                                      px // 2 + (cx >> 3), py // 2 + (cy >> 3)))
                ld = int(p["luma_log2_denom"] if pl == 0 else p["chroma_log2_denom"])
                wt = p["luma_weight"] if pl == 0 else p["chroma_weight"][pl - 1]
                off = int(p["luma_offset"] if pl == 0 else p["chroma_offset"][pl - 1])
                if mode == h264.INTER_BI_W:
                    oracle and O.ffo_h264_biweight_bd(bd, pw, _at(dst, 0, 0), _at(tmp, 0, 0), stride, phh, ld, int(wt[0]), int(wt[1]), off)
                    calls.append(("w", pl, 1, px >> (pl > 0), py >> (pl > 0), pw, phh, ld, int(wt[0]), int(wt[1]), off))
                elif mode == h264.INTER_UNI_W and (pl == 0 or p["chroma_weighted"]):
                    oracle and O.ffo_h264_weight_bd(bd, pw, _at(dst, 0, 0), stride, phh, ld, int(wt[0]), off)
                    calls.append(("w", pl, 0, px >> (pl > 0), py >> (pl > 0), pw, phh, ld, int(wt[0]), 0, off))
                ox, oy = (px, py) if pl == 0 else (px // 2, py // 2)
                want[pl][oy:oy + phh, ox:ox + pw] = dst[:phh, :pw]
    return want, plans, cover


def picture_records(pic, calls, strides, ref_bytes):
    """model()'s calls as the records a decoder puts into the picture object (h264.Picture): [(member name, leading arguments, record
    array)] in decoder order.  strides: the planes' row pitches in bytes, shared by the destination and the references; the references
    of plane p lie ref_bytes[p] apart behind one base, slot 0 first.  Every motion record is an FFHIP_MC_EMU one: its source is read
    at clamped coordinates of the reference picture."""
    ps = np.dtype(sample_dtype(pic.bd)).itemsize
    out = []
    for c in calls:
        pl = c[1]
        if c[0] == "w":
            _, _, bi, x, y, w, h, ld, wd, ws, off = c
            r = np.zeros(1, h264.WEIGHT_DTYPE)
            r["dst_offset"] = r["src_offset"] = y * strides[pl] + x * ps
            r["w_idx"], r["height"], r["log2_denom"], r["bi"] = {16: 0, 8: 1, 4: 2, 2: 3}[w], h, ld, bi
            r["weightd"], r["weights"], r["offset"] = wd, ws, off
            out.append(("weight", (pl,), r))
            continue
        _, _, stage, x, y, w, h, fx, fy, slot, sx, sy = c
        r = np.zeros(1, h264.QPEL_DTYPE if pl == 0 else h264.CHROMA_DTYPE)
        r["dst_offset"], r["src_offset"] = y * strides[pl] + x * ps, slot * ref_bytes[pl]
        r["flags"], r["src_x"], r["src_y"], r["avg"] = h264.MC_EMU, sx, sy, int(stage == h264.MC_AVG)
        if pl == 0:
            r["mcxy"], r["size_idx"] = fx + 4 * fy, {16: 0, 8: 1, 4: 2}[w]
            out.append(("mc_luma", (stage,), r))
        else:
            r["w_idx"], r["h"], r["x"], r["y"] = {8: 0, 4: 1, 2: 2}[w], h, fx, fy
            out.append(("mc_chroma", (pl, stage), r))
    return out


def record(obj, records):
    """the records into the picture object, call by call as a decoder's host thread makes them"""
    obj.begin()
    for name, lead, r in records:
        getattr(obj, name)(*lead, r)


# ------------------------------------------------------------------------------------------------------------------ the picture sets
#: name -> (seed, [InterPicture arguments per picture]); all pictures of a set share the geometry, the depth and the format
SET = {
    "1x1": (9501, [dict(mb_w=1, mb_h=1, nslices=1, p_intra=0.0, types="B")] * 3),
    "3x2": (9502, [dict(mb_w=3, mb_h=2)] * 3),
    "5x4": (9503, [dict(mb_w=5, mb_h=4, nslices=3)]),
    "5x4_free": (9504, [dict(mb_w=5, mb_h=4, nslices=3, free=True, types="B")]),
    "11x9": (9505, [dict(mb_w=11, mb_h=9, nslices=4, nrefs=5)]),
    "3x2_10": (9506, [dict(mb_w=3, mb_h=2, bd=10)] * 3),
    "5x4_10_free": (9507, [dict(mb_w=5, mb_h=4, bd=10, nslices=3, free=True, types="B")]),
    "5x4_10": (9511, [dict(mb_w=5, mb_h=4, bd=10, nslices=3)] * 3),
    "11x9_10": (9512, [dict(mb_w=11, mb_h=9, bd=10, nslices=4, nrefs=5)]),
    "3x2_mono": (9508, [dict(mb_w=3, mb_h=2, chroma=False)]),
    "3x2_x17": (9509, [dict(mb_w=3, mb_h=2, nslices=2)] * (h264.INTER_PICS_PER_LAUNCH + 1)),
    "1x1_10": (9510, [dict(mb_w=1, mb_h=1, bd=10, nslices=1, p_intra=0.0, types="B", free=True)]),
}
NAMES = list(SET)


@functools.lru_cache(None)
def picture_set(name):
    """(pictures, [model(picture)]) of a set, made once and shared: do not write to them"""
    seed, args = SET[name]
    rng = np.random.default_rng(seed)
    pics = [InterPicture(rng, **a) for a in args]
    return pics, [model(p) for p in pics]
