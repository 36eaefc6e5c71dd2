"""The DC-wrap cell of the H.264 inverse transforms, for the 8-bit faces and the depth-8 instantiation of the `_hbd` faces.

At 8 bits idct_add / idct8_add store block[0] + 32 back as int16_t, so a DC of 32736 .. 32767 wraps there; idct_dc_add / idct8_dc_add
sum in int and do not (h264idct_template.c:33-175).  Over samples of 128 a block with nothing but such a DC comes out as 0 through the
transform ((int16)(dc + 32) >> 6 = -512) and as 255 through the DC form ((dc + 32) >> 6 = 512); at 32735 both give 255.

cases() builds one block or macroblock per (DC, form) for every face and the setting that sends it down each form; want() runs the
oracle over a case; assert_cell() checks on the oracle's outputs alone that the cell is what the paragraph above says, so that a test
which then compares a device with the oracle cannot pass vacuously."""
import ctypes as C

import numpy as np

import ffi
from ffi import ptr, u8p, i16p, i32p

DCS = (32735, 32736, 32760, 32767, -32768, -32, 31)
WRAPS = (32736, 32760, 32767)
FORMS = ("dc", "tx")
# (DC, form) of macroblock m of a dispatcher case
PAIRS = [(dc, form) for dc in DCS for form in FORMS]


def _scan8(s):
    """scan8[s] of all three planes (h264_parse.h:40-57): plane s // 16, its sixteen entries laid out as the luma ones, five rows further down"""
    t = s % 16
    return 4 + (t & 1) + 2 * ((t >> 2) & 1) + 8 * (1 + ((t >> 1) & 1) + 2 * (t >> 3) + 5 * (s // 16))


def cases(hbd):
    """-> list of dicts: face 'list' (arg = kind 0 .. 3), 'mb' (arg = which 0 .. 2) or 'add8' (arg = which 3: idct_add8, and for the `_hbd`
    faces, which alone have it, 4: idct_add8_422); planes of 128, strides in samples = bytes, coefs, and `cells`: (dc, form, plane, y, x, n)
    of the block each (DC, form) pair lands on"""
    out = []
    for kind, n, form in ((0, 4, "tx"), (1, 8, "tx"), (2, 4, "dc"), (3, 8, "dc")):
        coefs = np.zeros((len(DCS), n * n), np.int16)
        coefs[:, 0] = DCS
        out.append(dict(face="list", arg=kind, n=n, stride=n * len(DCS), planes=[np.full((n, n * len(DCS)), 128, np.uint8)],
                        offs=(np.arange(len(DCS)) * n).astype(np.int32), coefs=coefs,
                        cells=[(dc, form, 0, 0, n * i, n) for i, dc in enumerate(DCS)]))
    nmb = len(PAIRS)
    stride = 16 * nmb
    bo = np.array([(i & 1) * 4 + ((i >> 1) & 1) * 4 * stride + ((i >> 2) & 1) * 8 + (i >> 3) * 8 * stride for i in range(16)], np.int32)
    for which in range(3):
        n = 8 if which == 1 else 4
        coefs, nnzc, cells = np.zeros((nmb, 256), np.int16), np.zeros((nmb, 40), np.uint8), []
        for m, (dc, form) in enumerate(PAIRS):
            i = 4 * (m % 4) if which == 1 else m % 16
            coefs[m, 16 * i] = dc
            # idct_add16 / idct8_add4: a count of 1 with block[0] set takes *_dc_add, any other count the transform; idct_add16intra: a
            # count of 0 with block[0] set takes idct_dc_add, any count the transform (h264idct_template.c:177-214)
            nnzc[m, _scan8(i)] = {"dc": 0, "tx": 1}[form] if which == 2 else {"dc": 1, "tx": 2}[form]
            cells.append((dc, form, 0, int(bo[i]) // stride, 16 * m + int(bo[i]) % stride, n))
        out.append(dict(face="mb", arg=which, n=n, stride=stride, planes=[np.full((16, stride), 128, np.uint8)],
                        mb_off=(np.arange(nmb) * 16).astype(np.int32), bo=bo, coefs=coefs, nnzc=nnzc, cells=cells))
    stride = 8 * nmb
    for which in (3, 4) if hbd else (3,):
        # idct_add8: four blocks a plane; idct_add8_422: eight, blocks 4 .. 7 of a plane with their offsets and counts four slots later
        # (h264idct_template.c:216-257).  A count takes the transform, block[0] alone idct_dc_add
        nblk = 4 if which == 3 else 8
        slot = lambda j, r: 16 * j + r + (4 if r >= 4 else 0)
        bo = np.zeros(48, np.int32)
        for j in (1, 2):
            for r in range(nblk):
                bo[slot(j, r)] = (r & 1) * 4 + (r >> 1) * 4 * stride
        coefs, nnzc, cells = np.zeros((nmb, 768), np.int16), np.zeros((nmb, 120), np.uint8), []
        for m, (dc, form) in enumerate(PAIRS):
            j, r = 1 + (m >> 1) % 2, ((m >> 1) + 3) % nblk      # 4:2:2: the three wrapping DCs land on blocks 4, 5, 6
            coefs[m, 16 * (16 * j + r)] = dc
            nnzc[m, _scan8(slot(j, r))] = {"dc": 0, "tx": 1}[form]
            cells.append((dc, form, j - 1, 4 * (r >> 1), 8 * m + 4 * (r & 1), 4))
        out.append(dict(face="add8", arg=which, n=4, stride=stride, planes=[np.full((2 * nblk, stride), 128, np.uint8) for _ in range(2)],
                        mb_off=(np.arange(nmb) * 8).astype(np.int32), bo=bo, coefs=coefs, nnzc=nnzc, cells=cells))
    return out


def want(O, c, hbd):
    """the oracle over case c, block by block: the 8-bit functions, or (hbd) the any-depth restatement at depth 8 -> (planes, coefs)"""
    O.ffo_h264_idct_bd.argtypes = [C.c_int, C.c_int, u8p, i16p, C.c_ssize_t]
    O.ffo_h264_idct_mb_bd.argtypes = [C.c_int, C.c_int, u8p, i32p, i16p, C.c_ssize_t, u8p]
    O.ffo_h264_idct_add8_bd.argtypes = [C.c_int, C.c_int, C.POINTER(u8p), i32p, i16p, C.c_ssize_t, u8p]
    planes, coefs, s = [p.copy() for p in c["planes"]], c["coefs"].copy(), c["stride"]
    at = lambda p, off: C.cast(p.ctypes.data + int(off), u8p)
    for i in range(coefs.shape[0]):
        if c["face"] == "list":
            if hbd:
                O.ffo_h264_idct_bd(8, c["arg"], at(planes[0], c["offs"][i]), ptr(coefs[i], i16p), s)
            else:
                fn = [O.ffo_h264_idct_add, O.ffo_h264_idct8_add, O.ffo_h264_idct_dc_add, O.ffo_h264_idct8_dc_add][c["arg"]]
                fn(at(planes[0], c["offs"][i]), ptr(coefs[i], i16p), s)
        elif c["face"] == "mb":
            if hbd:
                O.ffo_h264_idct_mb_bd(8, c["arg"], at(planes[0], c["mb_off"][i]), ptr(c["bo"], i32p), ptr(coefs[i], i16p), s, ptr(c["nnzc"][i]))
            else:
                fn = [O.ffo_h264_idct_add16, O.ffo_h264_idct8_add4, O.ffo_h264_idct_add16intra][c["arg"]]
                fn(at(planes[0], c["mb_off"][i]), ptr(c["bo"], i32p), ptr(coefs[i], i16p), s, ptr(c["nnzc"][i]))
        else:
            dp = (u8p * 2)(at(planes[0], c["mb_off"][i]), at(planes[1], c["mb_off"][i]))
            if hbd:
                O.ffo_h264_idct_add8_bd(8, int(c["arg"] == 4), dp, ptr(c["bo"], i32p), ptr(coefs[i], i16p), s, ptr(c["nnzc"][i]))
            else:
                O.ffo_h264_idct_add8(dp, ptr(c["bo"], i32p), ptr(coefs[i], i16p), s, ptr(c["nnzc"][i]))
    return planes, coefs


def assert_cell(done):
    """done: [(case, oracle planes)] of every case.  Per face and block size: the two forms differ for 32736, 32760 and 32767 (0 through
    the transform, 255 through the DC form) and agree for 32735 (255); nothing but the cells' blocks is touched"""
    got, seen = {}, 0
    for c, planes in done:
        rest = [p.copy() for p in planes]
        for dc, form, pl, y, x, n in c["cells"]:
            blk = planes[pl][y:y + n, x:x + n]
            assert blk.shape == (n, n) and (blk == blk[0, 0]).all(), (c["face"], c["arg"], dc, form)
            got[(c["face"], c["arg"] if c["face"] != "list" else n, dc, form)] = int(blk[0, 0])
            rest[pl][y:y + n, x:x + n] = 128
        assert all((r == 128).all() for r in rest), (c["face"], c["arg"])
    for (face, arg, dc, form), v in got.items():
        if form != "tx":
            continue
        d = got[(face, arg, dc, "dc")]
        if dc in WRAPS:
            assert (v, d) == (0, 255), (face, arg, dc, v, d)
            seen += 1
        elif dc == 32735:
            assert (v, d) == (255, 255), (face, arg, dc, v, d)
            seen += 1
        else:
            assert v == d == min(max(128 + ((dc + 32) >> 6), 0), 255), (face, arg, dc, v, d)
    # four DCs x (4x4 and 8x8 lists, three luma dispatchers, idct_add8 and, where the face has it, idct_add8_422)
    assert seen == 4 * (2 + 3 + sum(c["face"] == "add8" for c, _ in done)) and seen >= 24
