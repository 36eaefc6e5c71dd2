"""Pictures for the VP9 loop-filter table face (ffhip_vp9_lf_tables_pictures_dev / _host): a random block and transform partition per
superblock, emitted as FFHipVp9LfBlock records, and the model of what the face must make of them: the VP9Filter by the rules
include/ffhip.h states (mask_edges is vp9_lf_gen's restatement), and from it the tables through the per-superblock host faces
ffhip_vp9_lf_sb_tables / _ctables, which the existing loop-filter tests pin.

A generator of its own, not vp9_lf_gen.structured(): it draws a real `bs` for every block, derives uvtx by the face's rule, leaves
mask[1] untouched at 4:4:4 and zero-fills the levels.  Test infrastructure."""
import ctypes as C

import numpy as np

from vp9_lf_gen import FILTER_DT, filter_lut, mask_edges

BLOCK_DT = np.dtype([("pos", "u1"), ("bs", "u1"), ("tx_skip", "u1"), ("lvl_idx", "u1")])
#: enum BlockSize -> (w8, h8) in 8x8 cells, and whether the size is below 8x8
BS_WH = [(8, 8), (8, 4), (4, 8), (4, 4), (4, 2), (2, 4), (2, 2), (2, 1), (1, 2), (1, 1), (1, 1), (1, 1), (1, 1)]
BS_OF = {(8, 8): 0, (8, 4): 1, (4, 8): 2, (4, 4): 3, (4, 2): 4, (2, 4): 5, (2, 2): 6, (2, 1): 7, (1, 2): 8, (1, 1): 9}
SS = [(1, 1), (0, 0), (1, 0), (0, 1)]            # 4:2:0, 4:4:4, 4:2:2, 4:4:0
GUARD = 0xA5


def max_tx(bs):
    w8, h8 = BS_WH[bs]
    return 0 if bs > 9 else min(3, int(np.log2(min(w8, h8))) + 1)


def rec(r7, c7, bs, tx, skip, lvl_idx):
    return (r7 << 3 | c7, bs, tx | skip << 2, lvl_idx)


def record_ok(r, sb_row, sb_col, cols, rows):
    """the face's rules for a record it does not skip"""
    pos, bs, ts, li = (int(v) for v in r)
    if bs > 12 or ts & ~7 or pos & 0xC0 or li > 63 or (ts & 3) > max_tx(bs):
        return False
    w8, h8 = BS_WH[bs]
    r7, c7 = pos >> 3, pos & 7
    return not (c7 & (w8 - 1)) and not (r7 & (h8 - 1)) and sb_row * 8 + r7 < rows and sb_col * 8 + c7 < cols


def apply_record(level, mask, r, sb_row, sb_col, cols, rows, ss, lvl_tab):
    """steps 2..5 of the face's semantics for one record, on int64 arrays level[8, 8] and mask[2, 2, 8, 4]"""
    ss_h, ss_v = ss
    if not record_ok(r, sb_row, sb_col, cols, rows):
        return
    pos, bs, ts, li = (int(v) for v in r)
    lvl = int(lvl_tab[li])
    if not lvl:
        return
    w8, h8 = BS_WH[bs]
    r7, c7, tx, skip = pos >> 3, pos & 7, ts & 3, ts >> 2
    row, col = sb_row * 8 + r7, sb_col * 8 + c7
    uvtx = tx - int((ss_h and w8 * 2 == 1 << tx) or (ss_v and h8 * 2 == 1 << tx))
    x_end, y_end = min(cols - col, w8), min(rows - row, h8)
    level[r7:r7 + h8, c7:c7 + w8] = lvl
    mask_edges(mask[0], 0, 0, r7, c7, x_end, y_end, 0, 0, tx, skip)
    if ss_h | ss_v:
        mask_edges(mask[1], ss_h, ss_v, r7, c7, x_end, y_end, (cols & 7) if (cols & 1 and col + w8 >= cols) else 0,
                   (rows & 7) if (rows & 1 and row + h8 >= rows) else 0, uvtx, skip)


def filter_of(records, sb_row, sb_col, cols, rows, ss, lvl_tab):
    level, mask = np.zeros((8, 8), np.int64), np.zeros((2, 2, 8, 4), np.int64)
    for r in records:
        apply_record(level, mask, r, sb_row, sb_col, cols, rows, ss, lvl_tab)
    assert (mask >> 8 == 0).all()
    f = np.zeros((), FILTER_DT)
    f["level"], f["mask"] = level.reshape(64), mask
    return f


def partition(rng, sb_row, sb_col, cols, rows, p_skip=.3):
    """the records of one superblock: a random quad-tree down to 8x8, each leaf whole, split in two or (at 8x8) below 8x8; blocks whose
    first cell lies outside the picture are not decoded"""
    out = []

    def block(r7, c7, w8, h8, sub8):
        if sb_row * 8 + r7 >= rows or sb_col * 8 + c7 >= cols:
            return
        bs = int(rng.integers(10, 13)) if sub8 else BS_OF[(w8, h8)]
        out.append(rec(r7, c7, bs, int(rng.integers(0, max_tx(bs) + 1)), int(rng.random() < p_skip), int(rng.integers(0, 64))))

    def part(r7, c7, n):
        k = rng.random()
        h = n // 2
        if n > 1 and k < .5:
            for dr, dc in ((0, 0), (0, h), (h, 0), (h, h)):
                part(r7 + dr, c7 + dc, h)
        elif n > 1 and k < .65:
            block(r7, c7, n, h, False)
            block(r7 + h, c7, n, h, False)
        elif n > 1 and k < .8:
            block(r7, c7, h, n, False)
            block(r7, c7 + h, h, n, False)
        else:
            block(r7, c7, n, n, n == 1 and rng.random() < .5)
    part(0, 0, 8)
    return out


class TabPicture:
    """one picture: per-superblock record lists -> blocks / sb_first, the level table and the luts"""

    def __init__(self, cols, rows, ss, sb_records, level=None, sharp=0, seed=0):
        self.cols, self.rows, self.ss = cols, rows, tuple(ss)
        self.sb_cols, self.sb_rows = (cols + 7) >> 3, (rows + 7) >> 3
        self.nsb = self.sb_cols * self.sb_rows
        assert len(sb_records) == self.nsb
        self.sb_records = [list(r) for r in sb_records]
        flat = [r for sb in self.sb_records for r in sb]
        self.blocks = np.array(flat, np.uint8).reshape(len(flat), 4).view(BLOCK_DT).reshape(len(flat))
        self.sb_first = np.cumsum([0] + [len(sb) for sb in self.sb_records]).astype(np.uint32)
        self.nblocks = len(flat)
        if level is None:
            rng = np.random.default_rng(seed + 77)
            level = rng.integers(1, 64, 64)
            level[rng.random(64) < .1] = 0
        self.level = np.asarray(level, np.uint8)
        self.lim, self.mblim = filter_lut(sharp)

    @classmethod
    def random(cls, seed, cols, rows, ss, **kw):
        rng = np.random.default_rng(seed)
        sbc, sbr = (cols + 7) >> 3, (rows + 7) >> 3
        return cls(cols, rows, ss, [partition(rng, i // sbc, i % sbc, cols, rows) for i in range(sbc * sbr)], sharp=int(rng.integers(0, 8)),
                   seed=seed, **kw)

    def model_filters(self, sb_records=None):
        sb_records = self.sb_records if sb_records is None else sb_records
        f = np.zeros(self.nsb, FILTER_DT)
        for i, recs in enumerate(sb_records):
            f[i] = filter_of(recs, i // self.sb_cols, i % self.sb_cols, self.cols, self.rows, self.ss, self.level)
        return f

    def model(self, sb_records=None):
        """(filters, tables uint32 [nsb, 320], ctables uint32 [nsb, 128] or None)"""
        from ffmpeg_amd import _lib
        L = _lib.lib()
        f = self.model_filters(sb_records)
        ss_h, ss_v = self.ss
        tabs = np.zeros((self.nsb, 320), np.uint32)
        ctabs = np.zeros((self.nsb, 128), np.uint32) if ss_h != ss_v else None
        for i in range(self.nsb):
            r, c = divmod(i, self.sb_cols)
            a = (f[i:i + 1].ctypes.data, 8 * r, 8 * c, ss_h, ss_v, self.lim.ctypes.data, self.mblim.ctypes.data)
            assert L.ffhip_vp9_lf_sb_tables(tabs[i].ctypes.data, *a) == 0, L.ffhip_last_error()
            if ctabs is not None:
                assert L.ffhip_vp9_lf_sb_ctables(ctabs[i].ctypes.data, *a) == 0, L.ffhip_last_error()
        return f, tabs, ctabs

    # ---- the face's arrays, each between two guard regions --------------------------------------------------
    GUARD_BYTES = 64

    def maps(self, filters=True, blocks=None, sb_first=None, nblocks=None):
        """the dict ffmpeg_amd.vp9.lf_tables_pictures_host() takes: numpy arrays; "_name" is the whole allocation of "name", guard regions
        of GUARD_BYTES on both sides, the outputs pre-filled with GUARD as well"""
        g = self.GUARD_BYTES
        m = {"nblocks": self.nblocks if nblocks is None else nblocks, "level": self.level, "lim_lut": self.lim, "mblim_lut": self.mblim}

        def put(name, payload, nbytes=None):
            payload = None if payload is None else np.ascontiguousarray(payload).view(np.uint8).reshape(-1)
            n = len(payload) if payload is not None else nbytes
            a = np.full(n + 2 * g, GUARD, np.uint8)
            if payload is not None:
                a[g:g + n] = payload
            m["_" + name], m[name] = a, a[g:g + n]
        put("blocks", self.blocks if blocks is None else blocks)
        put("sb_first", self.sb_first if sb_first is None else np.asarray(sb_first, np.uint32))
        put("tables", None, self.nsb * 1280)
        if self.ss[0] != self.ss[1]:
            put("ctables", None, self.nsb * 512)
        else:
            m["ctables"] = None
        if filters:
            put("filters", None, self.nsb * 192)
        else:
            m["filters"] = None
        return m


OUTPUTS = ("tables", "ctables", "filters")
INPUTS = ("blocks", "sb_first")


def expected(m, model):
    """name -> the whole allocation the face must leave: the model between intact guards"""
    g = TabPicture.GUARD_BYTES
    out = {}
    for name, want in zip(("filters", "tables", "ctables"), model):
        if m.get(name) is None:
            continue
        e = np.full(len(m["_" + name]), GUARD, np.uint8)
        e[g:-g] = np.ascontiguousarray(want).view(np.uint8).reshape(-1)
        out[name] = e
    return out


def entry_census(tabs, ctabs, ss):
    """(set of (dir, width index) that occur, set of dirs with a luma inner-4 entry, count of 16-wide chroma entries on a tile's last
    position) over the tables of a picture"""
    seen, inner = set(), set()
    t = np.asarray(tabs, np.uint32).reshape(-1, 320)
    y = t[:, :256].reshape(-1, 2, 16, 8)
    for d in (0, 1):
        v = y[:, d][y[:, d] >> 31 == 1]
        seen |= {(d, int(w)) for w in np.unique((v >> 24) & 3)}
        if (y[:, d, 1::2] >> 31).any():
            inner.add(d)
    wide_last = 0
    is16 = lambda a: int(((a >> 31 == 1) & (((a >> 24) & 3) == 2)).sum())
    if ss == (1, 1):
        uv = t[:, 256:].reshape(-1, 2, 8, 4)
        for d in (0, 1):
            v = uv[:, d][uv[:, d] >> 31 == 1]
            seen |= {("c", d, int(w)) for w in np.unique((v >> 24) & 3)}
        wide_last = is16(uv[:, :, 7])
    elif ctabs is not None:
        c = np.asarray(ctabs, np.uint32).reshape(-1, 128)
        npc, nsc, npr, nsr = (8 if ss[0] else 16), (4 if ss[1] else 8), (8 if ss[1] else 16), (4 if ss[0] else 8)
        parts = (c[:, :npc * nsc].reshape(-1, npc, nsc), c[:, npc * nsc:].reshape(-1, npr, nsr))
        for d, p in enumerate(parts):
            v = p[p >> 31 == 1]
            seen |= {("c", d, int(w)) for w in np.unique((v >> 24) & 3)}
            wide_last += is16(p[:, -1])
    return seen, inner, wide_last


def malformed_cases(cols=13, rows=11):
    """[(name, sb index, the bad record)] for a picture of cols x rows (2 x 2 superblocks, both edges cut): each record must be skipped"""
    return [("bs13", 0, rec(0, 0, 13, 0, 0, 5)), ("bs255", 0, rec(2, 2, 255, 0, 0, 5)), ("tx_bit3", 0, (0, 9, 8, 5)),
            ("tx_over_8x8", 0, rec(1, 1, 9, 2, 0, 5)), ("tx_over_sub8", 0, rec(1, 1, 12, 1, 0, 5)), ("tx_over_16x8", 0, rec(0, 2, 7, 3, 0, 5)),
            ("misaligned_col", 0, rec(0, 1, 6, 1, 0, 5)), ("misaligned_row", 0, rec(2, 0, 2, 2, 0, 5)),
            ("outside_col", 1, rec(0, 5, 9, 1, 0, 5)), ("outside_row", 2, rec(3, 0, 9, 1, 1, 5)), ("lvl_idx64", 0, rec(0, 0, 9, 0, 0, 64)),
            ("pos_bit6", 0, (0x40, 9, 0, 5))]


def ptr(a):
    return C.c_void_p(a.ctypes.data)
