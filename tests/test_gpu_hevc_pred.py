"""HEVC intra prediction on the GPU (ffhip_hevc_intra_batch_dev, ff_hevc_pred_init_hip), byte for byte against the restatement of
H.265 8.4.4.2 in hevc_pred_ref.py."""
import ctypes as C

import numpy as np
import pytest

import hevc_pred_ref as R
from ffmpeg_amd import hevc

pytestmark = pytest.mark.gpu

SENT = 0x5A5A
F = hevc


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


class Batch:
    """blocks laid out in cells of 36 x 34 samples with a sentinel around each; lines concatenated in one buffer"""

    def __init__(self, bd, cols=24, skew=0):
        self.bd, self.cols, self.skew = bd, cols, skew
        self.ps = 1 if bd == 8 else 2
        self.blocks, self.lines, self.wants = [], [], []

    def add(self, N, mode, c_idx, line, want, flags=0, al=0, at=0, luh=0, luv=0, log2=None):
        self.blocks.append((N, mode, c_idx, flags, al, at, luh, luv, N.bit_length() - 1 if log2 is None else log2))
        self.lines.append(np.asarray(line, np.int64))
        self.wants.append(want)

    def run(self):
        torch = _torch()
        n = len(self.blocks)
        rows = (n + self.cols - 1) // self.cols
        W = self.cols * 36 + 3 + self.skew
        H = rows * 34 + 1
        dt = np.uint8 if self.bd == 8 else np.uint16
        plane = np.full((H, W), SENT & ((1 << (8 * self.ps)) - 1), dt)
        want = plane.copy()
        rec = np.zeros(n, hevc.INTRA_DTYPE)
        edges, off = [], 0
        for i, ((N, mode, c_idx, flags, al, at, luh, luv, log2), line, w) in enumerate(zip(self.blocks, self.lines, self.wants)):
            r, c = divmod(i, self.cols)
            y0, x0 = r * 34 + 1, c * 36 + 1 + (i % 3)      # columns on and off the dword grid
            rec[i] = (y0 * W * self.ps + x0 * self.ps, off, al, at, log2, mode, flags, hevc.intra_c_idx_unit(c_idx, luh, luv))
            edges.append(line.astype(dt))
            off += len(line) * self.ps
            if w is not None:
                want[y0:y0 + N, x0:x0 + N] = w
        e = np.concatenate(edges)
        d_plane = torch.from_numpy(plane.view(np.uint8).copy()).cuda()
        d_e = torch.from_numpy(e.view(np.uint8).copy()).cuda()
        d_rec = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
        hevc.intra_batch(d_plane, W * self.ps, d_e, d_rec, n, bit_depth=self.bd)
        torch.cuda.synchronize()
        got = d_plane.cpu().numpy().view(dt).reshape(H, W)
        bad = np.argwhere(got != want)
        assert not len(bad), "%d mismatches, first %s (got %s want %s)" % (len(bad), bad[:3], got[tuple(bad[0])], want[tuple(bad[0])])


def _lines(rng, bd, N, k):
    """random lines, with 0 / max stripes and near-flat lines among them"""
    mx = (1 << bd) - 1
    out = []
    for j in range(k):
        if j % 4 == 1:
            line = rng.choice(np.array([0, mx]), 4 * N + 1)
        elif j % 4 == 2:
            line = np.clip(int(rng.integers(0, mx)) + rng.integers(-2, 3, 4 * N + 1), 0, mx)
        else:
            line = rng.integers(0, mx + 1, 4 * N + 1)
        out.append(line)
    return out


@pytest.mark.parametrize("bd", (8, 10, 12))
@pytest.mark.parametrize("skew", (0, 1))
def test_prepared_lines(bd, skew):
    """every size x all 35 modes x c_idx 0 / 1, rows on and off the dword grid, a sentinel around every block"""
    rng = np.random.default_rng(100 + bd + skew)
    b = Batch(bd, skew=skew)
    for N in (4, 8, 16, 32):
        for c_idx in (0, 1):
            for mode, line in zip(range(35), _lines(rng, bd, N, 35)):
                b.add(N, mode, c_idx, line, R.predict(line, N, mode, c_idx, bd))
    b.run()


@pytest.mark.parametrize("bd", (8, 10, 12))
def test_raw_lines(bd):
    """substitution by random masks (unit 4; unit 2 for chroma), corner only, nothing available, smoothing flags"""
    rng = np.random.default_rng(200 + bd)
    b = Batch(bd)

    def add(N, mode, c_idx, line, flags, al, at, luh, luv):
        av = R.availability(N, al, at, flags & F.INTRA_CORNER, luh, luv)
        want = R.predict_raw(line, N, mode, c_idx, bd, av, bool(flags & F.INTRA_STRONG), bool(flags & F.INTRA_NO_SMOOTH),
                             bool(flags & F.INTRA_CHROMA444))
        b.add(N, mode, c_idx, line, want, flags | F.INTRA_RAW, al, at, luh, luv)

    for N in (4, 8, 16, 32):
        for j, line in enumerate(_lines(rng, bd, N, 48)):
            mode, c_idx = int(rng.integers(0, 35)), j % 3
            lu = 1 if (c_idx and N <= 16 and j % 2) else 2
            nu = (2 * N) >> lu
            al, at = int(rng.integers(0, 1 << nu)), int(rng.integers(0, 1 << nu))
            flags = int(rng.integers(0, 32)) & ~F.INTRA_RAW
            if j % 8 == 0:
                al = at = 0                      # the corner alone, or nothing at all
            add(N, mode, c_idx, line, flags, al, at, lu, lu)
        for mode in (0, 2, 18, 34):              # ChromaArrayType 3 chroma, filtered and not
            for flags in (F.INTRA_CORNER, F.INTRA_CORNER | F.INTRA_CHROMA444, F.INTRA_CORNER | F.INTRA_CHROMA444 | F.INTRA_NO_SMOOTH):
                add(N, mode, 1, rng.integers(0, 1 << bd, 4 * N + 1), flags, (1 << ((2 * N) >> 2)) - 1, (1 << ((2 * N) >> 2)) - 1, 2, 2)
    # strong smoothing on and off next to its threshold, on either side
    thr, c = 1 << (bd - 5), 1 << (bd - 1)
    for dev in (thr - 1, thr, -(thr - 1), -thr):
        for side in (0, 1):
            for strong in (0, F.INTRA_STRONG):
                left, top = [c + int(v) for v in rng.integers(-1, 2, 64)], [c + int(v) for v in rng.integers(-1, 2, 64)]
                left[31] = top[31] = c
                (top if side else left)[63] = c + dev
                (left if side else top)[63] = c
                for mode in (0, 2, 30):
                    add(32, mode, 0, R.join(left, c, top), strong | F.INTRA_CORNER, 0xFFFF, 0xFFFF, 2, 2)
    b.run()


def test_large_mixed_batch():
    """thousands of blocks of every size and mode over one 4K plane, raw and prepared; sampled blocks checked"""
    torch = _torch()
    rng = np.random.default_rng(300)
    bd, W, H = 10, 3840, 2160
    recs, lines, metas, off = [], [], [], 0
    for cy in range(0, H - 31, 32):
        for cx in range(0, W - 31, 32):
            N = int(rng.choice([4, 8, 16, 32]))
            for y in range(cy, cy + 32, N):
                for x in range(cx, cx + 32, N):
                    if rng.random() < 0.75:
                        continue
                    mode, raw = int(rng.integers(0, 35)), bool(rng.random() < 0.5)
                    al = at = 0
                    flags = 0
                    if raw:
                        flags = hevc.INTRA_RAW | int(rng.integers(0, 32)) & ~hevc.INTRA_RAW
                        al, at = int(rng.integers(0, 1 << (2 * N >> 2))), int(rng.integers(0, 1 << (2 * N >> 2)))
                    line = rng.integers(0, 1 << bd, 4 * N + 1)
                    recs.append(((y * W + x) * 2, off, al, at, N.bit_length() - 1, mode, flags, hevc.intra_c_idx_unit(0, 2, 2)))
                    lines.append(line.astype(np.uint16))
                    metas.append((x, y, N, mode, flags, al, at, line))
                    off += len(line) * 2
    n = len(recs)
    assert n > 2000
    rec = np.array(recs, hevc.INTRA_DTYPE)
    plane = np.full((H, W), SENT, np.uint16)
    d_plane = torch.from_numpy(plane.view(np.uint8).copy()).cuda()
    hevc.intra_batch(d_plane, W * 2, torch.from_numpy(np.concatenate(lines).view(np.uint8).copy()).cuda(),
                     torch.from_numpy(rec.view(np.uint8).copy()).cuda(), n, bit_depth=bd)
    torch.cuda.synchronize()
    got = d_plane.cpu().numpy().view(np.uint16).reshape(H, W)
    for i in rng.choice(n, 300, replace=False):
        x, y, N, mode, flags, al, at, line = metas[i]
        if flags & hevc.INTRA_RAW:
            av = R.availability(N, al, at, flags & hevc.INTRA_CORNER, 2, 2)
            want = R.predict_raw(line, N, mode, 0, bd, av, bool(flags & hevc.INTRA_STRONG), bool(flags & hevc.INTRA_NO_SMOOTH), False)
        else:
            want = R.predict(line, N, mode, 0, bd)
        assert (got[y:y + N, x:x + N] == want).all(), (i, N, mode, flags)
    written = np.zeros((H, W), bool)
    for x, y, N, *_ in metas:
        written[y:y + N, x:x + N] = True
    assert (got[~written] == SENT).all()


def test_ignored_records_and_bad_arguments():
    torch = _torch()
    rng = np.random.default_rng(400)
    b = Batch(8)
    line = rng.integers(0, 256, 129)
    b.add(32, 35, 0, line, None)                        # mode 35: writes nothing
    b.add(32, 3, 0, line, None, log2=6)                 # log2_size 6: writes nothing
    b.add(8, 3, 0, line[:33], R.predict(line[:33], 8, 3, 0, 8))
    b.run()
    d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    rec = torch.zeros(16, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError):
        hevc.intra_batch(d, 64, d, rec, 1, bit_depth=9)
    with pytest.raises(RuntimeError):
        hevc.intra_batch(d[1:], 64, d, rec, 1, bit_depth=10)     # misaligned 16-bit dst
    with pytest.raises(RuntimeError):
        hevc.intra_batch(d, 64, d, rec, -1, bit_depth=8)
    assert hevc.intra_batch(d, 64, d, rec, 0, bit_depth=8) == 0


@pytest.mark.parametrize("bd", (8, 10, 12))
def test_host_faces(bd):
    """the nine members, called as the decoder calls them: top / left point into the same buffer as src"""
    _torch()
    c = hevc.pred_init(bd)
    assert not any(c.intra_pred)
    rng = np.random.default_rng(500 + bd)
    dt = np.uint8 if bd == 8 else np.uint16
    ps = np.dtype(dt).itemsize
    for i, N in enumerate((4, 8, 16, 32)):
        for mode in range(35):
            for c_idx in (0, 1):
                W = 3 * N + 7
                buf = rng.integers(0, 1 << bd, (N + 4, W)).astype(dt)
                y0, x0 = 3, 1                                   # the block; its top row above it, left[] laid out in row 0
                corner = int(buf[y0 - 1, x0 - 1])
                buf[0, 0] = corner                              # left[-1]
                top = buf[y0 - 1, x0:x0 + 2 * N].astype(np.int64)
                left = buf[0, 1:1 + 2 * N].astype(np.int64)
                want = buf.copy()
                want[y0:y0 + N, x0:x0 + N] = R.predict(R.join(left, corner, top), N, mode, c_idx, bd)
                base = buf.ctypes.data
                src, tp, lp = base + (y0 * W + x0) * ps, base + ((y0 - 1) * W + x0) * ps, base + 1 * ps
                if mode == 0:
                    c.pred_planar[i](src, tp, lp, W * ps)
                elif mode == 1:
                    c.pred_dc(src, tp, lp, W * ps, i + 2, c_idx)
                else:
                    c.pred_angular[i](src, tp, lp, W * ps, c_idx, mode)
                assert np.array_equal(buf, want), (bd, N, mode, c_idx)


def test_pred_init_refuses_other_depths():
    c = hevc.HEVCPredContext()
    with pytest.raises(RuntimeError):
        hevc.pred_init(9, c)
    assert not bytes(memoryview(c)).strip(b"\0")
    assert C.sizeof(c) == 13 * C.sizeof(C.c_void_p)
