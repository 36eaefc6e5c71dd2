"""The per-call path a decoder takes today for a picture's in-loop filters, on the batch faces: host-built FFHipHevcEdge records ->
loop_filter_batch for the vertical then the horizontal edges -> a copy of the deblocked picture -> sao_batch + sao_restore_batch
from that copy -> the bypass samples' deblocked values put back (no face does that step: a torch.where here).  Each plane lives in a
work buffer with a 1-row / 4-sample border (8 rows below: a chroma edge record covers 8 lines, and the batch kernel loads the
lines of a group it then leaves alone), so that the filters' reads past the picture stay inside it."""
import numpy as np

import hevc_lf_picture_gen as G
from ffmpeg_amd import hevc


class BatchPath:
    def __init__(self, torch, pic):
        self.torch, self.pic = torch, pic
        self.ps = 1 if pic.bd == 8 else 2
        self.geo, self.rec = [], []
        calls = G.edges(pic)
        blocks = G.sao_blocks(pic)
        for p in range(pic.nplanes):
            ph, pw = pic.src[p].shape
            st = ((pw + 8) * self.ps + 63) // 64 * 64
            org = st + 4 * self.ps
            off = lambda x, y: org + y * st + x * self.ps
            dirs = []
            for d in calls:
                e = [c for c in d if c[0] == p]
                r = np.zeros(max(len(e), 1), hevc.EDGE_DTYPE)
                for i, (_, vertical, chroma, x, y, beta, tc, nop, noq) in enumerate(e):
                    r[i] = (off(x, y), int(vertical) | int(chroma) << 1, beta, nop, noq, tc, (0, 0))
                dirs.append((torch.from_numpy(r.view(np.uint8).copy()).cuda(), len(e)))
            sb = [b for b in blocks if b[0] == p]
            sao = np.zeros(max(len(sb), 1), hevc.SAO_DTYPE)
            eb = [b for b in sb if b[6] == 2]
            res = np.zeros(max(len(eb), 1), hevc.RESTORE_DTYPE)
            for i, (_, a, x0, y0, w, h, t, k, ov) in enumerate(sb):
                sao[i] = (off(x0, y0), off(x0, y0), ov, int(t == 2), k, w, h, (0, 0))
            for i, (_, a, x0, y0, w, h, t, k, ov) in enumerate(eb):
                R = pic.ctbs[a]
                bord = sum(v << j for j, v in enumerate(pic.borders(a)))
                res[i] = (off(x0, y0), off(x0, y0), ov[0], w, h, k, R["restore"], bord, R["vert_edge"], R["horiz_edge"], R["diag_edge"], (0, 0))
            mask = torch.from_numpy(np.pad(pic.bypass_mask(p), ((1, 8), (4, (st // self.ps) - pw - 4)))).cuda()
            self.geo.append((ph, pw, st, org))
            self.rec.append((dirs, (torch.from_numpy(sao.view(np.uint8).copy()).cuda(), len(sb)),
                             (torch.from_numpy(res.view(np.uint8).copy()).cuda(), len(eb)), mask))
        # per plane: the edge launches, the copy, sao, restore, the bypass copy-back
        self.launches = sum(sum(1 for _, n in d if n) + 1 + (s[1] > 0) + (r[1] > 0) + 1 for d, s, r, m in self.rec)

    def upload(self, planes):
        """the work buffers holding `planes` (device tensors of (ph, pw) samples, or numpy int64 planes)"""
        torch, dt = self.torch, np.uint8 if self.pic.bd == 8 else np.uint16
        out = []
        for p, (ph, pw, st, org) in enumerate(self.geo):
            host = np.zeros((ph + 9, st // self.ps), dt)
            host[1:1 + ph, 4:4 + pw] = planes[p]
            out.append(torch.from_numpy(host.view(np.uint8).reshape(ph + 9, st).copy()).cuda())
        return out

    def run(self, work):
        """filter the work buffers in place; returns the deblocked copies"""
        torch, bd = self.torch, self.pic.bd
        dbks = []
        for p, (dirs, (sao, ns), (res, nr), mask) in enumerate(self.rec):
            st = self.geo[p][2]
            for d, n in dirs:
                if n:
                    hevc.loop_filter_batch(work[p], st, d, n, bit_depth=bd)
            dbk = work[p].clone()
            if ns:
                hevc.sao_batch(work[p], st, dbk, st, sao, ns, bit_depth=bd)
            if nr:
                hevc.sao_restore_batch(work[p], st, dbk, st, res, nr, bit_depth=bd)
            view = (lambda t: t) if bd == 8 else (lambda t: t.view(torch.int16))
            w16, d16 = view(work[p]), view(dbk)
            w16.copy_(torch.where(mask, d16, w16))
            dbks.append(dbk)
        return dbks

    def planes(self, work):
        """the picture's samples of each work buffer (numpy int64)"""
        out = []
        for p, (ph, pw, st, org) in enumerate(self.geo):
            a = work[p].cpu().numpy()
            a = a if self.pic.bd == 8 else a.view(np.uint16)
            out.append(a[1:1 + ph, 4:4 + pw].astype(np.int64))
        return out
