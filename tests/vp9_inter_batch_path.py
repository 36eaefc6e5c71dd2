"""A frame of vp9_inter_frame_gen.py through the per-call batch faces that predate ffhip_vp9_inter_frames_dev: references copied into
buffers with a G.BORDER-sample edge-replicated border, ffhip_vp9_mc_batch_dev once per (plane, put / avg, reference), then
ffhip_vp9_itxfm_add_batch_dev once per (plane, transform size) on a copy of the coefficients (the batch face consumes them).  Only
valid while every window stays inside the border (no far MVs) and no block overhangs the decoded area (frames of whole superblocks):
the cross-check of the new face and the comparison leg of tools/bench_vp9_inter_frame.py."""
import numpy as np

import vp9_inter_frame_gen as G
from ffmpeg_amd import vp9


class BatchPath:
    def __init__(self, torch, fr, dst_strides):
        self.torch, self.fr, self.strides = torch, fr, dst_strides
        bd = fr.bd
        dt = np.uint8 if bd == 8 else np.uint16
        ps = 1 if bd == 8 else 2
        self.pads = [[(torch.from_numpy(G.padded(ref[p], dt).view(np.uint8).copy()).cuda(), G.padded(ref[p], dt).shape[1] * ps)
                      for p in range(3)] for ref in fr.refs]
        self.mc, self.tx = [], []
        for p in range(3):
            chroma = int(p > 0)
            for avg in (0, 1):
                for r in range(fr.nrefs):
                    recs = [rec for rec in fr.preds
                            if (rec["flags"] >> 1) & 1 == chroma and (avg == 0 or rec["flags"] & 1) and rec["ref"][avg] == r]
                    if not recs:
                        continue
                    blk = np.zeros(len(recs), vp9.MC_DTYPE)
                    pst = self.pads[r][p][1] // ps
                    for j, rec in enumerate(recs):
                        xi, yi, mx, my = G.rec_geometry(fr, rec, p, avg)
                        assert 3 - G.BORDER <= xi and xi + rec["w"] + 5 <= fr.rw[p] + G.BORDER and 3 - G.BORDER <= yi and \
                            yi + rec["h"] + 5 <= fr.rh[p] + G.BORDER, "window outside the border"
                        assert rec["x"] + rec["w"] <= fr.dw[p] and rec["y"] + rec["h"] <= fr.dh[p], "a block overhangs the decoded area"
                        blk[j] = (rec["y"] * dst_strides[p] + rec["x"] * ps, ((yi + G.BORDER) * pst + xi + G.BORDER) * ps, rec["w"], rec["h"],
                                  rec["filter"], mx, my, avg, 0)
                    self.mc.append((p, r, torch.from_numpy(blk.view(np.uint8).copy()).cuda(), len(recs)))
            for tx in range(5):
                tl = [t for t in fr.tus[p] if t["tx"] == tx]
                if not tl:
                    continue
                rec = np.zeros(len(tl), vp9.TU_DTYPE)
                for j, t in enumerate(tl):
                    rec[j] = (t["coeff_offset"], t["y"] * dst_strides[p] + t["x"] * ps, t["txtp"], t["dc_only"], 0)
                self.tx.append((p, tx, torch.from_numpy(rec.view(np.uint8).copy()).cuda(), len(tl)))
        self.coeffs = [torch.from_numpy(fr.coeff_array(p)).cuda() for p in range(3)]
        self.work = [c.clone() for c in self.coeffs]

    def launches(self):
        """kernel launches per frame (the coefficient copies that stand in for the decoder's own buffers are not counted)"""
        return len(self.mc) + len(self.tx)

    def run(self, dst):
        """dst: the three destination plane tensors (strides as given)"""
        bd = self.fr.bd
        for w, c in zip(self.work, self.coeffs):
            w.copy_(c)
        for p, r, blk, n in self.mc:
            pad, pst = self.pads[r][p]
            vp9.mc_batch(dst[p], self.strides[p], pad, pst, blk, n, bit_depth=bd)
        for p, tx, rec, n in self.tx:
            vp9.itxfm_add_batch(tx, self.work[p], dst[p], self.strides[p], rec, n, bit_depth=bd)
