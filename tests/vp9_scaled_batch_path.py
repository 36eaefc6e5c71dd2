"""A frame of vp9_scaled_frame_gen.py through the per-call batch faces: references copied into buffers with an S.BORDER-sample
edge-replicated border, then per (plane, put / avg, reference) one ffhip_vp9_scaled_mc_batch_dev[_hbd] launch for the calls of the
scaled rule and one ffhip_vp9_mc_batch_dev[_hbd] launch for the others, then ffhip_vp9_itxfm_add_batch_dev[_hbd] once per (plane,
transform size) on a copy of the coefficients.  Valid while every window stays inside the border and no block overhangs the decoded
area (or the destination planes are whole superblocks, overhang=True): the cross-check of ffhip_vp9_inter_frames_scaled_dev and the
comparison leg of tools/bench_vp9_scaled_frame.py."""
import numpy as np

import vp9_inter_frame_gen as G
import vp9_scaled_frame_gen as S
from ffmpeg_amd import vp9

#: FFHipVp9ScaledBlock (include/ffhip.h)
SCALED_DTYPE = np.dtype([("dst_offset", np.int32), ("src_offset", np.int32), ("width", np.uint8), ("height", np.uint8), ("filter", np.uint8),
                         ("mx", np.uint8), ("my", np.uint8), ("avg", np.uint8), ("dx", np.uint8), ("dy", np.uint8)])


class BatchPath:
    def __init__(self, torch, fr, dst_strides, overhang=False):
        self.torch, self.fr, self.strides = torch, fr, dst_strides
        bd = fr.bd
        dt = np.uint8 if bd == 8 else np.uint16
        ps = 1 if bd == 8 else 2
        self.pads = [[(torch.from_numpy(S.padded(ref[p], dt).view(np.uint8).copy()).cuda(), S.padded(ref[p], dt).shape[1] * ps)
                      for p in range(3)] for ref in fr.refs]
        self.mc, self.tx = [], []
        for p in range(3):
            chroma = int(p > 0)
            for avg in (0, 1):
                for r in range(fr.nrefs):
                    recs = [rec for rec in fr.preds
                            if (rec["flags"] >> 1) & 1 == chroma and (avg == 0 or rec["flags"] & 1) and rec["ref"][avg] == r]
                    pst = self.pads[r][p][1] // ps
                    for scaled in (False, True):
                        sel = [rec for rec in recs if bool(rec["flags"] & S.SCALED and fr.scaled(r)) == scaled]
                        if not sel:
                            continue
                        blk = np.zeros(len(sel), SCALED_DTYPE if scaled else vp9.MC_DTYPE)
                        for j, rec in enumerate(sel):
                            assert overhang or (rec["x"] + rec["w"] <= fr.dw[p] and rec["y"] + rec["h"] <= fr.dh[p]), \
                                "a block overhangs the decoded area"
                            if scaled:
                                xi, yi, mx, my, dx, dy = S.scaled_geometry(fr, rec, p, avg)
                                x_hi, y_hi = xi + (((rec["w"] - 1) * dx + mx) >> 4) + 5, yi + (((rec["h"] - 1) * dy + my) >> 4) + 4
                            else:
                                xi, yi, mx, my = G.rec_geometry(fr, rec, p, avg)
                                x_hi, y_hi = xi + rec["w"] + 5, yi + rec["h"] + 4
                            assert xi - 3 >= -S.BORDER and yi - 3 >= -S.BORDER and x_hi < fr.refs[r][p].shape[1] + S.BORDER and \
                                y_hi < fr.refs[r][p].shape[0] + S.BORDER, "window outside the border"
                            at = (rec["y"] * dst_strides[p] + rec["x"] * ps, ((yi + S.BORDER) * pst + xi + S.BORDER) * ps, rec["w"], rec["h"],
                                  rec["filter"], mx, my, avg)
                            blk[j] = at + ((dx, dy) if scaled else (0,))
                        self.mc.append((p, r, scaled, torch.from_numpy(blk.view(np.uint8).copy()).cuda(), len(sel)))
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
        for p, r, scaled, blk, n in self.mc:
            pad, pst = self.pads[r][p]
            (vp9.scaled_mc_batch if scaled else vp9.mc_batch)(dst[p], self.strides[p], pad, pst, blk, n, bit_depth=bd)
        for p, tx, rec, n in self.tx:
            vp9.itxfm_add_batch(tx, self.work[p], dst[p], self.strides[p], rec, n, bit_depth=bd)
