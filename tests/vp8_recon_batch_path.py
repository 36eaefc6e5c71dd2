"""The per-call route to a VP8 frame, through faces that existed before ffhip_vp8_recon_frames_dev: ffhip_vp8_mc_batch_dev on
edge-padded references, ffhip_h264_pred_batch_dev (FFHIP_H264_PRED_CODEC for the VP8 forms, the H.264 kinds for the forms VP8
shares with it), ffhip_vp8_luma_dc_wht_batch_dev and ffhip_vp8_idct_add_batch_dev, issued macroblock by macroblock in raster order
(sub-block by sub-block inside an I4x4 macroblock) — the launch chain a decoder needs without the whole-frame face.

The frame sits in device planes with the virtual border written out: one row of 127 above (the corner and the run to the right
included), 129 in the column to the left.  The slots are the ones ffhip_vp8_intra_modes() reports, the calls the ones ffhip_vp8_mb_preds()
reports; plan() lists the launches and their records, run() uploads the records once and issues them."""
import numpy as np

from ffmpeg_amd import h264, vp8

import vp8_recon_model as RM

LM, PAD = 16, 32          # the frame planes' left margin (bytes; one row above), the references' replicated border
CODEC = 8                 # FFHIP_H264_PRED_CODEC
SUB = {RM.B_VERT: (CODEC, 2), RM.B_HOR: (CODEC, 3), RM.B_VL: (CODEC, 9), RM.B_TM: (CODEC, 12), RM.B_DC_127: (CODEC, 0), RM.B_DC_129: (CODEC, 1),
       RM.B_VERT_PLAIN: (h264.PRED4x4, 0), RM.B_HOR_PLAIN: (h264.PRED4x4, 1), RM.B_DC: (h264.PRED4x4, 2), RM.B_DDL: (h264.PRED4x4, 3),
       RM.B_DDR: (h264.PRED4x4, 4), RM.B_VR: (h264.PRED4x4, 5), RM.B_HD: (h264.PRED4x4, 6), RM.B_HU: (h264.PRED4x4, 8)}
BLK16 = {RM.PRED_TM: (CODEC, 34), RM.PRED_DC_127: (CODEC, 35), RM.PRED_DC_129: (CODEC, 36)}       # else PRED16x16 with the slot's number
BLK8 = {RM.PRED_DC: (CODEC, 16), RM.PRED_LEFT_DC: (CODEC, 17), RM.PRED_TOP_DC: (CODEC, 18), RM.PRED_TM: (CODEC, 19),
        RM.PRED_DC_127: (CODEC, 20), RM.PRED_DC_129: (CODEC, 21)}                                  # else PRED8x8 with the slot's number


def strides(mb_w):
    return 16 * mb_w + 2 * LM, 8 * mb_w + 2 * LM


def plan(mbs, coeff_count, refs_present, mb_w, mb_h, fullpel):
    """(ops, pred records, idct records, wht records, mc records): ops in issue order"""
    sy, suv = strides(mb_w)
    st = (sy, suv, suv)
    org = lambda p: st[p] + LM   # noqa: E731  byte offset of the plane's sample (0, 0)
    ops, pred, idct, wht, mc = [], [], [], [], []

    def add_idct(mb, mb_x, mb_y, blocks):
        for b in blocks:
            c = RM.code(mb, b)
            if not c:
                continue
            if b < 16:
                p, y, x = 0, 16 * mb_y + 4 * (b >> 2), 16 * mb_x + 4 * (b & 3)
            else:
                q = (b - 16) & 3
                p, y, x = 1 + ((b - 16) >> 2), 8 * mb_y + 4 * (q >> 1), 8 * mb_x + 4 * (q & 1)
            idct.append((org(p) + y * st[p] + x, 2 * (int(mb["coeff_offset"]) + 16 * b), c == 1))
            ops.append(("idct", p, len(idct) - 1))

    def add_wht(mb):
        if mb["y2"]:
            wht.append((2 * (int(mb["coeff_offset"]) + 384), 2 * int(mb["coeff_offset"]), mb["y2"] == 1))
            ops.append(("wht", 0, len(wht) - 1))

    def add_pred(p, kind, mode, off, aux=0):
        pred.append((off, aux, mode))
        ops.append(("pred", p, len(pred) - 1, kind))

    for m in range(mb_w * mb_h):
        mb, mb_x, mb_y = mbs[m], m % mb_w, m // mb_w
        if not RM.well_formed(mb, refs_present, coeff_count):
            continue
        if mb["ref_frame"]:
            for c in vp8.mb_preds(mb, mb_x, mb_y, fullpel):
                p = int(c["plane"])
                N, W, H = (8, 8 * mb_w, 8 * mb_h) if p else (16, 16 * mb_w, 16 * mb_h)
                w, h = int(c["w"]), int(c["h"])
                sx = min(max(int(c["sx"]), -(w + 8)), W + 8)     # beyond that every tap reads the replicated border alike
                sy_ = min(max(int(c["sy"]), -(h + 8)), H + 8)
                mc.append((org(p) + (N * mb_y + int(c["y"])) * st[p] + N * mb_x + int(c["x"]), (PAD + sy_) * (W + 2 * PAD) + PAD + sx, w, h,
                           int(c["mx"]), int(c["my"]), int(c["hslot"]), int(c["vslot"])))
                ops.append(("mc", p, len(mc) - 1, int(mb["ref_frame"]) - 1))
            add_wht(mb)
            add_idct(mb, mb_x, mb_y, range(24))
            continue
        im = vp8.intra_modes(mb, mb_x, mb_y)
        for p in (1, 2):
            kind, mode = BLK8.get(int(im["chroma"]), (h264.PRED8x8, int(im["chroma"])))
            add_pred(p, kind, mode, org(p) + 8 * mb_y * suv + 8 * mb_x)
        if im["mode16"] != RM.PRED_NONE:
            kind, mode = BLK16.get(int(im["mode16"]), (h264.PRED16x16, int(im["mode16"])))
            add_pred(0, kind, mode, org(0) + 16 * mb_y * sy + 16 * mb_x)
            add_wht(mb)
            add_idct(mb, mb_x, mb_y, range(24))
            continue
        add_wht(mb)
        if mb_y and mb_x == mb_w - 1:
            ops.append(("splat", 0, 16 * mb_y - 1))   # the four samples right of the frame in the row above: its last sample, repeated
        for b in range(16):
            bx, by = b & 3, b >> 2
            off = org(0) + (16 * mb_y + 4 * by) * sy + 16 * mb_x + 4 * bx
            tr = org(0) + (16 * mb_y - 1) * sy + 16 * mb_x + 16 if bx == 3 else off - sy + 4
            kind, mode = SUB[int(im["sub"][b])]
            add_pred(0, kind, mode, off, tr)
            add_idct(mb, mb_x, mb_y, [b])
        add_idct(mb, mb_x, mb_y, range(16, 24))
    P = np.zeros(len(pred), h264.PRED_DTYPE)
    for i, (o, a, md) in enumerate(pred):
        P[i]["offset"], P[i]["aux"], P[i]["mode"] = o, a, md
    I = np.zeros(len(idct), vp8.IDCT_DTYPE)
    for i, (o, c, d) in enumerate(idct):
        I[i]["dst_offset"], I[i]["coeff_offset"], I[i]["dc_only"] = o, c, d
    Wt = np.zeros(len(wht), vp8.WHT_DTYPE)
    for i, (d, b, o) in enumerate(wht):
        Wt[i]["dc_offset"], Wt[i]["block_offset"], Wt[i]["dc_only"] = d, b, o
    Mc = np.zeros(len(mc), vp8.MC_DTYPE)
    for i, r in enumerate(mc):
        (Mc[i]["dst_offset"], Mc[i]["src_offset"], Mc[i]["width"], Mc[i]["h"], Mc[i]["mx"], Mc[i]["my"], Mc[i]["htaps"], Mc[i]["vtaps"]) = r
    return ops, P, I, Wt, Mc


class Frame:
    """the device state of one frame on this route"""

    def __init__(self, torch, mbs, coeffs, refs, init, mb_w, mb_h, bilinear=0, fullpel=0):
        self.torch, self.mb_w, self.mb_h = torch, mb_w, mb_h
        self.st = strides(mb_w) + strides(mb_w)[1:]
        self.ops, P, I, Wt, Mc = plan(mbs, len(coeffs), refs, mb_w, mb_h, fullpel)
        Mc["bilinear"] = bilinear
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()   # noqa: E731
        self.P, self.I, self.W, self.M = up(P), up(I), up(Wt), up(Mc)
        self.co_host = coeffs
        self.co = torch.from_numpy(coeffs.copy() if len(coeffs) else np.zeros(16, np.int16)).cuda()   # consumed by the batch faces
        self.init = []
        for p, a in enumerate(init):
            b = np.full((a.shape[0] + 1, self.st[p]), 129, np.uint8)
            b[0] = 127
            b[1:, LM:LM + a.shape[1]] = a
            self.init.append(b)
        self.planes = [up(b) for b in self.init]
        self.refs = [None if r is None else [up(np.pad(q, PAD, mode="edge")) for q in r] for r in refs]

    def reset(self):
        for d, b in zip(self.planes, self.init):
            d.copy_(self.torch.from_numpy(b.reshape(-1)))
        if len(self.co_host):
            self.co.copy_(self.torch.from_numpy(self.co_host))

    def issue(self):
        """every launch of the frame, in order, on the default stream; returns their number"""
        for op in self.ops:
            what, p, i = op[0], op[1], op[2]
            if what == "pred":
                h264.pred_batch(op[3], self.planes[p], self.st[p], self.P[12 * i:], 1)
            elif what == "idct":
                vp8.idct_add_batch(self.planes[p], self.st[p], self.co, self.I[12 * i:], 1)
            elif what == "wht":
                vp8.luma_dc_wht_batch(self.co, self.W[12 * i:], 1)
            elif what == "mc":
                W = (8 if p else 16) * self.mb_w
                vp8.mc_batch(self.planes[p], self.st[p], self.refs[op[3]][p], W + 2 * PAD, self.M[16 * i:], 1)
            else:   # splat
                row = self.planes[0].view(-1, self.st[0])[i + 1]
                row[LM + 16 * self.mb_w:LM + 16 * self.mb_w + 4] = row[LM + 16 * self.mb_w - 1]
        return len(self.ops)

    def result(self):
        out = []
        for p, d in enumerate(self.planes):
            a = d.cpu().numpy().reshape(-1, self.st[p])
            out.append(a[1:, LM:LM + (8 if p else 16) * self.mb_w].copy())
        return out
