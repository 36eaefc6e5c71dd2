"""The per-call route to a frame's intra blocks: for each record in decoding order, the edge lines gathered on the host from the plane
as the device holds it (the rules of include/ffhip.h, vp9_intra_frame_gen.edges), then one intra_pred_batch and one itxfm_add_batch
launch on a scratch block, whose samples inside the decoded area are copied into the plane — the launch-and-read-back chain a
decoder would need without the whole-frame face."""
import numpy as np

import vp9_intra_frame_gen as G
from ffmpeg_amd import vp9


def run(torch, fr, planes, strides):
    """reconstruct fr's records into the device byte images planes[p] ((rows, strides[p]) uint8 tensors)"""
    ps = 1 if fr.bd == 8 else 2
    dt = np.uint8 if fr.bd == 8 else np.uint16
    for p in range(3):
        dw, dh = fr.dw[p], fr.dh[p]
        for r in sorted(fr.recs[p], key=lambda r: r["sb"]):
            if not G.well_formed(fr, p, r):
                continue
            host = planes[p].cpu().numpy()
            P = host[:dh, :dw * ps].copy().view(dt).astype(np.int64)
            mode, left, top = G.edges(fr, P, p, r)
            tx = r["tx"]
            N = 4 if tx == 4 else 4 << tx
            line = np.concatenate([left, top]).astype(dt)                  # left[0..N-1], the corner, top[0..max(N, 8) - 1]
            d_line = torch.from_numpy(line.view(np.uint8).copy()).cuda()
            blk = torch.zeros(N * N * ps, dtype=torch.uint8, device="cuda")
            rec = np.zeros(1, vp9.INTRA_DTYPE)
            rec["mode"] = mode
            d_rec = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
            vp9.intra_pred_batch(0 if tx == 4 else tx, blk, N * ps, d_line, d_rec, 1, bit_depth=fr.bd)
            if r["flags"] & G.RESIDUAL:
                co = fr.coeff_array(p)[r["coeff_offset"]:r["coeff_offset"] + N * N].copy()
                d_co = torch.from_numpy(co).cuda()
                tu = np.zeros(1, vp9.TU_DTYPE)
                tu["txtp"], tu["dc_only"] = r["txtp"], 1 if r["flags"] & G.DC_ONLY else 0
                d_tu = torch.from_numpy(tu.view(np.uint8).copy()).cuda()
                vp9.itxfm_add_batch(tx, d_co, blk, N * ps, d_tu, 1, bit_depth=fr.bd)
            x, y = r["x"], r["y"]
            h, w = min(N, dh - y), min(N, dw - x)
            planes[p][y:y + h, x * ps:(x + w) * ps] = blk.view(N, N * ps)[:h, :w * ps]
