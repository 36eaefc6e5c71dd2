"""The per-call path a decoder has today for a picture's residuals, on the batch face (idct_batch with dst = NULL): each record's
coefficients copied into a scratch buffer, then one launch per (kind, log2 size) in place: IDCT, IDCT_DC, DST_4X4 and DEQUANT,
then RDPCM_H / RDPCM_V on the transform-skip and bypass records that use them.  Rotation and cross-component have no per-call
face: records that use them are not expressible here (expressible() says which)."""
import numpy as np

import hevc_res_picture_gen as G
from ffmpeg_amd import hevc

_KIND = {G.DCT: hevc.IDCT, G.DC: hevc.IDCT_DC, G.DST: hevc.DST_4X4, G.SKIP: hevc.DEQUANT}


def expressible(t):
    kf = int(t["kind_flags"])
    return not kf & (G.ROTATE | G.CROSS) and kf & 7 != G.ZERO


class BatchPath:
    """one plane: the launches it needs (built on the host once), run() -> the scratch buffer of residuals (record k at 16-aligned
    offset base[k])"""

    def __init__(self, torch, D, bd):
        self.torch, self.bd = torch, bd
        ks = [k for k in range(len(D.tus)) if expressible(D.tus[k])]
        self.base, off = {}, 0
        host = []
        for k in ks:
            t = D.tus[k]
            n = 1 << (2 * int(t["log2_size"]))
            self.base[k] = off
            host.append(D.coeffs[int(t["coeff_offset"]):int(t["coeff_offset"]) + n])
            off += n
        self.src = torch.from_numpy(np.concatenate(host) if host else np.zeros(16, np.int16)).cuda()
        self.calls = []
        groups = {}
        for k in ks:
            t = D.tus[k]
            kf, log2 = int(t["kind_flags"]), int(t["log2_size"])
            if kf & 7 in _KIND:
                groups.setdefault((_KIND[kf & 7], log2), []).append((k, int(t["col_limit"])))
        for k in ks:
            t = D.tus[k]
            kf, log2 = int(t["kind_flags"]), int(t["log2_size"])
            if kf & G.RDPCM_H:
                groups.setdefault((hevc.RDPCM_H, log2), []).append((k, 0))
            elif kf & G.RDPCM_V:
                groups.setdefault((hevc.RDPCM_V, log2), []).append((k, 0))
        for (kind, log2), recs in groups.items():       # dict order: every transform / dequant group before the RDPCM ones
            tu = np.zeros(len(recs), hevc.TU_DTYPE)
            for i, (k, cl) in enumerate(recs):
                tu[i] = (self.base[k], -1, cl)
            self.calls.append((kind, log2, torch.from_numpy(tu.view(np.uint8).copy()).cuda(), len(recs)))

    def run(self, stream=None):
        buf = self.src.clone()
        for kind, log2, tus, n in self.calls:
            hevc.idct_batch(kind, log2, buf, None, 0, tus, n, stream=stream, bit_depth=self.bd)
        return buf
