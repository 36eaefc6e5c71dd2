"""A picture of hevc_inter_picture_gen.py through the per-call batch faces that predate ffhip_hevc_inter_pictures_dev: references
copied into buffers with an 80-sample edge-replicated border, ffhip_hevc_mc_batch_dev (uni, or list 0 into int16 rows) and
ffhip_hevc_mc_w_batch_dev (uni_w, bi, bi_w) once per (plane, stage, reference), then ffhip_hevc_idct_batch_dev (add only) once per
(plane, TU size).  Only valid while every window stays inside the border (no far MVs): the cross-check of the new face and the
comparison leg of tools/bench_hevc_inter_picture.py."""
import numpy as np

import hevc_inter_picture_gen as G
from ffmpeg_amd import hevc

BORDER = 80


def pad_refs(torch, pic):
    """per slot, per plane: (device tensor of the padded plane, stride in bytes)"""
    out = []
    for ref in pic.refs:
        planes = []
        for p in range(pic.nplanes):
            a = np.pad(ref[p], BORDER, mode="edge").astype(np.uint8 if pic.bd == 8 else np.uint16)
            planes.append((torch.from_numpy(a.view(np.uint8).copy()).cuda(), a.shape[1] * a.itemsize))
        out.append(planes)
    return out


def plan(pic, dst_strides):
    """the prediction launches in order: (plane, chroma, kind, slot, records, bi blocks of the plane); kind "put" (list 0 of the bi
    blocks into int16 rows), "uni", or hevc.MC_UNI_W / MC_BI / MC_BI_W"""
    ps = 1 if pic.bd == 8 else 2
    launches = []
    for p in range(pic.nplanes):
        pw, ph = pic.W >> pic.hs[p], pic.H >> pic.vs[p]
        pst = pw + 2 * BORDER                                   # padded row, samples
        groups, nbi = {}, 0
        for pu in pic.pus:
            S = pic.slices[pu["slice"]]
            g = [G.pu_geometry(pic, pu, p, l) for l in range(2)]
            bx, by, bw, bh = g[0][:4]
            slot = [int(S["ref"][l][pu["ref_idx"][l]]) for l in range(2)]
            denom = S["chroma_log2_denom"] if p else S["luma_log2_denom"]

            def wo(l):
                ri = pu["ref_idx"][l]
                return (int(S["chroma_weight"][l][ri][p - 1]), int(S["chroma_offset"][l][ri][p - 1])) if p else \
                    (int(S["luma_weight"][l][ri]), int(S["luma_offset"][l][ri]))

            def blk(l, **kw):
                xi, yi, mx, my = g[l][4:]
                assert 3 - BORDER <= xi and xi + bw + 4 <= pw + BORDER and 3 - BORDER <= yi and yi + bh + 4 <= ph + BORDER, \
                    "window outside the border"
                return dict(kw, src_offset=((yi + BORDER) * pst + xi + BORDER) * ps, width=bw, height=bh, mx=mx, my=my)

            dofs = by * dst_strides[p] + bx * ps
            if pu["flags"] == 3:
                (w0, o0), (w1, o1) = wo(0), wo(1)
                mode = hevc.MC_BI_W if S["weighted"] else hevc.MC_BI
                groups.setdefault(("put", slot[0]), []).append(blk(0, dst_offset=nbi * 4096))
                groups.setdefault((mode, slot[1]), []).append(blk(1, dst_offset=dofs, src2_offset=nbi * 4096, wx0=w0, wx1=w1, ox=o0 + o1,
                                                                  denom=denom))
                nbi += 1
            elif S["weighted"]:
                l = pu["flags"] >> 1
                w, o = wo(l)
                groups.setdefault((hevc.MC_UNI_W, slot[l]), []).append(blk(l, dst_offset=dofs, wx0=w, ox=o, denom=denom))
            else:
                l = pu["flags"] >> 1
                groups.setdefault(("uni", slot[l]), []).append(blk(l, dst_offset=dofs))
        for (kind, slot), recs in sorted(groups.items(), key=lambda kv: (kv[0][0] != "put", str(kv[0][0]), kv[0][1])):
            dt = hevc.MC_DTYPE if kind in ("put", "uni") else hevc.MCW_DTYPE
            arr = np.zeros(len(recs), dt)
            for i, r in enumerate(recs):
                for f, v in r.items():
                    arr[i][f] = v
            launches.append((p, int(p > 0), kind, slot, arr, nbi))
    return launches


def residual_plan(pic, dst_strides):
    """the residual launches: (plane, log2 size, int16 residual blocks, FFHipHevcTU records)"""
    ps = 1 if pic.bd == 8 else 2
    out = []
    for p in range(pic.nplanes):
        for lg in (2, 3, 4, 5):
            tl = [t for t in pic.tus[p] if t["log2_size"] == lg and t["res_offset"] >= 0]
            if not tl:
                continue
            N = 1 << lg
            coeffs = np.concatenate([pic.res[p][t["res_offset"]:t["res_offset"] + N * N] for t in tl]).astype(np.int16)
            tus = np.zeros(len(tl), hevc.TU_DTYPE)
            tus["coeff_offset"] = np.arange(len(tl)) * N * N
            tus["dst_offset"] = [t["y"] * dst_strides[p] + t["x"] * ps for t in tl]
            tus["col_limit"] = N
            out.append((p, lg, coeffs, tus))
    return out


class BatchPath:
    """the device side of plan() / residual_plan() for one picture, uploaded once; run() issues the launches"""

    def __init__(self, torch, pic, dst_strides, prefs=None):
        self.pic, self.strides = pic, dst_strides
        self.prefs = pad_refs(torch, pic) if prefs is None else prefs
        self.mc = [(p, c, k, s, torch.from_numpy(a.view(np.uint8).copy()).cuda(), len(a)) for p, c, k, s, a, nbi in plan(pic, dst_strides)]
        nbi = max([1] + [nb for *_, nb in plan(pic, dst_strides)])
        self.tmp = [torch.zeros(nbi * 4096, dtype=torch.int16, device="cuda") for _ in range(pic.nplanes)]
        self.res = [(p, lg, torch.from_numpy(c).cuda(), torch.from_numpy(t.view(np.uint8).copy()).cuda(), len(t))
                    for p, lg, c, t in residual_plan(pic, dst_strides)]

    def launches(self):
        return len(self.mc) + len(self.res)

    def run(self, dst, stream=None):
        """predict into dst[p] (device tensors), then add the residuals (ADD_ONLY leaves the residual blocks as they are)"""
        bd = self.pic.bd
        for p, chroma, kind, slot, blocks, n in self.mc:
            src, sst = self.prefs[slot][p]
            if kind == "put":
                hevc.mc_batch(chroma, 0, self.tmp[p], 0, src, sst, blocks, n, stream=stream, bit_depth=bd)
            elif kind == "uni":
                hevc.mc_batch(chroma, 1, dst[p], self.strides[p], src, sst, blocks, n, stream=stream, bit_depth=bd)
            else:
                hevc.mc_w_batch(chroma, kind, dst[p], self.strides[p], src, sst, self.tmp[p] if kind != hevc.MC_UNI_W else None, blocks, n,
                                stream=stream, bit_depth=bd)
        for p, lg, coeffs, tus, n in self.res:
            hevc.idct_batch(hevc.ADD_ONLY, lg, coeffs, dst[p], self.strides[p], tus, n, stream=stream, bit_depth=bd)
