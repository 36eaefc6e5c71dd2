"""HEVC residuals of whole pictures on the GPU (ffhip_hevc_residual_pictures_dev), byte for byte against the sequential model of
hevc_res_picture_gen.py (the oracle's per-call transforms in the reference's order) on res buffers pre-filled with a sentinel, the
coefficients checked unchanged; and against today's per-call path on the batch face.  Every call is followed by
ffhip_stream_synchronize(None) == 0."""
import numpy as np
import pytest

import hevc_res_batch_path as B
import hevc_res_picture_gen as G
from ffmpeg_amd import _lib, hevc

pytestmark = pytest.mark.gpu

SENT = 0x5A5A


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _upload(torch, pics):
    """device tensors per picture and plane: (coeffs, res pre-filled with the sentinel, tus, size_start)"""
    dev = []
    for planes in pics:
        d = []
        for D in planes:
            d.append((torch.from_numpy(D.coeffs.copy()).cuda(), torch.full((D.nres,), SENT, dtype=torch.int16, device="cuda"),
                      torch.from_numpy(np.ascontiguousarray(D.tus).view(np.uint8).copy()).cuda(), D.size_start))
        dev.append(d)
    return dev


def _sync():
    assert _lib.lib().ffhip_stream_synchronize(None) == 0, _lib.lib().ffhip_last_error()


def _compare(pics, dev, bd, cfi, wants=None):
    """the res buffers of _upload()'s tensors against the model (computed here unless given), the coefficients unchanged"""
    for i, planes in enumerate(pics):
        want = G.model(planes, bd, cfi, fill=SENT) if wants is None else wants[i]
        for p, D in enumerate(planes):
            got = dev[i][p][1].cpu().numpy()
            assert np.array_equal(got, want[p]), (i, p, np.nonzero(got != want[p])[0][:8])
            assert np.array_equal(dev[i][p][0].cpu().numpy(), D.coeffs), "coeffs were written"


def _run_and_check(pics, bd, cfi, stream=None):
    torch = _torch()
    dev = _upload(torch, pics)
    hevc.residual_pictures(dev, chroma_format_idc=cfi, bit_depth=bd, stream=stream)
    assert _lib.lib().ffhip_stream_synchronize(stream) == 0, _lib.lib().ffhip_last_error()
    _compare(pics, dev, bd, cfi)
    return dev


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("cfi", [0, 1, 2, 3])
def test_formats_and_depths(bd, cfi):
    rng = np.random.default_rng(10 * bd + cfi)
    pics = [G.build_planes(rng, [[70, 30, 12, 5], [25, 9, 4, 2], [25, 9, 4, 2]], cfi, big=bool(i & 1)) for i in range(3)]
    _run_and_check(pics, bd, cfi)


_COMBOS = [(G.DCT, 0), (G.DC, 0), (G.SKIP, 0), (G.SKIP, G.RDPCM_H), (G.SKIP, G.RDPCM_V), (G.BYPASS, 0), (G.BYPASS, G.RDPCM_H),
           (G.BYPASS, G.RDPCM_V), (G.ZERO, 0), (G.DST, 0), (G.SKIP, G.ROTATE), (G.SKIP, G.ROTATE | G.RDPCM_V),
           (G.BYPASS, G.ROTATE | G.RDPCM_H), (G.BYPASS, G.ROTATE)]


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("combo", _COMBOS, ids=lambda c: "k%d_f%02x" % c)
def test_each_kind_alone_with_cross(bd, combo):
    """one kind at each size it allows, luma and 4:4:4 chroma; every chroma record uses cross-component prediction"""
    kind, fl = combo
    rng = np.random.default_rng(bd + 7 * kind + fl)
    sizes = [2] if kind == G.DST or fl & G.ROTATE else [2, 3, 4, 5]
    counts = [[37 if s + 2 in sizes else 0 for s in range(4)]] * 3
    kinds = lambda r, log2, p: (kind, fl) if kind != G.DST or p == 0 else (G.DCT, 0)
    _run_and_check([G.build_planes(rng, counts, 3, p_cross=1.0, big=True, kinds=kinds)], bd, 3)


@pytest.mark.parametrize("log2", [2, 3, 4, 5])
def test_col_limit_edges(log2):
    """DCT records whose last significant position sits at each col_limit boundary of cabac.c"""
    n = 1 << log2
    rng = np.random.default_rng(log2)
    cs, recs = [], []
    for lx, ly in [(1, 0), (0, 1), (3, 3), (4, 0), (0, 4), (7, 7), (8, 0), (11, 11), (12, 0), (n - 1, n - 1), (n - 1, 0), (0, n - 1)]:
        if lx >= n or ly >= n:
            continue
        for order_kind in ((0, 1, 2) if log2 <= 3 else (0,)):
            order = G.scan_order(log2, order_kind)
            last = order.index((lx, ly))
            c = np.zeros((n, n), np.int16)
            for x, y in order[:last + 1]:
                c[y, x] = rng.integers(-3000, 3000)
            c[ly, lx] = 77
            cs.append(c.reshape(-1))
            recs.append(G.col_limit_of(lx, ly))
    tus = np.zeros(len(recs), G.RES_TU_DTYPE)
    for k, cl in enumerate(recs):
        tus[k] = (k * n * n, (len(recs) - 1 - k) * (n * n + 16), 0, log2, G.DCT, 0, cl)
    ss = [0] * (log2 - 1) + [len(recs)] * (6 - log2)
    D = G.ResPlane(np.concatenate(cs), len(recs) * n * n + 16 * len(recs), tus, ss)
    for bd in (8, 10, 12):
        _run_and_check([[D]], bd, 0)


def test_1080p_420_and_444_cross():
    rng = np.random.default_rng(1080)
    # a 1080p 4:2:0 picture's worth of TUs: about 60 % of it coded
    luma = [9000, 3500, 900, 200]
    pics = [G.build_planes(rng, [luma, [2200, 900, 220, 50], [2200, 900, 220, 50]], 1)]
    _run_and_check(pics, 8, 1)
    pics = [G.build_planes(rng, [[3000, 1200, 300, 60]] * 3, 3, p_cross=0.5)]
    _run_and_check(pics, 10, 3)


@pytest.mark.parametrize("npics", [16, 17])
def test_many_pictures_per_call(npics):
    """16 pictures go in one launch, 17 in two; the pictures' records differ in count and content"""
    rng = np.random.default_rng(npics)
    pics = [G.build_planes(rng, [[int(rng.integers(0, 60)), int(rng.integers(0, 20)), int(rng.integers(0, 6)), int(rng.integers(0, 3))],
                                 [10, 4, 1, 1], [int(rng.integers(0, 12)), 3, 2, 0]], 1) for _ in range(npics)]
    _run_and_check(pics, 8, 1)
    pics = [G.build_planes(rng, [[20, 8, 3, 1]] * 3, 3) for _ in range(npics)]
    _run_and_check(pics, 12, 3)


def _malformed(rng):
    """a 4:4:4 picture with one well-formed and one malformed copy of several records: (planes, which (p, k) are malformed)"""
    planes = G.build_planes(rng, [[12, 6, 3, 2]] * 3, 3, p_cross=0.5, gap=64)
    Y, U = planes[0], planes[1]
    bad = []

    def spoil(D, p, k, **kw):
        for key, v in kw.items():
            D.tus[k][key] = v
        bad.append((p, k))

    spoil(Y, 0, 0, kind_flags=6)                                   # unknown kind
    spoil(Y, 0, 1, kind_flags=G.DCT | G.RDPCM_H)                   # RDPCM on a transform
    spoil(Y, 0, 2, kind_flags=G.SKIP | G.RDPCM_H | G.RDPCM_V)      # both RDPCM flags
    spoil(Y, 0, 3, log2_size=3)                                    # not its group's size
    spoil(Y, 0, 12, kind_flags=G.DST)                              # DST at 8x8
    spoil(Y, 0, 13, kind_flags=G.SKIP | G.ROTATE)                  # rotation at 8x8
    spoil(Y, 0, 4, kind_flags=G.DCT | G.ROTATE)                    # rotation on a transform
    spoil(Y, 0, 5, coeff_offset=int(Y.tus[5]["coeff_offset"]) + 8)  # misaligned
    spoil(Y, 0, 6, res_offset=Y.nres - 8)                          # past nres
    spoil(Y, 0, 7, coeff_offset=Y.coeffs.size)                     # past ncoeffs
    spoil(Y, 0, 8, kind_flags=G.BYPASS | G.CROSS)                  # cross-component on luma
    spoil(U, 1, 9, kind_flags=G.SKIP | G.CROSS, res_scale_val=3)   # a scale outside the set
    spoil(U, 1, 10, kind_flags=G.BYPASS | G.CROSS, luma=12)        # a luma record of another size
    spoil(U, 1, 11, kind_flags=G.BYPASS | G.CROSS, luma=10 ** 6)   # out of range
    spoil(U, 1, 0, kind_flags=G.BYPASS | G.CROSS, luma=0)          # its luma record is malformed
    spoil(U, 1, 18, res_offset=-16)                                # negative
    spoil(Y, 0, 9, log2_size=1)                                    # log2 below 2
    spoil(Y, 0, 21, log2_size=6)                                   # log2 above 5
    spoil(Y, 0, 10, kind_flags=G.DCT | 0x80)                       # the reserved bit
    return planes, bad


def test_malformed_records_write_nothing():
    rng = np.random.default_rng(77)
    planes, bad = _malformed(rng)
    for p, k in bad:
        assert not G.record_ok(planes, p, k, 3), (p, k)
    dev = _run_and_check([planes], 8, 3)
    # the spoiled records' own slots kept the sentinel where no well-formed record writes
    for p, k in bad:
        t = planes[p].tus[k]
        ro, n = int(t["res_offset"]), 1 << (2 * int(t["log2_size"]))
        if 0 <= ro and ro + n <= planes[p].nres:
            got = dev[0][p][1].cpu().numpy()[ro:ro + n]
            covered = np.zeros(planes[p].nres, bool)
            for j in range(len(planes[p].tus)):
                if G.record_ok(planes, p, j, 3):
                    tj = planes[p].tus[j]
                    covered[int(tj["res_offset"]):int(tj["res_offset"]) + (1 << (2 * int(tj["log2_size"])))] = True
            assert np.all(got[~covered[ro:ro + n]] == SENT), (p, k)
    # chroma format 1: a _CROSS record is malformed
    planes = G.build_planes(rng, [[8, 4, 2, 1]] * 3, 1)
    planes[1].tus[0]["kind_flags"] = G.BYPASS | G.CROSS
    assert not G.record_ok(planes, 1, 0, 1)
    _run_and_check([planes], 10, 1)


@pytest.mark.parametrize("bd", [8, 10])
def test_same_residuals_as_the_batch_path(bd):
    torch = _torch()
    rng = np.random.default_rng(bd)
    planes = G.build_planes(rng, [[300, 120, 40, 10], [80, 30, 10, 3], [80, 30, 10, 3]], 1, big=True)
    dev = _run_and_check([planes], bd, 1)
    n_checked = 0
    for p, D in enumerate(planes):
        path = B.BatchPath(torch, D, bd)
        out = path.run()
        _sync()
        out = out.cpu().numpy()
        got = dev[0][p][1].cpu().numpy()
        for k, base in path.base.items():
            t = D.tus[k]
            n = 1 << (2 * int(t["log2_size"]))
            ro = int(t["res_offset"])
            assert np.array_equal(got[ro:ro + n], out[base:base + n]), (p, k, int(t["kind_flags"]))
            n_checked += 1
    assert n_checked > 500


class Chain:
    """residual face -> inter pictures -> intra pictures -> loop filter pictures on one stream, with no host sync in between: the DPB
    planes equal those of the same chain of models fed with the model's residuals.  One residual launch makes both res buffers per
    plane (the inter TUs' and the intra TUs', as two pictures of the call); the faces take them at the TU records' res_offset.
    upload() draws the pictures and puts them on the device, call(stream) queues the four faces, compare() runs the models;
    inputs() / outputs() are the device tensors the chain only reads / writes (tests/picture_faces.py: run_staged)."""
    name = "hevc_residual+inter+intra+loop_filter"

    def __init__(self, bd, cfi):
        self.bd, self.cfi = bd, cfi

    def upload(self, torch):
        import hevc_inter_picture_gen as PG
        import hevc_intra_picture_gen as IG
        import hevc_lf_picture_gen as LG
        import test_gpu_hevc_inter_picture as TI
        import test_gpu_hevc_lf_picture as TL
        bd, cfi = self.bd, self.cfi
        rng = np.random.default_rng(9100 + 10 * bd + cfi)
        W, H, lc = self.geom = 192, 128, 5
        hs, vs = int(cfi in (1, 2)), int(cfi == 1)
        ip = IG.Picture(rng, W, H, lc, bd, cfi, p_intra=0.5)
        pic = PG.InterPicture(rng, W, H, lc, bd, cfi, nrefs=3, nslices=1, slice_types=["P"], p_inter=1.0, p_pcm=0.0)
        nplanes = pic.nplanes
        pus, tus = [], [[] for _ in range(nplanes)]
        blocks, nres = [[] for _ in range(nplanes)], [0] * nplanes
        for y in range(0, H, 8):
            for x in range(0, W, 8):
                if ip.intra[y >> 2, x >> 2]:
                    continue
                a = (y >> lc) * pic.ctb_w + (x >> lc)
                pus.append(dict(x=x, y=y, w=8, h=8, flags=1, ref_idx=[int(rng.integers(0, pic.slices[0]["num_ref"][0])), 0], slice=0,
                                mv=[[int(v) for v in rng.integers(-80, 81, 2)], [0, 0]], ctb=a, part="2Nx2N"))
                for p in range(nplanes):
                    # the CU's transform blocks: 8x8 luma; chroma 4x4 (4:2:0), two 4x4 stacked (4:2:2), 8x8 (4:4:4)
                    if p == 0 or cfi == 3:
                        boxes = [(x, y, 3)]
                    else:
                        boxes = [(x >> hs, (y >> vs) + 4 * j, 2) for j in range(1 if vs else 2)]
                    for bx, by, log2 in boxes:
                        if rng.random() < 0.15:          # cbf 0: no residual
                            continue
                        tus[p].append(dict(x=bx, y=by, res_offset=nres[p], log2_size=log2, ctb=a))
                        blocks[p].append((bx, by, log2, nres[p]))
                        nres[p] += 1 << (2 * log2)
        pic.pus, pic.tus = pus, tus
        inter_planes = G.planes_for_blocks(rng, blocks, [max(n, 16) for n in nres], cfi, intra=False)
        iblocks = [[(r["x"], r["y"], r["log2_size"], r["res_offset"]) for r in ip.recs[p] if r["res_offset"] >= 0] for p in range(nplanes)]
        intra_planes = G.planes_for_blocks(rng, iblocks, [ip.res[p].size for p in range(nplanes)], cfi, intra=True)
        assert any(int(t["kind_flags"]) & G.CROSS for D in inter_planes + intra_planes for t in D.tus) == (cfi == 3)
        dev = _upload(torch, [inter_planes, intra_planes])
        # the faces' inputs; their res buffers are the residual face's outputs
        pic.res = [np.zeros(max(n, 16), np.int16) for n in nres]
        start = [pl.copy() for pl in ip.planes]
        a, dst, keep = TI.upload(torch, pic, planes=start)
        for p in range(nplanes):
            d, st, d_tus, d_st, _ = a[0][p]
            a[0][p] = (d, st, d_tus, d_st, dev[0][p][1])
        intra_args = []
        for p in range(nplanes):
            arr, starts = ip.pack(p, dtype=hevc.INTRA_TU_DTYPE)
            d_tus = torch.from_numpy(arr.view(np.uint8).copy()).cuda()
            d_st = torch.from_numpy(starts).cuda()
            keep += [d_tus, d_st]
            intra_args.append((dst[p][1], a[0][p][1], d_tus, d_st, dev[1][p][1]))
        lf = LG.LfPicture(rng, W, H, lc, bd, cfi, tiles=(2, 1), nslices=2)
        maps = TL.upload_maps(torch, lf)
        outs, lf_planes = [], []
        for p in range(lf.nplanes):
            h, w = lf.src[p].shape
            ds = TL._stride(w, bd, 16)
            dh = np.full((h, ds), 0x5A, np.uint8)
            d = torch.from_numpy(dh.copy()).cuda()
            outs.append((d, dh))
            lf_planes.append((dst[p][1], a[0][p][1], d, ds))
        self.ip, self.pic, self.lf, self.start = ip, pic, lf, start
        self.inter_planes, self.intra_planes = inter_planes, intra_planes
        self.dev, self.a, self.dst, self.keep, self.intra_args, self.maps, self.outs, self.lf_planes = dev, a, dst, keep, intra_args, maps, outs, lf_planes

    def call(self, stream):
        (W, H, lc), bd, cfi = self.geom, self.bd, self.cfi
        hevc.residual_pictures(self.dev, chroma_format_idc=cfi, bit_depth=bd, stream=stream)
        hevc.inter_pictures([self.a], W, H, lc, chroma_format_idc=cfi, bit_depth=bd, stream=stream)
        hevc.intra_pictures([self.intra_args], W, H, lc, chroma_format_idc=cfi, bit_depth=bd, stream=stream)
        hevc.loop_filter_pictures([(self.lf_planes, self.maps)], W, H, lc, self.lf.lmc, chroma_format_idc=cfi, bit_depth=bd, stream=stream)

    def inputs(self):
        pl, pus, pst, sl, refs = self.a
        ins = [t for d in self.dev for q in d for t in (q[0], q[2])] + [t for q in pl for t in q[2:4]] + [pus, pst, sl]
        ins += [t for ref in refs for t, _ in ref] + [t for q in self.intra_args for t in q[2:4]]
        return ins + [t for t in self.maps.values() if hasattr(t, "is_cuda")]

    def outputs(self):
        """the res buffers, the DPB planes reconstructed in place, the filtered planes"""
        return [q[1] for d in self.dev for q in d] + [d for _, d in self.dst] + [d for d, _ in self.outs]

    def compare(self, view=lambda t: t):
        import hevc_inter_picture_gen as PG
        import hevc_intra_picture_gen as IG
        import hevc_lf_picture_gen as LG
        bd, cfi, pic, ip = self.bd, self.cfi, self.pic, self.ip
        # the same chain of models, fed with the model's residuals
        pic.res = G.model(self.inter_planes, bd, cfi)
        ip.res = G.model(self.intra_planes, bd, cfi)
        ip.planes = PG.model(pic, planes=self.start)
        recon = IG.model(ip)
        want = LG.model(self.lf, planes=recon)
        ps = 1 if bd == 8 else 2
        for p, (d, dh) in enumerate(self.outs):
            h, w = want[p].shape
            exp = dh.copy()
            exp[:, :w * ps] = want[p].astype(np.uint8 if bd == 8 else np.uint16).view(np.uint8).reshape(h, w * ps)
            assert np.array_equal(view(d).cpu().numpy(), exp), "plane %d differs from the chained models" % p


@pytest.mark.parametrize("bd,cfi", [(8, 0), (8, 1), (10, 2), (10, 3), (8, 3), (12, 1)])
def test_chained_into_inter_intra_and_loop_filter_pictures(bd, cfi):
    """Chain on the NULL stream (tests/test_gpu_picture_streams.py runs it on a created one)"""
    torch = _torch()
    chain = Chain(bd, cfi)
    chain.upload(torch)
    chain.call(None)
    _sync()
    torch.cuda.synchronize()
    chain.compare()
