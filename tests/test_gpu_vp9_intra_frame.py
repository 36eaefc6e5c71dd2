"""VP9 intra reconstruction of whole frames on the GPU (ffhip_vp9_intra_frames_dev), byte for byte against the sequential plane model
of vp9_intra_frame_gen.py (the oracle's vp9 intra_pred and itxfm_add on host-built edge lines), stride padding and the rows below the
decoded area included.  Every call is followed by ffhip_stream_synchronize(None) == 0."""
import numpy as np
import pytest

import vp9_intra_frame_gen as G
from ffmpeg_amd import _lib, vp9

pytestmark = pytest.mark.gpu

SS = [(1, 1), (1, 0), (0, 1), (0, 0)]


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _dt(bd):
    return np.uint8 if bd == 8 else np.uint16


def _stride(w, bd, extra):
    ps = 1 if bd == 8 else 2
    return (w * ps + 63) // 64 * 64 + extra


def image(rng, a, bd, stride, below=3):
    """a plane (int64 samples of the decoded area) as a (rows + below, stride) byte image; the padding right of it and the rows below
    it random garbage"""
    h, w = a.shape
    ps = 1 if bd == 8 else 2
    host = rng.integers(0, 256, (h + below, stride)).astype(np.uint8)
    host[:h, :w * ps] = a.astype(_dt(bd)).view(np.uint8).reshape(h, w * ps)
    return host


def upload(torch, fr, extra=0, recs=None, planes=None):
    """(the face's tuple for this frame, the destination (host image, device tensor) per plane, tensors to keep alive)"""
    recs = fr.recs if recs is None else recs
    src = fr.planes if planes is None else planes
    pl, dst, keep = [], [], []
    for p in range(3):
        st = _stride(src[p].shape[1], fr.bd, extra + 4 * p * (1 if fr.bd == 8 else 2))
        host = image(fr.rng, src[p], fr.bd, st)
        d = torch.from_numpy(host.copy()).cuda()
        arr, starts = fr.pack(p, recs[p])
        d_recs = torch.from_numpy(arr.view(np.uint8).copy() if len(arr) else np.zeros(12, np.uint8)).cuda()
        d_st = torch.from_numpy(starts).cuda()
        d_co = torch.from_numpy(fr.coeff_array(p)).cuda()
        keep += [d, d_recs, d_st, d_co]
        pl.append((d, st, d_recs, d_st, d_co))
        dst.append((host, d))
    return (pl, fr.log2_tile_cols), dst, keep


def compare(fr, dst, want):
    ps = 1 if fr.bd == 8 else 2
    for p, (host, d) in enumerate(dst):
        h, w = want[p].shape
        exp = host.copy()
        exp[:h, :w * ps] = want[p].astype(_dt(fr.bd)).view(np.uint8).reshape(h, w * ps)
        got = d.cpu().numpy()
        bad = np.argwhere(got != exp)
        assert not len(bad), "plane %d: %d mismatches, first (row, byte) %s: got %s want %s" % (
            p, len(bad), bad[:3].tolist(), got[tuple(bad[0])], exp[tuple(bad[0])])


def sync():
    assert _lib.lib().ffhip_stream_synchronize(None) == 0, _lib.lib().ffhip_last_error()


def run(frames, extra=0, recs=None):
    """reconstruct the frames (one geometry) in one call, with the records `recs` when given (the frame's own plus malformed ones),
    and compare every plane, padding included, with the model of the frame's own records"""
    torch = _torch()
    F0 = frames[0]
    args, dsts, keep = [], [], []
    for i, fr in enumerate(frames):
        a, dst, k = upload(torch, fr, extra, recs[i] if recs else None)
        args.append(a)
        dsts.append(dst)
        keep.append(k)
    vp9.intra_frames(args, F0.W, F0.H, ss=(F0.ss_h, F0.ss_v), bit_depth=F0.bd)
    sync()
    torch.cuda.synchronize()
    for fr, dst in zip(frames, dsts):
        compare(fr, dst, G.model(fr))


@pytest.mark.parametrize("bd", (8, 10, 12))
@pytest.mark.parametrize("ss", SS, ids=["420", "422", "440", "444"])
def test_depth_subsampling(bd, ss):
    rng = np.random.default_rng(7000 + bd * 10 + SS.index(ss))
    run([G.IntraFrame(rng, 203, 141, bd, *ss)])                       # not multiples of 8 or 64
    run([G.IntraFrame(rng, 128, 64, bd, *ss, lossless=True)])         # the WHT


@pytest.mark.parametrize("log2", (0, 1, 2))
def test_tile_columns(log2):
    rng = np.random.default_rng(7100 + log2)
    run([G.IntraFrame(rng, 1024, 200, 8, 1, 1, log2_tile_cols=log2)])


def test_1080p_keyframe():
    run([G.IntraFrame(np.random.default_rng(7200), 1920, 1080, 8, 1, 1, log2_tile_cols=2)])


def test_sixteen_frames():
    rng = np.random.default_rng(7300)
    run([G.IntraFrame(rng, 96, 72, 10, 1, 1, log2_tile_cols=i % 2) for i in range(16)])


def test_seventeen_frames_are_split():
    rng = np.random.default_rng(7400)
    run([G.IntraFrame(rng, 72, 40, 8, 1, 0) for i in range(17)])


def test_tall_frames_split_their_counters():
    """16 frames of 256 superblock rows: 3 * 256 counters a frame, so the call needs several launches"""
    rng = np.random.default_rng(7500)
    run([G.IntraFrame(rng, 64, 16384, 8, 1, 1, min_log2=4) for _ in range(16)])


def test_stride_padding_survives():
    rng = np.random.default_rng(7600)
    run([G.IntraFrame(rng, 136, 90, 8, 1, 1)], extra=72)
    run([G.IntraFrame(rng, 130, 88, 12, 0, 0)], extra=40)


def test_intra_holes_of_inter_frames():
    """the inter samples around the holes are read as edges and never written"""
    rng = np.random.default_rng(7700)
    for bd, ss in ((8, (1, 1)), (10, (0, 0)), (12, (1, 0))):
        fr = G.IntraFrame(rng, 200, 136, bd, *ss, inter=True, p_intra=0.3)
        assert fr.recs[0]
        run([fr])


def test_malformed_records_write_nothing():
    """each class of malformed record, inserted among the real ones (the real ones keep their order): the planes are those of the
    real records alone"""
    rng = np.random.default_rng(7800)
    fr = G.IntraFrame(rng, 200, 128, 8, 1, 1)
    nsb = fr.sb_w * fr.sb_h
    recs = []
    for p in range(3):
        real = list(fr.recs[p])
        Cw = 64 >> fr.hs[p]
        out = []
        for j, r in enumerate(real):
            out.append(r)
            if j % 7:
                continue
            b = dict(r)
            kind = (j // 7) % 11
            if kind == 0:
                b["tx"] = 5
            elif kind == 1:
                b["mode"] = 10
            elif kind == 2:
                b["txtp"] = 4
            elif kind == 3:
                b["flags"] = r["flags"] | 8                         # an unknown flag
            elif kind == 4:
                b["flags"] = G.DC_ONLY                              # dc_only without residual
            elif kind == 5:
                b["x"] = r["x"] + 2                                 # not a multiple of N
            elif kind == 6:
                b["sb"] = (r["sb"] + 1) % nsb                       # listed under another superblock
            elif kind == 7:
                b["x"], b["tx"] = (r["x"] // Cw) * Cw + Cw - 16, 3  # across its superblock's right edge
            elif kind == 8:
                b["y"] = fr.dh[p] + 4                               # origin below the decoded area
            elif kind == 9:
                b["x"], b["tx"], b["flags"] = (r["x"] // Cw) * Cw + Cw - 4, 0, G.HAVE_RIGHT  # top-right outside the superblock
            else:
                b["tx"], b["flags"] = 4, 16
            b["flags"] |= G.RESIDUAL if kind not in (4, 9, 10) else 0
            out.append(b)
        recs.append(out)
    for p in range(3):
        assert sum(not G.well_formed(fr, p, r) for r in recs[p]) >= 11
    run([fr], recs=[recs])


class Chain:
    """inter face -> intra face -> ffhip_vp9_loopfilter_frames_dev on the same planes and stream: equal to the loop filter run on the
    model chain's planes.  upload / call(stream) / compare, inputs() / outputs() as tests/picture_faces.py has them."""
    name = "vp9_inter+intra+loopfilter"

    def upload(self, torch):
        import vp9_inter_frame_gen as IG
        import vp9_lf_gen as LG
        import test_gpu_vp9_inter_frame as TI
        rng = np.random.default_rng(7900)
        lim, mblim = LG.filter_lut(2)
        self.fr = fr = G.IntraFrame(rng, 200, 136, 8, 1, 1, inter=True, p_intra=0.3)
        ifr = fr.inter
        self.cols, self.rows, sbc, sbr = fr.cols, fr.rows, fr.sb_w, fr.sb_h
        big = [np.zeros(((sbr * 64) >> fr.vs[p], (sbc * 64) >> fr.hs[p]), np.int64) for p in range(3)]
        for p in range(3):
            big[p][:fr.dh[p], :fr.dw[p]] = ifr.planes[p]               # what the inter stage starts from
        # the device chain: inter face, intra face, loop filter
        self.a_inter, dst, self.keep = TI.upload(torch, ifr, planes=big)
        self.planes = [dst[p][1] for p in range(3)]
        self.strides = [self.a_inter[0][p][1] for p in range(3)]
        self.intra_pl = []
        for p in range(3):
            arr, starts = fr.pack(p)
            d_recs = torch.from_numpy(arr.view(np.uint8).copy()).cuda()
            d_st = torch.from_numpy(starts).cuda()
            d_co = torch.from_numpy(fr.coeff_array(p)).cuda()
            self.intra_pl.append((self.planes[p], self.strides[p], d_recs, d_st, d_co))
        filt = np.zeros(sbr * sbc, LG.FILTER_DT)
        for r in range(sbr):
            for c in range(sbc):
                filt[r * sbc + c] = LG.structured(rng, r, c, self.cols, self.rows)
        self.tabs = torch.from_numpy(vp9.lf_sb_tables(filt.view(np.uint8).reshape(sbr * sbc, 192), sbc, sbr, lim, mblim).view(np.int32)).cuda()
        # the model chain's planes, filtered by a launch of their own
        m = G.model(fr, planes=IG.model(ifr, planes=big))
        self.other = [torch.from_numpy(TI._plane_bytes(m[p], fr.bd, self.strides[p])).cuda() for p in range(3)]

    def call(self, stream):
        fr, planes, other, strides = self.fr, self.planes, self.other, self.strides
        vp9.inter_frames([self.a_inter], fr.W, fr.H, ss=(1, 1), bit_depth=8, stream=stream)
        vp9.intra_frames([(self.intra_pl, 0)], fr.W, fr.H, ss=(1, 1), bit_depth=8, stream=stream)
        vp9.loopfilter_frames([(planes[0], planes[1], planes[2], self.tabs)], strides[0], strides[1], self.cols, self.rows, bit_depth=8, stream=stream)
        vp9.loopfilter_frames([(other[0], other[1], other[2], self.tabs)], strides[0], strides[1], self.cols, self.rows, bit_depth=8, stream=stream)

    def inputs(self):
        pl, preds, pst, refs = self.a_inter
        return [t for q in pl for t in q[2:]] + [preds, pst] + [t for ref in refs for t, _ in ref] + [t for q in self.intra_pl for t in q[2:]] + [self.tabs]

    def outputs(self):
        return self.planes + self.other

    def compare(self, view=lambda t: t):
        import torch
        for p in range(3):
            assert torch.equal(view(self.planes[p]), view(self.other[p])), p


def test_chained_with_inter_and_the_loop_filter_on_one_stream():
    """Chain on the NULL stream (tests/test_gpu_picture_streams.py runs it on a created one)"""
    torch = _torch()
    chain = Chain()
    chain.upload(torch)
    chain.call(None)
    sync()
    torch.cuda.synchronize()
    chain.compare()


@pytest.mark.parametrize("bd,ss", [(8, (1, 1)), (10, (0, 0)), (12, (1, 0))])
def test_same_planes_as_the_batch_faces(bd, ss):
    """the per-call route: intra_pred_batch + itxfm_add_batch record by record, edges gathered on the host from the current plane"""
    import vp9_intra_batch_path as BP
    torch = _torch()
    rng = np.random.default_rng(8000 + bd)
    fr = G.IntraFrame(rng, 72, 40, bd, *ss, log2_tile_cols=0)
    a, dst, keep = upload(torch, fr)
    other = [torch.from_numpy(host.copy()).cuda() for host, _ in dst]
    vp9.intra_frames([a], fr.W, fr.H, ss=ss, bit_depth=bd)
    sync()
    BP.run(torch, fr, other, [pl[1] for pl in a[0]])
    sync()
    torch.cuda.synchronize()
    for p in range(3):
        assert torch.equal(dst[p][1], other[p]), "plane %d differs from the batch faces" % p
    compare(fr, dst, G.model(fr))
