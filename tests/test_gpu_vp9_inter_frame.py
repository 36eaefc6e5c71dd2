"""VP9 inter reconstruction of whole frames on the GPU (ffhip_vp9_inter_frames_dev), byte for byte against the sequential model of
vp9_inter_frame_gen.py (the oracle's vp9 MC and itxfm_add on clamped windows), stride padding included.  Every call is followed by
ffhip_stream_synchronize(None) == 0."""
import numpy as np
import pytest

import vp9_inter_frame_gen as G
from ffmpeg_amd import _lib, vp9

pytestmark = pytest.mark.gpu

SENT = 0x5A


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _dt(bd):
    return np.uint8 if bd == 8 else np.uint16


def _plane_bytes(a, bd, stride, rows=None, fill=SENT):
    """a plane (int64 samples) as a (rows, stride) byte image; the padding right of it (and rows below it) filled with `fill`"""
    h, w = a.shape
    ps = 1 if bd == 8 else 2
    host = np.full((h if rows is None else rows, stride), fill, np.uint8)
    host[:h, :w * ps] = a.astype(_dt(bd)).view(np.uint8).reshape(h, w * ps)
    return host


def _stride(w, bd, extra):
    ps = 1 if bd == 8 else 2
    return (w * ps + 63) // 64 * 64 + extra


def upload_refs(torch, fr, extra=0):
    """the references on the device, each plane in a buffer of the decoded area whose samples past the real size are garbage (a read
    there would show): per reference, per plane (tensor, stride)"""
    out = []
    for ref in fr.refs:
        planes = []
        for p in range(3):
            st = _stride(fr.dw[p], fr.bd, extra + 8 * p)
            host = _plane_bytes(ref[p], fr.bd, st, rows=fr.dh[p] + 2, fill=0)
            host[:, ref[p].shape[1] * (1 if fr.bd == 8 else 2):] = fr.rng.integers(0, 256, host[:, ref[p].shape[1] * (1 if fr.bd == 8 else 2):].shape)
            host[ref[p].shape[0]:] = fr.rng.integers(0, 256, host[ref[p].shape[0]:].shape)
            if fr.bd > 8:
                host.view(np.uint16)[...] &= fr.maxv
            planes.append((torch.from_numpy(host).cuda(), st))
        out.append(planes)
    return out


def upload(torch, fr, extra=0, preds=None, tus=None, refs=None, planes=None):
    """(the face's tuple for this frame, the destination (host image, device tensor) per plane, tensors to keep alive)"""
    preds = fr.preds if preds is None else preds
    tus = fr.tus if tus is None else tus
    src = fr.planes if planes is None else planes
    keep, dst, pl = [], [], []
    for p in range(3):
        h, w = src[p].shape
        st = _stride(w, fr.bd, extra)
        host = _plane_bytes(src[p], fr.bd, st)
        d = torch.from_numpy(host.copy()).cuda()
        arr, starts = fr.pack(tus[p], vp9.INTER_TU_DTYPE, G.TU_FIELDS)
        d_tus = torch.from_numpy(arr.view(np.uint8).copy() if len(arr) else np.zeros(16, np.uint8)).cuda()
        d_st = torch.from_numpy(starts).cuda()
        d_co = torch.from_numpy(fr.coeff_array(p)).cuda()
        keep += [d, d_tus, d_st, d_co]
        pl.append((d, st, d_tus, d_st, d_co))
        dst.append((host, d))
    arr, starts = fr.pack(preds, vp9.INTER_PRED_DTYPE, G.PRED_FIELDS)
    d_preds = torch.from_numpy(arr.view(np.uint8).copy() if len(arr) else np.zeros(20, np.uint8)).cuda()
    d_pst = torch.from_numpy(starts).cuda()
    refs = upload_refs(torch, fr) if refs is None else refs
    keep += [d_preds, d_pst, refs]
    return (pl, d_preds, d_pst, refs), dst, keep


def compare(fr, dst, want):
    ps = 1 if fr.bd == 8 else 2
    for p, (host, d) in enumerate(dst):
        h, w = want[p].shape
        exp = host.copy()
        exp[:, :w * ps] = want[p].astype(_dt(fr.bd)).view(np.uint8).reshape(h, w * ps)
        got = d.cpu().numpy()
        bad = np.argwhere(got != exp)
        assert not len(bad), "plane %d: %d mismatches, first (row, byte) %s: got %s want %s" % (
            p, len(bad), bad[:3].tolist(), got[tuple(bad[0])], exp[tuple(bad[0])])


def run(frames, extra=0, preds=None, tus=None):
    """reconstruct the frames (one geometry) in one call, with the records `preds` / `tus` when given (the frame's own plus malformed
    ones), and compare every plane, padding included, with the model of the frame's own records"""
    torch = _torch()
    F0 = frames[0]
    args, dsts, keep = [], [], []
    for i, fr in enumerate(frames):
        a, dst, k = upload(torch, fr, extra, preds[i] if preds else None, tus[i] if tus else None)
        args.append(a)
        dsts.append(dst)
        keep.append(k)
    vp9.inter_frames(args, F0.W, F0.H, ss=(F0.ss_h, F0.ss_v), bit_depth=F0.bd)
    assert _lib.lib().ffhip_stream_synchronize(None) == 0, _lib.lib().ffhip_last_error()
    torch.cuda.synchronize()
    for fr, dst in zip(frames, dsts):
        compare(fr, dst, G.model(fr))   # the frame's own (well-formed) records


SS = [(1, 1), (1, 0), (0, 1), (0, 0)]


@pytest.mark.parametrize("bd", (8, 10, 12))
@pytest.mark.parametrize("ss", SS, ids=["420", "422", "440", "444"])
def test_depth_subsampling(bd, ss):
    rng = np.random.default_rng(3000 + bd * 10 + SS.index(ss))
    run([G.InterFrame(rng, 203, 141, bd, *ss)])                       # not multiples of 8 or 64
    run([G.InterFrame(rng, 128, 64, bd, *ss, lossless=True)])         # the WHT


def test_1080p():
    run([G.InterFrame(np.random.default_rng(5), 1920, 1080, 8, 1, 1, nrefs=3, min_log2=3, p_intra=0.05)])


def test_sixteen_frames():
    rng = np.random.default_rng(6)
    run([G.InterFrame(rng, 96, 72, 10, 1, 1, nrefs=1 + i % 3) for i in range(16)])


def test_seventeen_frames_are_split():
    rng = np.random.default_rng(7)
    run([G.InterFrame(rng, 72, 40, 8, 1, 0) for i in range(17)])


def test_stride_padding_and_intra_holes_survive():
    rng = np.random.default_rng(8)
    run([G.InterFrame(rng, 136, 90, 8, 1, 1, p_intra=0.4)], extra=72)
    run([G.InterFrame(rng, 130, 88, 12, 0, 0, p_intra=0.4)], extra=40)


def test_far_out_mvs():
    rng = np.random.default_rng(9)
    run([G.InterFrame(rng, 128, 96, 8, 1, 1, p_far=0.4, p_edge=0.3)])
    run([G.InterFrame(rng, 100, 70, 10, 0, 0, p_far=0.4, p_edge=0.3)])


def test_malformed_records_write_nothing():
    """each class of malformed record, inserted beside the real ones: the planes are those of the real records alone"""
    rng = np.random.default_rng(10)
    fr = G.InterFrame(rng, 200, 128, 8, 1, 1, nrefs=2, p_intra=0.4)
    sb_of = lambda x, y: (y >> 6) * fr.sb_w + (x >> 6)
    holes = [(bs, row, col) for bs, row, col, k in fr.blocks if k == "intra" and bs <= 9]
    assert len(holes) >= 9
    bad = []
    for j, (bs, row, col) in enumerate(holes[:18]):
        x, y = col * 8, row * 8
        b = dict(x=x, y=y, w=8, h=8, filter=1, flags=0, ref=[0, 0], mv=[[5, -3], [-7, 2]], sb=sb_of(x, y))
        kind = j % 9
        if kind == 0:
            b["w"] = 6                                      # not a power of two
        elif kind == 1:
            b["h"] = 128                                    # too large
        elif kind == 2:
            b["w"] = 2
        elif kind == 3:
            b["sb"] = (b["sb"] + 1) % (fr.sb_w * fr.sb_h)   # listed under another superblock
        elif kind == 4:
            b["filter"] = 4
        elif kind == 5:
            b["ref"] = [fr.nrefs, 0]                        # no such reference
        elif kind == 6:
            b["flags"], b["ref"] = 1, [0, 3]                # compound, its second reference missing
        elif kind == 7:
            b["flags"] = 4                                  # an unknown flag
        else:
            b["x"], b["w"] = (x & ~63) + 48, 32             # across its superblock's right edge
        bad.append(b)
    tus = []
    for p in range(3):
        tl = list(fr.tus[p])
        Cw = 64 >> fr.hs[p]
        for j, t in enumerate(fr.tus[p][:9]):
            b = dict(t)
            kind = j % 3
            if kind == 0:
                b["tx"] = 5
            elif kind == 1:
                b["sb"] = (t["sb"] + 1) % (fr.sb_w * fr.sb_h)  # outside its superblock
            else:
                b["x"] = t["x"] + 2                           # not aligned to its size
            tl.append(b)
        tus.append(tl)
    run([fr], preds=[fr.preds + bad], tus=[tus])


def test_chained_with_the_loop_filter_on_one_stream():
    """inter frames, then ffhip_vp9_loopfilter_frames_dev on the same planes and stream: equal to the loop filter run on the model's
    planes"""
    import vp9_lf_gen as LG
    torch = _torch()
    rng = np.random.default_rng(11)
    frames = [G.InterFrame(rng, 200, 136, 8, 1, 1, p_intra=0.0) for _ in range(2)]
    fr0 = frames[0]
    lim, mblim = LG.filter_lut(2)
    cols, rows, sbc, sbr = fr0.cols, fr0.rows, fr0.sb_w, fr0.sb_h
    # the loop filter reads whole superblocks of its planes: planes of the decoded area, rounded up to superblocks
    args, dsts, keep, lf, want_lf = [], [], [], [], []
    for fr in frames:
        big = [np.zeros(((sbr * 64) >> fr.vs[p], (sbc * 64) >> fr.hs[p]), np.int64) for p in range(3)]
        for p in range(3):
            big[p][:fr.dh[p], :fr.dw[p]] = fr.planes[p]
        a, dst, k = upload(torch, fr, planes=big)
        filt = np.zeros(sbr * sbc, LG.FILTER_DT)
        for r in range(sbr):
            for c in range(sbc):
                filt[r * sbc + c] = LG.structured(rng, r, c, cols, rows)
        tabs = torch.from_numpy(vp9.lf_sb_tables(filt.view(np.uint8).reshape(sbr * sbc, 192), sbc, sbr, lim, mblim).view(np.int32)).cuda()
        args.append(a)
        dsts.append(dst)
        keep.append((k, tabs))
        lf.append((dst[0][1], dst[1][1], dst[2][1], tabs))
        # the model's planes, filtered by a launch of their own
        m = G.model(fr, planes=big)
        other = [torch.from_numpy(_plane_bytes(m[p], fr.bd, a[0][p][1])).cuda() for p in range(3)]
        want_lf.append((other[0], other[1], other[2], tabs))
    sy, suv = args[0][0][0][1], args[0][0][1][1]
    vp9.inter_frames(args, fr0.W, fr0.H, ss=(1, 1), bit_depth=8)
    vp9.loopfilter_frames(lf, sy, suv, cols, rows, bit_depth=8)
    vp9.loopfilter_frames(want_lf, sy, suv, cols, rows, bit_depth=8)
    assert _lib.lib().ffhip_stream_synchronize(None) == 0, _lib.lib().ffhip_last_error()
    torch.cuda.synchronize()
    for i in range(len(frames)):
        for p in range(3):
            assert torch.equal(lf[i][p], want_lf[i][p]), (i, p)


@pytest.mark.parametrize("bd,ss", [(8, (1, 1)), (10, (1, 1)), (8, (0, 0)), (12, (1, 0))])
def test_same_planes_as_the_batch_faces(bd, ss):
    """for MVs that keep every window inside a 96-sample edge-replicated border and a frame of whole superblocks, the new face gives
    the planes of mc_batch (put, then avg, per reference) on padded references + itxfm_add_batch per transform size"""
    torch = _torch()
    rng = np.random.default_rng(5000 + bd * 10 + ss[0] * 2 + ss[1])
    fr = G.InterFrame(rng, 256, 192, bd, *ss, nrefs=3, p_far=0.0, p_edge=0.0)
    a, dst, keep = upload(torch, fr)
    vp9.inter_frames([a], fr.W, fr.H, ss=ss, bit_depth=bd)
    import vp9_inter_batch_path as BP
    other = [torch.from_numpy(host.copy()).cuda() for host, _ in dst]
    path = BP.BatchPath(torch, fr, [pl[1] for pl in a[0]])
    path.run(other)
    assert _lib.lib().ffhip_stream_synchronize(None) == 0, _lib.lib().ffhip_last_error()
    torch.cuda.synchronize()
    for p in range(3):
        assert torch.equal(dst[p][1], other[p]), "plane %d differs from the batch faces" % p
    compare(fr, dst, G.model(fr))
