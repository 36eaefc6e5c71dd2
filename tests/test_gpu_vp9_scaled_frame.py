"""VP9 inter reconstruction from references of another size on the GPU (ffhip_vp9_inter_frames_scaled_dev), byte for byte against the
model of vp9_scaled_frame_gen.py, stride padding and untouched samples included.  References sit in buffers larger than their real
size whose extra samples are garbage, so a read past a reference's edge shows.  Every call is followed by
ffhip_stream_synchronize(None) == 0."""
import numpy as np
import pytest

import vp9_inter_frame_gen as G
import vp9_scaled_frame_gen as S
from ffmpeg_amd import _lib, vp9

pytestmark = pytest.mark.gpu

SENT = 0x5A
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


def _image(a, bd, stride, rows, fill):
    h, w = a.shape
    ps = 1 if bd == 8 else 2
    host = np.full((rows, stride), fill, np.uint8)
    host[:h, :w * ps] = a.astype(_dt(bd)).view(np.uint8).reshape(h, w * ps)
    return host


def upload_refs(torch, fr):
    """each reference plane in a buffer 24 samples wider and 6 rows taller than its real size, the extra samples garbage"""
    out = []
    for ref in fr.refs:
        planes = []
        for p in range(3):
            h, w = ref[p].shape
            ps = 1 if fr.bd == 8 else 2
            st = _stride(w + 24, fr.bd, 8 * p)
            host = _image(ref[p], fr.bd, st, h + 6, 0)
            host[:, w * ps:] = fr.rng.integers(0, 256, host[:, w * ps:].shape)
            host[h:] = fr.rng.integers(0, 256, host[h:].shape)
            if fr.bd > 8:
                host.view(np.uint16)[...] &= fr.maxv
            planes.append((torch.from_numpy(host).cuda(), st))
        out.append(planes)
    return out


def upload(torch, fr, preds=None, extra=0):
    preds = fr.preds if preds is None else preds
    keep, dst, pl = [], [], []
    for p in range(3):
        h, w = fr.planes[p].shape
        st = _stride(w, fr.bd, extra)
        host = _image(fr.planes[p], fr.bd, st, h, SENT)
        d = torch.from_numpy(host.copy()).cuda()
        arr, starts = fr.pack(fr.tus[p], vp9.INTER_TU_DTYPE, G.TU_FIELDS)
        d_tus = torch.from_numpy(arr.view(np.uint8).copy() if len(arr) else np.zeros(16, np.uint8)).cuda()
        d_st = torch.from_numpy(starts).cuda()
        d_co = torch.from_numpy(fr.coeff_array(p)).cuda()
        keep += [d, d_tus, d_st, d_co]
        pl.append((d, st, d_tus, d_st, d_co))
        dst.append((host, d))
    arr, starts = fr.pack(preds, vp9.INTER_PRED_DTYPE, S.PRED_FIELDS)
    d_preds = torch.from_numpy(arr.view(np.uint8).copy() if len(arr) else np.zeros(20, np.uint8)).cuda()
    d_pst = torch.from_numpy(starts).cuda()
    refs = upload_refs(torch, fr)
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


def _sync():
    assert _lib.lib().ffhip_stream_synchronize(None) == 0, _lib.lib().ffhip_last_error()
    _torch().cuda.synchronize()


def run(frames, preds=None, extra=0, face="scaled"):
    """reconstruct the frames in one call (records `preds` when given: the frame's own plus malformed ones) and compare every plane
    with the model of the frame's own records; returns the device planes"""
    torch = _torch()
    F0 = frames[0]
    args, dsts, keep = [], [], []
    for i, fr in enumerate(frames):
        a, dst, k = upload(torch, fr, preds[i] if preds else None, extra)
        args.append(a)
        dsts.append(dst)
        keep.append(k)
    if face == "scaled":
        vp9.inter_frames_scaled(args, [fr.ref_sizes for fr in frames], F0.W, F0.H, ss=(F0.ss_h, F0.ss_v), bit_depth=F0.bd)
    else:
        vp9.inter_frames(args, F0.W, F0.H, ss=(F0.ss_h, F0.ss_v), bit_depth=F0.bd)
    _sync()
    for fr, dst in zip(frames, dsts):
        compare(fr, dst, S.model(fr))
    return [[d for _, d in dst] for dst in dsts]


@pytest.mark.parametrize("bd", (8, 10, 12))
@pytest.mark.parametrize("ss", SS, ids=["420", "422", "440", "444"])
def test_depth_subsampling_ratios(bd, ss):
    for case, ((W, H), sizes) in enumerate(S.RATIOS):
        rng = np.random.default_rng(6000 + 100 * bd + 10 * SS.index(ss) + case)
        run([S.ScaledFrame(rng, W, H, bd, *ss, sizes, p_comp=0.5, p_far=0.1, p_edge=0.2)])


def test_large_blocks_at_2x_down_and_far_mvs():
    rng = np.random.default_rng(61)
    run([S.ScaledFrame(rng, 128, 128, 8, 1, 1, [(256, 256)], p_intra=0.0, min_log2=6)])
    run([S.ScaledFrame(rng, 128, 128, 10, 0, 0, [(256, 255), (128, 128)], p_intra=0.0, min_log2=5, p_comp=0.7)])
    run([S.ScaledFrame(rng, 96, 80, 12, 1, 1, [(180, 100), (7, 5)], p_far=0.5, p_edge=0.3)])


def test_1080p_from_720p():
    rng = np.random.default_rng(62)
    run([S.ScaledFrame(rng, 1920, 1088, 8, 1, 1, [(1280, 720), (1920, 1088)], min_log2=3, p_intra=0.05, mv_range=200)])


def test_sixteen_frames():
    rng = np.random.default_rng(63)
    run([S.ScaledFrame(rng, 96, 72, 10, 1, 1, [(144, 108), (48, 36), (96, 72)][:1 + i % 3]) for i in range(16)])


def test_seventeen_frames_are_split():
    """the last frame alone in the second launch; its references have the frame's size, so that launch runs the unscaled kernel"""
    rng = np.random.default_rng(64)
    frames = [S.ScaledFrame(rng, 72, 40, 8, 1, 0, [(100, 80)]) for i in range(16)]
    run(frames + [S.ScaledFrame(rng, 72, 40, 8, 1, 0, [(72, 40)])])


def test_malformed_scaled_records_write_nothing():
    """beside the frame's own records: boxes that do not hold the call, log2 sizes outside 2..6, an unknown flag bit beside
    INTER_SCALED; each lies over an intra hole, which must survive"""
    rng = np.random.default_rng(65)
    fr = S.ScaledFrame(rng, 192, 128, 8, 1, 1, [(288, 192)], p_intra=0.5)
    holes = [(bs, row, col) for bs, row, col, kind in fr.blocks if kind == "intra" and bs <= 9]   # 8x8 and up: an 8x8 call fits
    assert len(holes) >= 8
    bad = []
    for k, (bs, row, col) in enumerate(holes[:8]):
        rec = S.block_preds_scaled(9, row, col, [[[3, 5], [0, 0]]] * 4, 0, [0, 0], 1, 1, 1)[0]   # the 8x8 luma call
        rec["box"] = [[4, 3 | 3 << 4], [0, 1 | 3 << 4], [0, 7 | 3 << 4], [0x40, 3 | 3 << 4], [0, 3 | 2 << 4], [0x11, 3 | 3 << 4],
                      [0, 0], [0, 3 | 3 << 4]][k]
        if k == 7:
            rec["flags"] |= 8                                        # an unknown flag bit
        rec["sb"] = (row >> 3) * fr.sb_w + (col >> 3)
        bad.append(rec)
    run([fr], preds=[fr.preds + bad])


def test_unscaled_frames_give_the_same_bytes_through_both_faces():
    rng = np.random.default_rng(66)
    mk = lambda: S.ScaledFrame(np.random.default_rng(67), 133, 77, 10, 1, 0, [(133, 77), (133, 77)], p_far=0.2)
    a = run([mk()], face="scaled")
    b = run([mk()], face="plain")
    for p in range(3):
        assert bool((a[0][p] == b[0][p]).all()), p
    # and an unscaled frame beside a scaled one: the scaled kernel's unscaled path
    run([S.ScaledFrame(rng, 133, 77, 8, 0, 1, [(133, 77)]), S.ScaledFrame(rng, 133, 77, 8, 0, 1, [(200, 150)])])


def test_the_batch_faces_give_the_same_planes():
    """a third route: per call, ffhip_vp9_scaled_mc_batch_dev[_hbd] / ffhip_vp9_mc_batch_dev[_hbd] on edge-padded references, then
    ffhip_vp9_itxfm_add_batch_dev[_hbd]"""
    import vp9_scaled_batch_path as B
    torch = _torch()
    for bd, ss in ((8, (1, 1)), (10, (1, 0)), (12, (0, 0))):
        rng = np.random.default_rng(68 + bd)
        fr = S.ScaledFrame(rng, 128, 64, bd, *ss, [(192, 96), (128, 64)], p_far=0.0, p_edge=0.2, p_comp=0.5)
        _, dst, keep = upload(torch, fr)
        st = [_stride(fr.planes[p].shape[1], bd, 0) for p in range(3)]
        B.BatchPath(torch, fr, st).run([d for _, d in dst])
        _sync()
        compare(fr, dst, S.model(fr))


def test_chain_with_intra_and_loop_filter():
    """inter (scaled) -> ffhip_vp9_intra_frames_dev -> ffhip_vp9_loopfilter_frames_dev on one stream equals the loop filter run on the
    model chain's planes"""
    import vp9_intra_frame_gen as IG
    import vp9_lf_gen as LG
    torch = _torch()
    rng = np.random.default_rng(69)
    lim, mblim = LG.filter_lut(2)
    # IntraFrame(inter=True) builds its inter frame through vp9_inter_frame_gen: have it build a scaled one
    saved = IG.vg.InterFrame, IG.vg.model
    IG.vg.InterFrame = lambda rng, W, H, bd, ss_h, ss_v, **kw: S.ScaledFrame(rng, W, H, bd, ss_h, ss_v, [(300, 204), (200, 136)], **kw)
    IG.vg.model = S.model
    try:
        fr = IG.IntraFrame(rng, 200, 136, 8, 1, 1, inter=True, p_intra=0.3)
    finally:
        IG.vg.InterFrame, IG.vg.model = saved
    sfr = fr.inter
    assert any(r["flags"] & S.SCALED for r in sfr.preds)
    cols, rows, sbc, sbr = fr.cols, fr.rows, fr.sb_w, fr.sb_h
    big = [np.zeros(((sbr * 64) >> fr.vs[p], (sbc * 64) >> fr.hs[p]), np.int64) for p in range(3)]
    for p in range(3):
        big[p][:fr.dh[p], :fr.dw[p]] = sfr.planes[p]
    sfr.planes = big                                               # the loop filter reads whole superblocks of its planes
    a_inter, dst, keep = upload(torch, sfr)
    planes = [dst[p][1] for p in range(3)]
    strides = [a_inter[0][p][1] for p in range(3)]
    intra_pl, keep2 = [], []
    for p in range(3):
        arr, starts = fr.pack(p)
        d_recs = torch.from_numpy(arr.view(np.uint8).copy()).cuda()
        d_st = torch.from_numpy(starts).cuda()
        d_co = torch.from_numpy(fr.coeff_array(p)).cuda()
        keep2 += [d_recs, d_st, d_co]
        intra_pl.append((planes[p], strides[p], d_recs, d_st, d_co))
    filt = np.zeros(sbr * sbc, LG.FILTER_DT)
    for r in range(sbr):
        for c in range(sbc):
            filt[r * sbc + c] = LG.structured(rng, r, c, cols, rows)
    tabs = torch.from_numpy(vp9.lf_sb_tables(filt.view(np.uint8).reshape(sbr * sbc, 192), sbc, sbr, lim, mblim).view(np.int32)).cuda()
    m = IG.model(fr, planes=S.model(sfr))
    other = [torch.from_numpy(_image(m[p], 8, strides[p], m[p].shape[0], SENT)).cuda() for p in range(3)]
    vp9.inter_frames_scaled([a_inter], [sfr.ref_sizes], fr.W, fr.H, ss=(1, 1), bit_depth=8)
    vp9.intra_frames([(intra_pl, 0)], fr.W, fr.H, ss=(1, 1), bit_depth=8)
    vp9.loopfilter_frames([(planes[0], planes[1], planes[2], tabs)], strides[0], strides[1], cols, rows, bit_depth=8)
    vp9.loopfilter_frames([(other[0], other[1], other[2], tabs)], strides[0], strides[1], cols, rows, bit_depth=8)
    _sync()
    for p in range(3):
        assert torch.equal(planes[p], other[p]), p
