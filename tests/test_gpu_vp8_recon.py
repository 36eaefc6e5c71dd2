"""ffhip_vp8_recon_frames_dev on the GPU, byte for byte against the plane-rule model (vp8_recon_model.recon_frame): keyframes and inter
frames over edge sizes, MVs far outside the frame, the bilinear and full-pel-chroma variants, 1 / 3 / 16 / 17 frames per call, stride
padding, references and coefficients untouched, malformed records, and the chain into ffhip_vp8_loopfilter_frames_dev with the
filtered frame as the next frame's reference.

A 1920x1088 key frame and inter frame go against the model too, and small frames against the independent route through the per-call
batch faces that existed before (vp8_recon_batch_path)."""
import numpy as np
import pytest

import vp8_recon_batch_path as BP
import vp8_recon_gen as G
import vp8_recon_model as RM
import vp8dsp_model as M
from ffmpeg_amd import _lib, vp8

pytestmark = pytest.mark.gpu
SENT = 0xA5


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _sync():
    assert _lib.lib().ffhip_stream_synchronize(None) == 0


def _padded(planes, sy, suv):
    """the planes inside strides sy / suv, the padding holding sentinel bytes"""
    out = []
    for p, a in enumerate(planes):
        b = np.full((a.shape[0], suv if p else sy), SENT, np.uint8)
        b[:, :a.shape[1]] = a
        out.append(b)
    return out


def _up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _upload(torch, frames, mb_w, mb_h, pad=(16, 12)):
    """frames: [(mbs, coeffs, refs (host planes or None), initial planes)]; (the face's pictures, per frame the device (planes,
    references, coefficients), the strides)"""
    sy, suv = 16 * mb_w + pad[0], 8 * mb_w + pad[1]
    pics, keep = [], []
    for mbs, co, refs, init in frames:
        d = [_up(torch, a) for a in _padded(init, sy, suv)]
        dr = [None if r is None else [_up(torch, a) for a in _padded(r, sy, suv)] for r in refs]
        dco = torch.from_numpy(co.copy()).cuda() if len(co) else None
        pics.append(dict(y=d[0], u=d[1], v=d[2], refs=dr, mbs=_up(torch, mbs), coeffs=dco))
        keep.append((d, dr, dco))
    return pics, keep, sy, suv


def _download(frames, keep, sy, suv):
    """the device's frames as host arrays, after checking that the stride padding, the references and the coefficients are as they
    were"""
    got = []
    for (mbs, co, refs, init), (d, dr, dco) in zip(frames, keep):
        out = []
        for p in range(3):
            g = d[p].cpu().numpy().reshape(init[p].shape[0], suv if p else sy)
            assert (g[:, init[p].shape[1]:] == SENT).all(), "stride padding of plane %d written" % p
            out.append(g[:, :init[p].shape[1]].copy())
        for r, hr in zip(dr, refs):
            if r is not None:
                for p in range(3):
                    assert np.array_equal(r[p].cpu().numpy(), _padded(hr, sy, suv)[p].reshape(-1)), "a reference was written"
        if dco is not None:
            assert np.array_equal(dco.cpu().numpy(), co), "the coefficients were written"
        got.append(out)
    return got


def _run(frames, mb_w, mb_h, bilinear=0, fullpel=0, pad=(16, 12), stream=None):
    """reconstruct the frames in one call; returns the device's frames as host arrays (see _download)"""
    torch = _torch()
    pics, keep, sy, suv = _upload(torch, frames, mb_w, mb_h, pad)
    vp8.recon_frames(pics, mb_w, mb_h, sy, suv, bilinear, fullpel, stream=stream)
    assert _lib.lib().ffhip_stream_synchronize(stream) == 0
    return _download(frames, keep, sy, suv)


def _check(got, want, what=""):
    for p in range(3):
        if not np.array_equal(got[p], want[p]):
            bad = np.argwhere(got[p] != want[p])
            raise AssertionError("%s plane %d: %d samples differ, first at %s (got %d, want %d)" % (
                what, p, len(bad), bad[0], got[p][tuple(bad[0])], want[p][tuple(bad[0])]))


def _frame(seed, mb_w, mb_h, key, **kw):
    mbs, co = G.frame(seed, mb_w, mb_h, keyframe=key, **kw)
    refs = [G.planes(100 * seed + r, mb_w, mb_h) for r in range(3)]
    return mbs, co, refs, G.planes(7 + seed, mb_w, mb_h)


def _want(fr, mb_w, mb_h, bilinear=0, fullpel=0):
    mbs, co, refs, init = fr
    return RM.recon_frame([a.copy() for a in init], mbs, co, refs, mb_w, mb_h, bilinear, fullpel)


SIZES = [(1, 1), (1, 9), (11, 1), (2, 2), (20, 12)]


@pytest.mark.parametrize("mb_w,mb_h", SIZES)
def test_keyframes(mb_w, mb_h):
    fr = _frame(40 + mb_w, mb_w, mb_h, True)
    _check(_run([fr], mb_w, mb_h)[0], _want(fr, mb_w, mb_h))


@pytest.mark.parametrize("mb_w,mb_h", SIZES)
def test_inter_frames(mb_w, mb_h):
    fr = _frame(50 + mb_w, mb_w, mb_h, False, intra=0.15)
    _check(_run([fr], mb_w, mb_h)[0], _want(fr, mb_w, mb_h))


@pytest.mark.parametrize("key", [True, False])
def test_1920x1088(key):
    fr = _frame(65 + key, 120, 68, key, intra=0.1, far=0.02)
    _check(_run([fr], 120, 68)[0], _want(fr, 120, 68))


def test_mvs_far_outside_the_frame():
    fr = _frame(61, 7, 5, False, intra=0.1, far=0.8)
    mv = fr[0]["mv"].astype(np.int64)
    assert (mv[..., 0] < -4 * 16 * 7).any() and (mv[..., 0] > 4 * 16 * 7).any() and (mv[..., 1] < -4 * 16 * 5).any() and (mv[..., 1] > 4 * 16 * 5).any()
    _check(_run([fr], 7, 5)[0], _want(fr, 7, 5))


@pytest.mark.parametrize("bilinear,fullpel", [(1, 0), (1, 1), (0, 1)])
def test_profiles(bilinear, fullpel):
    fr = _frame(70 + 2 * bilinear + fullpel, 6, 5, False, intra=0.15, far=0.1)
    _check(_run([fr], 6, 5, bilinear, fullpel)[0], _want(fr, 6, 5, bilinear, fullpel))


@pytest.mark.parametrize("npics", [1, 3, 16, 17])
def test_frames_per_call(npics):
    mb_w, mb_h = 5, 4
    frames = [_frame(80 + i, mb_w, mb_h, i % 3 == 0, intra=0.2) for i in range(npics)]
    got = _run(frames, mb_w, mb_h)
    for i, fr in enumerate(frames):
        _check(got[i], _want(fr, mb_w, mb_h), "frame %d" % i)


def test_missing_references_and_no_coefficients():
    """a NULL reference nobody names, and a frame with nothing coded and no coefficient array"""
    mb_w, mb_h = 4, 3
    mbs, co, refs, init = _frame(90, mb_w, mb_h, False, intra=0.2, refs=(2,), skip=1.0)
    refs = [None, refs[1], None]
    fr = (mbs, np.zeros(0, np.int16), refs, init)
    _check(_run([fr], mb_w, mb_h)[0], _want(fr, mb_w, mb_h))


def test_malformed_records_write_nothing():
    mb_w, mb_h = 6, 5
    mbs, co, refs, init = _frame(95, mb_w, mb_h, False, intra=0.4)
    refs = [refs[0], refs[1], None]
    rng = np.random.default_rng(3)
    victims = rng.choice(mb_w * mb_h, 14, replace=False)
    for k, m in enumerate(victims):
        mb = mbs[m]
        kind = k % 7
        if kind == 0:
            mb["ref_frame"] = 4 + k
        elif kind == 1:
            mb["ref_frame"] = 3                     # names the NULL reference
        elif kind == 2:
            if mb["ref_frame"]:
                mb["partitioning"] = 5
            else:
                mb["mode"] = 5
        elif kind == 3:
            G.set_code(mb, int(rng.integers(0, 24)), 3)
        elif kind == 4:
            mb["coeff_offset"] += 8
            mb["y2"] = 1
        elif kind == 5:
            mb["coeff_offset"] = len(co) - 384      # a multiple of 16 that runs 16 coefficients past the end
            mb["y2"] = 1
        else:
            mb["coeff_offset"] = -400               # aligned, before the array
            mb["y2"] = 1
    for m, mb in enumerate(mbs):                    # nobody else names reference 3
        if m not in victims and mb["ref_frame"] == 3:
            mb["ref_frame"] = 1
    assert len(co) % 16 == 0 and sum(not RM.well_formed(mb, refs, len(co)) for mb in mbs) >= 12
    fr = (mbs, co, refs, init)
    _check(_run([fr], mb_w, mb_h)[0], _want(fr, mb_w, mb_h))


@pytest.mark.parametrize("seed,key,bilinear,fullpel", [(120, True, 0, 0), (121, False, 0, 0), (122, False, 1, 1), (123, False, 0, 1)])
def test_batch_face_route_equals_the_frame_face(seed, key, bilinear, fullpel):
    """the launch chain through ffhip_vp8_mc_batch_dev / ffhip_h264_pred_batch_dev / the WHT and IDCT batch faces == the frame face"""
    mb_w, mb_h = 6, 5
    fr = _frame(seed, mb_w, mb_h, key, intra=0.3, far=0.15)
    mbs, co, refs, init = fr
    face = _run([fr], mb_w, mb_h, bilinear, fullpel)[0]
    route = BP.Frame(_torch(), mbs, co, refs, init, mb_w, mb_h, bilinear, fullpel)
    assert route.issue() > 100
    _sync()
    _check(route.result(), face, "batch route")


class Chain:
    """recon_frames then loopfilter_frames on one stream, twice: the second frame predicts from the first filtered one.
    upload / call(stream) / compare, inputs() / outputs() as tests/picture_faces.py has them."""
    name = "vp8_recon+loopfilter"
    mb_w, mb_h, sy, suv = 9, 7, 16 * 9 + 16, 8 * 9 + 8

    def upload(self, torch):
        mb_w, mb_h, sy, suv = self.mb_w, self.mb_h, self.sy, self.suv
        rng = np.random.default_rng(21)
        self.st = st = np.zeros((mb_h, mb_w), vp8.STRENGTH_DTYPE)
        st["filter_level"], st["inner_limit"], st["inner_filter"] = rng.integers(0, 64, st.shape), rng.integers(0, 10, st.shape), rng.integers(0, 2, st.shape)
        self.k_mbs, self.k_co = G.frame(31, mb_w, mb_h, keyframe=True)
        self.i_mbs, self.i_co = G.frame(32, mb_w, mb_h, intra=0.15, refs=(1,))
        self.d1 = [_up(torch, a) for a in _padded(G.planes(1, mb_w, mb_h), sy, suv)]
        self.d2 = [_up(torch, a) for a in _padded(G.planes(2, mb_w, mb_h), sy, suv)]
        self.dst = _up(torch, st)
        self.keep = [_up(torch, self.k_mbs), torch.from_numpy(self.k_co.copy()).cuda(), _up(torch, self.i_mbs), torch.from_numpy(self.i_co.copy()).cuda()]

    def call(self, stream):
        """the device: four calls on the stream, no wait"""
        mb_w, mb_h, sy, suv, d1, d2, keep = self.mb_w, self.mb_h, self.sy, self.suv, self.d1, self.d2, self.keep
        vp8.recon_frames([dict(y=d1[0], u=d1[1], v=d1[2], refs=None, mbs=keep[0], coeffs=keep[1])], mb_w, mb_h, sy, suv, stream=stream)
        vp8.loopfilter_frames([(d1[0], d1[1], d1[2], self.dst)], 0, 1, mb_w, mb_h, sy, suv, stream=stream)
        vp8.recon_frames([dict(y=d2[0], u=d2[1], v=d2[2], refs=[d1, None, None], mbs=keep[2], coeffs=keep[3])], mb_w, mb_h, sy, suv, stream=stream)
        vp8.loopfilter_frames([(d2[0], d2[1], d2[2], self.dst)], 0, 0, mb_w, mb_h, sy, suv, stream=stream)

    def inputs(self):
        return [self.dst] + self.keep

    def outputs(self):
        return self.d1 + self.d2

    def compare(self, view=lambda t: t):
        mb_w, mb_h, st = self.mb_w, self.mb_h, self.st
        # the model
        w1 = RM.recon_frame(G.planes(1, mb_w, mb_h), self.k_mbs, self.k_co, [None] * 3, mb_w, mb_h)
        M.loop_filter_frame(w1[0], w1[1], w1[2], st, 0, 1)
        w2 = RM.recon_frame(G.planes(2, mb_w, mb_h), self.i_mbs, self.i_co, [w1, None, None], mb_w, mb_h)
        M.loop_filter_frame(w2[0], w2[1], w2[2], st, 0, 0)
        for d, w, what in ((self.d1, w1, "key frame"), (self.d2, w2, "inter frame")):
            got = [view(d[p]).cpu().numpy().reshape(w[p].shape[0], -1)[:, :w[p].shape[1]] for p in range(3)]
            _check(got, w, what)


def test_chain_with_the_loop_filter():
    """Chain on the NULL stream (tests/test_gpu_picture_streams.py runs it on a created one)"""
    chain = Chain()
    chain.upload(_torch())
    chain.call(None)
    _sync()
    chain.compare()
