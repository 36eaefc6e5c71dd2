"""One adapter per whole-picture face (14 faces: five HEVC, five VP9, two VP8, two H.264) for the tests that run the faces on a caller's stream:
tests/test_picture_faces_cpu.py (the staged tests can fail), tests/test_gpu_picture_streams.py and tests/picture_stream_child.py.

An adapter splits a face's test into the steps a stream test has to interleave with its own work:
  build(seed)      one small picture with the face's generator, and the planes / maps the model says the face must give (host only)
  upload(torch)    the device tensors, through the upload helper of the face's own GPU test file
  call(stream)     the Python face on that stream
  inputs()         the device tensors the face only reads;  outputs(): the ones it writes (in-place planes count as outputs)
  compare(view)    the compare helper of the face's own GPU test file; view(t) is the tensor to look at in place of the output tensor
                   t (a snapshot taken on the stream), and is the identity by default
For the CPU tier: wants() the model's outputs, prefill() what the same samples hold before the call (a sentinel, or for in-place
faces the source plane), alt_wants(seed) the model's outputs when the input samples alone are drawn again with another seed.

Shapes are the smallest of the existing GPU tests at which each face still has its structure: 200 x 136 or 264 x 200 with 32 x 32
CTBs, tiles and slices (HEVC), 200 x 136 (VP9: 4 x 3 superblocks), 5 x 4 macroblocks with intra and inter macroblocks (VP8), 6 x 4 macroblocks,
30 % of them intra (H.264: the picture object alone and three of them as a batch; 4:2:2 and 4:4:4 flushes are not covered here)."""
import copy

import numpy as np

#: what every input and output tensor holds before a stream test stages the real bytes.  One byte repeated: record ranges read from
#: it are empty (start == end), offsets and indices are negative or out of range, so a face that reads it writes nothing it should.
POISON = 0xC3


def _alt_like(rng, a, maxv):
    return rng.integers(0, maxv + 1, a.shape).astype(a.dtype)


class Face:
    name = codec = None
    bd = 8

    def build(self, seed):
        raise NotImplementedError

    def fresh(self):
        """a copy that shares the host picture and the model's outputs and takes device tensors of its own"""
        return copy.copy(self)


# ================================================================================================================== HEVC
class HevcResidual(Face):
    name, codec, bd, cfi = "hevc_residual", "hevc", 10, 1

    def build(self, seed):
        import hevc_res_picture_gen as G
        import test_gpu_hevc_res_picture as T
        rng = np.random.default_rng(seed)
        self.pics = [G.build_planes(rng, [[70, 30, 12, 5], [25, 9, 4, 2], [25, 9, 4, 2]], self.cfi, big=bool(i & 1)) for i in range(2)]
        self.want = [G.model(planes, self.bd, self.cfi, fill=T.SENT) for planes in self.pics]
        return self

    def wants(self):
        return [w for want in self.want for w in want]

    def prefill(self):
        import test_gpu_hevc_res_picture as T
        return [np.full_like(w, T.SENT) for w in self.wants()]

    def alt_wants(self, seed):
        import hevc_res_picture_gen as G
        import test_gpu_hevc_res_picture as T
        rng = np.random.default_rng(seed)
        out = []
        for planes in self.pics:
            alt = [G.ResPlane(rng.integers(-200, 201, D.coeffs.shape).astype(D.coeffs.dtype), D.nres, D.tus, D.size_start) for D in planes]
            out += G.model(alt, self.bd, self.cfi, fill=T.SENT)
        return out

    def upload(self, torch):
        import test_gpu_hevc_res_picture as T
        self.dev = T._upload(torch, self.pics)

    def call(self, stream):
        from ffmpeg_amd import hevc
        hevc.residual_pictures(self.dev, chroma_format_idc=self.cfi, bit_depth=self.bd, stream=stream)

    def inputs(self):
        return [t for d in self.dev for pl in d for t in (pl[0], pl[2])]

    def outputs(self):
        return [pl[1] for d in self.dev for pl in d]

    def compare(self, view=lambda t: t):
        import test_gpu_hevc_res_picture as T
        dev = [[(pl[0], view(pl[1]), pl[2], pl[3]) for pl in d] for d in self.dev]
        T._compare(self.pics, dev, self.bd, self.cfi, self.want)


class HevcInter(Face):
    name, codec = "hevc_inter", "hevc"

    def build(self, seed):
        import hevc_inter_picture_gen as G
        self.pic = G.InterPicture(np.random.default_rng(seed), 200, 136, 5, self.bd, 1, nrefs=3, nslices=2)
        self.want = G.model(self.pic)
        return self

    def wants(self):
        return self.want

    def prefill(self):
        return self.pic.planes

    def alt_wants(self, seed):
        import hevc_inter_picture_gen as G
        rng = np.random.default_rng(seed)
        return G.model(self.pic, planes=[_alt_like(rng, pl, (1 << self.bd) - 1) for pl in self.pic.planes])

    def upload(self, torch):
        import test_gpu_hevc_inter_picture as T
        self.arg, self.dst, self.keep = T.upload(torch, self.pic)

    def call(self, stream):
        from ffmpeg_amd import hevc
        p = self.pic
        hevc.inter_pictures([self.arg], p.W, p.H, p.log2_ctb, chroma_format_idc=p.cfi, bit_depth=p.bd, stream=stream)

    def inputs(self):
        pl, pus, pst, sl, refs = self.arg
        return [t for q in pl for t in q[2:]] + [pus, pst, sl] + [t for ref in refs for t, _ in ref]

    def outputs(self):
        return [d for _, d in self.dst]

    def compare(self, view=lambda t: t):
        import test_gpu_hevc_inter_picture as T
        T.compare(self.pic, [(host, view(d)) for host, d in self.dst], self.want)


class HevcIntra(Face):
    name, codec, bd = "hevc_intra", "hevc", 10

    def build(self, seed):
        import hevc_intra_picture_gen as G
        self.pic = G.Picture(np.random.default_rng(seed), 200, 136, 5, self.bd, 1, p_intra=0.8, tiles=(2, 2), slices=3)
        self.want = G.model(self.pic)
        return self

    def wants(self):
        return self.want

    def prefill(self):
        return self.pic.planes

    def alt_wants(self, seed):
        import hevc_intra_picture_gen as G
        rng = np.random.default_rng(seed)
        alt = copy.copy(self.pic)
        alt.planes = [_alt_like(rng, pl, (1 << self.bd) - 1) for pl in self.pic.planes]
        return G.model(alt)

    def upload(self, torch):
        import test_gpu_hevc_intra_picture as T
        self.args, self.hosts, self.keep = T.upload(torch, [self.pic])

    def call(self, stream):
        from ffmpeg_amd import hevc
        p = self.pic
        hevc.intra_pictures(self.args, p.W, p.H, p.log2_ctb, chroma_format_idc=p.cfi, bit_depth=p.bd, stream=stream)

    def inputs(self):
        return [t for planes in self.args for q in planes for t in q[2:]]

    def outputs(self):
        return [h[3] for h in self.hosts]

    def compare(self, view=lambda t: t):
        import test_gpu_hevc_intra_picture as T
        T.compare([h[:3] + (view(h[3]),) + h[4:] for h in self.hosts], {id(self.pic): self.want})


class HevcLoopFilter(Face):
    name, codec = "hevc_loop_filter", "hevc"

    def build(self, seed):
        import hevc_lf_picture_gen as G
        self.pic = G.LfPicture(np.random.default_rng(seed), 264, 200, 5, self.bd, 1, tiles=(2, 2), nslices=3)
        self.want = G.model(self.pic)
        return self

    def wants(self):
        return self.want

    def prefill(self):
        import test_gpu_hevc_lf_picture as T
        return [np.full_like(w, T.SENT) for w in self.want]

    def alt_wants(self, seed):
        import hevc_lf_picture_gen as G
        rng = np.random.default_rng(seed)
        return G.model(self.pic, planes=[_alt_like(rng, pl, (1 << self.bd) - 1) for pl in self.pic.src])

    def upload(self, torch):
        import test_gpu_hevc_lf_picture as T
        self.arg, self.io = T.upload(torch, self.pic)

    def call(self, stream):
        from ffmpeg_amd import hevc
        p = self.pic
        hevc.loop_filter_pictures([self.arg], p.W, p.H, p.log2_ctb, p.lmc, chroma_format_idc=p.cfi, bit_depth=p.bd, stream=stream)

    def inputs(self):
        maps = self.arg[1]
        return [s for s, _, _, _ in self.io] + [maps[k] for k in ("bs_ver", "bs_hor", "qp_y", "bypass", "ctbs") if maps.get(k) is not None]

    def outputs(self):
        return [d for _, _, d, _ in self.io]

    def compare(self, view=lambda t: t):
        import test_gpu_hevc_lf_picture as T
        T.compare(self.pic, [(s, sh, view(d), dh) for s, sh, d, dh in self.io], self.want)


class HevcBoundaryStrengths(Face):
    name, codec, pad = "hevc_boundary_strengths", "hevc", 3

    def build(self, seed):
        import hevc_bs_picture_gen as G
        self.pic = G.BsPicture(np.random.default_rng(seed), 200, 136, 5, tiles=(2, 2), nslices=3)
        self.want = list(G.model_a_of(self.pic)[:2])
        return self

    def wants(self):
        return self.want

    def prefill(self):
        import test_gpu_hevc_bs_picture as T
        return [np.full_like(w, T.GUARD) for w in self.want]

    def alt_wants(self, seed):
        import hevc_bs_picture_gen as G
        rng = np.random.default_rng(seed)
        alt = copy.copy(self.pic)
        alt.mvf = self.pic.mvf.copy()
        alt.mvf["mv"] = rng.integers(-64, 65, alt.mvf["mv"].shape)
        alt.tu = rng.integers(0, 8, self.pic.tu.shape).astype(self.pic.tu.dtype)
        return list(G.model_a_of(alt)[:2])

    def upload(self, torch):
        import test_gpu_hevc_bs_picture as T
        self.d, self.m = T.upload(torch, self.pic, self.pad)

    def call(self, stream):
        from ffmpeg_amd import hevc
        p = self.pic
        hevc.boundary_strengths_pictures([self.d], p.W, p.H, p.log2_ctb, stream=stream)

    def inputs(self):
        return [self.d[k] for k in ("mvf", "tu", "ctb_slice", "slices", "ctb_tile") if self.d[k] is not None]

    def outputs(self):
        return [self.d["_ver"], self.d["_hor"]]

    def compare(self, view=lambda t: t):
        import test_gpu_hevc_bs_picture as T
        d = dict(self.d)
        d["_ver"], d["_hor"] = view(self.d["_ver"]), view(self.d["_hor"])
        T.compare([self.pic], [(d, self.m)])


# =================================================================================================================== VP9
class Vp9Inter(Face):
    name, codec = "vp9_inter", "vp9"

    def _gen(self):
        import vp9_inter_frame_gen as G
        return G

    def _test(self):
        import test_gpu_vp9_inter_frame as T
        return T

    def _frame(self, rng):
        return self._gen().InterFrame(rng, 200, 136, self.bd, 1, 1)

    def build(self, seed):
        self.fr = self._frame(np.random.default_rng(seed))
        self.want = self._gen().model(self.fr)
        return self

    def wants(self):
        return self.want

    def prefill(self):
        return self.fr.planes

    def alt_wants(self, seed):
        rng = np.random.default_rng(seed)
        return self._gen().model(self.fr, planes=[_alt_like(rng, pl, (1 << self.bd) - 1) for pl in self.fr.planes])

    def upload(self, torch):
        self.arg, self.dst, self.keep = self._test().upload(torch, self.fr)

    def call(self, stream):
        from ffmpeg_amd import vp9
        f = self.fr
        vp9.inter_frames([self.arg], f.W, f.H, ss=(f.ss_h, f.ss_v), bit_depth=f.bd, stream=stream)

    def inputs(self):
        pl, preds, pst, refs = self.arg
        return [t for q in pl for t in q[2:]] + [preds, pst] + [t for ref in refs for t, _ in ref]

    def outputs(self):
        return [d for _, d in self.dst]

    def compare(self, view=lambda t: t):
        self._test().compare(self.fr, [(host, view(d)) for host, d in self.dst], self.want)


class Vp9InterScaled(Vp9Inter):
    name = "vp9_inter_scaled"

    def _gen(self):
        import vp9_scaled_frame_gen as S
        return S

    def _test(self):
        import test_gpu_vp9_scaled_frame as T
        return T

    def _frame(self, rng):
        return self._gen().ScaledFrame(rng, 200, 136, self.bd, 1, 1, [(300, 204), (200, 136)], p_comp=0.5)

    def call(self, stream):
        from ffmpeg_amd import vp9
        f = self.fr
        vp9.inter_frames_scaled([self.arg], [f.ref_sizes], f.W, f.H, ss=(f.ss_h, f.ss_v), bit_depth=f.bd, stream=stream)


class Vp9Intra(Face):
    name, codec = "vp9_intra", "vp9"

    def build(self, seed):
        import vp9_intra_frame_gen as G
        # the intra blocks of an inter frame: a key frame's planes depend on nothing they held before
        self.fr = G.IntraFrame(np.random.default_rng(seed), 200, 136, self.bd, 1, 1, inter=True, p_intra=0.3)
        assert self.fr.recs[0]
        self.want = G.model(self.fr)
        return self

    def wants(self):
        return self.want

    def prefill(self):
        return self.fr.planes

    def alt_wants(self, seed):
        import vp9_intra_frame_gen as G
        rng = np.random.default_rng(seed)
        return G.model(self.fr, planes=[_alt_like(rng, pl, (1 << self.bd) - 1) for pl in self.fr.planes])

    def upload(self, torch):
        import test_gpu_vp9_intra_frame as T
        self.arg, self.dst, self.keep = T.upload(torch, self.fr)

    def call(self, stream):
        from ffmpeg_amd import vp9
        f = self.fr
        vp9.intra_frames([self.arg], f.W, f.H, ss=(f.ss_h, f.ss_v), bit_depth=f.bd, stream=stream)

    def inputs(self):
        return [t for q in self.arg[0] for t in q[2:]]

    def outputs(self):
        return [d for _, d in self.dst]

    def compare(self, view=lambda t: t):
        import test_gpu_vp9_intra_frame as T
        T.compare(self.fr, [(host, view(d)) for host, d in self.dst], self.want)


class Vp9LoopFilter(Face):
    """200 x 136 at 4:2:0: 25 x 17 blocks of 8 x 8 in 4 x 3 superblocks, the planes whole superblocks plus stride padding"""
    name, codec, ss = "vp9_loopfilter", "vp9", (1, 1)
    cols, rows, sbc, sbr = 25, 17, 4, 3

    def _planes(self, rng):
        import test_gpu_vp9_lf_frame as T
        cw, ch = 64 >> self.ss[0], 64 >> self.ss[1]
        return [T._plane(rng, 64 * self.sbr, 64 * self.sbc, 12, self.bd), T._plane(rng, ch * self.sbr, cw * self.sbc, 4, self.bd),
                T._plane(rng, ch * self.sbr, cw * self.sbc, 4, self.bd)]

    def _model(self, before):
        import test_gpu_vp9_lf_frame as T
        out = [p.copy() for p in before]
        T.oracle_frame(out, self.filt, self.sbc, self.sbr, self.bd, self.ss, self.lim, self.mblim)
        return out

    def build(self, seed):
        import vp9_lf_gen as G
        rng = np.random.default_rng(seed)
        self.lim, self.mblim = G.filter_lut(2)
        self.before = self._planes(rng)
        self.filt = np.zeros(self.sbr * self.sbc, G.FILTER_DT)
        for r in range(self.sbr):
            for c in range(self.sbc):
                self.filt[r * self.sbc + c] = G.structured(rng, r, c, self.cols, self.rows, *self.ss)
        self.want = self._model(self.before)
        return self

    def wants(self):
        return self.want

    def prefill(self):
        return self.before

    def alt_wants(self, seed):
        return self._model(self._planes(np.random.default_rng(seed)))

    def _tables(self):
        from ffmpeg_amd import vp9
        return [vp9.lf_sb_tables(self.filt.view(np.uint8).reshape(self.sbr * self.sbc, 192), self.sbc, self.sbr, self.lim, self.mblim)]

    def upload(self, torch):
        self.dev = [torch.from_numpy(b.view(np.uint8).reshape(-1).copy()).cuda() for b in self.before]
        self.tabs = [torch.from_numpy(t.view(np.int32)).cuda() for t in self._tables()]

    def call(self, stream):
        from ffmpeg_amd import vp9
        vp9.loopfilter_frames([tuple(self.dev) + tuple(self.tabs)], self.before[0].strides[0], self.before[1].strides[0], self.cols, self.rows,
                              bit_depth=self.bd, ss=self.ss, stream=stream)

    def inputs(self):
        return list(self.tabs)

    def outputs(self):
        return list(self.dev)

    def compare(self, view=lambda t: t):
        import test_gpu_vp9_lf_frame as T
        T.compare([view(d) for d in self.dev], self.want, self.before, self.cols, self.rows, self.ss)


class Vp9LoopFilterSsc(Vp9LoopFilter):
    """the same picture at 4:2:2: chroma tables of their own"""
    name, ss = "vp9_loopfilter_ssc", (1, 0)

    def _tables(self):
        from ffmpeg_amd import vp9
        return list(vp9.lf_sb_tables_ss(self.filt.view(np.uint8).reshape(self.sbr * self.sbc, 192), self.sbc, self.sbr, self.lim, self.mblim, self.ss))

    def call(self, stream):
        from ffmpeg_amd import vp9
        vp9.loopfilter_frames_ssc([tuple(self.dev) + tuple(self.tabs)], self.before[0].strides[0], self.before[1].strides[0], self.cols, self.rows,
                                  self.ss, bit_depth=self.bd, stream=stream)


# =================================================================================================================== VP8
class Vp8Recon(Face):
    """5 x 4 macroblocks, an inter frame with 30 % intra macroblocks: both kernels of the call have work, four rows hand off"""
    name, codec, mb_w, mb_h = "vp8_recon", "vp8", 5, 4

    def build(self, seed):
        import test_gpu_vp8_recon as T
        self.frame = T._frame(seed, self.mb_w, self.mb_h, False, intra=0.3)
        mbs = self.frame[0]
        assert (mbs["ref_frame"] == 0).any() and (mbs["ref_frame"] != 0).any(), "the frame needs intra and inter macroblocks"
        self.want = T._want(self.frame, self.mb_w, self.mb_h)
        return self

    def wants(self):
        return self.want

    def prefill(self):
        return self.frame[3]

    def alt_wants(self, seed):
        import test_gpu_vp8_recon as T
        import vp8_recon_gen as G
        mbs, co, refs, init = self.frame
        alt = (mbs, co, [G.planes(1000 * seed + r, self.mb_w, self.mb_h) for r in range(3)], G.planes(seed, self.mb_w, self.mb_h))
        return T._want(alt, self.mb_w, self.mb_h)

    def upload(self, torch):
        import test_gpu_vp8_recon as T
        self.pics, self.keep, self.sy, self.suv = T._upload(torch, [self.frame], self.mb_w, self.mb_h)

    def call(self, stream):
        from ffmpeg_amd import vp8
        vp8.recon_frames(self.pics, self.mb_w, self.mb_h, self.sy, self.suv, stream=stream)

    def inputs(self):
        d, dr, dco = self.keep[0]
        return [self.pics[0]["mbs"]] + ([dco] if dco is not None else []) + [t for r in dr if r is not None for t in r]

    def outputs(self):
        return list(self.keep[0][0])

    def compare(self, view=lambda t: t):
        import test_gpu_vp8_recon as T
        d, dr, dco = self.keep[0]
        got = T._download([self.frame], [([view(t) for t in d], dr, dco)], self.sy, self.suv)
        T._check(got[0], self.want, self.name)


class Vp8LoopFilter(Face):
    """5 x 4 macroblocks, the normal filter on an inter frame"""
    name, codec, mb_w, mb_h, filter_type, keyframe = "vp8_loopfilter", "vp8", 5, 4, 0, 0

    def build(self, seed):
        import test_gpu_vp8dsp as T
        frames, wants, self.sy, self.suv = T._frame_host(np.random.default_rng(seed), 1, self.mb_w, self.mb_h, self.filter_type, self.keyframe)
        self.before, self.st, self.want = list(frames[0][:3]), frames[0][3], wants[0]
        return self

    def wants(self):
        return self.want

    def prefill(self):
        return self.before

    def alt_wants(self, seed):
        import test_gpu_vp8dsp as T
        import vp8dsp_model as M
        rng = np.random.default_rng(seed)
        w = [b.copy() for b in self.before]
        for p, a in enumerate(w):
            h, wd = (16 * self.mb_h, 16 * self.mb_w) if p == 0 else (8 * self.mb_h, 8 * self.mb_w)
            a[:h, :wd] = T._content(rng, h, wd)
        M.loop_filter_frame(w[0], w[1], w[2], self.st, self.filter_type, self.keyframe)
        return w

    def upload(self, torch):
        import test_gpu_vp8dsp as T
        self.pics, self.hosts, self.keep = T._frames_to_device(torch, [tuple(self.before) + (self.st,)])

    def call(self, stream):
        from ffmpeg_amd import vp8
        vp8.loopfilter_frames(self.pics, self.filter_type, self.keyframe, self.mb_w, self.mb_h, self.sy, self.suv, stream=stream)

    def inputs(self):
        return [self.pics[0][3]]

    def outputs(self):
        return list(self.hosts[0])

    def compare(self, view=lambda t: t):
        import test_gpu_vp8dsp as T
        T._frame_compare([[view(t) for t in self.hosts[0]]], [self.want])


# ================================================================================================================= H.264
class H264Picture(Face):
    """One 4:2:0 picture of 6 x 4 macroblocks, 30 % of them intra, recorded into a picture object and flushed on the stream: MC, weights,
    residuals, an intra wavefront, and the chroma planes' in-loop filter beside the luma plane's on the object's second stream.
    The records travel from host memory at the flush, so the inputs on the device are the reference planes alone."""
    name, codec, mb_w, mb_h, pad, npics = "h264_picture", "h264", 6, 4, 32, 1

    def _p_intra(self, i):
        return 0.3

    def _record(self, seed, alt=None):
        """the pictures of `seed` recorded into picture objects of their own and decoded by the oracle: (objects, references, planes
        before, planes wanted).  alt: the references and the planes before (the samples, not the records) drawn with that seed"""
        import ffi
        import test_gpu_h264_picture as T
        from ffmpeg_amd import h264
        rng = np.random.default_rng(seed)
        H, P = 16 * self.mb_h, self.pad
        sy, sc = self.strides[0], self.strides[1]
        refs = [rng.integers(0, 256, (2 * (H + 2 * P), sy), dtype=np.uint8), rng.integers(0, 256, (2 * (H // 2 + P), sc), dtype=np.uint8),
                rng.integers(0, 256, (2 * (H // 2 + P), sc), dtype=np.uint8)]
        arng = None if alt is None else np.random.default_rng(alt)
        if arng is not None:
            refs = [_alt_like(arng, r, 255) for r in refs]
        pics, before, want = [], [], []
        for i in range(self.npics):
            planes = None if arng is None else [arng.integers(0, 256, (h, s), dtype=np.uint8) for h, s in ((H, sy), (H // 2, sc), (H // 2, sc))]
            pics.append(h264.Picture(self.mb_w, self.mb_h))
            d, w = T._record_one(pics[-1], rng, ffi.oracle(), h264, self.mb_w, self.mb_h, P, refs, self.strides, self._p_intra(i), planes)
            before.append(d)
            want.append(w)
        return pics, refs, before, want

    @property
    def strides(self):
        sy, sc = 16 * self.mb_w + 2 * self.pad, 8 * self.mb_w + self.pad
        return [sy, sc, sc]

    def _lists(self, pic):
        import ctypes as C

        import test_h264_picture_cpu as TC
        from ffmpeg_amd import _lib
        ls = TC.Lists()
        assert _lib.lib().ffhip_h264_picture_lists(pic._p, C.byref(ls)) == 0
        return ls

    def build(self, seed):
        self.seed = seed
        self.pics, self.refs, self.before, self.want = self._record(seed)
        for i, pic in enumerate(self.pics):
            ls = self._lists(pic)
            assert bool(ls.nintra[0]) == bool(self._p_intra(i)), "picture %d: intra macroblocks" % i
            assert all(ls.nqpel[0]) and all(ls.nwt) and all(ls.edges), "picture %d needs every MC stage, weights and edges in three planes" % i
        return self

    def fresh(self):
        """the object owns staging buffers and streams: a copy records the same pictures into objects of its own.  (The decoy of a
        late=True run flushes its recorded lists once per pool slot, in place on planes of its own: a flush keeps the lists until the
        next begin(), and what the repeated flushes leave in those planes is never compared.  The objects are closed when collected.)"""
        g = copy.copy(self)
        g.pics = self._record(self.seed)[0]
        return g

    def wants(self):
        return [pl for w in self.want for pl in w]

    def prefill(self):
        return [pl for d in self.before for pl in d]

    def alt_wants(self, seed):
        pics, _, _, want = self._record(self.seed, alt=seed)
        for p in pics:
            p.close()
        return [pl for w in want for pl in w]

    def upload(self, torch):
        self.d_refs = [torch.from_numpy(r).cuda() for r in self.refs]
        self.d_dst = [[torch.from_numpy(a.copy()).cuda() for a in d] for d in self.before]

    def call(self, stream):
        self.pics[0].flush(self.d_dst[0], self.strides, self.d_refs, stream=stream)

    def inputs(self):
        return list(self.d_refs)

    def outputs(self):
        return [t for d in self.d_dst for t in d]

    def compare(self, view=lambda t: t):
        for i, (d, w) in enumerate(zip(self.d_dst, self.want)):
            for pl in range(3):
                got = view(d[pl]).cpu().numpy()
                assert np.array_equal(got, w[pl]), "%s: picture %d plane %d: %d mismatches" % (self.name, i, pl, (got != w[pl]).sum())


class H264PicturesBatch(H264Picture):
    """three such pictures flushed together, the second without an intra macroblock: the smallest batch whose front halves run on
    threads of the call, with the intra wavefronts and the in-loop filter of all three shared"""
    name, npics = "h264_pictures_batch", 3

    def _p_intra(self, i):
        return 0.0 if i == 1 else 0.3

    def call(self, stream):
        from ffmpeg_amd import h264
        h264.pictures_flush(self.pics, self.d_dst, self.strides, [self.d_refs] * self.npics, stream=stream)


FACES = [HevcResidual, HevcInter, HevcIntra, HevcLoopFilter, HevcBoundaryStrengths,
         Vp9Inter, Vp9InterScaled, Vp9Intra, Vp9LoopFilter, Vp9LoopFilterSsc, Vp8Recon, Vp8LoopFilter, H264Picture, H264PicturesBatch]
NAMES = [F.name for F in FACES]
#: the codecs whose faces chain, run on frame threads and have a first-use child (the H.264 picture object has none of the three)
CODECS = ["hevc", "vp9", "vp8"]
#: the seeds of the stream tests; tests/test_picture_faces_cpu.py shows that with them a staged test cannot pass by accident
SEED = {name: 8800 + i for i, name in enumerate(NAMES)}
ALT_SEED = 99


def make(name, seed=None):
    F = FACES[NAMES.index(name)]
    return F().build(SEED[name] if seed is None else seed)


def of_codec(codec):
    return [F.name for F in FACES if F.codec == codec]


# ======================================================================================================= running on a stream
#: the delay queued on the stream ahead of the staging copies: DELAY_COPIES device-to-device copies of DELAY_CHUNK bytes.  16 x 256 MiB
#: = 4 GiB written (and as much read); at the 8 TB/s HBM peak of an MI355X that keeps the stream busy for about 1 ms at the very least,
#: some hundred times what a kernel launch takes to start, so work a face leaves on another stream runs long before the real inputs land.
DELAY_CHUNK, DELAY_COPIES = 256 << 20, 16
SNAP_FILL = 0x3C
#: the slots of the progress pool (progress_pool.hip), handed out in turn
POOL_SLOTS = 64


class Delay:
    def __init__(self, torch):
        self.a = torch.full((DELAY_CHUNK,), 1, dtype=torch.uint8, device="cuda")
        self.b = torch.empty_like(self.a)

    def queue(self):
        """on torch's current stream"""
        for _ in range(DELAY_COPIES):
            self.b.copy_(self.a, non_blocking=True)

    @property
    def bytes_moved(self):
        return DELAY_CHUNK * DELAY_COPIES


def _bytes(torch, t):
    return t.view(torch.uint8)


def run_staged(torch, L, stream, faces, delay, late=False):
    """The staged run of `faces` (adapters or chains that are built, not yet uploaded) on the created stream `stream` (a c_void_p).

    late=False, work left on another stream runs too EARLY: every input and output tensor holds POISON when the device is
    synchronised for the only time; then, on the stream alone, the delay, the copies that put the real bytes in place, each face's
    call in order, and a copy of every output tensor to a snapshot.  Foreign work that reads device memory (a kernel) sees poison.

    late=True, work left on another stream runs too LATE: what a launcher leaves on the NULL stream and that reads host memory only
    (the copy of the picture structs into a pool slot, the memset of a slot's counters) is harmless early and harmful late.  So
    first every pool slot is dirtied: POOL_SLOTS calls of each face on a decoy (the same host picture, so the same geometry, in
    device tensors of its own), which leaves in every slot structs that point at the decoy and counters of a finished launch.  The
    real bytes are in place when the device is synchronised for the only time.  Then the delay goes on the NULL stream, where the
    test itself queues nothing else, and the faces and the snapshots on the created stream as before: a struct copy or memset
    that waits behind the delay leaves the kernel with the decoy's slot, and the real outputs keep their pre-call fill.

    ffhip_stream_synchronize(stream) must return 0; check_staged() then puts the snapshots through each face's compare and requires
    the inputs to equal what was staged.  Every tensor stays referenced until the end: the caching allocator knows nothing about
    the stream."""
    ext = torch.cuda.ExternalStream(stream.value)
    decoys = []
    if late:
        for f in faces:
            g = f.fresh()
            g.upload(torch)
            decoys.append(g)
        torch.cuda.synchronize()
        for g in decoys:
            for _ in range(POOL_SLOTS):
                g.call(stream.value)
        assert L.ffhip_stream_synchronize(stream) == 0, L.ffhip_last_error()
    for f in faces:
        f.upload(torch)
    seen, tensors = set(), []
    for f in faces:
        for t in f.inputs() + f.outputs():
            if id(t) not in seen:
                seen.add(id(t))
                tensors.append(t)
    outs = {id(t): t for f in faces for t in f.outputs()}
    real = [t.clone() for t in tensors]
    snaps = {k: torch.empty_like(t) for k, t in outs.items()}
    if not late:
        for t in tensors:
            _bytes(torch, t).fill_(POISON)
    for t in snaps.values():
        _bytes(torch, t).fill_(SNAP_FILL)
    torch.cuda.synchronize()
    # ---- from here to the synchronise below the test queues nothing on another stream but the late variant's delay
    try:
        if late:
            delay.queue()                               # torch's current stream here is the NULL stream
        else:
            with torch.cuda.stream(ext):
                delay.queue()
                for t, r in zip(tensors, real):
                    t.copy_(r, non_blocking=True)
        for f in faces:
            f.call(stream.value)
        with torch.cuda.stream(ext):
            for k, t in outs.items():
                snaps[k].copy_(t, non_blocking=True)
        assert L.ffhip_stream_synchronize(stream) == 0, L.ffhip_last_error()
    finally:
        if late:
            torch.cuda.synchronize()                    # the delay, and whatever waited behind it, before any tensor goes
    view = lambda t: snaps.get(id(t), t)
    ins = [(f.name, t, r) for f in faces for t in f.inputs() for u, r in zip(tensors, real) if u is t and id(t) not in outs]
    return view, ins, (tensors, real, snaps, decoys)


def check_staged(torch, faces, view, ins):
    for f in faces:
        f.compare(view)
    for name, t, r in ins:
        assert torch.equal(t, r), "%s: an input tensor no longer holds what was staged" % name
