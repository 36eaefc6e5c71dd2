"""Host-side mirror of the reference's me_cmp table / ff_me_search_esa for the batched device faces."""
from . import _lib

SAD, SATD = 0, 1
# the filter's search methods (== AV_ME_METHOD_*); EPZS and UMH take the neighbouring blocks' vectors: search_pred_batch()
ESA, TSS, TDLS, NTSS, FSS, DS, HEXBS, EPZS, UMH = range(1, 10)


def _stream(stream):
    import torch
    return torch.cuda.current_stream().cuda_stream if stream is None else stream


def cmp_batch(kind, width, h, blk1, off1, blk2, off2, stride, out, stream=None):
    """out[i] = me_cmp[kind](blk1 + off1[i], blk2 + off2[i], stride, h); tensors on the device."""
    return _lib.check(_lib.lib().ffhip_me_cmp_batch_dev(kind, width, h, blk1.data_ptr(), off1.data_ptr(), blk2.data_ptr(),
                                                        off2.data_ptr(), stride, out.data_ptr(), off1.numel(),
                                                        _stream(stream)), "ffhip_me_cmp_batch_dev")


def esa_batch(cur, ref, width, height, stride, frame_pitch, nframes, mb_size, search_param, cost_kind, mv_out, cost_out,
              stream=None):
    """Exhaustive search of every mb_size block of `cur` in `ref` (ff_me_search_esa semantics), nframes pairs."""
    return _lib.check(_lib.lib().ffhip_me_esa_batch_dev(cur.data_ptr(), ref.data_ptr(), width, height, stride, frame_pitch,
                                                        nframes, mb_size, search_param, cost_kind, mv_out.data_ptr(),
                                                        cost_out.data_ptr(), _stream(stream)), "ffhip_me_esa_batch_dev")


def search_batch(method, cur, ref, width, height, stride, frame_pitch, nframes, mb_size, search_param, cost_kind, mv_out, cost_out,
                 stream=None):
    """The filter's per-block search `method` (ESA .. HEXBS) of every mb_size block of `cur` in `ref`, nframes pairs in one launch;
    tensors on the device, outputs as esa_batch()."""
    return _lib.check(_lib.lib().ffhip_me_search_batch_dev(method, cur.data_ptr(), ref.data_ptr(), width, height, stride, frame_pitch,
                                                           nframes, mb_size, search_param, cost_kind, mv_out.data_ptr(),
                                                           cost_out.data_ptr(), _stream(stream)), "ffhip_me_search_batch_dev")


def _host_counts():
    """(blocks searched, costs evaluated) of this thread's last *_frames_host call"""
    import ctypes as C
    blocks, costs = C.c_uint64(), C.c_uint64()
    _lib.lib().ffhip_me_search_host_counts(C.byref(blocks), C.byref(costs))
    return blocks.value, costs.value


def search_frames_host(method, cur, ref, width, height, stride, frame_pitch, nframes, mb_size, search_param, cost_kind, mv_out, cost_out):
    """The same rules on the CPU (device-free): numpy arrays (uint8 planes, int16 vectors, uint32 costs).  Returns (blocks searched,
    costs evaluated)."""
    _lib.check(_lib.lib().ffhip_me_search_frames_host(method, cur.ctypes.data, ref.ctypes.data, width, height, stride, frame_pitch,
                                                      nframes, mb_size, search_param, cost_kind, mv_out.ctypes.data,
                                                      cost_out.ctypes.data), "ffhip_me_search_frames_host")
    return _host_counts()


def search_pred_batch(method, cur, ref, width, height, stride, frame_pitch, nframes, mb_size, search_param, cost_kind, prev1, prev2,
                      mv_out, cost_out, stream=None):
    """The filter's predictive search `method` (EPZS or UMH) of every mb_size block of `cur` in `ref`, nframes independent pairs in
    one launch; tensors on the device, outputs as esa_batch().  prev1 / prev2: the vector fields (laid out as mv_out) of the previous
    and the one-before-previous pair, or None for zero vectors."""
    p = lambda t: None if t is None else t.data_ptr()
    return _lib.check(_lib.lib().ffhip_me_search_pred_batch_dev(method, cur.data_ptr(), ref.data_ptr(), width, height, stride, frame_pitch,
                                                                nframes, mb_size, search_param, cost_kind, p(prev1), p(prev2),
                                                                mv_out.data_ptr(), cost_out.data_ptr(), _stream(stream)),
                      "ffhip_me_search_pred_batch_dev")


def search_pred_frames_host(method, cur, ref, width, height, stride, frame_pitch, nframes, mb_size, search_param, cost_kind, prev1, prev2,
                            mv_out, cost_out):
    """The same rules on the CPU (device-free): numpy arrays (uint8 planes, int16 vectors, uint32 costs), prev1 / prev2 arrays or
    None.  Returns (blocks searched, costs evaluated)."""
    p = lambda a: None if a is None else a.ctypes.data
    _lib.check(_lib.lib().ffhip_me_search_pred_frames_host(method, cur.ctypes.data, ref.ctypes.data, width, height, stride, frame_pitch,
                                                           nframes, mb_size, search_param, cost_kind, p(prev1), p(prev2),
                                                           mv_out.ctypes.data, cost_out.ctypes.data), "ffhip_me_search_pred_frames_host")
    return _host_counts()


def search_pred_sequence(method, frames, width, height, stride, frame_pitch, nframes, seq_pitch, nseq, direction, mb_size, search_param,
                         cost_kind, init1, init2, mv_out, cost_out, stream=None):
    """The predictive search `method` (EPZS or UMH) of nseq sequences of nframes pictures in one launch, pair k chained to the fields
    of pairs k - 1 and k - 2; tensors on the device.  Picture p of sequence s is at frames + s * seq_pitch + p * frame_pitch;
    direction 0: cur = picture k + 1, ref = picture k, 1: the other way round.  Outputs pair-major: step k's nseq fields are one batch
    in search_pred_batch()'s layout.  init1 / init2: nseq fields each, those of the pairs before pair 0, or None for zero vectors."""
    p = lambda t: None if t is None else t.data_ptr()
    return _lib.check(_lib.lib().ffhip_me_search_pred_sequence_dev(method, frames.data_ptr(), width, height, stride, frame_pitch, nframes,
                                                                   seq_pitch, nseq, direction, mb_size, search_param, cost_kind, p(init1),
                                                                   p(init2), mv_out.data_ptr(), cost_out.data_ptr(), _stream(stream)),
                      "ffhip_me_search_pred_sequence_dev")


def search_pred_sequence_host(method, frames, width, height, stride, frame_pitch, nframes, seq_pitch, nseq, direction, mb_size, search_param,
                              cost_kind, init1, init2, mv_out, cost_out):
    """The same loop on the CPU (device-free): numpy arrays, init1 / init2 arrays or None.  Returns (blocks searched, costs
    evaluated) over all pairs."""
    p = lambda a: None if a is None else a.ctypes.data
    _lib.check(_lib.lib().ffhip_me_search_pred_sequence_host(method, frames.ctypes.data, width, height, stride, frame_pitch, nframes, seq_pitch,
                                                             nseq, direction, mb_size, search_param, cost_kind, p(init1), p(init2),
                                                             mv_out.ctypes.data, cost_out.ctypes.data), "ffhip_me_search_pred_sequence_host")
    return _host_counts()


# ---- bilateral motion estimation (vf_minterpolate's me_mode=bilat): one search per pair, half-vectors ------------------------------
def search_bilat_batch(method, cur, ref, width, height, stride, frame_pitch, nframes, mb_size, search_param, prev1, prev2, mv_out, cost_out,
                       stream=None):
    """EPZS or UMH under the bilateral cost, nframes independent pairs in one launch: picture A is `cur`, picture B `ref`, and a block's
    vector is the half-vector v with A sampled at +v and B at -v.  Arguments and outputs as search_pred_batch(), without cost_kind."""
    return _lib.check(_lib.lib().ffhip_me_search_bilat_batch_dev(method, _ptr(cur), _ptr(ref), width, height, stride, frame_pitch, nframes,
                                                                 mb_size, search_param, _ptr(prev1), _ptr(prev2), _ptr(mv_out),
                                                                 _ptr(cost_out), _stream(stream)), "ffhip_me_search_bilat_batch_dev")


def search_bilat_frames_host(method, cur, ref, width, height, stride, frame_pitch, nframes, mb_size, search_param, prev1, prev2, mv_out,
                             cost_out):
    """The same rules on the CPU (device-free): numpy arrays, prev1 / prev2 arrays or None.  Returns (blocks searched, costs
    evaluated)."""
    _lib.check(_lib.lib().ffhip_me_search_bilat_frames_host(method, _ptr(cur), _ptr(ref), width, height, stride, frame_pitch, nframes, mb_size,
                                                            search_param, _ptr(prev1), _ptr(prev2), _ptr(mv_out), _ptr(cost_out)),
               "ffhip_me_search_bilat_frames_host")
    return _host_counts()


def search_bilat_cost_host(cur, ref, width, height, stride, mb_size, search_param, bx, by, x, y, pred):
    """A test hook, not for callers: cost(x, y) of block (bx, by) of the pair (cur, ref) under the bilateral rule with the predictor
    `pred`, on the CPU"""
    import ctypes as C
    c = C.c_uint32()
    _lib.check(_lib.lib().ffhip_me_search_bilat_cost_host(_ptr(cur), _ptr(ref), width, height, stride, mb_size, search_param, bx, by, x, y,
                                                          pred[0], pred[1], C.addressof(c)), "ffhip_me_search_bilat_cost_host")
    return c.value


def search_bilat_sequence(method, frames, width, height, stride, frame_pitch, nframes, seq_pitch, nseq, mb_size, search_param, init1, init2,
                          mv_out, cost_out, stream=None):
    """The bilateral search of nseq sequences of nframes pictures in one launch, pair k (pictures k and k + 1) chained to the fields of
    pairs k - 1 and k - 2; tensors on the device.  Layouts as search_pred_sequence(), without cost_kind and direction."""
    return _lib.check(_lib.lib().ffhip_me_search_bilat_sequence_dev(method, _ptr(frames), width, height, stride, frame_pitch, nframes, seq_pitch,
                                                                    nseq, mb_size, search_param, _ptr(init1), _ptr(init2), _ptr(mv_out),
                                                                    _ptr(cost_out), _stream(stream)), "ffhip_me_search_bilat_sequence_dev")


def search_bilat_sequence_host(method, frames, width, height, stride, frame_pitch, nframes, seq_pitch, nseq, mb_size, search_param, init1, init2,
                               mv_out, cost_out):
    """The same loop on the CPU (device-free): numpy arrays.  Returns (blocks searched, costs evaluated) over all pairs."""
    _lib.check(_lib.lib().ffhip_me_search_bilat_sequence_host(method, _ptr(frames), width, height, stride, frame_pitch, nframes, seq_pitch, nseq,
                                                              mb_size, search_param, _ptr(init1), _ptr(init2), _ptr(mv_out), _ptr(cost_out)),
               "ffhip_me_search_bilat_sequence_host")
    return _host_counts()


# ---- vf_minterpolate's compensation (ffhip_me_interp_sequence_dev / _host) ----------------------------------------------------------
MCI, BLEND = 0, 1
INTERP_COUNTS = ("taken", "zero_weight", "capped", "malformed", "fallback", "clipped", "samples", "blend")


def _structs():
    import ctypes as C

    class Planes(C.Structure):              # FFHipMePlanes
        _fields_ = [("base", C.c_void_p * 3), ("stride", C.c_ssize_t * 3), ("frame_pitch", C.c_size_t * 3), ("seq_pitch", C.c_size_t * 3)]

    class Job(C.Structure):                 # FFHipMeInterpJob
        _fields_ = [("seq", C.c_int32), ("pair", C.c_int32), ("alpha", C.c_int32), ("mode", C.c_int32)]
    return Planes, Job


def _ptr(a):
    """an address: None, an int, a torch tensor or a numpy array"""
    if a is None or isinstance(a, int):
        return a
    return a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data


def planes(bases, strides, frame_pitches, seq_pitches=None):
    """An FFHipMePlanes: picture p of sequence s, plane i, is at bases[i] + s * seq_pitches[i] + p * frame_pitches[i].  One or three
    planes; a base is an address, a tensor or an array."""
    Planes, _ = _structs()
    P = Planes()
    for i, b in enumerate(bases):
        P.base[i] = _ptr(b)
        P.stride[i] = strides[i]
        P.frame_pitch[i] = frame_pitches[i]
        P.seq_pitch[i] = seq_pitches[i] if seq_pitches is not None else 0
    return P


def interp_jobs(jobs):
    """An FFHipMeInterpJob array of (seq, pair, alpha, mode) tuples"""
    _, Job = _structs()
    arr = (Job * max(len(jobs), 1))()
    for j, t in enumerate(jobs):
        arr[j] = Job(*t)
    return arr


def _interp_args(src, dst, nplanes, log2_chroma_w, log2_chroma_h, width, height, nframes, nseq, mb_size, mv_range, window, mv_fwd, mv_bwd, jobs):
    import ctypes as C
    import numpy as np
    window = np.ascontiguousarray(window, dtype=np.uint8)
    if window.size != 4 * mb_size * mb_size and mb_size in (8, 16):
        raise ValueError("window holds %d bytes, not (2 * mb_size)^2" % window.size)
    arr = interp_jobs(jobs)
    keep = (window, arr, src, dst)
    return keep, (C.addressof(src), C.addressof(dst), nplanes, log2_chroma_w, log2_chroma_h, width, height, nframes, nseq, mb_size, mv_range,
                  window.ctypes.data, _ptr(mv_fwd), _ptr(mv_bwd), C.addressof(arr), len(jobs))


def interp_sequence(src, dst, nplanes, log2_chroma_w, log2_chroma_h, width, height, nframes, nseq, mb_size, mv_range, window, mv_fwd, mv_bwd,
                    jobs, stream=None):
    """vf_minterpolate's compensation (mci / bidir / obmc, or the blend) of every job in one launch.  src, dst: planes() of device
    memory; window: (2 * mb_size)^2 bytes on the host; mv_fwd, mv_bwd: the direction-0 and direction-1 fields of
    search_pred_sequence(), on the device; jobs: (seq, pair, alpha, mode) tuples, job j writes output picture j."""
    keep, args = _interp_args(src, dst, nplanes, log2_chroma_w, log2_chroma_h, width, height, nframes, nseq, mb_size, mv_range, window, mv_fwd,
                              mv_bwd, jobs)
    r = _lib.lib().ffhip_me_interp_sequence_dev(*args, _stream(stream))
    del keep
    return _lib.check(r, "ffhip_me_interp_sequence_dev")


def interp_host_counts():
    """What this thread's last interp_sequence_host() did: a dict over INTERP_COUNTS"""
    import ctypes as C
    c = (C.c_uint64 * 8)()
    _lib.lib().ffhip_me_interp_host_counts(c)
    return dict(zip(INTERP_COUNTS, (int(v) for v in c)))


def interp_sequence_host(src, dst, nplanes, log2_chroma_w, log2_chroma_h, width, height, nframes, nseq, mb_size, mv_range, window, mv_fwd,
                         mv_bwd, jobs):
    """The same rule on the CPU (device-free): planes() of numpy memory, numpy fields.  Returns interp_host_counts()."""
    keep, args = _interp_args(src, dst, nplanes, log2_chroma_w, log2_chroma_h, width, height, nframes, nseq, mb_size, mv_range, window, mv_fwd,
                              mv_bwd, jobs)
    r = _lib.lib().ffhip_me_interp_sequence_host(*args)
    del keep
    _lib.check(r, "ffhip_me_interp_sequence_host")
    return interp_host_counts()


# ---- vf_minterpolate's scene-change detection (ffhip_me_scene_sequence_dev / _host) and the interpolation that takes its flags -------
SCENE_BLEND, SCENE_DUP = 1, 2


def scene_sequence(frames, depth, width, height, stride, frame_pitch, nframes, seq_pitch, nseq, threshold, mafd_in=None, mafd_out=None,
                   sad_out=None, score_out=None, flags_out=None, stream=None):
    """The scene-change detection of nseq sequences of nframes pictures, nothing read back: per pair (pair-major, k * nseq + s) the
    whole-picture SAD (sad_out, uint64), the score (score_out, float32) and the flag score >= threshold (flags_out, uint8); any of the
    three may be None, not all.  mafd_in / mafd_out: nseq doubles, the carried value before the first and after the last pair.
    Everything is an address or a tensor on the device; frames as in search_pred_sequence(), uint16 samples above depth 8."""
    return _lib.check(_lib.lib().ffhip_me_scene_sequence_dev(_ptr(frames), depth, width, height, stride, frame_pitch, nframes, seq_pitch, nseq,
                                                             threshold, _ptr(mafd_in), _ptr(mafd_out), _ptr(sad_out), _ptr(score_out),
                                                             _ptr(flags_out), _stream(stream)), "ffhip_me_scene_sequence_dev")


def scene_sequence_host(frames, depth, width, height, stride, frame_pitch, nframes, seq_pitch, nseq, threshold, mafd_in=None, mafd_out=None,
                        sad_out=None, score_out=None, flags_out=None):
    """The same rule on the CPU (device-free): addresses or numpy arrays."""
    return _lib.check(_lib.lib().ffhip_me_scene_sequence_host(_ptr(frames), depth, width, height, stride, frame_pitch, nframes, seq_pitch, nseq,
                                                              threshold, _ptr(mafd_in), _ptr(mafd_out), _ptr(sad_out), _ptr(score_out),
                                                              _ptr(flags_out)), "ffhip_me_scene_sequence_host")


def interp_sequence_scd(src, dst, nplanes, log2_chroma_w, log2_chroma_h, width, height, nframes, nseq, mb_size, mv_range, window, mv_fwd, mv_bwd,
                        jobs, scene, scene_action=SCENE_BLEND, stream=None):
    """interp_sequence() with the MCI-or-fallback choice taken from device memory: scene is scene_sequence()'s flags_out (or None); an
    MCI job whose pair is flagged runs scene_action (SCENE_BLEND, or SCENE_DUP: picture A when alpha <= 512, else picture B)."""
    keep, args = _interp_args(src, dst, nplanes, log2_chroma_w, log2_chroma_h, width, height, nframes, nseq, mb_size, mv_range, window, mv_fwd,
                              mv_bwd, jobs)
    r = _lib.lib().ffhip_me_interp_sequence_scd_dev(*args, _ptr(scene), scene_action, _stream(stream))
    del keep
    return _lib.check(r, "ffhip_me_interp_sequence_scd_dev")


def interp_sequence_scd_host(src, dst, nplanes, log2_chroma_w, log2_chroma_h, width, height, nframes, nseq, mb_size, mv_range, window, mv_fwd,
                             mv_bwd, jobs, scene, scene_action=SCENE_BLEND):
    """The same on the CPU (device-free): scene a numpy array of flags or None.  Returns interp_host_counts()."""
    keep, args = _interp_args(src, dst, nplanes, log2_chroma_w, log2_chroma_h, width, height, nframes, nseq, mb_size, mv_range, window, mv_fwd,
                              mv_bwd, jobs)
    r = _lib.lib().ffhip_me_interp_sequence_scd_host(*args, _ptr(scene), scene_action)
    del keep
    _lib.check(r, "ffhip_me_interp_sequence_scd_host")
    return interp_host_counts()


def _interp_bilat_args(src, dst, nplanes, log2_chroma_w, log2_chroma_h, width, height, nframes, nseq, mb_size, mv_range, window, mv, jobs):
    keep, a = _interp_args(src, dst, nplanes, log2_chroma_w, log2_chroma_h, width, height, nframes, nseq, mb_size, mv_range, window, mv, None, jobs)
    return keep, a[:13] + a[14:]        # one field: mv_bwd's place is dropped


def interp_bilat_sequence(src, dst, nplanes, log2_chroma_w, log2_chroma_h, width, height, nframes, nseq, mb_size, mv_range, window, mv, jobs,
                          scene=None, scene_action=SCENE_BLEND, stream=None):
    """The bilateral compensation (me_mode=bilat) of every job in one launch: interp_sequence_scd() with the one field `mv` of
    search_bilat_sequence()'s half-vectors in place of mv_fwd / mv_bwd; scene may be None."""
    keep, args = _interp_bilat_args(src, dst, nplanes, log2_chroma_w, log2_chroma_h, width, height, nframes, nseq, mb_size, mv_range, window, mv, jobs)
    r = _lib.lib().ffhip_me_interp_bilat_sequence_dev(*args, _ptr(scene), scene_action, _stream(stream))
    del keep
    return _lib.check(r, "ffhip_me_interp_bilat_sequence_dev")


def interp_bilat_sequence_host(src, dst, nplanes, log2_chroma_w, log2_chroma_h, width, height, nframes, nseq, mb_size, mv_range, window, mv, jobs,
                               scene=None, scene_action=SCENE_BLEND):
    """The same on the CPU (device-free).  Returns interp_host_counts()."""
    keep, args = _interp_bilat_args(src, dst, nplanes, log2_chroma_w, log2_chroma_h, width, height, nframes, nseq, mb_size, mv_range, window, mv, jobs)
    r = _lib.lib().ffhip_me_interp_bilat_sequence_host(*args, _ptr(scene), scene_action)
    del keep
    _lib.check(r, "ffhip_me_interp_bilat_sequence_host")
    return interp_host_counts()
