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
