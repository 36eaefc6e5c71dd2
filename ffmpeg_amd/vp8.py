"""ctypes mirror of the vp8dsp faces of libffhip (include/ffhip.h): VP8DSPContext (libavcodec/vp8dsp.h) through ff_vp78dsp_init_hip /
ff_vp8dsp_init_hip, the batch device faces (WHT, IDCT, MC), the whole-frame reconstruction and the whole-frame loop filter.  8 bits, the
only depth VP8 has."""
import ctypes as C

import numpy as np

from . import _lib

#: FFHipVp8WhtRec / FFHipVp8IdctRec / FFHipVp8McRec (include/ffhip.h); offsets in bytes
WHT_DTYPE = np.dtype([("dc_offset", np.int32), ("block_offset", np.int32), ("dc_only", np.uint8), ("pad", np.uint8, 3)])
IDCT_DTYPE = np.dtype([("dst_offset", np.int32), ("coeff_offset", np.int32), ("dc_only", np.uint8), ("pad", np.uint8, 3)])
MC_DTYPE = np.dtype([("dst_offset", np.int32), ("src_offset", np.int32), ("width", np.uint8), ("h", np.uint8), ("mx", np.uint8),
                     ("my", np.uint8), ("htaps", np.uint8), ("vtaps", np.uint8), ("bilinear", np.uint8), ("pad", np.uint8)])
#: FFHipVp8FilterStrength == VP8FilterStrength
STRENGTH_DTYPE = np.dtype([("filter_level", np.uint8), ("inner_limit", np.uint8), ("inner_filter", np.uint8)])
FILTER_NORMAL, FILTER_SIMPLE = 0, 1
#: FFHipVp8Mb: one macroblock of recon_frames(); block b's 2-bit code is (block_code[b >> 2] >> 2 * (b & 3)) & 3
MB_DTYPE = np.dtype([("coeff_offset", np.int32), ("mv", np.int16, (16, 2)), ("sub_mode", np.uint8, 16), ("block_code", np.uint8, 6),
                     ("ref_frame", np.uint8), ("mode", np.uint8), ("chroma_mode", np.uint8), ("partitioning", np.uint8), ("y2", np.uint8),
                     ("reserved", np.uint8)])
#: FFHipVp8Pred / FFHipVp8IntraModes
PRED_DTYPE = np.dtype([("plane", np.uint8), ("x", np.uint8), ("y", np.uint8), ("w", np.uint8), ("h", np.uint8), ("mx", np.uint8), ("my", np.uint8),
                       ("vslot", np.uint8), ("hslot", np.uint8), ("pad", np.uint8, 3), ("sx", np.int32), ("sy", np.int32)])
INTRA_MODES_DTYPE = np.dtype([("mode16", np.uint8), ("chroma", np.uint8), ("sub", np.uint8, 16), ("copy", np.uint8, 16)])
PRED_DC, PRED_HOR, PRED_VERT, PRED_TM, MODE_I4x4 = 0, 1, 2, 3, 4                      # FFHIP_VP8_PRED_* / FFHIP_VP8_MODE_I4x4
PRED_LEFT_DC, PRED_TOP_DC, PRED_DC_128, PRED_DC_127, PRED_DC_129 = 4, 5, 6, 7, 8      # slots only
PRED_NONE = 255                                                                       # intra_modes()'s mode16 of an I4x4 macroblock
B_VERT, B_HOR, B_DC, B_DDL, B_DDR, B_VR, B_HD, B_VL, B_HU, B_TM = range(10)           # FFHIP_VP8_B_*
B_VERT_PLAIN, B_DC_127, B_DC_129, B_HOR_PLAIN = 10, 12, 13, 14                        # slots only
PART_NONE, PART_16x8, PART_8x16, PART_8x8, PART_4x4 = range(5)                        # FFHIP_VP8_PART_*
MB_COEFFS = 400                                                                       # td->block[6][4][16] + td->block_dc[16]

_MC = C.CFUNCTYPE(None, C.c_void_p, C.c_ssize_t, C.c_void_p, C.c_ssize_t, C.c_int, C.c_int, C.c_int)
_LF = C.CFUNCTYPE(None, C.c_void_p, C.c_ssize_t, C.c_int, C.c_int, C.c_int)
_LFUV = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_ssize_t, C.c_int, C.c_int, C.c_int)
_LFS = C.CFUNCTYPE(None, C.c_void_p, C.c_ssize_t, C.c_int)
_WHT = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p)
_IDCT = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_ssize_t)


class VP8DSPContext(C.Structure):
    """FFHipVP8DSPContext: VP8DSPContext member for member"""
    _fields_ = [("vp8_luma_dc_wht", _WHT), ("vp8_luma_dc_wht_dc", _WHT), ("vp8_idct_add", _IDCT), ("vp8_idct_dc_add", _IDCT),
                ("vp8_idct_dc_add4y", _IDCT), ("vp8_idct_dc_add4uv", _IDCT),
                ("vp8_v_loop_filter16y", _LF), ("vp8_h_loop_filter16y", _LF), ("vp8_v_loop_filter8uv", _LFUV), ("vp8_h_loop_filter8uv", _LFUV),
                ("vp8_v_loop_filter16y_inner", _LF), ("vp8_h_loop_filter16y_inner", _LF), ("vp8_v_loop_filter8uv_inner", _LFUV),
                ("vp8_h_loop_filter8uv_inner", _LFUV), ("vp8_v_loop_filter_simple", _LFS), ("vp8_h_loop_filter_simple", _LFS),
                ("put_vp8_epel_pixels_tab", _MC * 3 * 3 * 3), ("put_vp8_bilinear_pixels_tab", _MC * 3 * 3 * 3)]


def dsp_init(c=None):
    """ff_vp78dsp_init_hip then ff_vp8dsp_init_hip on `c` (a fresh context when None): every member on the device"""
    c = VP8DSPContext() if c is None else c
    _lib.check(_lib.lib().ff_vp78dsp_init_hip(C.byref(c)), "ff_vp78dsp_init_hip")
    _lib.check(_lib.lib().ff_vp8dsp_init_hip(C.byref(c)), "ff_vp8dsp_init_hip")
    return c


def _st(stream):
    return None if stream is None else C.c_void_p(stream)


def luma_dc_wht_batch(coeffs, recs, n, stream=None):
    """coeffs: int16 device tensor holding every dc[16] and block[4][4][16]; recs: device uint8 [n * 12] WHT_DTYPE records"""
    return _lib.check(_lib.lib().ffhip_vp8_luma_dc_wht_batch_dev(coeffs.data_ptr(), recs.data_ptr(), n, _st(stream)),
                      "ffhip_vp8_luma_dc_wht_batch_dev")


def idct_add_batch(dst, stride, coeffs, recs, n, stream=None):
    """dst: uint8 device tensor; coeffs: int16 device tensor (consumed); recs: device uint8 [n * 12] IDCT_DTYPE records"""
    return _lib.check(_lib.lib().ffhip_vp8_idct_add_batch_dev(dst.data_ptr(), stride, coeffs.data_ptr(), recs.data_ptr(), n, _st(stream)),
                      "ffhip_vp8_idct_add_batch_dev")


def mc_batch(dst, dststride, src, srcstride, recs, n, stream=None):
    """recs: device uint8 [n * 16] MC_DTYPE records"""
    return _lib.check(_lib.lib().ffhip_vp8_mc_batch_dev(dst.data_ptr(), dststride, src.data_ptr(), srcstride, recs.data_ptr(), n, _st(stream)),
                      "ffhip_vp8_mc_batch_dev")


class LfPic(C.Structure):   # FFHipVp8LfPic
    _fields_ = [("y", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p), ("strength", C.c_void_p)]


def loopfilter_frames(pics, filter_type, keyframe, mb_w, mb_h, stride_y, stride_uv, stream=None):
    """ffhip_vp8_loopfilter_frames_dev: pics = [(y, u, v, strength)] device tensors (u / v may be None for the simple filter), strength
    = mb_w * mb_h STRENGTH_DTYPE records in raster order"""
    def p(t):
        return None if t is None else t.data_ptr()
    arr = (LfPic * len(pics))(*[LfPic(p(y), p(u), p(v), p(s)) for y, u, v, s in pics])
    return _lib.check(_lib.lib().ffhip_vp8_loopfilter_frames_dev(filter_type, keyframe, mb_w, mb_h, len(pics), C.cast(arr, C.c_void_p),
                                                                 stride_y, stride_uv, _st(stream)), "ffhip_vp8_loopfilter_frames_dev")


class ReconPic(C.Structure):   # FFHipVp8ReconPic
    _fields_ = [("y", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p), ("ref", C.c_void_p * 3 * 3), ("mbs", C.c_void_p),
                ("coeffs", C.c_void_p), ("coeff_count", C.c_int64)]


def mb_record_size():
    return _lib.lib().ffhip_vp8_mb_record_size()


def recon_frames(pics, mb_w, mb_h, stride_y, stride_uv, bilinear=0, fullpel_chroma=0, stream=None):
    """ffhip_vp8_recon_frames_dev: pics = [dict(y, u, v, refs, mbs, coeffs)] of device tensors: refs = up to three (y, u, v) triples (or
    None) for VP8_FRAME_PREVIOUS, _GOLDEN, _ALTREF; mbs = uint8 [mb_w * mb_h * 96] MB_DTYPE records in raster order; coeffs = int16 (or
    None when nothing is coded).  The coefficients are not cleared."""
    def p(t):
        return None if t is None else t.data_ptr()
    arr = (ReconPic * len(pics))()
    for a, d in zip(arr, pics):
        a.y, a.u, a.v, a.mbs = p(d["y"]), p(d["u"]), p(d["v"]), p(d["mbs"])
        for r, tri in enumerate(d.get("refs") or ()):
            if tri is not None:
                for k in range(3):
                    a.ref[r][k] = p(tri[k])
        co = d.get("coeffs")
        a.coeffs, a.coeff_count = p(co), 0 if co is None else co.numel()
    return _lib.check(_lib.lib().ffhip_vp8_recon_frames_dev(mb_w, mb_h, bilinear, fullpel_chroma, len(pics), C.cast(arr, C.c_void_p), stride_y,
                                                            stride_uv, _st(stream)), "ffhip_vp8_recon_frames_dev")


def mb_preds(mb, mb_x, mb_y, fullpel_chroma=0):
    """ffhip_vp8_mb_preds (device-free): the put_vp8_* calls of one inter MB_DTYPE record, a PRED_DTYPE array in inter_predict()'s order"""
    rec = np.ascontiguousarray(np.asarray(mb, MB_DTYPE).reshape(1))
    out = np.zeros(24, PRED_DTYPE)
    n = _lib.check(_lib.lib().ffhip_vp8_mb_preds(rec.ctypes.data, mb_x, mb_y, fullpel_chroma, out.ctypes.data), "ffhip_vp8_mb_preds")
    return out[:n]


def intra_modes(mb, mb_x, mb_y):
    """ffhip_vp8_intra_modes (device-free): the slots intra_predict() takes for one intra MB_DTYPE record, an INTRA_MODES_DTYPE scalar"""
    rec = np.ascontiguousarray(np.asarray(mb, MB_DTYPE).reshape(1))
    out = np.zeros(1, INTRA_MODES_DTYPE)
    _lib.check(_lib.lib().ffhip_vp8_intra_modes(rec.ctypes.data, mb_x, mb_y, out.ctypes.data), "ffhip_vp8_intra_modes")
    return out[0]
