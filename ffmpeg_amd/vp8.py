"""ctypes mirror of the vp8dsp faces of libffhip (include/ffhip.h): VP8DSPContext (libavcodec/vp8dsp.h) through ff_vp78dsp_init_hip /
ff_vp8dsp_init_hip, the batch device faces (WHT, IDCT, MC) and the whole-frame loop filter.  8 bits, the only depth VP8 has."""
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
