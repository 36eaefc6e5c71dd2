"""ctypes mirror of the hevcdsp inverse-transform faces of libffhip (include/ffhip.h): HEVCDSPContext.idct / idct_dc /
transform_4x4_luma / add_residual (libavcodec/hevc/dsp.h:46-61).  bit_depth = 8 (uint8 planes) or 10 / 12 (uint16 planes; strides and
record offsets stay in bytes): the *_hbd entry points."""
import ctypes as C

import numpy as np

from . import _lib

IDCT, IDCT_DC, DST_4X4, ADD_ONLY, DEQUANT, RDPCM_H, RDPCM_V = 0, 1, 2, 3, 4, 5, 6

#: FFHipHevcTU (include/ffhip.h)
TU_DTYPE = np.dtype([("coeff_offset", np.int32), ("dst_offset", np.int32), ("col_limit", np.int32)])


def _stream(stream):
    return None if stream is None else C.c_void_p(stream)


def idct_batch(kind, log2_size, coeffs, dst, stride, tus, n, stream=None, bit_depth=8):
    """coeffs: int16 device tensor (transformed in place); dst: uint8 / uint16 device tensor or None; tus: uint8 [n, 12] FFHipHevcTU"""
    return _lib.check(_lib.lib().ffhip_hevc_idct_batch_dev_hbd(bit_depth, kind, log2_size, coeffs.data_ptr(),
                                                               dst.data_ptr() if dst is not None else None, stride, tus.data_ptr(), n,
                                                               _stream(stream)), "ffhip_hevc_idct_batch_dev_hbd")


LF_H_LUMA, LF_V_LUMA, LF_H_CHROMA, LF_V_CHROMA = 0, 1, 2, 3

#: FFHipHevcEdge (include/ffhip.h)
EDGE_DTYPE = np.dtype([("offset", np.int32), ("kind", np.uint8), ("beta", np.uint8), ("no_p", np.uint8, 2), ("no_q", np.uint8, 2),
                       ("tc", np.int16, 2), ("pad", np.uint8, 2)])


def loop_filter_batch(base, stride, edges, n, stream=None, bit_depth=8):
    """edges: uint8 [n, 16] FFHipHevcEdge records whose pixels are disjoint (one direction of a picture per call)"""
    if bit_depth == 8:
        return _lib.check(_lib.lib().ffhip_hevc_loop_filter_batch_dev(base.data_ptr(), stride, edges.data_ptr(), n, _stream(stream)),
                          "ffhip_hevc_loop_filter_batch_dev")
    return _lib.check(_lib.lib().ffhip_hevc_loop_filter_batch_dev_hbd(bit_depth, base.data_ptr(), stride, edges.data_ptr(), n, _stream(stream)),
                      "ffhip_hevc_loop_filter_batch_dev_hbd")


#: FFHipHevcSao (include/ffhip.h)
SAO_DTYPE = np.dtype([("dst_offset", np.int32), ("src_offset", np.int32), ("offset_val", np.int16, 5), ("edge", np.uint8), ("cls", np.uint8),
                      ("width", np.uint8), ("height", np.uint8), ("pad", np.uint8, 2)])


def sao_batch(dst, stride_dst, src, stride_src, blocks, n, stream=None, bit_depth=8):
    """blocks: uint8 [n, 24] FFHipHevcSao records"""
    if bit_depth == 8:
        return _lib.check(_lib.lib().ffhip_hevc_sao_batch_dev(dst.data_ptr(), stride_dst, src.data_ptr(), stride_src, blocks.data_ptr(), n,
                                                              _stream(stream)), "ffhip_hevc_sao_batch_dev")
    return _lib.check(_lib.lib().ffhip_hevc_sao_batch_dev_hbd(bit_depth, dst.data_ptr(), stride_dst, src.data_ptr(), stride_src, blocks.data_ptr(),
                                                              n, _stream(stream)), "ffhip_hevc_sao_batch_dev_hbd")


#: FFHipHevcMcBlock (include/ffhip.h)
MC_DTYPE = np.dtype([("dst_offset", np.int32), ("src_offset", np.int32), ("width", np.uint8), ("height", np.uint8), ("mx", np.uint8),
                     ("my", np.uint8)])


def mc_batch(chroma, uni, dst, dststride, src, srcstride, blocks, n, stream=None, bit_depth=8):
    """blocks: uint8 [n, 12] FFHipHevcMcBlock records; dst: pixels (uni) or int16 (plain, rows 64 elements apart) device tensor"""
    if bit_depth == 8:
        return _lib.check(_lib.lib().ffhip_hevc_mc_batch_dev(chroma, uni, dst.data_ptr(), dststride, src.data_ptr(), srcstride, blocks.data_ptr(),
                                                             n, _stream(stream)), "ffhip_hevc_mc_batch_dev")
    return _lib.check(_lib.lib().ffhip_hevc_mc_batch_dev_hbd(bit_depth, chroma, uni, dst.data_ptr(), dststride, src.data_ptr(), srcstride,
                                                             blocks.data_ptr(), n, _stream(stream)), "ffhip_hevc_mc_batch_dev_hbd")


class SAOParams(C.Structure):
    """FFHipSAOParams == SAOParams (libavcodec/hevc/dsp.h:34-46)"""
    _fields_ = [("offset_abs", C.c_int * 4 * 3), ("offset_sign", C.c_int * 4 * 3), ("band_position", C.c_uint8 * 3), ("eo_class", C.c_int * 3),
                ("offset_val", C.c_int16 * 5 * 3), ("type_idx", C.c_uint8 * 3)]


#: FFHipHevcSaoRestore (include/ffhip.h)
RESTORE_DTYPE = np.dtype([("dst_offset", np.int32), ("src_offset", np.int32), ("offset0", np.int16), ("width", np.uint8), ("height", np.uint8),
                          ("eo", np.uint8), ("variant", np.uint8), ("borders", np.uint8), ("vert_edge", np.uint8), ("horiz_edge", np.uint8),
                          ("diag_edge", np.uint8), ("pad", np.uint8, 2)])


def sao_restore_batch(dst, stride_dst, src, stride_src, blocks, n, stream=None, bit_depth=8):
    """blocks: uint8 [n, 20] FFHipHevcSaoRestore records"""
    if bit_depth == 8:
        return _lib.check(_lib.lib().ffhip_hevc_sao_restore_batch_dev(dst.data_ptr(), stride_dst, src.data_ptr(), stride_src, blocks.data_ptr(),
                                                                      n, _stream(stream)), "ffhip_hevc_sao_restore_batch_dev")
    return _lib.check(_lib.lib().ffhip_hevc_sao_restore_batch_dev_hbd(bit_depth, dst.data_ptr(), stride_dst, src.data_ptr(), stride_src,
                                                                      blocks.data_ptr(), n, _stream(stream)), "ffhip_hevc_sao_restore_batch_dev_hbd")


MC_UNI_W, MC_BI, MC_BI_W = 2, 3, 4

#: FFHipHevcMcWBlock (include/ffhip.h)
MCW_DTYPE = np.dtype([("dst_offset", np.int32), ("src_offset", np.int32), ("src2_offset", np.int32), ("width", np.uint8), ("height", np.uint8),
                      ("mx", np.uint8), ("my", np.uint8), ("wx0", np.int16), ("wx1", np.int16), ("ox", np.int16), ("denom", np.uint8),
                      ("pad", np.uint8)])


def mc_w_batch(chroma, mode, dst, dststride, src, srcstride, src2, blocks, n, stream=None, bit_depth=8):
    """blocks: uint8 [n, 24] FFHipHevcMcWBlock records; src2: int16 device tensor (the other list's put_hevc_* output) or None for uni_w"""
    s2 = src2.data_ptr() if src2 is not None else None
    if bit_depth == 8:
        return _lib.check(_lib.lib().ffhip_hevc_mc_w_batch_dev(chroma, mode, dst.data_ptr(), dststride, src.data_ptr(), srcstride, s2,
                                                               blocks.data_ptr(), n, _stream(stream)), "ffhip_hevc_mc_w_batch_dev")
    return _lib.check(_lib.lib().ffhip_hevc_mc_w_batch_dev_hbd(bit_depth, chroma, mode, dst.data_ptr(), dststride, src.data_ptr(), srcstride, s2,
                                                               blocks.data_ptr(), n, _stream(stream)), "ffhip_hevc_mc_w_batch_dev_hbd")


_UNI_W = C.CFUNCTYPE(None, C.c_void_p, C.c_ssize_t, C.c_void_p, C.c_ssize_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_ssize_t, C.c_ssize_t, C.c_int)
_BI = C.CFUNCTYPE(None, C.c_void_p, C.c_ssize_t, C.c_void_p, C.c_ssize_t, C.c_void_p, C.c_int, C.c_ssize_t, C.c_ssize_t, C.c_int)
_BI_W = C.CFUNCTYPE(None, C.c_void_p, C.c_ssize_t, C.c_void_p, C.c_ssize_t, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_ssize_t,
                    C.c_ssize_t, C.c_int)


class HEVCDSPContext(C.Structure):
    """FFHipHEVCDSPContext: host-pointer faces with the reference's signatures"""
    _fields_ = [("add_residual", C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_ssize_t) * 4),
                ("transform_4x4_luma", C.CFUNCTYPE(None, C.c_void_p)),
                ("idct", C.CFUNCTYPE(None, C.c_void_p, C.c_int) * 4),
                ("idct_dc", C.CFUNCTYPE(None, C.c_void_p) * 4)] + \
               [(nm, C.CFUNCTYPE(None, C.c_void_p, C.c_ssize_t, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p)
                 if "luma" in nm else C.CFUNCTYPE(None, C.c_void_p, C.c_ssize_t, C.c_void_p, C.c_void_p, C.c_void_p))
                for nm in ("hevc_h_loop_filter_luma", "hevc_v_loop_filter_luma", "hevc_h_loop_filter_chroma", "hevc_v_loop_filter_chroma",
                           "hevc_h_loop_filter_luma_c", "hevc_v_loop_filter_luma_c", "hevc_h_loop_filter_chroma_c",
                           "hevc_v_loop_filter_chroma_c")] + \
               [("sao_band_filter", C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_ssize_t, C.c_ssize_t, C.c_void_p, C.c_int, C.c_int, C.c_int) * 5),
                ("sao_edge_filter", C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_ssize_t, C.c_void_p, C.c_int, C.c_int, C.c_int) * 5),
                ("put_hevc_qpel", C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_ssize_t, C.c_int, C.c_ssize_t, C.c_ssize_t, C.c_int) * 2 * 2 * 10),
                ("put_hevc_qpel_uni", C.CFUNCTYPE(None, C.c_void_p, C.c_ssize_t, C.c_void_p, C.c_ssize_t, C.c_int, C.c_ssize_t, C.c_ssize_t, C.c_int) * 2 * 2 * 10),
                ("put_hevc_epel", C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_ssize_t, C.c_int, C.c_ssize_t, C.c_ssize_t, C.c_int) * 2 * 2 * 10),
                ("put_hevc_epel_uni", C.CFUNCTYPE(None, C.c_void_p, C.c_ssize_t, C.c_void_p, C.c_ssize_t, C.c_int, C.c_ssize_t, C.c_ssize_t, C.c_int) * 2 * 2 * 10),
                ("dequant", C.CFUNCTYPE(None, C.c_void_p, C.c_int16)),
                ("transform_rdpcm", C.CFUNCTYPE(None, C.c_void_p, C.c_int16, C.c_int)),
                ("sao_edge_restore", C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_ssize_t, C.c_ssize_t, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                 C.c_int, C.c_void_p, C.c_void_p, C.c_void_p) * 2),
                ("put_hevc_qpel_uni_w", _UNI_W * 2 * 2 * 10), ("put_hevc_qpel_bi", _BI * 2 * 2 * 10), ("put_hevc_qpel_bi_w", _BI_W * 2 * 2 * 10),
                ("put_hevc_epel_uni_w", _UNI_W * 2 * 2 * 10), ("put_hevc_epel_bi", _BI * 2 * 2 * 10), ("put_hevc_epel_bi_w", _BI_W * 2 * 2 * 10)]


def dsp_init(bit_depth=8):
    c = HEVCDSPContext()
    _lib.check(_lib.lib().ff_hevc_dsp_init_hip(C.byref(c), bit_depth), "ff_hevc_dsp_init_hip")
    return c


# ---- intra prediction: HEVCPredContext (libavcodec/hevc/pred.h) and the batch face ------------------------------------------------
#: FFHipHevcIntra.flags (include/ffhip.h)
INTRA_RAW, INTRA_CORNER, INTRA_STRONG, INTRA_NO_SMOOTH, INTRA_CHROMA444 = 1, 2, 4, 8, 16

#: FFHipHevcIntra (include/ffhip.h).  The reference line at edge_offset holds 4N + 1 samples from bottom-left to top-right:
#: left[2N-1] .. left[0], the corner, top[0] .. top[2N-1].
INTRA_DTYPE = np.dtype([("dst_offset", np.int32), ("edge_offset", np.int32), ("avail_left", np.uint16), ("avail_top", np.uint16),
                        ("log2_size", np.uint8), ("mode", np.uint8), ("flags", np.uint8), ("c_idx_unit", np.uint8)])


def intra_c_idx_unit(c_idx, log2_uh=0, log2_uv=0):
    """FFHipHevcIntra.c_idx_unit: c_idx and the availability unit sizes (log2 of 1, 2 or 4 samples along the top / down the left)"""
    return c_idx | log2_uh << 2 | log2_uv << 4


def intra_batch(dst, stride, edges, blocks, n, stream=None, bit_depth=8):
    """dst: uint8 (8 bits) / uint16 device tensor; edges: device tensor of reference lines; blocks: uint8 [n, 16] FFHipHevcIntra records"""
    return _lib.check(_lib.lib().ffhip_hevc_intra_batch_dev(bit_depth, dst.data_ptr(), stride, edges.data_ptr(), blocks.data_ptr(), n,
                                                            _stream(stream)), "ffhip_hevc_intra_batch_dev")


#: FFHipHevcIntraTU (include/ffhip.h): one intra transform block of ffhip_hevc_intra_pictures_dev.  res_offset counts int16 entries
#: into its plane's residual array (N * N row-major; < 0: no residual); flags and c_idx_unit as INTRA_DTYPE (INTRA_RAW is implied).
INTRA_TU_DTYPE = np.dtype([("x", np.uint16), ("y", np.uint16), ("res_offset", np.int32), ("avail_left", np.uint16), ("avail_top", np.uint16),
                           ("log2_size", np.uint8), ("mode", np.uint8), ("flags", np.uint8), ("c_idx_unit", np.uint8)])


class IntraPlane(C.Structure):
    """FFHipHevcIntraPlane (device pointers)"""
    _fields_ = [("base", C.c_void_p), ("stride", C.c_ssize_t), ("tus", C.c_void_p), ("ctb_start", C.c_void_p), ("res", C.c_void_p)]


class IntraPic(C.Structure):
    """FFHipHevcIntraPic"""
    _fields_ = [("plane", IntraPlane * 3)]


def intra_pictures(pics, width, height, log2_ctb_size, chroma_format_idc=1, stream=None, bit_depth=8):
    """ffhip_hevc_intra_pictures_dev on npics = len(pics) pictures of one geometry.  pics[i]: one tuple per plane (1 for
    chroma_format_idc 0, else 3) of (plane, stride, tus, ctb_start, res) — device tensors but the stride (bytes): the plane (uint8 at
    8 bits, uint16 above), the INTRA_TU_DTYPE records as bytes sorted by raster CTB, the int32 CTB starts (ctb_w * ctb_h + 1) and the
    int16 residuals.  Asynchronous on `stream`: ffhip_stream_synchronize reports a lost row hand-off."""
    arr = (IntraPic * max(len(pics), 1))()
    for i, planes in enumerate(pics):
        for p, (plane, stride, tus, ctb_start, res) in enumerate(planes):
            arr[i].plane[p] = IntraPlane(plane.data_ptr(), stride, tus.data_ptr(), ctb_start.data_ptr(), res.data_ptr())
    return _lib.check(_lib.lib().ffhip_hevc_intra_pictures_dev(bit_depth, chroma_format_idc, width, height, log2_ctb_size, len(pics),
                                                               C.cast(arr, C.c_void_p), _stream(stream)), "ffhip_hevc_intra_pictures_dev")


#: FFHipHevcInterPU (include/ffhip.h): one luma prediction block of ffhip_hevc_inter_pictures_dev.  flags: bit 0 predFlagL0, bit 1
#: predFlagL1; mv: [list][x, y] in quarter luma samples; slice: index into the picture's slice table.
INTER_PU_DTYPE = np.dtype([("x", np.uint16), ("y", np.uint16), ("w", np.uint8), ("h", np.uint8), ("flags", np.uint8), ("pad", np.uint8),
                           ("ref_idx", np.uint8, 2), ("slice", np.uint16), ("mv", np.int16, (2, 2))])
#: FFHipHevcInterTU: one inter transform block of one plane; res_offset counts int16 entries into the plane's residuals (< 0: none).
INTER_TU_DTYPE = np.dtype([("x", np.uint16), ("y", np.uint16), ("res_offset", np.int32), ("log2_size", np.uint8), ("pad", np.uint8, 3)])
#: FFHipHevcInterSlice: ref[list][ref_idx] -> DPB slot; weights and offsets as hevcdec.c passes them to put_hevc_*_w.
INTER_SLICE_DTYPE = np.dtype([("ref", np.uint8, (2, 16)), ("num_ref", np.uint8, 2), ("weighted", np.uint8), ("luma_log2_denom", np.uint8),
                              ("chroma_log2_denom", np.uint8), ("pad", np.uint8, 3), ("luma_weight", np.int16, (2, 16)),
                              ("luma_offset", np.int16, (2, 16)), ("chroma_weight", np.int16, (2, 16, 2)),
                              ("chroma_offset", np.int16, (2, 16, 2))])


class InterPlane(C.Structure):
    """FFHipHevcInterPlane (device pointers)"""
    _fields_ = [("base", C.c_void_p), ("stride", C.c_ssize_t), ("tus", C.c_void_p), ("tu_ctb_start", C.c_void_p), ("res", C.c_void_p)]


class InterRef(C.Structure):
    """FFHipHevcInterRef (device pointers, strides in bytes)"""
    _fields_ = [("base", C.c_void_p * 3), ("stride", C.c_ssize_t * 3)]


class InterPic(C.Structure):
    """FFHipHevcInterPic"""
    _fields_ = [("plane", InterPlane * 3), ("pus", C.c_void_p), ("pu_ctb_start", C.c_void_p), ("slices", C.c_void_p), ("nslices", C.c_int32),
                ("nrefs", C.c_int32), ("ref", InterRef * 16)]


def inter_pictures(pics, width, height, log2_ctb_size, chroma_format_idc=1, stream=None, bit_depth=8):
    """ffhip_hevc_inter_pictures_dev on npics = len(pics) pictures of one geometry.  pics[i] = (planes, pus, pu_ctb_start, slices, refs):
    planes, one tuple per plane (1 for chroma_format_idc 0, else 3) of (plane, stride, tus, tu_ctb_start, res) as intra_pictures();
    pus the INTER_PU_DTYPE records as bytes sorted by raster CTB, pu_ctb_start the int32 CTB starts (ctb_w * ctb_h + 1), slices the
    INTER_SLICE_DTYPE table as bytes — device tensors; refs a list (the DPB slots) of per-plane (plane tensor, stride in bytes) tuples.
    Asynchronous on `stream`."""
    arr = (InterPic * max(len(pics), 1))()
    for i, (planes, pus, pu_ctb_start, slices, refs) in enumerate(pics):
        for p, (plane, stride, tus, tu_ctb_start, res) in enumerate(planes):
            arr[i].plane[p] = InterPlane(plane.data_ptr(), stride, tus.data_ptr(), tu_ctb_start.data_ptr(), res.data_ptr())
        arr[i].pus, arr[i].pu_ctb_start = pus.data_ptr(), pu_ctb_start.data_ptr()
        arr[i].slices = slices.data_ptr()
        arr[i].nslices = slices.numel() * slices.element_size() // INTER_SLICE_DTYPE.itemsize
        arr[i].nrefs = len(refs)
        for r, ref in enumerate(refs):
            for p, (plane, stride) in enumerate(ref):
                arr[i].ref[r].base[p] = plane.data_ptr()
                arr[i].ref[r].stride[p] = stride
    return _lib.check(_lib.lib().ffhip_hevc_inter_pictures_dev(bit_depth, chroma_format_idc, width, height, log2_ctb_size, len(pics),
                                                               C.cast(arr, C.c_void_p), _stream(stream)), "ffhip_hevc_inter_pictures_dev")


#: FFHipHevcLfCtb (include/ffhip.h): one CTB of ffhip_hevc_loop_filter_pictures_dev.  sao_type: 0 off, 1 band, 2 edge; sao_class:
#: band_position or eo_class; restore / vert_edge / horiz_edge / diag_edge: sao_filter_CTB's restore operands as bit sets.
LF_CTB_DTYPE = np.dtype([("beta_offset", np.int8), ("tc_offset", np.int8), ("sao_type", np.uint8, 3), ("sao_class", np.uint8, 3),
                         ("restore", np.uint8), ("vert_edge", np.uint8), ("horiz_edge", np.uint8), ("diag_edge", np.uint8),
                         ("sao_offset_val", np.int16, (3, 5)), ("pad", np.uint8, 2)])


class LfPlane(C.Structure):
    """FFHipHevcLfPlane (device pointers, strides in bytes)"""
    _fields_ = [("src", C.c_void_p), ("src_stride", C.c_ssize_t), ("dst", C.c_void_p), ("dst_stride", C.c_ssize_t)]


class LfPic(C.Structure):
    """FFHipHevcLfPic"""
    _fields_ = [("plane", LfPlane * 3), ("bs_ver", C.c_void_p), ("bs_hor", C.c_void_p), ("qp_y", C.c_void_p), ("bypass", C.c_void_p),
                ("ctbs", C.c_void_p), ("bs_stride", C.c_int32), ("cb_stride", C.c_int32), ("cb_qp_offset", C.c_int8),
                ("cr_qp_offset", C.c_int8), ("pad", C.c_uint8 * 6)]


def loop_filter_pictures(pics, width, height, log2_ctb_size, log2_min_cb_size, chroma_format_idc=1, stream=None, bit_depth=8):
    """ffhip_hevc_loop_filter_pictures_dev on npics = len(pics) pictures of one geometry.  pics[i] = (planes, maps): planes, one
    tuple per plane (1 for chroma_format_idc 0, else 3) of (src, src_stride, dst, dst_stride) — device tensors, strides in bytes;
    maps a dict with the device tensors bs_ver, bs_hor (uint8), qp_y (int8), ctbs (LF_CTB_DTYPE records as bytes), optionally
    bypass (uint8; absent or None: no bypass CUs), and the ints bs_stride, cb_stride, cb_qp_offset, cr_qp_offset.
    Asynchronous on `stream`."""
    arr = (LfPic * max(len(pics), 1))()
    for i, (planes, maps) in enumerate(pics):
        for p, (src, ss, dst, ds) in enumerate(planes):
            arr[i].plane[p] = LfPlane(src.data_ptr(), ss, dst.data_ptr(), ds)
        arr[i].bs_ver, arr[i].bs_hor = maps["bs_ver"].data_ptr(), maps["bs_hor"].data_ptr()
        arr[i].qp_y, arr[i].ctbs = maps["qp_y"].data_ptr(), maps["ctbs"].data_ptr()
        arr[i].bypass = maps["bypass"].data_ptr() if maps.get("bypass") is not None else None
        arr[i].bs_stride, arr[i].cb_stride = maps["bs_stride"], maps["cb_stride"]
        arr[i].cb_qp_offset, arr[i].cr_qp_offset = maps.get("cb_qp_offset", 0), maps.get("cr_qp_offset", 0)
    return _lib.check(_lib.lib().ffhip_hevc_loop_filter_pictures_dev(bit_depth, chroma_format_idc, width, height, log2_ctb_size,
                                                                     log2_min_cb_size, len(pics), C.cast(arr, C.c_void_p), _stream(stream)),
                      "ffhip_hevc_loop_filter_pictures_dev")


#: FFHipHevcMvField (include/ffhip.h): one 4 x 4 luma unit of the motion field.  mv: [list][x, y] in quarter samples; pred_flag: bit 0
#: L0, bit 1 L1, 0 intra.
BS_MVF_DTYPE = np.dtype([("mv", np.int16, (2, 2)), ("ref_idx", np.int8, 2), ("pred_flag", np.uint8), ("pad", np.uint8)])
#: FFHipHevcBsSlice: ref[list][ref_idx] -> DPB slot; flags: bit 0 deblocking disabled, bit 1 loop filter across slices enabled.
BS_SLICE_DTYPE = np.dtype([("ref", np.uint8, (2, 16)), ("num_ref", np.uint8, 2), ("flags", np.uint8), ("pad", np.uint8)])
BS_TU_LEFT, BS_TU_TOP, BS_TU_CBF = 1, 2, 4
BS_SLICE_DEBLOCK_OFF, BS_SLICE_ACROSS = 1, 2


class BsPic(C.Structure):
    """FFHipHevcBsPic"""
    _fields_ = [("mvf", C.c_void_p), ("tu", C.c_void_p), ("ctb_slice", C.c_void_p), ("ctb_tile", C.c_void_p), ("slices", C.c_void_p),
                ("bs_ver", C.c_void_p), ("bs_hor", C.c_void_p), ("mvf_stride", C.c_int32), ("tu_stride", C.c_int32),
                ("bs_stride", C.c_int32), ("nslices", C.c_int32), ("loop_filter_across_tiles", C.c_uint8), ("pad", C.c_uint8 * 7)]


def _bs_pics(pics, ptr):
    arr = (BsPic * max(len(pics), 1))()
    for i, m in enumerate(pics):
        arr[i].mvf, arr[i].tu, arr[i].ctb_slice, arr[i].slices = ptr(m["mvf"]), ptr(m["tu"]), ptr(m["ctb_slice"]), ptr(m["slices"])
        arr[i].ctb_tile = ptr(m["ctb_tile"]) if m.get("ctb_tile") is not None else None
        arr[i].bs_ver, arr[i].bs_hor = ptr(m["bs_ver"]), ptr(m["bs_hor"])
        arr[i].mvf_stride, arr[i].tu_stride, arr[i].bs_stride = m["mvf_stride"], m["tu_stride"], m["bs_stride"]
        arr[i].nslices, arr[i].loop_filter_across_tiles = m["nslices"], int(bool(m.get("loop_filter_across_tiles", 1)))
    return arr


def boundary_strengths_pictures(pics, width, height, log2_ctb_size, stream=None):
    """ffhip_hevc_boundary_strengths_pictures_dev on npics = len(pics) pictures of one geometry.  pics[i]: a dict with the device
    tensors mvf (BS_MVF_DTYPE records as bytes), tu (uint8), ctb_slice (uint16 as int16 or bytes), slices (BS_SLICE_DTYPE records as
    bytes), optionally ctb_tile (absent or None: one tile), the outputs bs_ver, bs_hor (uint8), and the ints mvf_stride, tu_stride,
    bs_stride (entries), nslices, loop_filter_across_tiles.  bs_ver / bs_hor / bs_stride are what loop_filter_pictures() takes.
    Asynchronous on `stream`."""
    arr = _bs_pics(pics, lambda t: t.data_ptr())
    return _lib.check(_lib.lib().ffhip_hevc_boundary_strengths_pictures_dev(width, height, log2_ctb_size, len(pics), C.cast(arr, C.c_void_p),
                                                                            _stream(stream)), "ffhip_hevc_boundary_strengths_pictures_dev")


def boundary_strengths_pictures_host(pics, width, height, log2_ctb_size):
    """ffhip_hevc_boundary_strengths_pictures_host (device-free): as boundary_strengths_pictures() with numpy arrays; bs_ver / bs_hor
    are written in place."""
    arr = _bs_pics(pics, lambda a: a.ctypes.data)
    return _lib.check(_lib.lib().ffhip_hevc_boundary_strengths_pictures_host(width, height, log2_ctb_size, len(pics), C.cast(arr, C.c_void_p)),
                      "ffhip_hevc_boundary_strengths_pictures_host")


def bs_mark_tu(tu, x0, y0, log2_size, cbf_luma):
    """ffhip_hevc_bs_mark_tu (device-free) on a 2-D uint8 numpy map of 4 x 4 units"""
    _lib.lib().ffhip_hevc_bs_mark_tu(tu.ctypes.data, tu.strides[0], x0, y0, log2_size, int(bool(cbf_luma)))


RES_DCT, RES_DC, RES_DST, RES_SKIP, RES_BYPASS, RES_ZERO = 0, 1, 2, 3, 4, 5
RES_ROTATE, RES_RDPCM_H, RES_RDPCM_V, RES_CROSS = 0x08, 0x10, 0x20, 0x40

#: FFHipHevcResTU (include/ffhip.h): one transform unit of ffhip_hevc_residual_pictures_dev; kind_flags = kind | RES_* flags
RES_TU_DTYPE = np.dtype([("coeff_offset", np.int32), ("res_offset", np.int32), ("luma", np.int32), ("log2_size", np.uint8),
                         ("kind_flags", np.uint8), ("res_scale_val", np.int8), ("col_limit", np.uint8)])


class ResPlane(C.Structure):
    """FFHipHevcResPlane (device pointers, lengths in int16 elements)"""
    _fields_ = [("coeffs", C.c_void_p), ("ncoeffs", C.c_int32), ("nres", C.c_int32), ("res", C.c_void_p), ("tus", C.c_void_p),
                ("size_start", C.c_int32 * 5), ("pad", C.c_int32)]


class ResPic(C.Structure):
    """FFHipHevcResPic"""
    _fields_ = [("plane", ResPlane * 3)]


def residual_pictures(pics, chroma_format_idc=1, stream=None, bit_depth=8):
    """ffhip_hevc_residual_pictures_dev on npics = len(pics) pictures.  pics[i]: one tuple per plane (1 for chroma_format_idc 0,
    else 3) of (coeffs, res, tus, size_start): coeffs / res int16 device tensors (their lengths are the planes' ncoeffs / nres), tus
    a device tensor of RES_TU_DTYPE records as bytes grouped by log2_size, size_start 5 ints (size 2 + s is records size_start[s] ..
    size_start[s + 1]).  Asynchronous on `stream`."""
    arr = (ResPic * max(len(pics), 1))()
    for i, planes in enumerate(pics):
        for p, (coeffs, res, tus, size_start) in enumerate(planes):
            pl = arr[i].plane[p]
            pl.coeffs, pl.ncoeffs = coeffs.data_ptr(), coeffs.numel()
            pl.res, pl.nres = res.data_ptr(), res.numel()
            pl.tus = tus.data_ptr()
            for s in range(5):
                pl.size_start[s] = int(size_start[s])
    return _lib.check(_lib.lib().ffhip_hevc_residual_pictures_dev(bit_depth, chroma_format_idc, len(pics), C.cast(arr, C.c_void_p),
                                                                  _stream(stream)), "ffhip_hevc_residual_pictures_dev")


class HEVCPredContext(C.Structure):
    """FFHipHEVCPredContext == HEVCPredContext: intra_pred[] is the decoder's and is left alone"""
    _fields_ = [("intra_pred", C.c_void_p * 4),
                ("pred_planar", C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p, C.c_ssize_t) * 4),
                ("pred_dc", C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p, C.c_ssize_t, C.c_int, C.c_int)),
                ("pred_angular", C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p, C.c_ssize_t, C.c_int, C.c_int) * 4)]


def pred_init(bit_depth=8, c=None):
    """ff_hevc_pred_init_hip on `c` (a fresh HEVCPredContext when None); raises, leaving `c` as it was, on failure"""
    c = HEVCPredContext() if c is None else c
    _lib.check(_lib.lib().ff_hevc_pred_init_hip(C.byref(c), bit_depth), "ff_hevc_pred_init_hip")
    return c
