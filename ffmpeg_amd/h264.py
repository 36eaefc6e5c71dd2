"""Host-side mirror of the reference's H264DSPContext / H264QpelContext batch faces (device tensors)."""
import ctypes as C

import numpy as np

from . import _lib

IDCT4, IDCT8, IDCT4_DC, IDCT8_DC, ADD_PIXELS4_CLEAR, ADD_PIXELS8_CLEAR = 0, 1, 2, 3, 4, 5


def _stream(stream):
    import torch
    return torch.cuda.current_stream().cuda_stream if stream is None else stream


def idct_add_batch(kind, dst, stride, dst_offset, blocks, stream=None):
    """dst: uint8 cuda tensor (plane), dst_offset: int32 [n], blocks: int16 [n, 16|64] (zeroed on return)."""
    n = dst_offset.numel()
    return _lib.check(_lib.lib().ffhip_h264_idct_add_batch_dev(kind, dst.data_ptr(), stride, dst_offset.data_ptr(),
                                                               blocks.data_ptr(), n, _stream(stream)),
                      "ffhip_h264_idct_add_batch_dev")


def idct_add8_batch(cb, cr, stride, mb_offset, blockoffset48, blocks, nnzc, stream=None):
    """idct_add8 (4:2:0) over a batch: blocks int16 [nmb, 768] (sl->mb), nnzc uint8 [nmb, 120], blockoffset48 int32 [48]."""
    nmb = mb_offset.numel()
    return _lib.check(_lib.lib().ffhip_h264_idct_add8_batch_dev(cb.data_ptr(), cr.data_ptr(), stride, mb_offset.data_ptr(),
                                                                blockoffset48.data_ptr(), blocks.data_ptr(), nnzc.data_ptr(), nmb,
                                                                _stream(stream)), "ffhip_h264_idct_add8_batch_dev")


def luma_dc_dequant_batch(output, inp, qmul, stream=None):
    """output int16 [n, 256], inp int16 [n, 16], qmul int32 [n]"""
    n = qmul.numel()
    return _lib.check(_lib.lib().ffhip_h264_luma_dc_dequant_idct_batch_dev(output.data_ptr(), output.stride(0), inp.data_ptr(), inp.stride(0),
                                                                           qmul.data_ptr(), n, _stream(stream)),
                      "ffhip_h264_luma_dc_dequant_idct_batch_dev")


def chroma_dc_dequant_batch(blocks, block_offset, qmul, stream=None):
    """in place on blocks[block_offset[m] + {0, 16, 32, 48}]"""
    n = qmul.numel()
    return _lib.check(_lib.lib().ffhip_h264_chroma_dc_dequant_idct_batch_dev(blocks.data_ptr(), block_offset.data_ptr(), qmul.data_ptr(), n,
                                                                             _stream(stream)), "ffhip_h264_chroma_dc_dequant_idct_batch_dev")


def idct_add_mb_batch(which, dst, stride, mb_offset, blockoffset16, blocks, nnzc, stream=None):
    nmb = mb_offset.numel()
    return _lib.check(_lib.lib().ffhip_h264_idct_add_mb_batch_dev(which, dst.data_ptr(), stride, mb_offset.data_ptr(),
                                                                  blockoffset16.data_ptr(), blocks.data_ptr(),
                                                                  nnzc.data_ptr(), nmb, _stream(stream)),
                      "ffhip_h264_idct_add_mb_batch_dev")


def loop_filter_batch(base, stride, edges, n, stream=None):
    return _lib.check(_lib.lib().ffhip_h264_loop_filter_batch_dev(base.data_ptr(), stride, edges.data_ptr(), n,
                                                                  _stream(stream)), "ffhip_h264_loop_filter_batch_dev")


def deblock_frame(luma, stride, mb_w, mb_h, edges, stream=None):
    return _lib.check(_lib.lib().ffhip_h264_deblock_frame_dev(luma.data_ptr(), stride, mb_w, mb_h, edges.data_ptr(),
                                                              _stream(stream)), "ffhip_h264_deblock_frame_dev")


def deblock_frames_chroma(plane, frame_pitch, nframes, stride, mb_w, mb_h, edges, stream=None):
    """one 4:2:0 chroma plane per frame (8x8 samples per MB), decoder order; edges: uint8 [nframes * mb_w * mb_h * 4, 12]"""
    return _lib.check(_lib.lib().ffhip_h264_deblock_frames_chroma_dev(plane.data_ptr(), frame_pitch, nframes, stride, mb_w, mb_h,
                                                                      edges.data_ptr(), _stream(stream)),
                      "ffhip_h264_deblock_frames_chroma_dev")


def deblock_frames(luma, frame_pitch, nframes, stride, mb_w, mb_h, edges, stream=None):
    """nframes independent pictures in one launch (edges: nframes * mb_w*mb_h*8 records)."""
    return _lib.check(_lib.lib().ffhip_h264_deblock_frames_dev(luma.data_ptr(), frame_pitch, nframes, stride, mb_w, mb_h,
                                                               edges.data_ptr(), _stream(stream)),
                      "ffhip_h264_deblock_frames_dev")


def deblock_frames_hbd(bit_depth, plane, frame_pitch, nframes, stride, mb_w, mb_h, edges, chroma=False, stream=None):
    """frame-order deblocking at 8 / 9 / 10 / 12 / 14 bits (uint16 samples above 8; stride and frame pitch in bytes); chroma: one
    4:2:0 chroma plane per frame"""
    return _lib.check(_lib.lib().ffhip_h264_deblock_frames_dev_hbd(bit_depth, 1 if chroma else 0, plane.data_ptr(), frame_pitch, nframes, stride,
                                                                   mb_w, mb_h, edges.data_ptr(), _stream(stream)),
                      "ffhip_h264_deblock_frames_dev_hbd")


def qpel_batch(dst, src, stride, blocks, n, stream=None, pic=None):
    """blocks: uint8 [n, 16] FFHipQpelBlock records; pic = (pic_w, pic_h): the _pic form, which honours FFHIP_MC_EMU records"""
    if pic is not None:
        return _lib.check(_lib.lib().ffhip_h264_qpel_batch_dev_pic(dst.data_ptr(), src.data_ptr(), stride, pic[0], pic[1], blocks.data_ptr(),
                                                                   n, _stream(stream)), "ffhip_h264_qpel_batch_dev_pic")
    return _lib.check(_lib.lib().ffhip_h264_qpel_batch_dev(dst.data_ptr(), src.data_ptr(), stride, blocks.data_ptr(),
                                                           n, _stream(stream)), "ffhip_h264_qpel_batch_dev")


def chroma_mc_batch(dst, src, stride, blocks, n, stream=None, pic=None):
    """blocks: uint8 [n, 20] FFHipChromaBlock records; pic = (pic_w, pic_h) of the chroma plane: the _pic form (FFHIP_MC_EMU)"""
    if pic is not None:
        return _lib.check(_lib.lib().ffhip_h264_chroma_mc_batch_dev_pic(dst.data_ptr(), src.data_ptr(), stride, pic[0], pic[1], blocks.data_ptr(),
                                                                        n, _stream(stream)), "ffhip_h264_chroma_mc_batch_dev_pic")
    return _lib.check(_lib.lib().ffhip_h264_chroma_mc_batch_dev(dst.data_ptr(), src.data_ptr(), stride, blocks.data_ptr(), n,
                                                                _stream(stream)), "ffhip_h264_chroma_mc_batch_dev")


def weight_batch(dst, src, stride, blocks, n, stream=None):
    """blocks: uint8 [n, 20] FFHipWeightBlock records; src may be None when no record is a biweight"""
    return _lib.check(_lib.lib().ffhip_h264_weight_batch_dev(dst.data_ptr(), src.data_ptr() if src is not None else None, stride,
                                                             blocks.data_ptr(), n, _stream(stream)), "ffhip_h264_weight_batch_dev")


MC_PUT, MC_TMP, MC_AVG = 0, 1, 2
MC_EMU = 1   # FFHIP_MC_EMU: the record's footprint is read at clamped coordinates of the reference picture (include/ffhip.h)
#: FFHipQpelBlock / FFHipChromaBlock / FFHipWeightBlock / FFHipH264Edge (include/ffhip.h)
QPEL_DTYPE = np.dtype([("dst_offset", "<i4"), ("src_offset", "<i4"), ("mcxy", "u1"), ("size_idx", "u1"), ("avg", "u1"), ("flags", "u1"),
                       ("src_x", "<i2"), ("src_y", "<i2")])
CHROMA_DTYPE = np.dtype([("dst_offset", "<i4"), ("src_offset", "<i4"), ("w_idx", "u1"), ("h", "u1"), ("x", "u1"), ("y", "u1"), ("avg", "u1"),
                         ("flags", "u1"), ("src_x", "<i2"), ("src_y", "<i2"), ("pad", "<i2")])
WEIGHT_DTYPE = np.dtype([("dst_offset", "<i4"), ("src_offset", "<i4"), ("w_idx", "u1"), ("height", "u1"), ("log2_denom", "u1"), ("bi", "u1"),
                         ("weightd", "<i2"), ("weights", "<i2"), ("offset", "<i2"), ("pad", "<i2")])
EDGE_DTYPE = np.dtype([("offset", "<i4"), ("kind", "u1"), ("alpha", "u1"), ("beta", "u1"), ("pad", "u1"), ("tc0", "i1", (4,))])
assert QPEL_DTYPE.itemsize == 16 and CHROMA_DTYPE.itemsize == 20 and WEIGHT_DTYPE.itemsize == 20 and EDGE_DTYPE.itemsize == 12


#: FFHipH264MvField (include/ffhip.h): one 4 x 4 luma block of the motion field.  mv: [list][x, y] in quarter samples; ref_idx < 0:
#: the list is unused.
BS_MVF_DTYPE = np.dtype([("mv", np.int16, (2, 2)), ("ref_idx", np.int8, 2), ("pad", np.uint8, 2)])
#: FFHipH264BsMb: one macroblock.  nnz: bit (bx + 4 * by) per 4 x 4 luma block; flags: BS_MB_INTRA, BS_MB_T8X8.
BS_MB_DTYPE = np.dtype([("slice", np.uint16), ("nnz", np.uint16), ("qp", np.uint8), ("flags", np.uint8), ("pad", np.uint8, 2)])
#: FFHipH264BsSlice: ref[list][ref_idx] -> picture identity; the offsets are the slice header's _div2 values times 2; flags: BS_SLICE_B.
BS_SLICE_DTYPE = np.dtype([("ref", np.uint8, (2, 32)), ("num_ref", np.uint8, 2), ("alpha_c0_offset", np.int8), ("beta_offset", np.int8),
                           ("idc", np.uint8), ("flags", np.uint8), ("pad", np.uint8, 2)])
assert BS_MVF_DTYPE.itemsize == 12 and BS_MB_DTYPE.itemsize == 8 and BS_SLICE_DTYPE.itemsize == 72
BS_MB_INTRA, BS_MB_T8X8 = 1, 2
BS_SLICE_B = 1
LF_V_LUMA, LF_H_LUMA, LF_V_CHROMA, LF_H_CHROMA, LF_V_LUMA_INTRA, LF_H_LUMA_INTRA, LF_V_CHROMA_INTRA, LF_H_CHROMA_INTRA = range(8)


class BsPic(C.Structure):
    """FFHipH264BsPic"""
    _fields_ = [("mb", C.c_void_p), ("mvf", C.c_void_p), ("slices", C.c_void_p), ("chroma_qp", C.c_void_p), ("luma", C.c_void_p),
                ("cb", C.c_void_p), ("cr", C.c_void_p), ("mvf_stride", C.c_int32), ("nslices", C.c_int32)]


def _bs_pics(pics, ptr):
    arr = (BsPic * max(len(pics), 1))()
    opt = lambda m, k: ptr(m[k]) if m.get(k) is not None else None
    for i, m in enumerate(pics):
        arr[i].mb, arr[i].mvf, arr[i].slices, arr[i].luma = ptr(m["mb"]), ptr(m["mvf"]), ptr(m["slices"]), ptr(m["luma"])
        arr[i].chroma_qp, arr[i].cb, arr[i].cr = opt(m, "chroma_qp"), opt(m, "cb"), opt(m, "cr")
        arr[i].mvf_stride, arr[i].nslices = m["mvf_stride"], m["nslices"]
    return arr


def edge_params_pictures(pics, mb_w, mb_h, field=0, qp_bd_offset=0, stream=None):
    """ffhip_h264_edge_params_pictures_dev on npics = len(pics) pictures of mb_w x mb_h macroblocks.  pics[i]: a dict with the device
    tensors mb (BS_MB_DTYPE records as bytes), mvf (BS_MVF_DTYPE), slices (BS_SLICE_DTYPE), optionally chroma_qp (uint8 [2, 88]), the
    outputs luma (EDGE_DTYPE records as bytes, mb_w * mb_h * 8 of them) and optionally cb, cr (mb_w * mb_h * 4 each), and the ints
    mvf_stride (records), nslices.  luma / cb / cr are what deblock_frames(), deblock_frames_chroma() and deblock_frames_hbd() take.
    Asynchronous on `stream`."""
    arr = _bs_pics(pics, lambda t: t.data_ptr())
    return _lib.check(_lib.lib().ffhip_h264_edge_params_pictures_dev(mb_w, mb_h, field, qp_bd_offset, len(pics), C.cast(arr, C.c_void_p),
                                                                     _stream(stream)), "ffhip_h264_edge_params_pictures_dev")


def edge_params_pictures_host(pics, mb_w, mb_h, field=0, qp_bd_offset=0):
    """ffhip_h264_edge_params_pictures_host (device-free): as edge_params_pictures() with numpy arrays; luma / cb / cr are written in
    place."""
    arr = _bs_pics(pics, lambda a: a.ctypes.data)
    return _lib.check(_lib.lib().ffhip_h264_edge_params_pictures_host(mb_w, mb_h, field, qp_bd_offset, len(pics), C.cast(arr, C.c_void_p)),
                      "ffhip_h264_edge_params_pictures_host")


#: records of a macroblock in the cb / cr tables of edge_params_pictures_fmt(), by chroma_format_idc
EDGE_CHROMA_RECORDS = (0, 4, 6, 8)


def edge_params_pictures_fmt(pics, mb_w, mb_h, field=0, qp_bd_offset=0, chroma_format_idc=1, stream=None):
    """ffhip_h264_edge_params_pictures_fmt_dev: edge_params_pictures() at chroma_format_idc 0 .. 3.  cb / cr hold
    EDGE_CHROMA_RECORDS[chroma_format_idc] records per macroblock: 4:2:2 six ([mb * 6 + k]: the vertical edges x = 0, 4, then the
    horizontal y = 0, 4, 8, 12), 4:4:4 eight in luma's layout and conventions; at 0 chroma_qp / cb / cr are ignored, at 1 the bytes are
    edge_params_pictures()'s.  The tables are what deblock_pictures_fmt() takes.  Asynchronous on `stream`."""
    arr = _bs_pics(pics, lambda t: t.data_ptr())
    return _lib.check(_lib.lib().ffhip_h264_edge_params_pictures_fmt_dev(chroma_format_idc, mb_w, mb_h, field, qp_bd_offset, len(pics),
                                                                         C.cast(arr, C.c_void_p), _stream(stream)),
                      "ffhip_h264_edge_params_pictures_fmt_dev")


def edge_params_pictures_fmt_host(pics, mb_w, mb_h, field=0, qp_bd_offset=0, chroma_format_idc=1):
    """ffhip_h264_edge_params_pictures_fmt_host (device-free): as edge_params_pictures_fmt() with numpy arrays; luma / cb / cr are
    written in place."""
    arr = _bs_pics(pics, lambda a: a.ctypes.data)
    return _lib.check(_lib.lib().ffhip_h264_edge_params_pictures_fmt_host(chroma_format_idc, mb_w, mb_h, field, qp_bd_offset, len(pics),
                                                                          C.cast(arr, C.c_void_p)), "ffhip_h264_edge_params_pictures_fmt_host")


class LfPic(C.Structure):
    """FFHipH264LfPic"""
    _fields_ = [("plane", C.c_void_p * 3), ("edges", C.c_void_p * 3)]


def lf_pics(pics):
    """the FFHipH264LfPic array of deblock_pictures_fmt()'s dicts (the caller keeps the tensors)"""
    arr = (LfPic * max(len(pics), 1))()
    ptr = lambda t: None if t is None else t if isinstance(t, int) else t.data_ptr()
    for i, m in enumerate(pics):
        for p in range(3):
            arr[i].plane[p] = ptr(m["planes"][p]) if p < len(m["planes"]) else None
            arr[i].edges[p] = ptr(m["edges"][p]) if p < len(m["edges"]) else None
    return arr


def deblock_pictures_fmt(pics, mb_w, mb_h, stride_y, stride_c, bit_depth=8, chroma_format_idc=1, stream=None):
    """ffhip_h264_deblock_pictures_fmt_dev: frame-order deblocking of npics = len(pics) whole pictures at chroma_format_idc 0 .. 3.
    pics[i]: a dict with planes (up to three device tensors or addresses) and edges (their tables, the luma / cb / cr of
    edge_params_pictures_fmt(); None: the plane is not filtered).  stride_y / stride_c in bytes.  Asynchronous on `stream`."""
    arr = lf_pics(pics)
    return _lib.check(_lib.lib().ffhip_h264_deblock_pictures_fmt_dev(bit_depth, chroma_format_idc, mb_w, mb_h, stride_y, stride_c, len(pics),
                                                                     C.cast(arr, C.c_void_p), _stream(stream)),
                      "ffhip_h264_deblock_pictures_fmt_dev")


#: FFHipH264InterSlice (include/ffhip.h): what the inter face reads from a slice.  ref[list][ref_idx] -> slot of InterPic.ref;
#: luma_weight[ref_idx][list][weight, offset]; chroma_weight[ref_idx][list][Cb, Cr][weight, offset]; implicit_weight[ref_idx0][ref_idx1].
INTER_SLICE_DTYPE = np.dtype([("ref", np.uint8, (2, 32)), ("num_ref", np.uint8, 2), ("use_weight", np.uint8), ("use_weight_chroma", np.uint8),
                              ("luma_log2_denom", np.uint8), ("chroma_log2_denom", np.uint8), ("pad", np.uint8, 2),
                              ("luma_weight", np.int16, (32, 2, 2)), ("chroma_weight", np.int16, (32, 2, 2, 2)),
                              ("implicit_weight", np.int16, (32, 32))])
#: FFHipH264InterBlockPlan: how the lists of one 4 x 4 block combine (mode: INTER_SKIP .. INTER_BI_W)
INTER_PLAN_DTYPE = np.dtype([("mode", np.uint8), ("list", np.uint8), ("slot", np.uint8, 2), ("chroma_weighted", np.uint8),
                             ("luma_log2_denom", np.uint8), ("chroma_log2_denom", np.uint8), ("pad", np.uint8),
                             ("luma_weight", np.int16, 2), ("luma_offset", np.int16), ("chroma_weight", np.int16, (2, 2)),
                             ("chroma_offset", np.int16, 2), ("pad2", np.int16)])
assert INTER_SLICE_DTYPE.itemsize == 2888 and INTER_PLAN_DTYPE.itemsize == 28
INTER_SKIP, INTER_UNI, INTER_UNI_W, INTER_BI_AVG, INTER_BI_W = range(5)
INTER_PICS_PER_LAUNCH = 16


class InterRef(C.Structure):
    """FFHipH264InterRef"""
    _fields_ = [("base", C.c_void_p * 3), ("stride", C.c_ssize_t * 3), ("chroma_dy", C.c_int8), ("pad", C.c_uint8 * 7)]


class InterPic(C.Structure):
    """FFHipH264InterPic"""
    _fields_ = [("dst", C.c_void_p * 3), ("dst_stride", C.c_ssize_t * 3), ("mb", C.c_void_p), ("mvf", C.c_void_p), ("slices", C.c_void_p),
                ("mvf_stride", C.c_int32), ("nslices", C.c_int32), ("nrefs", C.c_int32), ("pad", C.c_int32), ("ref", InterRef * 32)]


class InterPlanPic(C.Structure):
    """FFHipH264InterPlanPic"""
    _fields_ = [("mb", C.c_void_p), ("mvf", C.c_void_p), ("slices", C.c_void_p), ("plans", C.c_void_p), ("mvf_stride", C.c_int32),
                ("nslices", C.c_int32), ("nrefs", C.c_int32), ("pad", C.c_int32)]


def inter_pics(pics, ptr=None):
    """the FFHipH264InterPic array of inter_pictures()'s dicts (the pointers are taken as they are: the caller keeps the tensors);
    ptr: an entry's address (default: a tensor's data_ptr(); ints are taken as they are)"""
    arr = (InterPic * max(len(pics), 1))()
    at = ptr or (lambda t: t.data_ptr())
    ptr = lambda t: None if t is None else t if isinstance(t, int) else at(t)
    for i, m in enumerate(pics):
        a = arr[i]
        for p, (t, s) in enumerate(zip(m["dst"], m["dst_stride"])):
            a.dst[p], a.dst_stride[p] = ptr(t), s
        a.mb, a.mvf, a.slices = ptr(m["mb"]), ptr(m["mvf"]), ptr(m["slices"])
        a.mvf_stride, a.nslices, a.nrefs = m["mvf_stride"], m["nslices"], len(m["refs"])
        for k, r in enumerate(m["refs"]):
            for p, (t, s) in enumerate(zip(r["base"], r["stride"])):
                a.ref[k].base[p], a.ref[k].stride[p] = ptr(t), s
            a.ref[k].chroma_dy = r.get("chroma_dy", 0)
    return arr


def inter_pictures(pics, mb_w, mb_h, bit_depth=8, chroma_format_idc=1, stream=None):
    """ffhip_h264_inter_pictures_dev on npics = len(pics) pictures of mb_w x mb_h macroblocks.  pics[i]: a dict with dst (up to three
    device tensors or addresses, Cb / Cr None for luma only) and dst_stride (bytes), the device tensors mb (BS_MB_DTYPE records as
    bytes), mvf (BS_MVF_DTYPE) and slices (INTER_SLICE_DTYPE), the ints mvf_stride (records) and nslices, and refs: at most 32 dicts
    with base (three tensors or addresses), stride (bytes) and optionally chroma_dy.  mb and mvf are the arrays edge_params_pictures()
    takes.  Asynchronous on `stream`."""
    arr = inter_pics(pics)
    return _lib.check(_lib.lib().ffhip_h264_inter_pictures_dev(bit_depth, chroma_format_idc, mb_w, mb_h, len(pics), C.cast(arr, C.c_void_p),
                                                               _stream(stream)), "ffhip_h264_inter_pictures_dev")


def inter_pictures_fmt(pics, mb_w, mb_h, bit_depth=8, chroma_format_idc=1, stream=None):
    """ffhip_h264_inter_pictures_fmt_dev: inter_pictures() at chroma_format_idc 0 .. 3 (4:2:2: chroma planes of 8 mb_w x 16 mb_h samples,
    4:4:4: of 16 mb_w x 16 mb_h); at 0 and 1 the bytes of inter_pictures().  Asynchronous on `stream`."""
    arr = inter_pics(pics)
    return _lib.check(_lib.lib().ffhip_h264_inter_pictures_fmt_dev(bit_depth, chroma_format_idc, mb_w, mb_h, len(pics), C.cast(arr, C.c_void_p),
                                                                   _stream(stream)), "ffhip_h264_inter_pictures_fmt_dev")


def inter_pictures_fmt_host(pics, mb_w, mb_h, bit_depth=8, chroma_format_idc=1):
    """ffhip_h264_inter_pictures_fmt_host (device-free): as inter_pictures_fmt() with numpy arrays (or addresses) throughout; the
    destination planes are written in place."""
    arr = inter_pics(pics, lambda a: a.ctypes.data)
    return _lib.check(_lib.lib().ffhip_h264_inter_pictures_fmt_host(bit_depth, chroma_format_idc, mb_w, mb_h, len(pics), C.cast(arr, C.c_void_p)),
                      "ffhip_h264_inter_pictures_fmt_host")


def inter_plan_host(pics, mb_w, mb_h):
    """ffhip_h264_inter_plan_pictures_host (device-free): pics[i] is a dict with the numpy arrays mb, mvf, slices, plans (INTER_PLAN_DTYPE,
    16 * mb_w * mb_h records, written in place) and the ints mvf_stride, nslices, nrefs."""
    arr = (InterPlanPic * max(len(pics), 1))()
    for i, m in enumerate(pics):
        a = arr[i]
        a.mb, a.mvf, a.slices, a.plans = (m[k].ctypes.data for k in ("mb", "mvf", "slices", "plans"))
        a.mvf_stride, a.nslices, a.nrefs = m["mvf_stride"], m["nslices"], m["nrefs"]
    return _lib.check(_lib.lib().ffhip_h264_inter_plan_pictures_host(mb_w, mb_h, len(pics), C.cast(arr, C.c_void_p)),
                      "ffhip_h264_inter_plan_pictures_host")


#: FFHipH264ResMb (include/ffhip.h): one macroblock of residual_pictures(), parallel to BS_MB_DTYPE.  coeff_offset in coefficients (a
#: multiple of 16); chroma: bit j Cb block j, bit 4 + j Cr block j; chroma_dc: bit 0 Cb, bit 1 Cr; qmul: Cb, Cr.
RES_MB_DTYPE = np.dtype([("coeff_offset", np.int32), ("chroma", np.uint8), ("chroma_dc", np.uint8), ("pad", np.uint8, 2), ("qmul", np.int32, 2)])
#: the same 16 bytes with the names the _fmt faces read: chroma_lo422 (4:2:2: bit j - 4 Cb block j = 4..7, bit 4 + (j - 4) Cr) is
#: pad[0], nnz444 (4:4:4: the low 16 bits are the non-zero bits of Cb, Cr in BS_MB_DTYPE.nnz's layout) shares qmul's bytes.
RES_MB_FMT_DTYPE = np.dtype({"names": ["coeff_offset", "chroma", "chroma_dc", "chroma_lo422", "pad", "qmul", "nnz444"],
                             "formats": [np.int32, np.uint8, np.uint8, np.uint8, np.uint8, (np.int32, 2), (np.uint32, 2)],
                             "offsets": [0, 4, 5, 6, 7, 8, 8], "itemsize": 16})
assert RES_MB_DTYPE.itemsize == 16 and RES_MB_FMT_DTYPE.itemsize == 16
RES_PICS_PER_LAUNCH = 16


class ResPic(C.Structure):
    """FFHipH264ResPic"""
    _fields_ = [("dst", C.c_void_p * 3), ("dst_stride", C.c_ssize_t * 3), ("mb", C.c_void_p), ("res", C.c_void_p), ("coeffs", C.c_void_p),
                ("ncoeffs", C.c_int64)]


def res_pics(pics, ptr):
    """the FFHipH264ResPic array of residual_pictures()'s dicts; ptr: an entry's address (ints are taken as they are)"""
    arr = (ResPic * max(len(pics), 1))()
    at = lambda t: None if t is None else t if isinstance(t, int) else ptr(t)
    for i, m in enumerate(pics):
        a = arr[i]
        for p, (t, s) in enumerate(zip(m["dst"], m["dst_stride"])):
            a.dst[p], a.dst_stride[p] = at(t), s
        a.mb, a.res, a.coeffs, a.ncoeffs = at(m["mb"]), at(m["res"]), at(m["coeffs"]), m["ncoeffs"]
    return arr


def residual_pictures(pics, mb_w, mb_h, bit_depth=8, chroma_format_idc=1, stream=None):
    """ffhip_h264_residual_pictures_dev on npics = len(pics) pictures of mb_w x mb_h macroblocks.  pics[i]: a dict with dst (up to three
    device tensors or addresses, Cb / Cr None for luma only) and dst_stride (bytes), the device tensors mb (BS_MB_DTYPE records as bytes,
    the array inter_pictures() and edge_params_pictures() take), res (RES_MB_DTYPE) and coeffs (int16 at 8 bits, int32 above, never
    written), and the int ncoeffs.  Asynchronous on `stream`."""
    arr = res_pics(pics, lambda t: t.data_ptr())
    return _lib.check(_lib.lib().ffhip_h264_residual_pictures_dev(bit_depth, chroma_format_idc, mb_w, mb_h, len(pics), C.cast(arr, C.c_void_p),
                                                                  _stream(stream)), "ffhip_h264_residual_pictures_dev")


def residual_pictures_host(pics, mb_w, mb_h, bit_depth=8, chroma_format_idc=1):
    """ffhip_h264_residual_pictures_host (device-free): as residual_pictures() with numpy arrays; the planes are written in place."""
    arr = res_pics(pics, lambda a: a.ctypes.data)
    return _lib.check(_lib.lib().ffhip_h264_residual_pictures_host(bit_depth, chroma_format_idc, mb_w, mb_h, len(pics), C.cast(arr, C.c_void_p)),
                      "ffhip_h264_residual_pictures_host")


def residual_pictures_fmt(pics, mb_w, mb_h, bit_depth=8, chroma_format_idc=1, stream=None):
    """ffhip_h264_residual_pictures_fmt_dev: residual_pictures() at chroma_format_idc 0 .. 3; res holds RES_MB_FMT_DTYPE records (the
    bytes of RES_MB_DTYPE).  At 0 and 1 the bytes of residual_pictures().  Asynchronous on `stream`."""
    arr = res_pics(pics, lambda t: t.data_ptr())
    return _lib.check(_lib.lib().ffhip_h264_residual_pictures_fmt_dev(bit_depth, chroma_format_idc, mb_w, mb_h, len(pics), C.cast(arr, C.c_void_p),
                                                                      _stream(stream)), "ffhip_h264_residual_pictures_fmt_dev")


def residual_pictures_fmt_host(pics, mb_w, mb_h, bit_depth=8, chroma_format_idc=1):
    """ffhip_h264_residual_pictures_fmt_host (device-free): as residual_pictures_fmt() with numpy arrays; the planes are written in place."""
    arr = res_pics(pics, lambda a: a.ctypes.data)
    return _lib.check(_lib.lib().ffhip_h264_residual_pictures_fmt_host(bit_depth, chroma_format_idc, mb_w, mb_h, len(pics), C.cast(arr, C.c_void_p)),
                      "ffhip_h264_residual_pictures_fmt_host")


class Picture:
    """ctypes mirror of FFHipH264Picture: record a picture's per-block dsp calls on the host, flush them as a handful of
    launches (include/ffhip.h).  Records are numpy structured scalars / arrays of the batch faces' dtypes."""

    def __init__(self, mb_w, mb_h, bit_depth=8, chroma_format=1):
        """chroma_format: sps->chroma_format_idc, 1 (4:2:0) or 3 (4:4:4: Cb / Cr through the luma members)"""
        self._p = _lib.vp()
        _lib.check(_lib.lib().ffhip_h264_picture_create_fmt(C.byref(self._p), mb_w, mb_h, bit_depth, chroma_format), "ffhip_h264_picture_create_fmt")

    def close(self):
        if getattr(self, "_p", None) is not None and self._p and _lib is not None:   # _lib is gone during interpreter shutdown
            _lib.lib().ffhip_h264_picture_free(C.byref(self._p))
        self._p = None

    __del__ = close

    def begin(self):
        _lib.lib().ffhip_h264_picture_begin(self._p)

    def mc_luma(self, stage, rec):
        return _lib.check(_lib.lib().ffhip_h264_picture_mc_luma(self._p, stage, rec.ctypes.data), "ffhip_h264_picture_mc_luma")

    def mc_luma_plane(self, plane, stage, rec):
        return _lib.check(_lib.lib().ffhip_h264_picture_mc_luma_plane(self._p, plane, stage, rec.ctypes.data), "ffhip_h264_picture_mc_luma_plane")

    def mc_chroma(self, plane, stage, rec):
        return _lib.check(_lib.lib().ffhip_h264_picture_mc_chroma(self._p, plane, stage, rec.ctypes.data), "ffhip_h264_picture_mc_chroma")

    def weight(self, plane, rec):
        return _lib.check(_lib.lib().ffhip_h264_picture_weight(self._p, plane, rec.ctypes.data), "ffhip_h264_picture_weight")

    def idct_add(self, plane, kind, dst_offset, block):
        return _lib.check(_lib.lib().ffhip_h264_picture_idct_add(self._p, plane, kind, dst_offset, block.ctypes.data),
                          "ffhip_h264_picture_idct_add")

    def intra_mb(self, rec, nnzc, mb, luma_dc=None, pcm=None):
        """rec: one FFHipH264IntraMB (numpy structured, the decoder-side fields set); nnzc: uint8[120]; mb: int16[768], consumed"""
        return _lib.check(_lib.lib().ffhip_h264_picture_intra_mb(self._p, rec.ctypes.data, None if nnzc is None else nnzc.ctypes.data,
                                                                 None if mb is None else mb.ctypes.data,
                                                                 None if luma_dc is None else luma_dc.ctypes.data,
                                                                 None if pcm is None else pcm.ctypes.data), "ffhip_h264_picture_intra_mb")

    def deblock_mb(self, plane, mb_x, mb_y, edges):
        return _lib.check(_lib.lib().ffhip_h264_picture_deblock_mb(self._p, plane, mb_x, mb_y, edges.ctypes.data),
                          "ffhip_h264_picture_deblock_mb")

    def flush(self, dst, strides, ref, stream=None):
        """dst / ref: three uint8 cuda tensors each (Y, Cb, Cr) — or device addresses as ints (a field: the frame plane's address + one
        line for the bottom field, with twice the line size as stride); strides: the row pitches in bytes"""
        ptr = lambda t: t if isinstance(t, int) else t.data_ptr()
        dp = (C.c_void_p * 3)(*[ptr(t) for t in dst])
        rp = (C.c_void_p * 3)(*[ptr(t) for t in ref])
        st = (C.c_int * 3)(*strides)
        return _lib.check(_lib.lib().ffhip_h264_picture_flush(self._p, dp, st, rp, _stream(stream)), "ffhip_h264_picture_flush")


def pictures_flush(pics, dsts, strides, refs, stream=None):
    """ffhip_h264_pictures_flush: Picture objects flushed together; dsts / refs: per picture three uint8 cuda tensors"""
    n = len(pics)
    pp = (C.c_void_p * n)(*[p._p for p in pics])
    dp = (C.c_void_p * (3 * n))(*[t.data_ptr() for d in dsts for t in d])
    rp = (C.c_void_p * (3 * n))(*[t.data_ptr() for r in refs for t in r])
    st = (C.c_int * 3)(*strides)
    return _lib.check(_lib.lib().ffhip_h264_pictures_flush(pp, n, dp, st, rp, _stream(stream)), "ffhip_h264_pictures_flush")


# ---- H264PredContext (include/ffhip.h; libavcodec/h264pred.h:92-116) ----
PRED4x4, PRED8x8L, PRED8x8, PRED16x16, PRED4x4_ADD, PRED8x8L_ADD, PRED8x8L_FILTER_ADD, PRED8x16 = range(8)
PRED_TOPLEFT, PRED_TOPRIGHT, PRED_TR_SPLAT = 1, 2, 4
CODEC_ID_H264 = 27
#: FFHipH264Pred
PRED_DTYPE = np.dtype([("offset", np.int32), ("aux", np.int32), ("mode", np.uint8), ("flags", np.uint8), ("pad", np.uint8, 2)])


def pred_batch(kind, plane, stride, blocks, n, coeffs=None, stream=None):
    """n independent blocks of one kind predicted in place; blocks: uint8 [n, 12] FFHipH264Pred records (device)"""
    return _lib.check(_lib.lib().ffhip_h264_pred_batch_dev(kind, plane.data_ptr(), stride, None if coeffs is None else coeffs.data_ptr(),
                                                           blocks.data_ptr(), n, None if stream is None else C.c_void_p(stream)),
                      "ffhip_h264_pred_batch_dev")


class H264PredContext(C.Structure):
    _fields_ = [("pred4x4", C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_ssize_t) * 15),
                ("pred8x8l", C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int, C.c_ssize_t) * 12),
                ("pred8x8", C.CFUNCTYPE(None, C.c_void_p, C.c_ssize_t) * 11),
                ("pred16x16", C.CFUNCTYPE(None, C.c_void_p, C.c_ssize_t) * 9),
                ("pred4x4_add", C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_ssize_t) * 2),
                ("pred8x8l_add", C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_ssize_t) * 2),
                ("pred8x8l_filter_add", C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_ssize_t) * 2),
                ("pred8x8_add", C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p, C.c_ssize_t) * 3),
                ("pred16x16_add", C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p, C.c_ssize_t) * 3)]


def pred_init(codec_id=CODEC_ID_H264, bit_depth=8, chroma_format_idc=1):
    h = H264PredContext()
    _lib.check(_lib.lib().ff_h264_pred_init_hip(C.byref(h), codec_id, bit_depth, chroma_format_idc), "ff_h264_pred_init_hip")
    return h
