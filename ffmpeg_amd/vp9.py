"""ctypes mirror of the vp9dsp inverse-transform faces of libffhip (include/ffhip.h): VP9DSPContext.itxfm_add[tx][txtp]
(libavcodec/vp9dsp.h:71-75), 8 bits."""
import ctypes as C

import numpy as np

from . import _lib

#: FFHipVp9TU (include/ffhip.h)
TU_DTYPE = np.dtype([("coeff_offset", np.int32), ("dst_offset", np.int32), ("txtp", np.uint8), ("dc_only", np.uint8), ("pad", np.uint8, 2)])
DCT_DCT, DCT_ADST, ADST_DCT, ADST_ADST = 0, 1, 2, 3
TX_4X4, TX_8X8, TX_16X16, TX_32X32, TX_WHT = 0, 1, 2, 3, 4


def _st(stream):
    return None if stream is None else C.c_void_p(stream)


def itxfm_add_batch(tx, coeffs, dst, stride, tus, n, stream=None, bit_depth=8):
    """coeffs: int16 (bit_depth 8) / int32 (10, 12) device tensor (consumed); dst: device tensor of samples; tus: uint8 [n, 12] FFHipVp9TU"""
    if bit_depth != 8:
        return _lib.check(_lib.lib().ffhip_vp9_itxfm_add_batch_dev_hbd(bit_depth, tx, coeffs.data_ptr(), dst.data_ptr(), stride, tus.data_ptr(),
                                                                       n, _st(stream)), "ffhip_vp9_itxfm_add_batch_dev_hbd")
    return _lib.check(_lib.lib().ffhip_vp9_itxfm_add_batch_dev(tx, coeffs.data_ptr(), dst.data_ptr(), stride, tus.data_ptr(), n,
                                                               None if stream is None else C.c_void_p(stream)),
                      "ffhip_vp9_itxfm_add_batch_dev")


class VP9ItxfmContext(C.Structure):
    """FFHipVP9ItxfmContext: host-pointer faces with the reference's signature"""
    _fields_ = [("itxfm_add", C.CFUNCTYPE(None, C.c_void_p, C.c_ssize_t, C.c_void_p, C.c_int) * 4 * 5)]


def dsp_init(bpp=8):
    c = VP9ItxfmContext()
    _lib.check(_lib.lib().ff_vp9dsp_itxfm_init_hip(C.byref(c), bpp), "ff_vp9dsp_itxfm_init_hip")
    return c


#: FFHipVp9McBlock (include/ffhip.h)
MC_DTYPE = np.dtype([("dst_offset", np.int32), ("src_offset", np.int32), ("width", np.uint8), ("height", np.uint8), ("filter", np.uint8),
                     ("mx", np.uint8), ("my", np.uint8), ("avg", np.uint8), ("pad", np.uint8, 2)])
FILTER_SMOOTH, FILTER_REGULAR, FILTER_SHARP, FILTER_BILINEAR = 0, 1, 2, 3


def mc_batch(dst, dststride, src, srcstride, blocks, n, stream=None, bit_depth=8):
    """blocks: uint8 [n, 16] FFHipVp9McBlock records"""
    if bit_depth != 8:
        return _lib.check(_lib.lib().ffhip_vp9_mc_batch_dev_hbd(bit_depth, dst.data_ptr(), dststride, src.data_ptr(), srcstride,
                                                                blocks.data_ptr(), n, _st(stream)), "ffhip_vp9_mc_batch_dev_hbd")
    return _lib.check(_lib.lib().ffhip_vp9_mc_batch_dev(dst.data_ptr(), dststride, src.data_ptr(), srcstride, blocks.data_ptr(), n,
                                                        None if stream is None else C.c_void_p(stream)), "ffhip_vp9_mc_batch_dev")


class VP9McContext(C.Structure):
    """FFHipVP9McContext: mc[size][filter][avg][!!mx][!!my]"""
    _fields_ = [("mc", C.CFUNCTYPE(None, C.c_void_p, C.c_ssize_t, C.c_void_p, C.c_ssize_t, C.c_int, C.c_int, C.c_int) * 2 * 2 * 2 * 4 * 5)]


def mc_init(bpp=8):
    c = VP9McContext()
    _lib.check(_lib.lib().ff_vp9dsp_mc_init_hip(C.byref(c), bpp), "ff_vp9dsp_mc_init_hip")
    return c


#: FFHipVp9Edge (include/ffhip.h)
EDGE_DTYPE = np.dtype([("offset", np.int32), ("wd_idx", np.uint8), ("dir", np.uint8), ("E", np.uint8), ("I", np.uint8), ("H", np.uint8),
                       ("pad", np.uint8, 3)])


def loop_filter_batch(base, stride, edges, n, stream=None, bit_depth=8):
    """edges: uint8 [n, 12] FFHipVp9Edge records (8-sample segments that share no sample)"""
    if bit_depth != 8:
        return _lib.check(_lib.lib().ffhip_vp9_loop_filter_batch_dev_hbd(bit_depth, base.data_ptr(), stride, edges.data_ptr(), n, _st(stream)),
                          "ffhip_vp9_loop_filter_batch_dev_hbd")
    return _lib.check(_lib.lib().ffhip_vp9_loop_filter_batch_dev(base.data_ptr(), stride, edges.data_ptr(), n,
                                                                 None if stream is None else C.c_void_p(stream)),
                      "ffhip_vp9_loop_filter_batch_dev")


def lf_sb_tables(filters, sb_cols, sb_rows, lim_lut, mblim_lut):
    """host side of the decoder-order loop filter: filters = uint8 numpy [sb_rows * sb_cols, 192] VP9Filter records in raster
    order, the frame's filter_lut (uint8 [64] each) -> uint32 numpy [sb_rows * sb_cols, 320] FFHipVp9LfSb tables (4:2:0)"""
    import numpy as np
    filters = np.ascontiguousarray(filters, np.uint8).reshape(sb_rows * sb_cols, 192)
    lim_lut, mblim_lut = np.ascontiguousarray(lim_lut, np.uint8), np.ascontiguousarray(mblim_lut, np.uint8)
    out = np.zeros((sb_rows * sb_cols, 320), np.uint32)
    L = _lib.lib()
    for r in range(sb_rows):
        for c in range(sb_cols):
            k = r * sb_cols + c
            _lib.check(L.ffhip_vp9_lf_sb_tables(out[k].ctypes.data, filters[k].ctypes.data, 8 * r, 8 * c, 1, 1, lim_lut.ctypes.data,
                                                mblim_lut.ctypes.data), "ffhip_vp9_lf_sb_tables")
    return out


def loopfilter_frame(y, u, v, stride_y, stride_uv, cols, rows, tables, stream=None, bit_depth=8, ss=(1, 1)):
    """ff_vp9_loopfilter_sb over a picture of cols x rows 8x8 blocks in the decoder's order, one launch: y / u / v device tensors,
    strides in bytes, tables = device uint32 [sb_rows * sb_cols, 320] from lf_sb_tables (sb_* = (* + 7) >> 3); ss = (ss_h, ss_v):
    (1, 1) 4:2:0, (0, 0) 4:4:4 (all planes by the luma tables)"""
    if tuple(ss) != (1, 1):
        return _lib.check(_lib.lib().ffhip_vp9_loopfilter_frame_ss_dev(bit_depth, ss[0], ss[1], y.data_ptr(), u.data_ptr(), v.data_ptr(), stride_y,
                                                                       stride_uv, cols, rows, tables.data_ptr(), _st(stream)),
                          "ffhip_vp9_loopfilter_frame_ss_dev")
    return _lib.check(_lib.lib().ffhip_vp9_loopfilter_frame_dev(bit_depth, y.data_ptr(), u.data_ptr(), v.data_ptr(), stride_y, stride_uv, cols,
                                                                rows, tables.data_ptr(), _st(stream)), "ffhip_vp9_loopfilter_frame_dev")


class LfPic(C.Structure):   # FFHipVp9LfPic (include/ffhip.h)
    _fields_ = [("y", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p), ("tables", C.c_void_p)]


def loopfilter_frames(pics, stride_y, stride_uv, cols, rows, stream=None, bit_depth=8, ss=(1, 1)):
    """ffhip_vp9_loopfilter_frames_dev: pics = [(y, u, v, tables)] device tensors of pictures that share the geometry; one launch"""
    arr = (LfPic * len(pics))(*[LfPic(y.data_ptr(), u.data_ptr(), v.data_ptr(), t.data_ptr()) for y, u, v, t in pics])
    return _lib.check(_lib.lib().ffhip_vp9_loopfilter_frames_dev(bit_depth, ss[0], ss[1], len(pics), C.cast(arr, C.c_void_p), stride_y, stride_uv, cols,
                                                                 rows, _st(stream)), "ffhip_vp9_loopfilter_frames_dev")


class LfPicC(C.Structure):   # == FFHipVp9LfPicC
    _fields_ = [("y", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p), ("tables", C.c_void_p), ("ctables", C.c_void_p)]


def loopfilter_frames_ssc(pics, stride_y, stride_uv, cols, rows, ss, stream=None, bit_depth=8):
    """ffhip_vp9_loopfilter_frames_ssc_dev: pics = [(y, u, v, tables, ctables)] of 4:2:2 / 4:4:0 pictures that share the geometry; one launch"""
    arr = (LfPicC * len(pics))(*[LfPicC(y.data_ptr(), u.data_ptr(), v.data_ptr(), t.data_ptr(), c.data_ptr()) for y, u, v, t, c in pics])
    return _lib.check(_lib.lib().ffhip_vp9_loopfilter_frames_ssc_dev(bit_depth, ss[0], ss[1], len(pics), C.cast(arr, C.c_void_p), stride_y, stride_uv,
                                                                     cols, rows, _st(stream)), "ffhip_vp9_loopfilter_frames_ssc_dev")


#: FFHipVp9LfBlock (include/ffhip.h): one decoded block.  pos = (row & 7) << 3 | (col & 7), bs = enum BlockSize (0 = 64x64 .. 12 = 4x4),
#: tx_skip = b->tx | skip_inter << 2, lvl_idx = seg_id << 3 | (intra ? 0 : ref[0] + 1) << 1 | (mode[3] != ZEROMV)
LF_BLOCK_DTYPE = np.dtype([("pos", np.uint8), ("bs", np.uint8), ("tx_skip", np.uint8), ("lvl_idx", np.uint8)])
assert LF_BLOCK_DTYPE.itemsize == 4


class LfTabPic(C.Structure):   # FFHipVp9LfTabPic (include/ffhip.h)
    _fields_ = [("blocks", C.c_void_p), ("sb_first", C.c_void_p), ("nblocks", C.c_uint32), ("level", C.c_uint8 * 64),
                ("lim_lut", C.c_uint8 * 64), ("mblim_lut", C.c_uint8 * 64), ("tables", C.c_void_p), ("ctables", C.c_void_p),
                ("filters", C.c_void_p)]


def _lf_tab_pics(pics, ptr):
    arr = (LfTabPic * max(len(pics), 1))()
    opt = lambda m, k: ptr(m[k]) if m.get(k) is not None else None
    for i, m in enumerate(pics):
        arr[i].blocks, arr[i].sb_first, arr[i].nblocks = opt(m, "blocks"), opt(m, "sb_first"), m["nblocks"]
        for k in ("level", "lim_lut", "mblim_lut"):
            getattr(arr[i], k)[:] = np.ascontiguousarray(m[k], np.uint8).reshape(64).tolist()
        arr[i].tables, arr[i].ctables, arr[i].filters = opt(m, "tables"), opt(m, "ctables"), opt(m, "filters")
    return arr


def lf_tables_pictures(pics, cols, rows, ss=(1, 1), stream=None):
    """ffhip_vp9_lf_tables_pictures_dev on npics = len(pics) pictures of cols x rows 8x8 blocks.  pics[i]: a dict with the device tensors
    blocks (LF_BLOCK_DTYPE records as bytes, a superblock's contiguous), sb_first (int32 / uint32 [sb_rows * sb_cols + 1]), the int
    nblocks, the uint8 [64] arrays level, lim_lut, mblim_lut, and the outputs tables (uint32 [n, 320]), ctables (uint32 [n, 128], when
    ss[0] != ss[1], else None) and optionally filters (uint8 [n, 192]).  tables / ctables are what loopfilter_frames() and
    loopfilter_frames_ssc() take.  Asynchronous on `stream`."""
    arr = _lf_tab_pics(pics, lambda t: t.data_ptr())
    return _lib.check(_lib.lib().ffhip_vp9_lf_tables_pictures_dev(ss[0], ss[1], cols, rows, len(pics), C.cast(arr, C.c_void_p), _st(stream)),
                      "ffhip_vp9_lf_tables_pictures_dev")


def lf_tables_pictures_host(pics, cols, rows, ss=(1, 1)):
    """ffhip_vp9_lf_tables_pictures_host (device-free): as lf_tables_pictures() with numpy arrays; the outputs are written in place."""
    arr = _lf_tab_pics(pics, lambda a: a.ctypes.data)
    return _lib.check(_lib.lib().ffhip_vp9_lf_tables_pictures_host(ss[0], ss[1], cols, rows, len(pics), C.cast(arr, C.c_void_p)),
                      "ffhip_vp9_lf_tables_pictures_host")


_LF = C.CFUNCTYPE(None, C.c_void_p, C.c_ssize_t, C.c_int, C.c_int, C.c_int)


class VP9LoopFilterContext(C.Structure):
    _fields_ = [("loop_filter_8", _LF * 2 * 3), ("loop_filter_16", _LF * 2), ("loop_filter_mix2", _LF * 2 * 2 * 2)]


def lf_init(bpp=8):
    c = VP9LoopFilterContext()
    _lib.check(_lib.lib().ff_vp9dsp_loopfilter_init_hip(C.byref(c), bpp), "ff_vp9dsp_loopfilter_init_hip")
    return c


#: FFHipVp9Intra (include/ffhip.h)
INTRA_DTYPE = np.dtype([("dst_offset", np.int32), ("edge_offset", np.int32), ("mode", np.uint8), ("pad", np.uint8, 3)])


def intra_pred_batch(tx, dst, stride, edges, blocks, n, stream=None, bit_depth=8):
    """edges: device tensor of edge lines (left[0..N-1], corner, top[0..max(N,8)-1] per block; samples of the depth); blocks: uint8 [n, 12]"""
    if bit_depth != 8:
        return _lib.check(_lib.lib().ffhip_vp9_intra_pred_batch_dev_hbd(bit_depth, tx, dst.data_ptr(), stride, edges.data_ptr(),
                                                                        blocks.data_ptr(), n, _st(stream)), "ffhip_vp9_intra_pred_batch_dev_hbd")
    return _lib.check(_lib.lib().ffhip_vp9_intra_pred_batch_dev(tx, dst.data_ptr(), stride, edges.data_ptr(), blocks.data_ptr(), n,
                                                                None if stream is None else C.c_void_p(stream)),
                      "ffhip_vp9_intra_pred_batch_dev")


class VP9IntraContext(C.Structure):
    _fields_ = [("intra_pred", C.CFUNCTYPE(None, C.c_void_p, C.c_ssize_t, C.c_void_p, C.c_void_p) * 15 * 4)]


def intra_init(bpp=8):
    c = VP9IntraContext()
    _lib.check(_lib.lib().ff_vp9dsp_intrapred_init_hip(C.byref(c), bpp), "ff_vp9dsp_intrapred_init_hip")
    return c


#: FFHipVp9ScaledBlock (include/ffhip.h)
SMC_DTYPE = np.dtype([("dst_offset", np.int32), ("src_offset", np.int32), ("width", np.uint8), ("height", np.uint8), ("filter", np.uint8),
                      ("mx", np.uint8), ("my", np.uint8), ("avg", np.uint8), ("dx", np.uint8), ("dy", np.uint8)])


def scaled_mc_batch(dst, dststride, src, srcstride, blocks, n, stream=None, bit_depth=8):
    """blocks: uint8 [n, 16] FFHipVp9ScaledBlock records"""
    if bit_depth != 8:
        return _lib.check(_lib.lib().ffhip_vp9_scaled_mc_batch_dev_hbd(bit_depth, dst.data_ptr(), dststride, src.data_ptr(), srcstride,
                                                                       blocks.data_ptr(), n, _st(stream)), "ffhip_vp9_scaled_mc_batch_dev_hbd")
    return _lib.check(_lib.lib().ffhip_vp9_scaled_mc_batch_dev(dst.data_ptr(), dststride, src.data_ptr(), srcstride, blocks.data_ptr(), n,
                                                               None if stream is None else C.c_void_p(stream)),
                      "ffhip_vp9_scaled_mc_batch_dev")


class VP9ScaledMcContext(C.Structure):
    _fields_ = [("smc", C.CFUNCTYPE(None, C.c_void_p, C.c_ssize_t, C.c_void_p, C.c_ssize_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int) * 2 * 4 * 5)]


def smc_init(bpp=8):
    c = VP9ScaledMcContext()
    _lib.check(_lib.lib().ff_vp9dsp_scaled_mc_init_hip(C.byref(c), bpp), "ff_vp9dsp_scaled_mc_init_hip")
    return c


def lf_sb_tables_ss(filters, sb_cols, sb_rows, lim_lut, mblim_lut, ss):
    """4:2:2 (ss = (1, 0)) / 4:4:0 ((0, 1)): (tables uint32 [n, 320] with the luma part filled, ctables uint32 [n, 128]) of the picture's
    superblocks (ffhip_vp9_lf_sb_tables + ffhip_vp9_lf_sb_ctables)"""
    L = _lib.lib()
    n = sb_cols * sb_rows
    out, cout = np.zeros((n, 320), np.uint32), np.zeros((n, 128), np.uint32)
    for r in range(sb_rows):
        for c in range(sb_cols):
            k = r * sb_cols + c
            _lib.check(L.ffhip_vp9_lf_sb_tables(out[k].ctypes.data, filters[k].ctypes.data, 8 * r, 8 * c, ss[0], ss[1], lim_lut.ctypes.data,
                                                mblim_lut.ctypes.data), "ffhip_vp9_lf_sb_tables")
            _lib.check(L.ffhip_vp9_lf_sb_ctables(cout[k].ctypes.data, filters[k].ctypes.data, 8 * r, 8 * c, ss[0], ss[1], lim_lut.ctypes.data,
                                                 mblim_lut.ctypes.data), "ffhip_vp9_lf_sb_ctables")
    return out, cout


def loopfilter_frame_ssc(y, u, v, stride_y, stride_uv, cols, rows, tables, ctables, ss, stream=None, bit_depth=8):
    """ffhip_vp9_loopfilter_frame_ssc_dev: a 4:2:2 / 4:4:0 picture (rectangular chroma superblocks)"""
    return _lib.check(_lib.lib().ffhip_vp9_loopfilter_frame_ssc_dev(bit_depth, ss[0], ss[1], y.data_ptr(), u.data_ptr(), v.data_ptr(), stride_y,
                                                                    stride_uv, cols, rows, tables.data_ptr(), ctables.data_ptr(), _st(stream)),
                      "ffhip_vp9_loopfilter_frame_ssc_dev")


#: FFHipVp9InterPred (include/ffhip.h): one mc_luma_dir / mc_chroma_dir call of ffhip_vp9_inter_frames_dev.  flags: bit 0 compound,
#: bit 1 chroma, bit 2 a call of the SCALED template (INTER_SCALED); ref: indices into the frame's references; box: the SCALED call's
#: clip box, [px | py << 4, log2 pw | log2 ph << 4]; mv: [ref][x, y] in eighths of a luma sample.
INTER_PRED_DTYPE = np.dtype([("x", np.uint16), ("y", np.uint16), ("w", np.uint8), ("h", np.uint8), ("filter", np.uint8), ("flags", np.uint8),
                             ("ref", np.uint8, 2), ("box", np.uint8, 2), ("mv", np.int16, (2, 2))])
#: FFHipVp9InterTU: one itxfm_add call of inter_recon; coeff_offset counts coefficients (int16 at 8 bits, int32 above).
INTER_TU_DTYPE = np.dtype([("x", np.uint16), ("y", np.uint16), ("coeff_offset", np.int32), ("tx", np.uint8), ("txtp", np.uint8),
                           ("dc_only", np.uint8), ("pad", np.uint8)])
INTER_COMP, INTER_CHROMA, INTER_SCALED = 1, 2, 4


class InterPlane(C.Structure):
    """FFHipVp9InterPlane (device pointers)"""
    _fields_ = [("base", C.c_void_p), ("stride", C.c_ssize_t), ("tus", C.c_void_p), ("tu_sb_start", C.c_void_p), ("coeffs", C.c_void_p)]


class InterRef(C.Structure):
    """FFHipVp9InterRef (device pointers, strides in bytes)"""
    _fields_ = [("base", C.c_void_p * 3), ("stride", C.c_ssize_t * 3)]


class InterPic(C.Structure):
    """FFHipVp9InterPic"""
    _fields_ = [("plane", InterPlane * 3), ("preds", C.c_void_p), ("pred_sb_start", C.c_void_p), ("nrefs", C.c_int32), ("pad", C.c_int32),
                ("ref", InterRef * 3)]


def inter_frames(pics, width, height, ss=(1, 1), stream=None, bit_depth=8):
    """ffhip_vp9_inter_frames_dev on npics = len(pics) frames of one geometry.  pics[i] = (planes, preds, pred_sb_start, refs): planes,
    three tuples (Y, Cb, Cr) of (plane, stride, tus, tu_sb_start, coeffs); preds the INTER_PRED_DTYPE records as bytes sorted by raster
    superblock, pred_sb_start the int32 superblock starts (sb_w * sb_h + 1) — device tensors; refs a list (1..3) of per-plane (plane
    tensor, stride in bytes) tuples.  ss = (ss_h, ss_v).  Asynchronous on `stream`."""
    arr = (InterPic * max(len(pics), 1))()
    for i, (planes, preds, pred_sb_start, refs) in enumerate(pics):
        for p, (plane, stride, tus, tu_sb_start, coeffs) in enumerate(planes):
            arr[i].plane[p] = InterPlane(plane.data_ptr(), stride, tus.data_ptr(), tu_sb_start.data_ptr(), coeffs.data_ptr())
        arr[i].preds, arr[i].pred_sb_start = preds.data_ptr(), pred_sb_start.data_ptr()
        arr[i].nrefs = len(refs)
        for r, ref in enumerate(refs):
            for p, (plane, stride) in enumerate(ref):
                arr[i].ref[r].base[p] = plane.data_ptr()
                arr[i].ref[r].stride[p] = stride
    return _lib.check(_lib.lib().ffhip_vp9_inter_frames_dev(bit_depth, ss[0], ss[1], width, height, len(pics), C.cast(arr, C.c_void_p),
                                                            _st(stream)), "ffhip_vp9_inter_frames_dev")


class InterPicScaled(C.Structure):
    """FFHipVp9InterPicScaled: a frame and the luma size of each of its references"""
    _fields_ = [("pic", InterPic), ("ref_w", C.c_int32 * 3), ("ref_h", C.c_int32 * 3)]


def _inter_pic(arr, planes, preds, pred_sb_start, refs):
    for p, (plane, stride, tus, tu_sb_start, coeffs) in enumerate(planes):
        arr.plane[p] = InterPlane(plane.data_ptr(), stride, tus.data_ptr(), tu_sb_start.data_ptr(), coeffs.data_ptr())
    arr.preds, arr.pred_sb_start = preds.data_ptr(), pred_sb_start.data_ptr()
    arr.nrefs = len(refs)
    for r, ref in enumerate(refs):
        for p, (plane, stride) in enumerate(ref):
            arr.ref[r].base[p] = plane.data_ptr()
            arr.ref[r].stride[p] = stride


def inter_frames_scaled(pics, ref_sizes, width, height, ss=(1, 1), stream=None, bit_depth=8):
    """ffhip_vp9_inter_frames_scaled_dev: inter_frames() with references of any valid size; ref_sizes[i] lists the luma (width,
    height) of each reference of pics[i]"""
    arr = (InterPicScaled * max(len(pics), 1))()
    for i, (planes, preds, pred_sb_start, refs) in enumerate(pics):
        _inter_pic(arr[i].pic, planes, preds, pred_sb_start, refs)
        for r, (rw, rh) in enumerate(ref_sizes[i]):
            arr[i].ref_w[r], arr[i].ref_h[r] = rw, rh
    return _lib.check(_lib.lib().ffhip_vp9_inter_frames_scaled_dev(bit_depth, ss[0], ss[1], width, height, len(pics), C.cast(arr, C.c_void_p),
                                                                   _st(stream)), "ffhip_vp9_inter_frames_scaled_dev")


def inter_block_preds_scaled(bs, row, col, mv, comp, ref, filter, ss=(1, 1)):
    """ffhip_vp9_inter_block_preds_scaled: inter_block_preds() for a block of the SCALED template (every record with INTER_SCALED and
    its clip box)"""
    out = np.zeros(8, INTER_PRED_DTYPE)
    mvs = np.ascontiguousarray(np.asarray(mv, np.int16).reshape(4, 2, 2))
    refs = np.ascontiguousarray(np.asarray(ref, np.uint8).reshape(2))
    n = _lib.check(_lib.lib().ffhip_vp9_inter_block_preds_scaled(out.ctypes.data, bs, row, col, mvs.ctypes.data, int(comp), refs.ctypes.data,
                                                                 filter, ss[0], ss[1]), "ffhip_vp9_inter_block_preds_scaled")
    return out[:n]


def inter_block_preds(bs, row, col, mv, comp, ref, filter, ss=(1, 1)):
    """ffhip_vp9_inter_block_preds: the INTER_PRED_DTYPE records of one decoded block (enum BlockSize bs, row / col in 8-sample units,
    mv = b->mv as [4][2][2], comp, ref = b->ref, filter = b->filter), in vp9_mc_template.h's call order"""
    out = np.zeros(8, INTER_PRED_DTYPE)
    mvs = np.ascontiguousarray(np.asarray(mv, np.int16).reshape(4, 2, 2))
    refs = np.ascontiguousarray(np.asarray(ref, np.uint8).reshape(2))
    n = _lib.check(_lib.lib().ffhip_vp9_inter_block_preds(out.ctypes.data, bs, row, col, mvs.ctypes.data, int(comp), refs.ctypes.data, filter,
                                                          ss[0], ss[1]), "ffhip_vp9_inter_block_preds")
    return out[:n]


#: FFHipVp9IntraRec (include/ffhip.h): one iteration of intra_recon's loops (intra_pred[tx][mode], then itxfm_add); mode is the coded
#: enum IntraPredMode 0..9, tx 4 the lossless 4x4; coeff_offset counts coefficients (int16 at 8 bits, int32 above).
INTRA_REC_DTYPE = np.dtype([("x", np.uint16), ("y", np.uint16), ("coeff_offset", np.int32), ("tx", np.uint8), ("mode", np.uint8),
                            ("txtp", np.uint8), ("flags", np.uint8)])
INTRA_RESIDUAL, INTRA_DC_ONLY, INTRA_HAVE_RIGHT = 1, 2, 4


class IntraPlane(C.Structure):
    """FFHipVp9IntraPlane (device pointers)"""
    _fields_ = [("base", C.c_void_p), ("stride", C.c_ssize_t), ("recs", C.c_void_p), ("rec_sb_start", C.c_void_p), ("coeffs", C.c_void_p)]


class IntraPic(C.Structure):
    """FFHipVp9IntraPic"""
    _fields_ = [("plane", IntraPlane * 3), ("log2_tile_cols", C.c_int32), ("pad", C.c_int32)]


def intra_frames(pics, width, height, ss=(1, 1), stream=None, bit_depth=8):
    """ffhip_vp9_intra_frames_dev on npics = len(pics) frames of one geometry.  pics[i] = (planes, log2_tile_cols): planes, three tuples
    (Y, Cb, Cr) of (plane, stride, recs, rec_sb_start, coeffs) — device tensors; recs the INTRA_REC_DTYPE records as bytes sorted by raster
    superblock (in decoding order within one), rec_sb_start the int32 superblock starts (sb_w * sb_h + 1).  ss = (ss_h, ss_v).
    Asynchronous on `stream`."""
    arr = (IntraPic * max(len(pics), 1))()
    for i, (planes, log2_tile_cols) in enumerate(pics):
        for p, (plane, stride, recs, rec_sb_start, coeffs) in enumerate(planes):
            arr[i].plane[p] = IntraPlane(plane.data_ptr(), stride, recs.data_ptr(), rec_sb_start.data_ptr(), coeffs.data_ptr())
        arr[i].log2_tile_cols = log2_tile_cols
    return _lib.check(_lib.lib().ffhip_vp9_intra_frames_dev(bit_depth, ss[0], ss[1], width, height, len(pics), C.cast(arr, C.c_void_p),
                                                            _st(stream)), "ffhip_vp9_intra_frames_dev")


def intra_block_records(plane, bs, tx, row, col, mode, skip, eob, lossless, cols, rows, ss=(1, 1)):
    """ffhip_vp9_intra_block_records: the INTRA_REC_DTYPE records of one decoded block in one plane, in intra_recon's order (plane 0:
    tx = b->tx, mode = b->mode; planes 1 / 2: tx = b->uvtx, mode = [b->uvmode]; eob[n] as intra_recon reads it; coeff_offset = 16 n)"""
    out = np.zeros(256, INTRA_REC_DTYPE)
    modes = np.zeros(4, np.uint8)
    m = np.asarray(mode, np.uint8).reshape(-1)
    modes[:len(m)] = m
    eobs = np.zeros(256, np.uint16)
    if eob is not None:
        e = np.asarray(eob, np.uint16).reshape(-1)
        eobs[:len(e)] = e
    n = _lib.check(_lib.lib().ffhip_vp9_intra_block_records(out.ctypes.data, plane, bs, tx, row, col, modes.ctypes.data, int(skip),
                                                            eobs.ctypes.data, int(lossless), cols, rows, ss[0], ss[1]),
                   "ffhip_vp9_intra_block_records")
    return out[:n]
