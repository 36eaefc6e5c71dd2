"""The overlap checks of the whole-picture faces at their boundaries, through the C ABI (no device needed).

Every face that refuses a call whose planes, maps or ranges share bytes answers two questions with one span set
(kernels/picture_check.h): "do two members share a byte?" and "does this span share a byte with a member?".  For each such check
of each face, at 64 x 64, 8-bit, 4:2:0 (VP8: 4 x 4 macroblocks) with one, two or forty pictures:
  - the smallest overlap is refused, in both directions (the moved span's first bytes on the other's last, and its last on the
    other's first).  That is ONE byte wherever the face lets a span start at any byte (HEVC / VP9 references, the boundary-strength
    maps); where the face first demands aligned bases (4 bytes for 8-bit planes the kernels write, 16 bytes for the residual
    ranges, which are 2-byte samples) a smaller overlap cannot reach the overlap check, and the step is that alignment's smallest;
  - spans back to back (lo == other.hi), before and behind, are accepted;
  - a long span that contains a short one is refused whichever of the two is the set member;
  - the offending pair is found among forty pictures whichever of pictures 0 and 39 holds the member;
and for the residual face, empty ranges overlap nothing and a plane without records is not looked at.

"Accepted" is observed as the other tests do: without a device the call gets past the checks to FFHIP_ENOSYS (with a device it
would run on these host buffers, so the case is skipped); the boundary-strength host face runs anywhere and returns 0."""
import ctypes as C

import pytest

from ffmpeg_amd import _lib, hevc, vp8, vp9

# Every span sits in the middle of a 64 KiB cell of its own, so one moved next to, into or around another (none is longer than
# 16 KiB) touches no third one.  The memory is real and zeroed: the boundary-strength host face reads its maps.
_CELL = 1 << 16
_NCELLS = 640
_ARENA = (C.c_uint8 * ((_NCELLS + 1) * _CELL))()
_BASE = (C.addressof(_ARENA) + _CELL - 1) & ~(_CELL - 1)
_DUMMY = _BASE + _CELL // 2              # what pointers no check looks through point to


class _Cells:
    def __init__(self):
        self.k = 1                       # cell 0 is _DUMMY's

    def __call__(self):
        assert self.k < _NCELLS
        self.k += 1
        return _BASE + (self.k - 1) * _CELL + _CELL // 2


class _Slot:
    """one span of a call: where its base pointer is kept, and how many bytes it covers"""

    def __init__(self, get, put, length):
        self.get, self.put, self.length = get, put, length


def _attr(obj, name, length):
    return _Slot(lambda: getattr(obj, name), lambda a: setattr(obj, name, a), length)


def _item(arr, k, length):
    return _Slot(lambda: arr[k], lambda a: arr.__setitem__(k, a), length)


class _Check:
    """members[i] / probes[i]: the spans of picture i in the set, and those tested against it (the members themselves where the
    check is "no two members share a byte"); move: which side of a pair the test moves (the one the face lets start anywhere)"""

    def __init__(self, members, probes, move="probe"):
        self.members, self.probes, self.move = members, probes, move

    def pair(self, member, probe):
        """(fixed, moving)"""
        assert member is not probe
        return (member, probe) if self.move == "probe" else (probe, member)


class _Call:
    def __init__(self, run, pics, checks):
        self.run, self.pics, self.checks = run, pics, checks


def _plane_len(w, h, stride=256):
    return (h - 1) * stride + w


_YUV = [_plane_len(64, 64), _plane_len(32, 32), _plane_len(32, 32)]
_void = lambda a: C.cast(a, C.c_void_p)   # noqa: E731


def _hevc_lf(n, tight):
    A, pics = _Cells(), (hevc.LfPic * n)()
    dst, src = [], []
    for i in range(n):
        P = pics[i]
        for p in range(3):
            P.plane[p] = hevc.LfPlane(A(), 256, A(), 256)
        P.bs_ver = P.bs_hor = P.qp_y = P.ctbs = _DUMMY
        P.bs_stride, P.cb_stride = 16, 8
        dst.append([_attr(P.plane[p], "dst", _YUV[p]) for p in range(3)])
        src.append([_attr(P.plane[p], "src", _YUV[p]) for p in range(3)])
    return _Call(lambda: _lib.lib().ffhip_hevc_loop_filter_pictures_dev(8, 1, 64, 64, 5, 3, n, _void(pics), None), pics,
                 {"src-dst": _Check(dst, src)})


def _hevc_inter(n, tight):
    A, pics = _Cells(), (hevc.InterPic * n)()
    dst, ref = [], []
    for i in range(n):
        P = pics[i]
        P.pus = P.pu_ctb_start = _DUMMY
        P.nslices, P.nrefs = 0, 2
        for p in range(3):
            P.plane[p] = hevc.InterPlane(A(), 256, _DUMMY, _DUMMY, _DUMMY)
            for r in range(2):
                P.ref[r].base[p], P.ref[r].stride[p] = A(), 256
        dst.append([_attr(P.plane[p], "base", _YUV[p]) for p in range(3)])
        ref.append([_item(P.ref[r].base, p, _YUV[p]) for p in range(3) for r in range(2)])
    return _Call(lambda: _lib.lib().ffhip_hevc_inter_pictures_dev(8, 1, 64, 64, 5, n, _void(pics), None), pics,
                 {"ref-dst": _Check(dst, ref)})


def _hevc_res(n, tight):
    """luma ranges of 4096 samples and chroma ranges of 1024; tight: one sample more, so that a 16-byte aligned range can lie one
    sample into another"""
    A, pics = _Cells(), (hevc.ResPic * n)()
    res, coe = [], []
    for i in range(n):
        for p in range(3):
            D = pics[i].plane[p]
            D.ncoeffs = D.nres = (1024 if p else 4096) + (1 if tight else 0)
            D.coeffs, D.res, D.tus = A(), A(), _DUMMY
            for s, v in enumerate((0, 4, 4, 4, 4)):
                D.size_start[s] = v
        res.append([_attr(pics[i].plane[p], "res", 2 * pics[i].plane[p].nres) for p in range(3)])
        coe.append([_attr(pics[i].plane[p], "coeffs", 2 * pics[i].plane[p].ncoeffs) for p in range(3)])
    return _Call(lambda: _lib.lib().ffhip_hevc_residual_pictures_dev(8, 1, n, _void(pics), None), pics,
                 {"res-res": _Check(res, res), "coeffs-res": _Check(res, coe)})


def _hevc_bs(host):
    def make(n, tight):
        A, pics = _Cells(), (hevc.BsPic * n)()
        out, inp = [], []
        for i in range(n):
            P = pics[i]
            for f in ("mvf", "tu", "ctb_slice", "slices", "ctb_tile", "bs_ver", "bs_hor"):
                setattr(P, f, A())
            P.mvf_stride = P.tu_stride = P.bs_stride = 16
            P.nslices = 1
            out.append([_attr(P, "bs_ver", 256), _attr(P, "bs_hor", 256)])
            inp.append([_attr(P, "mvf", 256 * 12), _attr(P, "tu", 256), _attr(P, "slices", 36), _attr(P, "ctb_slice", 8),
                        _attr(P, "ctb_tile", 8)])
        L = _lib.lib()
        run = (lambda: L.ffhip_hevc_boundary_strengths_pictures_host(64, 64, 5, n, _void(pics))) if host else \
              (lambda: L.ffhip_hevc_boundary_strengths_pictures_dev(64, 64, 5, n, _void(pics), None))
        # the output maps may start at any byte, the motion field may not: the tests move the outputs
        return _Call(run, pics, {"out-out": _Check(out, out), "in-out": _Check(out, inp, move="member")})
    return make


def _vp9_intra(n, tight):
    A, pics = _Cells(), (vp9.IntraPic * n)()
    planes = []
    for i in range(n):
        for p in range(3):
            pics[i].plane[p] = vp9.IntraPlane(A(), 256, _DUMMY, _DUMMY, _DUMMY)
        planes.append([_attr(pics[i].plane[p], "base", _YUV[p]) for p in range(3)])
    return _Call(lambda: _lib.lib().ffhip_vp9_intra_frames_dev(8, 1, 1, 64, 64, n, _void(pics), None), pics,
                 {"plane-plane": _Check(planes, planes)})


def _vp9_inter_fill(P, A):
    P.preds = P.pred_sb_start = _DUMMY
    P.nrefs = 2
    for p in range(3):
        P.plane[p] = vp9.InterPlane(A(), 256, _DUMMY, _DUMMY, _DUMMY)
        for r in range(2):
            P.ref[r].base[p], P.ref[r].stride[p] = A(), 256


def _vp9_inter(n, tight):
    A, pics = _Cells(), (vp9.InterPic * n)()
    dst, ref = [], []
    for i in range(n):
        _vp9_inter_fill(pics[i], A)
        dst.append([_attr(pics[i].plane[p], "base", _YUV[p]) for p in range(3)])
        ref.append([_item(pics[i].ref[r].base, p, _YUV[p]) for p in range(3) for r in range(2)])
    return _Call(lambda: _lib.lib().ffhip_vp9_inter_frames_dev(8, 1, 1, 64, 64, n, _void(pics), None), pics,
                 {"ref-dst": _Check(dst, ref)})


def _vp9_scaled(n, tight):
    """references of 32 x 32: their spans are those of their own size"""
    A, pics = _Cells(), (vp9.InterPicScaled * n)()
    small = [_plane_len(32, 32), _plane_len(16, 16), _plane_len(16, 16)]
    dst, ref = [], []
    for i in range(n):
        _vp9_inter_fill(pics[i].pic, A)
        for r in range(2):
            pics[i].ref_w[r] = pics[i].ref_h[r] = 32
        dst.append([_attr(pics[i].pic.plane[p], "base", _YUV[p]) for p in range(3)])
        ref.append([_item(pics[i].pic.ref[r].base, p, small[p]) for p in range(3) for r in range(2)])
    return _Call(lambda: _lib.lib().ffhip_vp9_inter_frames_scaled_dev(8, 1, 1, 64, 64, n, _void(pics), None), pics,
                 {"ref-dst": _Check(dst, ref)})


def _vp8_lf(n, tight):
    A, pics = _Cells(), (vp8.LfPic * n)()
    planes = []
    for i in range(n):
        pics[i] = vp8.LfPic(A(), A(), A(), _DUMMY)
        planes.append([_attr(pics[i], f, _YUV[p]) for p, f in enumerate("yuv")])
    return _Call(lambda: _lib.lib().ffhip_vp8_loopfilter_frames_dev(0, 0, 4, 4, n, _void(pics), 256, 256, None), pics,
                 {"plane-plane": _Check(planes, planes)})


def _vp8_recon(n, tight):
    """two of the three reference frames: the third's planes are NULL, which the face skips"""
    A, pics = _Cells(), (vp8.ReconPic * n)()
    dst, ref = [], []
    for i in range(n):
        P = pics[i]
        P.y, P.u, P.v = A(), A(), A()
        P.mbs, P.coeffs, P.coeff_count = _DUMMY, _DUMMY, 16
        for r in range(2):
            for p in range(3):
                P.ref[r][p] = A()
        dst.append([_attr(P, f, _YUV[p]) for p, f in enumerate("yuv")])
        ref.append([_item(P.ref[r], p, _YUV[p]) for p in range(3) for r in range(2)])
    return _Call(lambda: _lib.lib().ffhip_vp8_recon_frames_dev(4, 4, 0, 0, n, _void(pics), 256, 256, None), pics,
                 {"dst-dst": _Check(dst, dst), "ref-dst": _Check(dst, ref)})


# name: (the C function, the builder, the smallest overlap a call that passes the face's alignment checks can have per check)
_FACES = {
    "hevc_lf": (b"ffhip_hevc_loop_filter_pictures_dev", _hevc_lf, {"src-dst": 4}),
    "hevc_inter": (b"ffhip_hevc_inter_pictures_dev", _hevc_inter, {"ref-dst": 1}),
    "hevc_res": (b"ffhip_hevc_residual_pictures_dev", _hevc_res, {"res-res": 2, "coeffs-res": 2}),
    "hevc_bs_host": (b"ffhip_hevc_boundary_strengths_pictures_host", _hevc_bs(True), {"out-out": 1, "in-out": 1}),
    "hevc_bs_dev": (b"ffhip_hevc_boundary_strengths_pictures_dev", _hevc_bs(False), {"out-out": 1, "in-out": 1}),
    "vp9_intra": (b"ffhip_vp9_intra_frames_dev", _vp9_intra, {"plane-plane": 4}),
    "vp9_inter": (b"ffhip_vp9_inter_frames_dev", _vp9_inter, {"ref-dst": 1}),
    "vp9_scaled": (b"ffhip_vp9_inter_frames_scaled_dev", _vp9_scaled, {"ref-dst": 1}),
    "vp8_lf": (b"ffhip_vp8_loopfilter_frames_dev", _vp8_lf, {"plane-plane": 4}),
    "vp8_recon": (b"ffhip_vp8_recon_frames_dev", _vp8_recon, {"dst-dst": 4, "ref-dst": 4}),
}
_CHECKS = [(f, c) for f, (_, _, steps) in _FACES.items() for c in steps]
_NO_DEVICE = pytest.mark.skipif(_lib.lib().ffhip_device_count() > 0, reason="a HIP device is present: the call would run")
# the cases that end in an accepted call
_ACCEPTING = [pytest.param(f, c, marks=() if f == "hevc_bs_host" else _NO_DEVICE, id="%s-%s" % (f, c)) for f, c in _CHECKS]
_REFUSING = [pytest.param(f, c, id="%s-%s" % (f, c)) for f, c in _CHECKS]


def _make(face, n, tight=False):
    return _FACES[face][1](n, tight)


def _refused(face, call):
    """FFHIP_EINVAL, by an overlap check, in the face's name"""
    rc = call.run()
    err = _lib.lib().ffhip_last_error()
    return rc == _lib.EINVAL and b"overlap" in err and err.startswith(_FACES[face][0] + b":")


def _accepted(face, call):
    return call.run() == (0 if face == "hevc_bs_host" else _lib.ENOSYS)


def _pairs(check, n):
    """(member, probe): two spans of picture 0, and one of picture 0 with one of picture n - 1"""
    m0, m1 = check.members[0][0], check.members[0][-1]
    same = next(q for q in check.probes[0] if q is not m0)
    other = next(q for q in check.probes[n - 1] if q is not m1)
    return [(m0, same), (m1, other)]


def _put(moving, fixed, how, step=0):
    lo, hi = fixed.get(), fixed.get() + fixed.length
    if how == "tail":            # moving's first `step` bytes are fixed's last
        moving.put(hi - step)
    elif how == "head":          # moving's last `step` bytes are fixed's first
        moving.put(lo - moving.length + step)
    elif how == "behind":        # back to back
        moving.put(hi)
    elif how == "before":
        moving.put(lo - moving.length)
    else:                        # "nested": the shorter inside the longer (equal lengths: the same bytes), bases 16-byte aligned
        a = lo + (fixed.length - moving.length) // 2 // 16 * 16
        moving.put(a)
        inner, outer = sorted(((lo, hi), (a, a + moving.length)), key=lambda s: s[1] - s[0])
        assert outer[0] <= inner[0] and inner[1] <= outer[1]


@pytest.mark.parametrize("face,chk", _REFUSING)
def test_the_smallest_overlap_is_refused_in_both_directions(face, chk):
    step = _FACES[face][2][chk]
    for how in ("tail", "head"):
        for k in range(2):
            call = _make(face, 2, tight=True)
            check = call.checks[chk]
            fixed, moving = check.pair(*_pairs(check, 2)[k])
            _put(moving, fixed, how, step)
            assert _refused(face, call), (how, k, _lib.lib().ffhip_last_error())


@pytest.mark.parametrize("face,chk", _ACCEPTING)
def test_back_to_back_is_accepted(face, chk):
    assert _accepted(face, _make(face, 2)), _lib.lib().ffhip_last_error()
    for how in ("behind", "before"):
        for k in range(2):
            call = _make(face, 2)
            check = call.checks[chk]
            fixed, moving = check.pair(*_pairs(check, 2)[k])
            _put(moving, fixed, how)
            assert _accepted(face, call), (how, k, _lib.lib().ffhip_last_error())


@pytest.mark.parametrize("face,chk", _REFUSING)
def test_a_long_span_containing_a_short_one_is_refused_in_either_order(face, chk):
    """the set member is the long one (the first span of a picture: luma, the motion field) and the other the short one (the
    last: chroma, the tile map), then the reverse"""
    for member, probe in ((0, -1), (-1, 0)):
        call = _make(face, 2)
        check = call.checks[chk]
        m, q = check.members[0][member], check.probes[1][probe]
        assert (m.length >= q.length) if member == 0 else (m.length <= q.length)
        fixed, moving = check.pair(m, q)
        _put(moving, fixed, "nested")
        assert _refused(face, call), (member, probe, _lib.lib().ffhip_last_error())


@pytest.mark.parametrize("face,chk", _REFUSING)
def test_the_pair_is_found_among_forty_pictures(face, chk):
    """more pictures than any launch takes, the offending pair at the two ends of the call, in either order"""
    step = _FACES[face][2][chk]
    for mi, qi in ((0, 39), (39, 0)):
        call = _make(face, 40, tight=True)
        check = call.checks[chk]
        fixed, moving = check.pair(check.members[mi][0], check.probes[qi][-1])
        _put(moving, fixed, "tail", step)
        assert _refused(face, call), (mi, qi, _lib.lib().ffhip_last_error())


@pytest.mark.parametrize("face", [pytest.param(f, marks=() if f == "hevc_bs_host" else _NO_DEVICE) for f in _FACES])
def test_forty_clean_pictures_are_accepted(face):
    assert _accepted(face, _make(face, 40)), _lib.lib().ffhip_last_error()


def test_vp8_recon_names_the_destinations_first():
    """a destination inside a destination, with a reference on it as well: the destinations' own check comes first"""
    call = _make("vp8_recon", 2)
    dst, ref = call.checks["ref-dst"].members, call.checks["ref-dst"].probes
    _put(dst[1][1], dst[0][0], "nested")
    _put(ref[0][0], dst[0][0], "nested")
    assert call.run() == _lib.EINVAL
    assert b"two destination planes of the call overlap" in _lib.lib().ffhip_last_error()
    # and the references' check alone says so
    call = _make("vp8_recon", 2)
    _put(call.checks["ref-dst"].probes[0][0], call.checks["ref-dst"].members[0][0], "nested")
    assert call.run() == _lib.EINVAL
    assert b"a reference plane overlaps a destination plane" in _lib.lib().ffhip_last_error()


def _res_case(edit):
    call = _make("hevc_res", 2)
    edit(call.pics)
    return call


def _empty_res(pics):
    pics[0].plane[1].res = pics[0].plane[0].res + 16
    pics[0].plane[1].nres = 0


def _empty_coeffs(pics):
    pics[1].plane[2].coeffs = pics[0].plane[0].res + 16
    pics[1].plane[2].ncoeffs = 0


def _no_records(pics):
    D = pics[1].plane[0]
    for s in range(5):
        D.size_start[s] = 0
    D.res, D.coeffs, D.tus = pics[0].plane[0].res + 16, None, None


@pytest.mark.parametrize("edit", [_empty_res, _empty_coeffs, _no_records])
def test_residual_ranges_that_hold_nothing_overlap_nothing(edit):
    """a plane with nres == 0 or ncoeffs == 0 whose pointer lies inside another plane's res range, and a plane without records
    (size_start[4] == 0) whose pointers are not looked at, NULL included.  The same pointers with something behind them are
    refused (anywhere); that the empty ones are accepted shows where no device stops the call"""
    def undo(pics):
        edit(pics)
        for i in range(2):
            for p in range(3):
                D = pics[i].plane[p]
                D.nres = D.nres or 64
                D.ncoeffs = D.ncoeffs or 64
                D.size_start[4] = D.size_start[4] or 4
                D.coeffs, D.tus = D.coeffs or _DUMMY, D.tus or _DUMMY
        pics[1].plane[0].size_start[1] = pics[1].plane[0].size_start[2] = pics[1].plane[0].size_start[3] = 4
    assert _refused("hevc_res", _res_case(undo)), _lib.lib().ffhip_last_error()
    if _lib.lib().ffhip_device_count() == 0:
        assert _accepted("hevc_res", _res_case(edit)), _lib.lib().ffhip_last_error()
