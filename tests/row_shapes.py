"""The launch arithmetic of the row-ordered frame launchers, restated: which launches a call becomes, how many work units (rows
that one wave walks) each launch holds, and the grid it runs on.  The geometry tests (test_row_shapes_cpu.py and the
test_gpu_*_shapes.py files) take their shapes from the tables at the end and ask these functions whether a shape reaches the launcher branch
it is meant to reach, for a given number of compute units.

Nothing here is imported from the library: a launcher that changes its arithmetic must be restated here, and the tests then say
which shapes no longer reach their branch."""

SLOT_INTS = 8192      # FFHIP_PROGRESS_SLOT_INTS, ffmpeg_amd/csrc/kernels/progress_pool.h:10
V8R_PICS = 16         # V8R_PICS, ffmpeg_amd/csrc/kernels/vp8_recon_frame.hip:39
V8R_PER_CU = 8        # V8R_PER_CU, ffmpeg_amd/csrc/kernels/vp8_recon_frame.hip:40
V8F_PICS = 16         # V8F_PICS, ffmpeg_amd/csrc/kernels/vp8_lf_frame.hip:30
V8F_PER_CU = 8        # V8F_PER_CU, ffmpeg_amd/csrc/kernels/vp8_lf_frame.hip:31
HIP_PICS = 16         # HIP_PICS, ffmpeg_amd/csrc/kernels/hevc_intra_pic.hip:28
HIP_PER_CU = 8        # no constant of the launcher (it has no cap): the workgroups of k_hevc_intra_pic one CU holds, 160 KiB of LDS over
                      # 2 * 65 * 129 (T, hevc_intra_pic.hip:52) + 2 * 4 * 132 (S0, S1, :53; HI_LINE, hevc_intra_rules.h:18) bytes, rounded down
VP8_MAX_MB = 1024     # the faces' limit on mb_w and mb_h, shims_vp8_recon.hip:45 and shims_vp8.hip:274
CHUNK = 64            # records per ballot of the intra search, vp8_recon_frame.hip:318


def _split(npics, per):
    return [min(per, npics - p0) for p0 in range(0, npics, per)]


def vp8_per(mb_h, pics=V8R_PICS):
    """frames per launch: vp8_recon_frame.hip:459-460, vp8_lf_frame.hip:211-212 (a launch's counters and its ticket in one slot)"""
    return min((SLOT_INTS - 1) // mb_h, pics)


def vp8_launches(mb_h, npics, pics=V8R_PICS):
    """frames of each launch of a call: the loop at vp8_recon_frame.hip:462-463, vp8_lf_frame.hip:214-215"""
    return _split(npics, vp8_per(mb_h, pics))


def vp8_units(mb_h, npics, pics=V8R_PICS):
    """work units (frame, macroblock row) of each launch: vp8_recon_frame.hip:471, vp8_lf_frame.hip:219"""
    return [n * mb_h for n in vp8_launches(mb_h, npics, pics)]


def vp8_cap(cus, per_cu=V8R_PER_CU):
    """vp8_recon_frame.hip:461, vp8_lf_frame.hip:213"""
    return cus * per_cu


def vp8_grids(mb_h, npics, cus, pics=V8R_PICS, per_cu=V8R_PER_CU):
    """workgroups (one wave each) of each launch: vp8_recon_frame.hip:473, vp8_lf_frame.hip:221"""
    return [min(u, vp8_cap(cus, per_cu)) for u in vp8_units(mb_h, npics, pics)]


def tickets_per_wave(units, grid):
    """(the fewest, the most) tickets a wave of a launch takes if the waves share the units evenly"""
    return units // grid, -(-units // grid)


def hevc_rows(height, log2_ctb, cfi):
    """progress counters of one picture, planes x CTB rows: hevc_intra_pic.hip:196-197"""
    return (3 if cfi else 1) * ((height + (1 << log2_ctb) - 1) >> log2_ctb)


def hevc_accepted(height, log2_ctb, cfi):
    """shims_hevc_pred.hip:80-81: a picture's counters fit one slot"""
    return hevc_rows(height, log2_ctb, cfi) <= SLOT_INTS


def hevc_per(height, log2_ctb, cfi):
    """pictures per launch: hevc_intra_pic.hip:198-199"""
    return min(SLOT_INTS // hevc_rows(height, log2_ctb, cfi), HIP_PICS)


def hevc_launches(height, log2_ctb, cfi, npics):
    """pictures of each launch: the loop at hevc_intra_pic.hip:200-201"""
    return _split(npics, hevc_per(height, log2_ctb, cfi))


def hevc_units(height, log2_ctb, cfi, npics):
    """waves of each launch, the whole grid (rows, n): hevc_intra_pic.hip:207; there is no cap"""
    return [n * hevc_rows(height, log2_ctb, cfi) for n in hevc_launches(height, log2_ctb, cfi, npics)]


def hevc_resident(cus):
    return cus * HIP_PER_CU


# ---- conditions: each returns None when the shape reaches its branch, or a sentence that says why it does not --------------------
def vp8_ticket_reuse(mb_w, mb_h, npics, cus):
    """one launch in which most waves take a second ticket and some a third"""
    if mb_w < 2:
        return "mb_w %d: the x + 2 rule needs two columns" % mb_w
    units, grids = vp8_units(mb_h, npics), vp8_grids(mb_h, npics, cus)
    if len(units) != 1:
        return "%d frames of %d rows split into launches of %s frames" % (npics, mb_h, vp8_launches(mb_h, npics))
    if units[0] < 2 * vp8_cap(cus):
        return "%d units against a cap of %d waves at %d CUs: fewer than two tickets a wave" % (units[0], vp8_cap(cus), cus)
    if grids[0] != vp8_cap(cus):
        return "grid %d is not the cap %d" % (grids[0], vp8_cap(cus))
    return None


def vp8_height_split(mb_h, npics, cus, want):
    """several launches, fewer than 16 frames each, the last shorter than the others; `want`: the split the shape is meant to give"""
    per, launches = vp8_per(mb_h), vp8_launches(mb_h, npics)
    if per >= V8R_PICS:
        return "%d rows: %d frames fit a slot, the height does not split the call" % (mb_h, per)
    if launches != list(want):
        return "launches of %s frames, not %s" % (launches, list(want))
    if len(launches) < 2 or launches[-1] >= launches[0]:
        return "launches of %s frames: the last is not the shorter one" % launches
    return None


def vp8_many_tickets(mb_h, npics, cus):
    """a launch of at least two caps of units"""
    if max(vp8_units(mb_h, npics)) < 2 * vp8_cap(cus):
        return "units %s against a cap of %d waves at %d CUs" % (vp8_units(mb_h, npics), vp8_cap(cus), cus)
    return None


def hevc_split(height, log2_ctb, cfi, npics, want):
    if not hevc_accepted(height, log2_ctb, cfi):
        return "%d counters a picture: refused" % hevc_rows(height, log2_ctb, cfi)
    per, launches = hevc_per(height, log2_ctb, cfi), hevc_launches(height, log2_ctb, cfi, npics)
    if per >= HIP_PICS:
        return "%d pictures fit a slot: no split" % per
    if launches != list(want):
        return "launches of %s pictures, not %s" % (launches, list(want))
    if len(launches) < 2 or launches[-1] >= launches[0]:
        return "launches of %s pictures: the last is not the shorter one" % launches
    return None


def hevc_past_residency(height, log2_ctb, cfi, npics, cus, factor=4):
    """one launch of at least `factor` times the waves the device holds at once"""
    units = hevc_units(height, log2_ctb, cfi, npics)
    if len(units) != 1:
        return "launches of %s pictures, not one" % hevc_launches(height, log2_ctb, cfi, npics)
    if units[0] < factor * hevc_resident(cus):
        return "%d waves against %d x %d resident at %d CUs" % (units[0], factor, hevc_resident(cus), cus)
    return None


# ---- the shapes of the GPU tests ---------------------------------------------------------------------------------------------------
CHUNK_EDGE_WIDTHS = (63, 64, 65, 128, 129)      # the last record of a ballot, a full ballot, one past it, two full ballots, one past
VP8_REUSE = dict(mb_w=2, mb_h=320, npics=16)    # 5120 units in one launch: >= 2 caps up to 320 CUs (2 x 256 rows stop at 256 CUs)
VP8_SPLIT_600 = dict(mb_w=1, mb_h=600, npics=16, launches=(13, 3))
VP8_SPLIT_1024 = dict(mb_w=1, mb_h=1024, npics=8, launches=(7, 1))     # and 7168 units in the first launch
VP8_WIDEST = ((1024, 1), (1024, 2))

# height, log2_ctb, chroma_format_idc, pictures, launches
HEVC_SPLIT_420 = dict(height=8192, log2_ctb=4, cfi=1, npics=11, launches=(5, 5, 1))    # 1536 counters a picture, per 5
HEVC_SPLIT_400 = dict(height=8208, log2_ctb=4, cfi=0, npics=16, launches=(15, 1))      # 513 counters a picture, per 15
# the largest picture the face takes: 3 * 2730 = 8190 counters (3 * 2731 = 8193 is refused; 8192 itself is not a multiple of 3, and
# a 4:0:0 picture has at most 65528 / 16 -> 4096 rows, so no geometry has exactly 8192)
HEVC_LIMIT = dict(height=16 * 2730, log2_ctb=4, cfi=1)
HEVC_PAST_LIMIT = dict(height=16 * 2731, log2_ctb=4, cfi=1)
# 16 pictures of 512 rows fill the slot: 8192 waves in one launch, the most a launch can have
HEVC_RESIDENCY = dict(height=8192, log2_ctb=4, cfi=0, npics=16)


def chunk_patterns(mb_w, mb_h=3):
    """the placed frames of one chunk-edge width: [(name, {(row, column)} intra, {(row, column)} of them I4x4)].  The I4x4 frame puts
    an I4x4 macroblock in row 1 at the last column of every ballot chunk, and an intra macroblock above-right of it in row 0: the
    first record of the next chunk, where the frame is wide enough to have one."""
    assert mb_h == 3
    rows, cols = range(mb_h), range(mb_w)
    pats = [("column 0", {(r, 0) for r in rows}, set()),
            ("last column", {(r, mb_w - 1) for r in rows}, set()),
            ("every column", {(r, c) for r in rows for c in cols}, set()),
            ("inter middle row", {(r, c) for r in (0, 2) for c in cols}, set()),
            ("inter first row", {(r, c) for r in (1, 2) for c in cols}, set())]
    edge = [c for c in (CHUNK - 1, CHUNK) if c < mb_w]
    if edge:
        pats.append(("columns 63 and 64", {(r, c) for r in rows for c in edge}, set()))
    ends = list(range(CHUNK - 1, mb_w, CHUNK))
    if ends:
        pats.append(("I4x4 at a chunk's end", {(1, c) for c in ends} | {(0, c + 1) for c in ends if c + 1 < mb_w}, {(1, c) for c in ends}))
    return pats
