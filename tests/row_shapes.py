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
DB_PTRS = 32          # FFHIP_DB_PTRS, ffmpeg_amd/csrc/kernels/h264_kernels.h:78
DB_BAND_ROWS = 2048   # frames x rows above which the band kernel takes 16 rows a band, ffmpeg_amd/csrc/kernels/h264_deblock.hip:830
DB_XCD_SIMDS = 128    # the SIMDs of one XCD shared by its pictures, h264_deblock.hip:866
DB_XCDS = 8           # h264_deblock.hip:865, :870
INTRA_PICS = 32       # FFHIP_INTRA_PICS, h264_kernels.h:58
INTRA_SPLIT_WGS = 576 # workgroups up to which chroma gets a wavefront of its own, ffmpeg_amd/csrc/kernels/h264_intra.hip:404
INTRA_LDS = 64 * 1024 # the LDS a workgroup of k_h264_intra_frame may take, h264_intra.hip:393
# the workgroups of k_h264_intra_frame one CU holds AS COMPILED: the kernel keeps well over 128 vector registers a lane at either depth (a
# little over 200 when this was written; h264_intra.hip:84), so a SIMD holds 2 of its waves, a CU 8, and a workgroup has 4 (W = 4).  This is no upper bound:
# __launch_bounds__(256, 2), h264_intra.hip:86, asks the compiler to keep two workgroups a CU achievable and caps nothing, and no test
# pins the register count.  The bound that does hold is h264_intra()'s resident_bound (waves and LDS: 8 a CU at the narrow widths).
INTRA_WG_PER_CU = 2
# sizeof(ImbTileT<PIX>), ffmpeg_amd/csrc/kernels/h264_intra_mb.h:49-56: y[17 * 32] + c[2][9 * 16] samples, t8[4][64] + dcq[16] + edge[32] ints,
# zero[16] coefficients (int16_t at 8 bits, int32_t above: H264Coef, h264_tx_rules.h:23-24)
IMB_TILE = {1: 17 * 32 + 2 * 9 * 16 + 4 * (4 * 64 + 16 + 32) + 2 * 16, 2: 2 * (17 * 32 + 2 * 9 * 16) + 4 * (4 * 64 + 16 + 32) + 4 * 16}
IMB_REC = 108         # sizeof(FFHipH264IntraMB), include/ffhip.h:819-837
IMB_TABS = 2 * 12 * 16 + 4 * 32 + 9 * 64    # IMB_P4_TAB + IMB_P8_EDGE_TAB + IMB_P8_TAB, h264_intra_mb.h:234, :258, :259, :317
VP9_LF_PICS = 32      # FFHIP_VP9_LF_PICS, h264_kernels.h:135
CU_LDS = 160 * 1024   # the LDS of one CU of gfx950
CU_WAVES = 32         # the waves one CU holds at most (8 a SIMD)
VLF_ROWS_420 = 8 * 2047   # the lone 4:2:0 face's limit on rows (8x8 blocks), ffmpeg_amd/csrc/h264_api.hip:440
VLF_ROWS = 8 * 1364       # every other loop filter face's, h264_api.hip:456, :475, :489, :507


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


def _cdiv(a, b):
    return -(-a // b)


# ---- H.264 frame-order deblocking: deblock_frames(), ffmpeg_amd/csrc/kernels/h264_deblock.hip:790-894 ----------------------------
def h264_deblock(mb_w, mb_h, nf, cus=256, chroma=False, bd=8, align=16, edges_align=16, ptrs=False):
    """what deblock_frames() does with nf pictures of mb_w x mb_h macroblocks.  align: the largest power of two (up to 16) that
    divides the plane's address, the stride and the frame pitch; edges_align: the same of the edge records' address; ptrs: pictures by
    pointer table (ffhip_launch_h264_deblock_pictures_bd).  The launcher does not look at the CU count (cus is taken for symmetry).
    Returns None for a call the launcher refuses, else a dict: kernel ('skew' / 'band' / 'row'), bw, nbands, per_frame, launches
    (frames of each launch) and grids (one per launch); for skew also, per launch, wpb, per_xcd, bwaves, wgs (workgroups a picture),
    superbands and walked (the fewest, the most super-bands a workgroup of a picture walks)."""
    aligned = align % 4 == 0                                            # :808
    if chroma and not aligned:                                          # :809-812
        return None
    amask = 8 if chroma and bd == 8 else 16                             # :818
    skew = align % amask == 0 and edges_align % 16 == 0                 # :819 (no FFHIP_DEBLOCK_OLD in the product build)
    if bd > 8 and not skew:                                             # :820-823
        return None
    band = not skew and aligned                                         # :824
    bw = (8 if chroma else 4) if skew else 16 if nf * mb_h > DB_BAND_ROWS else 4     # :829-830
    nbands = _cdiv(mb_h, bw)                                            # :831
    per_frame = nbands if band or skew else mb_h + 1                    # :832
    if per_frame > SLOT_INTS or (ptrs and not skew):                    # :833-841
        return None
    per_launch = SLOT_INTS // per_frame                                 # :842
    if ptrs:
        per_launch = min(per_launch, DB_PTRS)                           # :843-844
    launches = _split(nf, per_launch)                                   # :845-846
    d = dict(kernel="skew" if skew else "band" if band else "row", bw=bw, nbands=nbands, per_frame=per_frame, per_launch=per_launch,
             launches=launches, last_band_rows=mb_h - (nbands - 1) * bw)
    if not skew:
        d["grids"] = [(nbands, n) if band else (mb_h, n) for n in launches]         # :883, :882
        d["threads"] = 64 * bw if band else 64
        return d
    wpb = 3 if bd > 8 and not chroma else 4                             # :862-864
    d.update(wpb=wpb, superbands=_cdiv(nbands, wpb), idle_waves=_cdiv(nbands, wpb) * wpb - nbands, per_xcd=[], bwaves=[], wgs=[], grids=[],
             walked=[], floor_wins=[])
    for n in launches:
        per_xcd = _cdiv(n, DB_XCDS)                                     # :865
        bwaves, floor = DB_XCD_SIMDS // per_xcd, _cdiv(nbands, 4)      # :866-867
        d["floor_wins"].append(bwaves < floor)
        bwaves = min(max(bwaves, floor), nbands)                        # :867-868
        bwaves = _cdiv(bwaves, wpb) * wpb                               # :869
        wgs = bwaves // wpb
        d["per_xcd"].append(per_xcd)
        d["bwaves"].append(bwaves)
        d["wgs"].append(wgs)
        d["grids"].append(DB_XCDS * wgs * per_xcd)                      # :870; blocks of pictures f >= n leave at once, :569-571
        d["walked"].append((d["superbands"] // wgs, _cdiv(d["superbands"], wgs)))   # :584: sb = sb0, sb0 + wgs, ...
    d["threads"] = 64 * wpb
    return d


# ---- H.264 intra pictures: ffhip_launch_h264_intra_frames_bd(), ffmpeg_amd/csrc/kernels/h264_intra.hip:358-431 ---------------------
def h264_intra_fixed(bd):
    """the static LDS of k_h264_intra_frame as the launcher counts it: h264_intra.hip:385-386 (four tiles, eight records, the coefficient
    runs 4 x 2 x NDW x 256 bytes with NDW 3 / 7, the counters, the prediction tables)"""
    ps = 2 if bd > 8 else 1
    return IMB_TILE[ps] * 4 + IMB_REC * 8 + 4 * 2 * (7 if bd > 8 else 3) * 256 + 64 + IMB_TABS * 4


def h264_intra(mb_w, mb_h, npics, cus=256, bd=8, luma_only=False):
    """None for a refused call, else W (rows a workgroup), lds (dynamic bytes), nwg, split, parts (what one workgroup set reconstructs:
    3 luma and chroma, else 1 and 2 apart), per, launches, grids [(x, y)], resident (workgroups the device holds with the kernel as
    compiled, INTRA_WG_PER_CU: not a bound) and resident_bound (the most it could hold, by 32 waves and 160 KB of LDS a CU)"""
    ps = 2 if bd > 8 else 1
    fixed, line = h264_intra_fixed(bd), mb_w * 32 * ps                  # :385-387
    W = 4
    while W > 1 and fixed + (W - 1) * line > INTRA_LDS:                 # :393-394
        W -= 1
    W = min(W, mb_h)                                                    # :395
    lds, nwg = (W - 1) * line, _cdiv(mb_h, W)                           # :396-397
    if mb_h + 1 > SLOT_INTS:                                            # :398-401
        return None
    split = not luma_only and npics * nwg * 2 <= INTRA_SPLIT_WGS        # :404
    if (mb_h + 1) * 2 > SLOT_INTS:                                      # :409-410
        split = False
    per = min(SLOT_INTS // ((mb_h + 1) * (2 if split else 1)), INTRA_PICS)         # :411-412
    launches = _split(npics, per)                                       # :413-414
    return dict(W=W, fixed=fixed, lds=lds, nwg=nwg, split=split, parts=(1,) if luma_only else (1, 2) if split else (3,), per=per,
                launches=launches, grids=[(2 * nwg if split else nwg, n) for n in launches],        # :422, :424
                resident=INTRA_WG_PER_CU * cus, resident_bound=min(CU_WAVES // W, CU_LDS // (fixed + lds)) * cus)


def h264_intra_widths(bd):
    """(the largest mb_w with W = 4, the smallest with W = 3, the smallest with W = 2) by the loop at h264_intra.hip:393-394"""
    room, ps = INTRA_LDS - h264_intra_fixed(bd), 2 if bd > 8 else 1
    return room // (3 * 32 * ps), room // (3 * 32 * ps) + 1, room // (2 * 32 * ps) + 1


# ---- VP9 loop filter of whole frames: ffmpeg_amd/csrc/kernels/vp9_lf.hip:976-1033 (wg) and :519-557 (ssc) -------------------------------
def vp9_lf(rows, npics, cus=256, bd=8, planes444=False):
    """ffhip_launch_vp9_lf_frames(): rows in 8x8 blocks.  None for a refused call, else sb_rows, per_pic, per, launches, W, nwg, grids,
    threads, lds (dynamic bytes a workgroup), wg_per_cu (by LDS alone), resident"""
    sb_rows = (rows + 7) >> 3                                           # :979
    per_pic = (3 if planes444 else 2) * sb_rows                         # :992
    if per_pic + 1 > SLOT_INTS:                                         # :993-994
        return None
    per = min((SLOT_INTS - 1) // per_pic, VP9_LF_PICS)                  # :999-1000
    launches = _split(npics, per)                                       # :1001-1002
    W = 4 if bd == 8 else 2                                             # :1017-1018
    ps, nwg = 1 if bd == 8 else 2, _cdiv(sb_rows, W)                    # :1019
    luma = (2 * (8 + W * 64) * (76 * ps // 4) + W * 256 + 2 * W) * 4    # :1020
    chroma = (4 * (8 + W * 32) * (44 * ps // 4) + W * 64 + 2 * W) * 4
    lds = (max(luma, chroma) + 15) & ~15                                # :1021
    return dict(sb_rows=sb_rows, per_pic=per_pic, per=per, launches=launches, W=W, nwg=nwg, lds=lds, threads=64 * W,
                grids=[((3 if planes444 else 2) * nwg, n) for n in launches],              # :1023, :1025
                wg_per_cu=CU_LDS // lds, resident=CU_LDS // lds * cus)


def vp9_lf_ssc(rows, npics, cus=256):
    """ffhip_launch_vp9_lf_frames_ssc() (4:2:2 / 4:4:0): one wave a superblock row and plane, vp9_lf.hip:519-557"""
    sb_rows = (rows + 7) >> 3                                           # :522
    per_pic = 3 * sb_rows                                               # :535
    if per_pic + 1 > SLOT_INTS:                                         # :536-537
        return None
    per = min((SLOT_INTS - 1) // per_pic, VP9_LF_PICS)                  # :538-539
    launches = _split(npics, per)                                       # :540-541
    return dict(sb_rows=sb_rows, per_pic=per_pic, per=per, launches=launches, grids=[(3 * sb_rows, n) for n in launches],  # :548, :550
                threads=64, resident=CU_WAVES * cus)


def vp9_lf_face_accepts(rows, lone_420):
    """the faces' limits on rows: ffmpeg_amd/csrc/h264_api.hip:440 (ffhip_vp9_loopfilter_frame_dev) and :456, :475, :489, :507"""
    return rows <= (VLF_ROWS_420 if lone_420 else VLF_ROWS)


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


def _launches_are(got, want, what="frames"):
    if got != list(want):
        return "launches of %s %s, not %s" % (got, what, list(want))
    return None


def db_superbands(g, cus, walked=4, ragged=None, idle=None):
    """the skewed-rows kernel, a lone picture whose workgroups each walk `walked` super-bands; ragged: rows of the last band; idle: the
    idle waves of the last super-band (None: not asked)"""
    d = h264_deblock(cus=cus, **g)
    if d is None or d["kernel"] != "skew":
        return "not the skewed-rows kernel: %s" % (d and d["kernel"])
    if len(d["launches"]) != 1:
        return "launches of %s frames, not one" % d["launches"]
    if d["bwaves"][0] >= d["nbands"]:
        return "%d waves for %d bands: a wave a band, no workgroup walks a second super-band" % (d["bwaves"][0], d["nbands"])
    if d["walked"][0] != (walked, walked) and idle is None or d["walked"][0][1] != walked:
        return "%d workgroups walk %s super-bands of %d, not %d" % (d["wgs"][0], d["walked"][0], d["superbands"], walked)
    if ragged is not None and d["last_band_rows"] != ragged:
        return "the last band has %d rows, not %d" % (d["last_band_rows"], ragged)
    if idle is not None and (d["idle_waves"] == 0) == bool(idle):
        return "%d bands in super-bands of %d waves: %d idle waves in the last" % (d["nbands"], d["wpb"], d["idle_waves"])
    return None


def db_floor(g, cus):
    """the floor cdiv(nbands, 4) wins over 128 / per_xcd, and some workgroups belong to no picture"""
    d = h264_deblock(cus=cus, **g)
    if d is None or d["kernel"] != "skew":
        return "not the skewed-rows kernel: %s" % (d and d["kernel"])
    if len(d["launches"]) != 1:
        return "launches of %s frames, not one" % d["launches"]
    if not d["floor_wins"][0]:
        return "%d SIMDs over %d pictures an XCD leave %d waves, the floor is only %d" % (DB_XCD_SIMDS, d["per_xcd"][0],
                                                                                        DB_XCD_SIMDS // d["per_xcd"][0], _cdiv(d["nbands"], 4))
    if d["per_xcd"][0] * DB_XCDS == d["launches"][0]:
        return "%d pictures fill %d an XCD: no workgroup is without a picture" % (d["launches"][0], d["per_xcd"][0])
    if d["walked"][0][1] < 2:
        return "no workgroup walks a second super-band"
    return None


def db_split(g, cus, want, kernel="skew"):
    """the counters of the call do not fit one slot: several launches, the last one shorter"""
    d = h264_deblock(cus=cus, **g)
    if d is None or d["kernel"] != kernel:
        return "not the %s kernel: %s" % (kernel, d and d["kernel"])
    if d["per_launch"] * d["per_frame"] > SLOT_INTS or (d["per_launch"] + 1) * d["per_frame"] <= SLOT_INTS:
        return "%d frames of %d counters: not what a slot of %d holds" % (d["per_launch"], d["per_frame"], SLOT_INTS)
    why = _launches_are(d["launches"], want)
    if why:
        return why
    if len(d["launches"]) < 2 or d["launches"][-1] >= d["launches"][0]:
        return "launches of %s frames: the last is not the shorter one" % d["launches"]
    return None


def db_ptrs(g, cus, want):
    """pictures by pointer table (ffhip_launch_h264_deblock_pictures_bd): the table of FFHIP_DB_PTRS entries, not the slot, cuts the call"""
    d = h264_deblock(cus=cus, **g)
    if not g.get("ptrs") or d is None or d["kernel"] != "skew":
        return "not the skewed-rows kernel by pointer table: %s" % (d and d["kernel"])
    if SLOT_INTS // d["per_frame"] <= DB_PTRS:
        return "%d counters a picture: a slot holds %d pictures, no more than the table's %d" % (d["per_frame"], SLOT_INTS // d["per_frame"], DB_PTRS)
    if d["per_launch"] != DB_PTRS:
        return "%d pictures a launch, not the table's %d" % (d["per_launch"], DB_PTRS)
    why = _launches_are(d["launches"], want, "pictures")
    if why:
        return why
    if len(d["launches"]) < 2 or d["launches"][-1] >= d["launches"][0]:
        return "launches of %s pictures: the last is not the shorter one" % d["launches"]
    return None


def db_hbd_wpb3(g, cus):
    d = h264_deblock(cus=cus, **g)
    if d is None or d["kernel"] != "skew":
        return "refused or not the skewed-rows kernel"
    if d["wpb"] != 3:
        return "%d waves a workgroup, not 3" % d["wpb"]
    if d["nbands"] % 3 == 0:
        return "%d bands are whole super-bands of 3" % d["nbands"]
    if d["superbands"] <= d["wgs"][0]:
        return "%d super-bands for %d workgroups: none walks a second" % (d["superbands"], d["wgs"][0])
    return None


def db_band16(g, cus, partial):
    """the band kernel with 16 rows a band, chosen by frames x rows alone"""
    d = h264_deblock(cus=cus, **g)
    if d is None or d["kernel"] != "band":
        return "not the band kernel: %s" % (d and d["kernel"])
    if d["bw"] != 16:
        return "%d frames of %d rows against %d: bands of %d rows, not 16" % (g["nf"], g["mb_h"], DB_BAND_ROWS, d["bw"])
    if len(d["launches"]) != 1:
        return "launches of %s frames, not one" % d["launches"]
    if partial and d["last_band_rows"] == 16:
        return "%d rows: the last band is whole" % g["mb_h"]
    return None


def if_unsplit(g, cus):
    """one workgroup set for luma and chroma (parts == 3) in one launch"""
    d = h264_intra(cus=cus, **g)
    if d is None:
        return "refused"
    if d["split"]:
        return "%d pictures x %d workgroups x 2 = %d <= %d: chroma keeps its own wavefront" % (g["npics"], d["nwg"], 2 * g["npics"] * d["nwg"],
                                                                                               INTRA_SPLIT_WGS)
    if len(d["launches"]) != 1:
        return "launches of %s pictures, not one" % d["launches"]
    return None


def if_height_split(g, cus, want, factor=3):
    """the height splits the call, and the first launch has `factor` times the workgroups the device holds with the kernel as compiled
    (two a CU by its register count; against the hardware's bound of eight a CU no launch of this kernel is past residency at all)"""
    d = h264_intra(cus=cus, **g)
    if d is None:
        return "refused"
    if d["per"] >= INTRA_PICS:
        return "%d pictures fit a slot: the height does not split the call" % d["per"]
    why = _launches_are(d["launches"], want, "pictures")
    if why:
        return why
    if len(d["launches"]) < 2 or d["launches"][-1] >= d["launches"][0]:
        return "launches of %s pictures: the last is not the shorter one" % d["launches"]
    wgs = d["grids"][0][0] * d["grids"][0][1]
    if wgs < factor * d["resident"]:
        return "%d workgroups against %d x %d resident (%d a CU as compiled) at %d CUs" % (wgs, factor, d["resident"], INTRA_WG_PER_CU, cus)
    return None


def if_w(g, cus, want):
    """the launcher's own sizing of W: `want` rows a workgroup, and one column less would give one more (want < 4) or this is the last
    width of W = 4"""
    d = h264_intra(cus=cus, **g)
    if d is None:
        return "refused"
    if d["W"] != want:
        return "%d macroblocks wide at %d bits: W = %d, not %d" % (g["mb_w"], g.get("bd", 8), d["W"], want)
    other = h264_intra(cus=cus, **dict(g, mb_w=g["mb_w"] + (1 if want == 4 else -1)))
    if other["W"] != (3 if want == 4 else want + 1):
        return "%d macroblocks wide is not the edge of W = %d" % (g["mb_w"], want)
    if d["fixed"] + d["lds"] > INTRA_LDS:
        return "%d + %d bytes of LDS" % (d["fixed"], d["lds"])
    return None


def vlf_split(g, cus, want, factor=2, workgroups=None):
    """ffhip_launch_vp9_lf_frames: the height splits the call, and the first launch is `factor` times what the device holds by LDS"""
    d = vp9_lf(cus=cus, **g)
    if d is None:
        return "refused"
    if d["per"] >= VP9_LF_PICS:
        return "%d pictures fit a slot: the height does not split the call" % d["per"]
    why = _launches_are(d["launches"], want, "pictures")
    if why:
        return why
    wgs = d["grids"][0][0] * d["grids"][0][1]
    if workgroups is not None and wgs != workgroups:
        return "%d workgroups in the first launch, not %d" % (wgs, workgroups)
    if wgs < factor * d["resident"]:
        return "%d workgroups against %d x %d resident (%d a CU by %d bytes of LDS) at %d CUs" % (wgs, factor, d["resident"], d["wg_per_cu"],
                                                                                                 d["lds"], cus)
    return None


def vlf_ssc_split(g, cus, want, grid):
    d = vp9_lf_ssc(cus=cus, **g)
    if d is None:
        return "refused"
    if d["per"] >= VP9_LF_PICS:
        return "%d pictures fit a slot: the height does not split the call" % d["per"]
    why = _launches_are(d["launches"], want, "pictures")
    if why:
        return why
    if d["grids"][0] != tuple(grid):
        return "a first launch of %s workgroups, not %s" % (d["grids"][0], tuple(grid))
    return None


def vlf_tallest(rows, lone_420, planes444, ssc, per):
    """the tallest picture a face takes: accepted by the face and the launcher, one more block row refused by the face"""
    if not vp9_lf_face_accepts(rows, lone_420) or vp9_lf_face_accepts(rows + 1, lone_420):
        return "%d rows is not the face's limit" % rows
    d = vp9_lf_ssc(rows, 1) if ssc else vp9_lf(rows, 1, planes444=planes444)
    if d is None:
        return "%d rows: the launcher refuses what the face accepts" % rows
    if d["per"] != per:
        return "%d pictures a launch, not %d" % (d["per"], per)
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


# H.264 deblocking: the keywords of h264_deblock()
DB_SUPERBANDS = dict(mb_w=2, mb_h=2048, nf=1)                  # 512 bands, 128 waves: 32 workgroups of 4 super-bands each
DB_SUPERBANDS_RAGGED = dict(mb_w=2, mb_h=2046, nf=1)           # and a last band of 2 rows
DB_SUPERBANDS_ODD = dict(mb_w=2, mb_h=2044, nf=1)              # 511 bands: the last super-band has an idle wave
DB_FLOOR = dict(mb_w=1, mb_h=2048, nf=9)                       # per_xcd 2: 128 / 2 = 64 < cdiv(512, 4) = 128; 7 of 16 picture places are empty
DB_SPLIT = dict(mb_w=1, mb_h=2048, nf=17)                      # 512 counters a frame, 16 a slot: launches (16, 1)
DB_SPLIT_CHROMA = dict(mb_w=1, mb_h=4096, nf=17, chroma=True, align=8)
DB_HBD_WPB3 = dict(mb_w=2, mb_h=1000, nf=1, bd=10)             # 250 bands, 84 super-bands of 3, 43 workgroups
DB_BAND16 = dict(mb_w=3, mb_h=2057, nf=1, align=4)             # stride 16 * mb_w + 4; 129 bands, the last of 9 rows
DB_BAND16_CHROMA = dict(mb_w=3, mb_h=70, nf=33, chroma=True, align=4)      # stride 8 * mb_w + 4; 33 * 70 = 2310 > 2048
DB_ROW_SPLIT = dict(mb_w=2, mb_h=600, nf=14, align=1)          # stride 16 * mb_w + 3; 601 counters a frame: launches (13, 1)
# 33 picture objects of 3 x 9 macroblocks through ffhip_h264_pictures_flush (h264_picture.hip:1423, :1427): 33 luma planes by pointer table,
# launches (32, 1), and their 66 chroma planes, launches (32, 32, 2); 3 luma bands (the last of 1 row), 2 chroma bands
DB_PTRS_SPLIT = dict(mb_w=3, mb_h=9, nf=33, ptrs=True)
DB_PTRS_SPLIT_CHROMA = dict(mb_w=3, mb_h=9, nf=66, chroma=True, align=8, ptrs=True)

# H.264 intra: the keywords of h264_intra()
IF_UNSPLIT = dict(mb_w=4, mb_h=40, npics=32)                   # 32 * 10 * 2 = 640 > 576
IF_UNSPLIT_HBD = dict(mb_w=3, mb_h=40, npics=32, bd=10)
IF_HEIGHT_SPLIT = dict(mb_w=2, mb_h=256, npics=32)             # 8192 // 257 = 31: launches (31, 1), 31 * 64 = 1984 workgroups
# (bit depth, W) -> mb_w: the last width of W = 4, the first of W = 3 and of W = 2 (h264_intra_widths)
IF_WIDTHS = {(10, 4): 177, (10, 3): 178, (10, 2): 267, (8, 4): 477, (8, 3): 478, (8, 2): 716}
IF_W_ROWS, IF_W_PICS = 9, 2

# VP9 loop filter: rows in 8x8 blocks; the keywords of vp9_lf() / vp9_lf_ssc()
VLF_SPLIT_420 = dict(rows=8 * 128 - 3, npics=32)               # 128 superblock rows, 256 counters: 8191 // 256 = 31
VLF_SPLIT_420_HBD = dict(rows=8 * 128 - 3, npics=32, bd=10)
VLF_SPLIT_444 = dict(rows=8 * 86 - 5, npics=32, planes444=True)    # 258 counters a picture; 86 rows in workgroups of 4: the last has 2
VLF_SSC_SPLIT = dict(rows=8 * 128 - 3, npics=32)               # 384 counters a picture: 8191 // 384 = 21, launches (21, 11)
# the tallest pictures: (face, rows, pictures a launch)
VLF_TALLEST = dict(lone_420=(VLF_ROWS_420, 2), frames_420=(VLF_ROWS, 3), frames_444=(VLF_ROWS, 2), frames_ssc=(VLF_ROWS, 2),
                   lone_444=(VLF_ROWS, 2), lone_ssc=(VLF_ROWS, 2))


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
