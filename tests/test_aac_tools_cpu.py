"""AACDecDSP's stereo tools and long-term prediction, CPU side: the oracle's restatements
(oracle/ffo_aac.c) against the reference's own members run in place (oracle/_ref: aacdec_dsp_template.c:83-160,225-320 through
ff_aac_decode_init_float's dsp table) — bit-identical.  Everywhere, with or without oracle/_ref, the outputs of each test hash to its
digest in tests/golden/pins.npz (ffi.Pin); without the reference the decoder's window tables come from tests/golden/round2.npz."""
import ctypes as C

import numpy as np
import pytest

import ffi
from ffi import ptr, f32p, i32p, u8p
import aac_gen as A
import test_golden as TG
from test_oracle_vs_ref import aac_tns_case, aac_tns_filters

u16p = C.POINTER(C.c_uint16)
i8p = C.POINTER(C.c_int8)


def _ref(member="ffref_aac_apply_ltp"):
    """the reference build, or None where it is not built"""
    R = ffi.ref()
    if R is not None and not hasattr(R, member):
        pytest.skip("oracle/_ref predates " + member)
    return R


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def ref_windows(R):
    """sine_1024, sine_128, kbd_long_1024, kbd_short_128 of the decoder: the reference's, or the stored copies of them"""
    if R is None:
        d = TG.load("round2")
        return [np.ascontiguousarray(d["win%d" % k]) for k in range(4)]
    return [np.ctypeslib.as_array(R.ffref_aac_window(k), (n,)).copy() for k, n in ((0, 1024), (1, 128), (2, 1024), (3, 128))]


@pytest.mark.parametrize("short", [0, 1])
def test_mid_side_and_intensity(short):
    R, O = _ref(), ffi.oracle()
    pin = ffi.Pin("aac_tools/mid_side_and_intensity-%d" % short)
    rng = np.random.default_rng(3100 + short)
    touched = 0
    for rep in range(200):
        c = A.cpe(rng, short)
        a0, a1 = A.spectrum(rng), A.spectrum(rng)
        b0, b1 = a0.copy(), a1.copy()
        args = (c["num_window_groups"], ptr(c["group_len"], u8p), c["max_sfb"], ptr(c["ms_mask"], u8p), ptr(c["band_type0"], i32p),
                ptr(c["band_type1"], i32p), ptr(c["swb"], u16p))
        if R is not None:
            assert R.ffref_aac_apply_mid_side_stereo(ptr(a0, f32p), ptr(a1, f32p), *args) == 0
        O.ffo_aac_apply_mid_side_stereo(ptr(b0, f32p), ptr(b1, f32p), *args)
        args = (c["num_window_groups"], ptr(c["group_len"], u8p), c["max_sfb"], c["ms_present"], ptr(c["ms_mask"], u8p),
                ptr(c["band_type1"], i32p), ptr(c["sf1"], f32p), ptr(c["swb"], u16p))
        before = b1.copy()
        if R is not None:
            assert R.ffref_aac_apply_intensity_stereo(ptr(a0, f32p), ptr(a1, f32p), *args) == 0
        O.ffo_aac_apply_intensity_stereo(ptr(b0, f32p), ptr(b1, f32p), *args)
        if R is not None:
            assert np.array_equal(bits(a0), bits(b0)) and np.array_equal(bits(a1), bits(b1))
        pin.add(b0, b1)
        touched += int((bits(b1) != bits(before)).sum())
    assert touched > 10000
    pin.check()


def test_apply_ltp():
    R, O = _ref(), ffi.oracle()
    pin = ffi.Pin("aac_tools/apply_ltp")
    rng = np.random.default_rng(3110)
    win = ref_windows(R)
    wp = (f32p * 4)(*[ptr(w, f32p) for w in win])
    m = O.ffo_mdct_create(0, 1024, np.float32(-32786.0 * 2 + 36))
    changed = 0
    for rep in range(120):
        c = A.ltp(rng)
        if rep % 10 == 9:
            c["seq"][0] = A.EIGHT_SHORT                     # the member does nothing on short windows
        t = aac_tns_case(rng, 0)
        t["swb"], t["num_swb"], t["max_sfb"] = c["swb"], c["num_swb"], c["max_sfb"]
        present = int(rep % 3 != 0)
        a = A.spectrum(rng)
        b = a.copy()
        pa, pb = np.zeros(1024, np.float32), np.zeros(1024, np.float32)
        assert R is None or R.ffref_aac_apply_ltp(ptr(a, f32p), ptr(c["ltp_state"], f32p), c["lag"], c["coef"], ptr(c["used"], i8p), ptr(c["seq"], i32p),
                                     ptr(c["kb"], i32p), c["max_sfb"], c["num_swb"], t["tns_max_bands"], ptr(c["swb"], u16p), present,
                                     ptr(t["n_filt"], i32p), ptr(t["length"], i32p), ptr(t["direction"], i32p), ptr(t["order"], i32p),
                                     ptr(t["coef"], f32p), ptr(pa, f32p)) == 0
        rec = aac_tns_filters(O, t) if present else np.zeros(0, np.uint8)
        O.ffo_aac_apply_ltp(m, wp, ptr(b, f32p), ptr(c["ltp_state"], f32p), c["lag"], c["coef"], ptr(c["used"], i8p), ptr(c["seq"], i32p),
                            ptr(c["kb"], i32p), c["max_sfb"], ptr(c["swb"], u16p), rec.ctypes.data if len(rec) else None, len(rec), ptr(pb, f32p))
        if R is not None:
            if c["seq"][0] != A.EIGHT_SHORT:
                assert np.array_equal(bits(pa), bits(pb)), rep
            assert np.array_equal(bits(a), bits(b)), rep
        pin.add(b, pb if c["seq"][0] != A.EIGHT_SHORT else np.zeros(0, np.float32))
        changed += int((bits(b) != bits(A.spectrum(np.random.default_rng(0)))).any())
    O.ffo_mdct_free(m)
    assert changed
    pin.check()


def test_update_ltp():
    R, O = _ref(), ffi.oracle()
    pin = ffi.Pin("aac_tools/update_ltp")
    rng = np.random.default_rng(3120)
    win = ref_windows(R)
    wp = (f32p * 4)(*[ptr(w, f32p) for w in win])
    for rep in range(64):
        seq0, kb0 = rep & 3, (rep >> 2) & 1
        buf, saved, out = A.spectrum(rng), A.spectrum(rng)[:512].copy(), A.spectrum(rng)
        sa = (rng.standard_normal(3072) * 100).astype(np.float32)
        sb = sa.copy()
        assert R is None or R.ffref_aac_update_ltp(ptr(sa, f32p), ptr(buf, f32p), ptr(saved, f32p), ptr(out, f32p), seq0, kb0) == 0
        O.ffo_aac_update_ltp(wp, ptr(sb, f32p), ptr(buf, f32p), ptr(saved, f32p), ptr(out, f32p), seq0, kb0)
        if R is not None:
            assert np.array_equal(bits(sa), bits(sb)), (seq0, kb0)
        pin.add(sb)
    pin.check()


def run_band_ops(rec, a, b):
    """FFHipAacBandOp records on host arrays of channel-frames, element by element as the kernel does"""
    for r in rec:
        x = a[r["frame0"], r["start"]:r["start"] + r["len"]].copy()
        y = b[r["frame1"], r["start"]:r["start"] + r["len"]].copy()
        if r["kind"] == 0:
            a[r["frame0"], r["start"]:r["start"] + r["len"]] = x + y
            b[r["frame1"], r["start"]:r["start"] + r["len"]] = x - y
        elif r["kind"] == 1:
            b[r["frame1"], r["start"]:r["start"] + r["len"]] = x * r["scale"]
        else:
            a[r["frame0"], r["start"]:r["start"] + r["len"]] = x + y


@pytest.mark.parametrize("short", [0, 1])
def test_band_walks_vs_oracle(short):
    """the product's host walks (ffhip_aac_ms_bands / is_bands / ltp_bands: no device involved) executed on host arrays == the oracle"""
    from ffmpeg_amd import aac
    O = ffi.oracle()
    rng = np.random.default_rng(3130 + short)
    nrec = 0
    for rep in range(150):
        c = A.cpe(rng, short)
        fr = np.stack([A.spectrum(rng) for _ in range(4)])
        want = fr.copy()
        args = (c["num_window_groups"], ptr(c["group_len"], u8p), c["max_sfb"], ptr(c["ms_mask"], u8p), ptr(c["band_type0"], i32p),
                ptr(c["band_type1"], i32p), ptr(c["swb"], u16p))
        O.ffo_aac_apply_mid_side_stereo(ptr(want[1], f32p), ptr(want[3], f32p), *args)
        O.ffo_aac_apply_intensity_stereo(ptr(want[1], f32p), ptr(want[3], f32p), c["num_window_groups"], ptr(c["group_len"], u8p), c["max_sfb"],
                                         c["ms_present"], ptr(c["ms_mask"], u8p), ptr(c["band_type1"], i32p), ptr(c["sf1"], f32p), ptr(c["swb"], u16p))
        rec = np.concatenate([aac.ms_bands(1, 3, c["num_window_groups"], c["group_len"], c["max_sfb"], c["ms_mask"], c["band_type0"],
                                           c["band_type1"], c["swb"]),
                              aac.is_bands(1, 3, c["num_window_groups"], c["group_len"], c["max_sfb"], c["ms_present"], c["ms_mask"],
                                           c["band_type1"], c["sf1"], c["swb"])])
        nrec += len(rec)
        run_band_ops(rec, fr, fr)
        assert np.array_equal(bits(fr), bits(want)), rep
    assert nrec > 500
    from ffmpeg_amd import _lib
    assert _lib.lib().ffhip_aac_ms_bands(None, 0, 1, 1, None, 1, None, None, None, None) < 0


def test_ltp_bands_walk():
    from ffmpeg_amd import aac
    rng = np.random.default_rng(3140)
    for rep in range(50):
        c = A.ltp(rng)
        co, pred = A.spectrum(rng)[None].copy(), A.spectrum(rng)[None].copy()
        want = co.copy()
        for sfb in range(min(c["max_sfb"], 40)):
            if c["used"][sfb]:
                want[0, c["swb"][sfb]:c["swb"][sfb + 1]] += pred[0, c["swb"][sfb]:c["swb"][sfb + 1]]
        run_band_ops(aac.ltp_bands(0, 0, c["max_sfb"], c["used"], c["swb"]), co, pred)
        assert np.array_equal(bits(co), bits(want))


@pytest.mark.parametrize("L", [960, 768])
def test_imdct_and_windowing_960_768(L):
    """AACDecDSP.imdct_and_windowing_960 / _768 (aacdec_dsp_template.c:389-512): the oracle's length-generic restatement against the
    members over every window-sequence transition.  960: the decoder's sine / KBD tables (regenerated by the same public
    functions).  768: this reference leaves its 768 / 96 tables zero-initialised (never filled), so the comparison runs on zero
    tables - it pins the inverse transforms, the copies and the state hand-over, not the window products."""
    R, O = _ref("ffref_aac_imdct_and_windowing_len"), ffi.oracle()
    pin = ffi.Pin("aac_tools/imdct_and_windowing-%d" % L)
    rng = np.random.default_rng(3150 + L)
    S = L // 8
    if R is not None:
        win = [np.ctypeslib.as_array(R.ffref_aac_window_len(L, k), (n,)).copy() for k, n in ((0, L), (1, S), (2, L), (3, S))]
    elif L == 960:                                                   # the stored copies of the reference's tables
        win = [np.ascontiguousarray(TG.load("round2")["w960_%d" % k]) for k in range(4)]
    else:
        win = [np.zeros(n, np.float32) for n in (L, S, L, S)]
    if L == 960:
        assert all(np.abs(w).max() > .9 for w in win)
    wp = (f32p * 4)(*[ptr(w, f32p) for w in win])
    ml, ms = O.ffo_mdct_create(1, L, np.float32((1.0 / L) / 32768.0)), O.ffo_mdct_create(1, S, np.float32((1.0 / S) / 32768.0))
    sa = (rng.standard_normal(L // 2) * .1).astype(np.float32)
    sb = sa.copy()
    prev = (0, 0)
    for f in range(200):
        seq, kb = int(rng.integers(0, 4)), int(rng.integers(0, 2))
        co = A.spectrum(rng) * np.float32(100)
        s2, k2 = np.array([seq, prev[0]], np.int32), np.array([kb, prev[1]], np.int32)
        oa, ob = np.zeros(L, np.float32), np.zeros(L, np.float32)
        assert R is None or R.ffref_aac_imdct_and_windowing_len(L, ptr(co, f32p), ptr(s2, i32p), ptr(k2, i32p), ptr(sa, f32p), ptr(oa, f32p)) == 0
        O.ffo_aac_imdct_and_windowing_len(L, 128 if L == 960 else 96, ml, ms, wp, ptr(co, f32p), ptr(s2, i32p), ptr(k2, i32p), ptr(sb, f32p),
                                          ptr(ob, f32p))
        if R is not None:
            assert np.array_equal(bits(oa), bits(ob)), (f, seq, prev)
            assert np.array_equal(bits(sa), bits(sb)), (f, seq, prev)
        pin.add(ob, sb)
        prev = (seq, kb)
    O.ffo_mdct_free(ml); O.ffo_mdct_free(ms)
    pin.check()


def test_imdct_and_windowing_ld_eld():
    """AACDecDSP.imdct_and_windowing_ld / _eld (AAC-LD, AAC-ELD at 512 and 480 samples, aacdec_dsp_template.c:516-602): the oracle
    against the members over runs of frames (the ELD history is three frames deep), the decoder's own tables.  LD's two tables are
    sine windows the oracle generates (held equal to the reference's where it is built) and its outputs are pinned; ELD's windows are
    literal tables of the reference, so the ELD half runs where oracle/_ref is built."""
    R, O = _ref("ffref_aac_imdct_and_windowing_ld"), ffi.oracle()
    pin = ffi.Pin("aac_tools/imdct_and_windowing_ld")
    rng = np.random.default_rng(3160)
    tabs = [np.zeros(n, np.float32) for n in (512, 128)]
    for t in tabs:
        O.ffo_aac_sine_window(ptr(t, f32p), len(t))
    if R is not None:
        ref_tabs = [np.ctypeslib.as_array(R.ffref_aac_ld_table(k), (n,)).copy() for k, n in ((0, 512), (1, 128), (2, 1920), (3, 1800))]
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(tabs, ref_tabs[:2]))
        tabs = ref_tabs
    m512, m480 = O.ffo_mdct_create(1, 512, np.float32((1.0 / 512) / 32768.0)), O.ffo_mdct_create(1, 480, np.float32((1.0 / 480) / 32768.0))
    sa = (rng.standard_normal(256) * .1).astype(np.float32)
    sb = sa.copy()
    for f in range(60):
        co = A.spectrum(rng) * np.float32(100)
        kbp = int(rng.integers(0, 2))
        oa, ob = np.zeros(512, np.float32), np.zeros(512, np.float32)
        assert R is None or R.ffref_aac_imdct_and_windowing_ld(ptr(co, f32p), kbp, ptr(sa, f32p), ptr(oa, f32p)) == 0
        O.ffo_aac_imdct_and_windowing_ld(m512, ptr(tabs[0], f32p), ptr(tabs[1], f32p), ptr(co, f32p), kbp, ptr(sb, f32p), ptr(ob, f32p))
        if R is not None:
            assert np.array_equal(bits(oa), bits(ob)) and np.array_equal(bits(sa), bits(sb)), f
        pin.add(ob, sb)
    pin.check()
    for n, m, w in ((512, m512, tabs[2]), (480, m480, tabs[3])) if R is not None else ():
        sa = (rng.standard_normal(3 * n) * .1).astype(np.float32)
        sb = sa.copy()
        for f in range(40):
            co = A.spectrum(rng) * np.float32(100)
            oa, ob = np.zeros(n, np.float32), np.zeros(n, np.float32)
            assert R.ffref_aac_imdct_and_windowing_eld(n, ptr(co, f32p), ptr(sa, f32p), ptr(oa, f32p)) == 0
            O.ffo_aac_imdct_and_windowing_eld(n, m, ptr(w, f32p), ptr(co, f32p), ptr(sb, f32p), ptr(ob, f32p))
            assert np.array_equal(bits(oa), bits(ob)), (n, f)
            assert np.array_equal(bits(sa), bits(sb)), (n, f)
    O.ffo_mdct_free(m512); O.ffo_mdct_free(m480)


def test_apply_prediction_and_coupling():
    """AAC Main's backward-adaptive predictors over runs of frames (state carried, resets by group, short windows resetting all,
    the never-initialised first frame) and the two channel-coupling members: oracle == reference, bit for bit"""
    R, O = _ref("ffref_aac_apply_prediction"), ffi.oracle()
    pin = ffi.Pin("aac_tools/apply_prediction_and_coupling")
    rng = np.random.default_rng(3170)
    sa = (rng.standard_normal(672 * 8)).astype(np.float32)          # garbage: the first frame must reset it
    sb = sa.copy()
    ia, ib = np.zeros(1, np.int32), np.zeros(1, np.int32)
    sampling_index = 4                                               # 44.1 kHz: pred_sfb_max 40
    added = 0
    base = (rng.standard_normal(1024) * 300).astype(np.float32)          # a tonal signal: the predictors lock on (var > 1)
    for f in range(80):
        is_long = int(f % 11 != 7)
        present = int(rng.integers(0, 3) > 0)
        used = rng.integers(0, 2, 41).astype(np.uint8)
        reset_group = int(rng.integers(0, 31)) if rng.integers(0, 4) == 0 else 0
        ca = (base * (1 + .05 * rng.standard_normal(1024))).astype(np.float32)
        cb = ca.copy()
        c0 = ca.copy()
        pmax = 40
        if R is not None:
            pmax = R.ffref_aac_apply_prediction(ptr(sa, f32p), ptr(ca, f32p), is_long, ptr(ia, i32p), present, ptr(used, u8p), sampling_index,
                                                ptr(A.SWB_1024, u16p), reset_group)
            assert pmax == 40
        O.ffo_aac_apply_prediction(ptr(sb, f32p), ptr(cb, f32p), is_long, ptr(ib, i32p), present, ptr(used, u8p), pmax, ptr(A.SWB_1024, u16p), reset_group)
        s6a, s6b = sa.reshape(672, 8)[:, :6], sb.reshape(672, 8)[:, :6]
        if R is not None:
            assert np.array_equal(bits(ca), bits(cb)), f
            assert np.array_equal(bits(s6a), bits(s6b)), f
        pin.add(cb, s6b)
        added += int((bits(cb) != bits(c0)).sum())
    assert added > 5000
    for short in (0, 1):
        for rep in range(30):
            c = A.ics(rng, short)
            bt = np.zeros(128, np.int32)
            bt[:c["num_window_groups"] * c["max_sfb"]] = rng.integers(0, 3, c["num_window_groups"] * c["max_sfb"])
            gain = (2.0 ** (rng.integers(-20, 20, 120) / 8.0)).astype(np.float32)
            src = A.spectrum(rng)
            da = A.spectrum(rng)
            db = da.copy()
            args = (c["num_window_groups"], ptr(c["group_len"], u8p), c["max_sfb"], ptr(bt, i32p), ptr(gain, f32p), ptr(c["swb"], u16p))
            assert R is None or R.ffref_aac_apply_dependent_coupling(ptr(da, f32p), ptr(src, f32p), *args) == 0
            O.ffo_aac_apply_dependent_coupling(ptr(db, f32p), ptr(src, f32p), *args)
            if R is not None:
                assert np.array_equal(bits(da), bits(db))
            pin.add(db)
    for ln in (1024, 2048):
        src, da = (rng.standard_normal(2048) * 100).astype(np.float32), (rng.standard_normal(2048) * 100).astype(np.float32)
        db = da.copy()
        assert R is None or R.ffref_aac_apply_independent_coupling(ptr(da, f32p), ptr(src, f32p), 0.7071, ln) == 0
        O.ffo_aac_apply_independent_coupling(ptr(db, f32p), ptr(src, f32p), 0.7071, ln)
        if R is not None:
            assert np.array_equal(bits(da), bits(db))
        pin.add(db)
    pin.check()
