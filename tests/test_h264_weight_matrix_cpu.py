"""CPU tier of the H.264 weighting matrix at every depth (tests/h264_weight_matrix.py): on the oracle's output alone, the case that
tests/test_gpu_h264_hbd.py::test_weight_matrix_hbd sends through k_h264_weight_hbd is not vacuous."""
import numpy as np
import pytest

import h264_weight_matrix as W


@pytest.mark.parametrize("bd", W.DEPTHS)
def test_the_case_is_not_vacuous(bd):
    c = W.case(bd)
    n = len(c.cells)
    assert n == 4 * 4 * 8 * (15 + 75 + 2) == 11776
    assert c.want.dtype == (np.uint16 if bd > 8 else np.uint8) and c.want.shape == c.dst0.shape == c.src.shape
    ins, maxv = c.inside, (1 << bd) - 1
    assert ins.sum() == sum((16 >> k[0]) * k[1] for k in c.cells), "the blocks do not overlap"
    assert (c.want[ins] != c.dst0[ins]).mean() > .5, "more than half of the in-block samples change"
    assert np.array_equal(c.want[~ins], c.dst0[~ins]), "nothing outside a block changes"
    assert (c.want[ins] == 0).any() and (c.want[ins] == maxv).any(), "both clips"
    assert c.dst0.max() == maxv and c.src.max() == maxv and c.want.max() <= maxv
    rec = c.rec
    for w_idx in range(4):
        for bi in (0, 1):
            sel = rec[(rec["w_idx"] == w_idx) & (rec["bi"] == bi)]
            assert {int(r["dst_offset"]) // c.px % 4 for r in sel} == {0, 1, 2, 3}, "every destination alignment, in samples"
            assert all(int(r["dst_offset"]) % c.px == 0 and int(r["src_offset"]) % c.px == 0 for r in sel)
    # a slot is private: block and slack of record i stay inside slot i
    for i, (py, px) in enumerate(c.geo):
        y, x = (i // W.PER_ROW) * W.SH, (i % W.PER_ROW) * W.SW
        assert y + W.S == py and x + W.S <= px and px + 16 + W.S <= x + W.SW and x + W.SW <= W.STRIDE


def test_depth_8_is_the_8_bit_oracle():
    """the _bd oracle at 8 bits against ffo_h264_weight / ffo_h264_biweight, which test_gpu_mc_matrix.py::test_h264_weight_matrix uses"""
    import ctypes as C
    import ffi
    from ffi import u8p
    c = W.case(8)
    O = ffi.oracle()
    want = c.dst0.copy()
    for r in c.rec:
        w = 16 >> int(r["w_idx"])
        pd = C.cast(want.ctypes.data + int(r["dst_offset"]), u8p)
        if r["bi"]:
            O.ffo_h264_biweight(w, pd, C.cast(c.src.ctypes.data + int(r["src_offset"]), u8p), W.STRIDE, int(r["height"]), int(r["log2_denom"]),
                                int(r["weightd"]), int(r["weights"]), int(r["offset"]))
        else:
            O.ffo_h264_weight(w, pd, W.STRIDE, int(r["height"]), int(r["log2_denom"]), int(r["weightd"]), int(r["offset"]))
    assert np.array_equal(want, c.want)
