"""tools/make_pins.py — (re)write tests/golden/pins.npz, the digests ffi.Pin checks: runs the tests that pin and records what they
hash (the reference's outputs where oracle/_ref is built, the oracle's otherwise).  Run it after a deliberate change of what one of
those tests computes; wherever oracle/_ref is built the tests also hold the reference's outputs to the recorded digests."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import ffi  # noqa: E402

FILES = ["tests/test_vp9_lf_sb_cpu.py", "tests/test_aac_tools_cpu.py"]

if __name__ == "__main__":
    os.chdir(ROOT)
    ffi.PIN_RECORD = {}
    rc = pytest.main(["-q", "-p", "no:cacheprovider", "-m", "not gpu"] + FILES)
    if rc != 0:
        sys.exit("the pinning tests did not all pass: nothing written")
    keys = sorted(ffi.PIN_RECORD)
    np.savez_compressed(ffi.PINS_NPZ, keys=np.array(keys), digests=np.array([ffi.PIN_RECORD[k] for k in keys]))
    print("%d digests -> %s (reference build: %s)" % (len(keys), os.path.relpath(ffi.PINS_NPZ, ROOT), ffi.have_ref()))
