"""The code object of the split-image kernels (fwi_fsplit.o): no scratch, no spilled registers, and the kernels that are
built: the pass along z or y (rows of vectors staged in LDS) and the pass along x (a wave's cells of one row staged in
LDS), each for fp32 (4 cells per thread) and fp64 (2 cells per thread)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import code_objects as co  # noqa: E402


def test_fsplit_kernels_use_no_scratch_and_spill_nothing():
    path = os.path.join(co.CSRC, "fwi_fsplit.o")
    if not co.tools_present() or not os.path.exists(path):
        pytest.skip("ROCm LLVM tools or the built objects are missing (run `make -C full_waveform_inversion_amd/csrc`)")
    ks = co.kernels([path])
    names = [k["name"] for k in ks]
    count = lambda s: sum(s in n for n in names)  # noqa: E731
    assert len(ks) == 4, names
    for t in ("float, 4", "double, 2"):
        assert count("fsplit_march<%s>" % t) == 1 and count("fsplit_row<%s>" % t) == 1, names
    bad = [k["name"] for k in ks if k.get("private_segment_fixed_size", 0) > 0 or k.get("vgpr_spill_count", 0) > 0
           or k.get("sgpr_spill_count", 0) > 0]
    assert not bad, bad
