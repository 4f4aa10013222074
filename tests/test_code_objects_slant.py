"""The code object of the slant-stack kernel (fwi_slant.o): no scratch, no spilled registers, and the kernels that are
built: ``slant_sum`` for fp32 (4 cells per thread) and for fp64 (2 cells per thread), two in all."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import code_objects as co  # noqa: E402


def test_slant_kernels_use_no_scratch_and_spill_nothing():
    path = os.path.join(co.CSRC, "fwi_slant.o")
    if not co.tools_present() or not os.path.exists(path):
        pytest.skip("ROCm LLVM tools or the built objects are missing (run `make -C full_waveform_inversion_amd/csrc`)")
    ks = co.kernels([path])
    names = [k["name"] for k in ks]
    count = lambda s: sum(s in n for n in names)  # noqa: E731
    assert len(ks) == 2, names
    assert count("slant_sum<float, 4>") == 1 and count("slant_sum<double, 2>") == 1, names
    bad = [k["name"] for k in ks if k.get("private_segment_fixed_size", 0) > 0 or k.get("vgpr_spill_count", 0) > 0
           or k.get("sgpr_spill_count", 0) > 0]
    assert not bad, bad
