"""The code object of the Gaussian smoothing kernels (fwi_smooth.o): no scratch, no spilled registers."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import code_objects as co  # noqa: E402


def test_smoothing_kernels_use_no_scratch_and_spill_nothing():
    path = os.path.join(co.CSRC, "fwi_smooth.o")
    if not co.tools_present() or not os.path.exists(path):
        pytest.skip("ROCm LLVM tools or the built objects are missing (run `make -C full_waveform_inversion_amd/csrc`)")
    ks = co.kernels([path])
    assert sum("smooth_x<" in k["name"] for k in ks) == 2 and sum("smooth_line<" in k["name"] for k in ks) == 2, \
        [k["name"] for k in ks]
    bad = [k["name"] for k in ks if k.get("private_segment_fixed_size", 0) > 0 or k.get("vgpr_spill_count", 0) > 0
           or k.get("sgpr_spill_count", 0) > 0]
    assert not bad, bad
