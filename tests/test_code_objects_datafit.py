"""The code object of the data-misfit kernels (fwi_data.o): no scratch, no spilled registers, and the kernels that are
built: the time filter for fp32 and fp64; the fixed-order sum of the partials is the shared one of fwi_reg.o."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import code_objects as co  # noqa: E402


def test_data_kernels_use_no_scratch_and_spill_nothing():
    path = os.path.join(co.CSRC, "fwi_data.o")
    if not co.tools_present() or not os.path.exists(path):
        pytest.skip("ROCm LLVM tools or the built objects are missing (run `make -C full_waveform_inversion_amd/csrc`)")
    ks = co.kernels([path])
    names = [k["name"] for k in ks]
    assert len(ks) == 2 and sum("fir_time<" in n for n in names) == 2 and sum("fir_sum" in n for n in names) == 0, names
    bad = [k["name"] for k in ks if k.get("private_segment_fixed_size", 0) > 0 or k.get("vgpr_spill_count", 0) > 0
           or k.get("sgpr_spill_count", 0) > 0]
    assert not bad, bad
