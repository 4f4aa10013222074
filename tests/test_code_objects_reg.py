"""The code object of the regularisation kernels (fwi_reg.o): a pinned kernel count, no scratch, no spilled registers."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import code_objects as co  # noqa: E402

# reg_apply <fp32, fp64> x <Tikhonov, TV> x <v = d, v given>, and the final sum of the block partials
REG_KERNELS = 9


def test_regularisation_kernels_are_pinned_use_no_scratch_and_spill_nothing():
    path = os.path.join(co.CSRC, "fwi_reg.o")
    if not co.tools_present() or not os.path.exists(path):
        pytest.skip("ROCm LLVM tools or the built objects are missing (run `make -C full_waveform_inversion_amd/csrc`)")
    ks = co.kernels([path])
    assert len(ks) == REG_KERNELS, [k["name"] for k in ks]
    assert sum("reg_apply<" in k["name"] for k in ks) == 8 and sum("reg_final" in k["name"] for k in ks) == 1, \
        [k["name"] for k in ks]
    bad = [k["name"] for k in ks if k.get("private_segment_fixed_size", 0) > 0 or k.get("vgpr_spill_count", 0) > 0
           or k.get("sgpr_spill_count", 0) > 0]
    assert not bad, bad
