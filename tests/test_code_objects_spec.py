"""The code object of the spectral-misfit kernels (fwi_spec.o): no scratch, no spilled registers, and the
kernels that are built: the analysis (the segment sums of S and O) for fp32 and fp64, the coefficients (G, phi, a, the
counts and the terms of J; fp64 only), the adjoint source for fp32 and fp64; the fixed-order sum of the terms is the
shared one of fwi_reg.o."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import code_objects as co  # noqa: E402


def test_spectral_kernels_use_no_scratch_and_spill_nothing():
    path = os.path.join(co.CSRC, "fwi_spec.o")
    if not co.tools_present() or not os.path.exists(path):
        pytest.skip("ROCm LLVM tools or the built objects are missing (run `make -C full_waveform_inversion_amd/csrc`)")
    ks = co.kernels([path])
    names = [k["name"] for k in ks]
    count = lambda s: sum(s in n for n in names)  # noqa: E731
    assert len(ks) == 5 and count("spec_analysis<") == 2 and count("spec_coeffs(") == 1 and count("spec_source<") == 2, names
    bad = [k["name"] for k in ks if k.get("private_segment_fixed_size", 0) > 0 or k.get("vgpr_spill_count", 0) > 0
           or k.get("sgpr_spill_count", 0) > 0]
    assert not bad, bad
    # the analysis runs 1024 threads per block: its registers must leave room for that
    assert all(k.get("vgpr_count", 0) <= 128 for k in ks if "spec_analysis<" in k["name"]), ks
