"""The code object of the adaptive-misfit kernels (fwi_awi.o): no scratch, no spilled registers, and the three kernels
that are built: the per-trace solve (G_j packed in LDS, Cholesky, the two pairs of substitutions, N_j, W_j, y_j and z_j;
fp64 only) and the adjoint source for fp32 and fp64.  The lag correlations are tt_xcorr of fwi_ttime.o and the
fixed-order sum of the terms is the shared one of fwi_reg.o: neither is instantiated here."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import code_objects as co  # noqa: E402


def test_adaptive_kernels_use_no_scratch_and_spill_nothing():
    path = os.path.join(co.CSRC, "fwi_awi.o")
    if not co.tools_present() or not os.path.exists(path):
        pytest.skip("ROCm LLVM tools or the built objects are missing (run `make -C full_waveform_inversion_amd/csrc`)")
    ks = co.kernels([path])
    names = [k["name"] for k in ks]
    count = lambda s: sum(s in n for n in names)  # noqa: E731
    assert len(ks) == 3 and count("awi_solve(") == 1 and count("awi_source<") == 2, names
    bad = [k["name"] for k in ks if k.get("private_segment_fixed_size", 0) > 0 or k.get("vgpr_spill_count", 0) > 0
           or k.get("sgpr_spill_count", 0) > 0]
    assert not bad, bad
    # two workgroups of either kernel share a CU's 160 KiB of LDS
    assert all(2 * k["group_segment_fixed_size"] <= 160 * 1024 for k in ks), [(k["name"], k["group_segment_fixed_size"]) for k in ks]
