"""The code object of the optimal-transport kernels (fwi_ot.o): no scratch, no spilled registers, and the kernels that are
built: the densities and the adjoint source for fp32 and fp64; the slice offsets, the CDFs, the sorted search, the dual
sums and the per-trace finish in fp64 only; the fixed-order sum of the terms is the shared one of fwi_reg.o."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import code_objects as co  # noqa: E402


def test_transport_kernels_use_no_scratch_and_spill_nothing():
    path = os.path.join(co.CSRC, "fwi_ot.o")
    if not co.tools_present() or not os.path.exists(path):
        pytest.skip("ROCm LLVM tools or the built objects are missing (run `make -C full_waveform_inversion_amd/csrc`)")
    ks = co.kernels([path])
    names = [k["name"] for k in ks]
    count = lambda s: sum(s in n for n in names)  # noqa: E731
    assert len(ks) == 9 and count("ot_density<") == 2 and count("ot_source<") == 2, names
    assert all(count(s) == 1 for s in ("ot_offsets(", "ot_cdf(", "ot_search(", "ot_dual(", "ot_finish(")), names
    bad = [k["name"] for k in ks if k.get("private_segment_fixed_size", 0) > 0 or k.get("vgpr_spill_count", 0) > 0
           or k.get("sgpr_spill_count", 0) > 0]
    assert not bad, bad
