"""The code object of the robust-misfit kernels (fwi_robust.o): no scratch, no spilled registers, and the thirteen
kernels that are built: the elementwise robust source per dtype and kind (six), the per-trace sum of its tiles, the
per-trace radix select of the median per dtype (two, 64 x 256 uint32 bins of LDS each) and the whole-gather select's
histogram and pick per dtype (four).  The filter passes are fir_time of fwi_data.o and the fixed-order sum of the block
sums is the shared one of fwi_reg.o: neither is instantiated here."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import code_objects as co  # noqa: E402


def test_robust_kernels_use_no_scratch_and_spill_nothing():
    path = os.path.join(co.CSRC, "fwi_robust.o")
    if not co.tools_present() or not os.path.exists(path):
        pytest.skip("ROCm LLVM tools or the built objects are missing (run `make -C full_waveform_inversion_amd/csrc`)")
    ks = co.kernels([path])
    names = [k["name"] for k in ks]
    count = lambda s: sum(s in n for n in names)  # noqa: E731
    assert len(ks) == 13 and count("robust_source<") == 6 and count("robust_terms(") == 1, names
    assert count("median_traces<") == 2 and count("median_hist<") == 2 and count("median_pick<") == 2, names
    bad = [k["name"] for k in ks if k.get("private_segment_fixed_size", 0) > 0 or k.get("vgpr_spill_count", 0) > 0
           or k.get("sgpr_spill_count", 0) > 0]
    assert not bad, bad
    # the per-trace select keeps its 64 x 256 bins in LDS, and two workgroups of any kernel share a CU's 160 KiB
    lds = {k["name"]: k["group_segment_fixed_size"] for k in ks}
    assert all(v >= 64 * 256 * 4 for n, v in lds.items() if "median_traces<" in n), lds
    assert all(2 * v <= 160 * 1024 for v in lds.values()), lds
