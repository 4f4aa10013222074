"""The code object of the eikonal kernels (fwi_eikonal.o): no scratch, no spilled registers, at most 80 KiB of LDS per
kernel, and the twenty-six kernels that are built: per dtype the fill and the init of the times, the block-Jacobi sweep
and the adjoint sweep in 2-D and 3-D, the gradient pass and its one-thread source term in 2-D and 3-D, and the scale,
add and gather of the point primitives."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import code_objects as co  # noqa: E402


def test_eikonal_kernels_use_no_scratch_spill_nothing_and_share_a_cu():
    path = os.path.join(co.CSRC, "fwi_eikonal.o")
    if not co.tools_present() or not os.path.exists(path):
        pytest.skip("ROCm LLVM tools or the built objects are missing (run `make -C full_waveform_inversion_amd/csrc`)")
    ks = co.kernels([path])
    names = [k["name"] for k in ks]
    count = lambda s: sum(s in n for n in names)  # noqa: E731
    assert len(ks) == 26 and count("eikonal_sweep<") == 4 and count("eikonal_adjoint_sweep<") == 4, names
    assert count("eikonal_gradient<") == 4 and count("eikonal_source_term<") == 4, names
    assert count("eikonal_fill<") == 2 and count("eikonal_init<") == 2, names
    assert count("points_scale<") == 2 and count("points_add<") == 2 and count("points_gather<") == 2, names
    bad = [k["name"] for k in ks if k.get("private_segment_fixed_size", 0) > 0 or k.get("vgpr_spill_count", 0) > 0
           or k.get("sgpr_spill_count", 0) > 0]
    assert not bad, bad
    lds = {k["name"]: k["group_segment_fixed_size"] for k in ks}
    assert all(v <= 80 * 1024 for v in lds.values()), lds
