"""The code object of the walled / slot-started eikonal kernels (fwi_eikonal_stage.o): no scratch, no spilled registers,
at most 80 KiB of LDS per kernel, and the 24 kernels that are built: per dtype the check of a start and the prologue of
the ping-pong pair, and in 2-D and 3-D the walled block-Jacobi sweep, the handover, the start and the one-thread list
kernel of the stage tangent and its block-Jacobi sweep.  The sweeps are the bodies of fwi_eikonal_device.h, so their LDS
is that of the sweeps they extend: one box of the tile with one cell of halo (18^2 or 10^3 values) for the walled
sweep, two for the tangent."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import code_objects as co  # noqa: E402


def _lds(obj, marker):
    return {k["name"].split(marker)[1].split(">")[0]: k["group_segment_fixed_size"]
            for k in co.kernels([os.path.join(co.CSRC, obj)]) if marker in k["name"]}


def test_eikonal_stage_kernels_use_no_scratch_spill_nothing_and_keep_the_lds_of_the_sweeps_they_extend():
    path = os.path.join(co.CSRC, "fwi_eikonal_stage.o")
    if not co.tools_present() or not os.path.exists(path):
        pytest.skip("ROCm LLVM tools or the built objects are missing (run `make -C full_waveform_inversion_amd/csrc`)")
    ks = co.kernels([path])
    names = [k["name"] for k in ks]
    count = lambda s: sum(s in n for n in names)  # noqa: E731
    assert len(ks) == 24, names
    for dtype in ("float", "double"):
        assert count("eikonal_stage_check<%s>" % dtype) == 1, names
        assert count("eikonal_stage_start<%s>" % dtype) == 1, names
        for nd in (2, 3):
            for kernel in ("eikonal_stage_sweep", "eikonal_handover", "eikonal_stage_tangent_start",
                           "eikonal_stage_tangent_list", "eikonal_stage_tangent_sweep"):
                assert count("%s<%s, %d>" % (kernel, dtype, nd)) == 1, (kernel, names)
    bad = [k["name"] for k in ks if k.get("private_segment_fixed_size", 0) > 0 or k.get("vgpr_spill_count", 0) > 0
           or k.get("sgpr_spill_count", 0) > 0]
    assert not bad, bad
    lds = {k["name"]: k["group_segment_fixed_size"] for k in ks}
    assert all(v <= 80 * 1024 for v in lds.values()), lds
    # one more read-only array costs no LDS: the figures of the sweeps of fwi_eikonal.o and fwi_eikonal_tangent.o
    walled, plain = _lds("fwi_eikonal_stage.o", "eikonal_stage_sweep<"), _lds("fwi_eikonal.o", "eikonal_sweep<")
    assert len(walled) == 4 and walled == plain, (walled, plain)
    staged = _lds("fwi_eikonal_stage.o", "eikonal_stage_tangent_sweep<")
    tangent = _lds("fwi_eikonal_tangent.o", "eikonal_tangent_sweep<")
    assert len(staged) == 4 and staged == tangent, (staged, tangent)
    # the elementwise kernels hold nothing in LDS but the check's two votes
    assert all(v == 0 for n, v in lds.items() if "handover<" in n or "tangent_start<" in n or "stage_start<" in n), lds
