"""The code object of the Fourier-store transforms (fwi_fourier.o): no scratch, no spilled registers, and the kernels that
are built: the analysis and the synthesis, each for fp32 and fp64, each with 16 bytes per thread (4 / 2 cells) and with one
cell per thread."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import code_objects as co  # noqa: E402


def test_fourier_kernels_use_no_scratch_and_spill_nothing():
    path = os.path.join(co.CSRC, "fwi_fourier.o")
    if not co.tools_present() or not os.path.exists(path):
        pytest.skip("ROCm LLVM tools or the built objects are missing (run `make -C full_waveform_inversion_amd/csrc`)")
    ks = co.kernels([path])
    names = [k["name"] for k in ks]
    count = lambda s: sum(s in n for n in names)  # noqa: E731
    assert len(ks) == 8, names
    for kern in ("fourier_analyse", "fourier_synthesise"):
        assert all(count("%s<%s>" % (kern, t)) == 1 for t in ("float, 4", "float, 1", "double, 2", "double, 1")), names
    bad = [k["name"] for k in ks if k.get("private_segment_fixed_size", 0) > 0 or k.get("vgpr_spill_count", 0) > 0
           or k.get("sgpr_spill_count", 0) > 0]
    assert not bad, bad
