"""The Born sweeps and the illumination against the oracle CELL BY CELL (tests/_pointwise_born.py on the harness of
tests/_pointwise.py): ``J dc`` observed at every cell and step, each sample within ``T_born u M_B`` of the fp64
restatement (tests/_born.py, tests/_born_imaging.py), ``M_B`` the Born majorant at that very cell and step -- where
test_gpu_born and test_gpu_born_imaging see 8 receivers in one relative L2 norm, blind to a border cell, an x-tile seam,
a z-chunk seam or a pad column of the fused ``IMAGE == 3`` variants of ``step3d_stream`` and of the scatter kernels.
The factor of a case is the smaller of the rigorous count ``T_rig_born`` and 4 x what the fp32 oracle itself needs on
that case; it never comes from an engine's output.  Every case asserts the kernel it meant to run, what the context
reports of its path, ``born_path`` after every sweep, clean padding, and that the scattered field reaches every cell.

The bf16 store gets NO oracle bound per cell here: a flipped bf16 rounding of one stored value is a 2^-8 effect at its
cell, against which a per-cell round-off bound says nothing.  Its fused and scatter paths read the same rounded store,
so they are compared with each other at every cell; the store itself stays with its norm-wise tests
(tests/test_gpu_born_imaging.py).

tools/pointwise_report.py runs the same cases and writes each one's measured figures to
profiles/pointwise_born_margins.json."""
import numpy as np
import pytest

import _pointwise as pw
import _pointwise_born as pb_
from test_gpu_parity import poison_device_memory

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("b", pb_.BORN_CASES, ids=pb_.born_case_id)
def test_born_every_cell_vs_oracle(gpu, b):
    R = pb_.born_reference(pw.problem_key(b.case))   # shared by the cases of one problem; never modified
    pb_.born_coverage(R)
    poison_device_memory(64)
    fields, path = pb_.engine_born(b, R)   # one context, closed before anything is judged; asserts kernel, path, born_path
    assert set(fields) == {(wrt, mode) for wrt in pb_.WRTS for mode in b.modes}
    for (wrt, mode), (worst, T) in pb_.judge_born(b, fields, R).items():
        print("%s born %s %s: err / (u M_B) = %.2f of T = %.1f" % (pb_.born_case_id(b), wrt, mode, worst, T))


@pytest.mark.parametrize("b", pb_.BF16_CASES, ids=pb_.born_case_id)
def test_bf16_store_paths_agree_at_every_cell(gpu, b):
    """One forward into the bf16 store, then the imaging Born sweep by either path from the same context: both read the
    same rounded store, so only fp32 arithmetic separates them -- each is within ``T_born u M_B`` of the exact sweep
    over that store, the two within twice that, ``T_born`` and ``M_B`` those of the native-store problem."""
    R = pb_.born_reference(pw.problem_key(b.case))
    pb_.born_coverage(R)
    poison_device_memory(64)
    out, path = pb_.engine_bf16_paths(b, R)
    T, M = 2.0 * pb_.born_factors(R)["velocity"], R["maj"]["velocity"]
    worst = pw.check(out["fused"], out["scatter"], M, R["u"], T, "%s, fused against scatter" % pb_.born_case_id(b),
                     b.case.shape, b.case.tile)   # (also: fused exactly zero where M_B == 0)
    assert np.any(out["scatter"]) and not np.any(out["scatter"].reshape(M.shape)[M == 0])
    print("%s fused - scatter: err / (u M_B) = %.2f of T = %.1f" % (pb_.born_case_id(b), worst, T))


@pytest.mark.parametrize("case", pb_.ILLUM_CASES, ids=pw.case_id)
def test_illumination_every_cell_vs_oracle(gpu, case):
    """``|h - H_m| <= T_fwd u E + (nt + 3) u H_m`` at every cell, ``H_m = (S / dt^4) sum q64^2`` from the fp64 oracle's
    store, ``E = (S / dt^4) sum 2 |q64| M_q``.  What this catches: a skipped or doubled step, a cell or row that was never
    accumulated, a wrong weight S (each moves a cell by a whole term of its sum).  What it does not: a 1e-3 error in one
    stored ``q`` -- E adds magnitudes; the Born cases above hold the stored term.  The conversion kernel is pinned
    separately: ``illumination("velocity")`` within 8 u (relative) of the same context's ``illumination("slowness2")``
    x (2 / c^3)^2 evaluated in fp64 from the rounded c, and ``illumination_vec`` equal to it bit for bit."""
    key = pw.problem_key(case)
    R = pb_.born_reference(key)
    T_fwd = pw.factors(pw.reference(key), case.kw.get("update_form", "standard"))["forward"]
    poison_device_memory(64)
    hm, hc, hv, path = pb_.engine_illumination(case, R)
    share, over_uE = pb_.check_illumination(hm, R, T_fwd, pw.case_id(case), case.shape)
    print("%s illumination: err / bound = %.2f, err / (u E) = %.2f, T_fwd = %.1f" % (pw.case_id(case), share, over_uE, T_fwd))
    worst = pb_.check_conversion(hm, hc, R["pb"], R["u"], pw.case_id(case))
    print("%s velocity against slowness2 x (2 / c^3)^2: %.2f u of 8" % (pw.case_id(case), worst))
    assert np.array_equal(hv, hc)
