"""Every stepping kernel against the oracle CELL BY CELL (tests/_pointwise.py): the whole forward field, the whole
adjoint field and the gradient, each sample within ``T u M`` of the fp64 oracle, M being the majorant of the scheme at
that very cell and step -- where the norm-wise suites (test_gpu_parity, test_gpu_cpml) see a few receivers in one
relative L2 norm, blind to an error at a border corner, a masked lane or a tile seam.  The factor T of a case is the
smaller of the rigorous operation count and 4 x what the fp32 oracle itself needs on that case; it never comes from an
engine's output.  Every case asserts the kernel it meant to run, what the context itself reports of its path (x border
in the lanes or in slabs, line launches, rows per tile, z chunk) and that the field reaches every cell (coverage).

tools/pointwise_report.py runs the same cases and writes each one's measured err / (u M) and T to
profiles/pointwise_margins.json."""
import pytest

import _pointwise as pw
from test_gpu_parity import poison_device_memory

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", pw.CASES, ids=pw.case_id)
def test_every_cell_vs_oracle(gpu, case):
    R = pw.reference(pw.problem_key(case))   # shared by the cases of one problem; never modified
    pw.coverage(R)
    poison_device_memory(64)
    fields = pw.engine_fields(case, R["pb"])  # one context, closed before anything is judged; asserts kernel and path
    assert fields.pop("kernel") == case.kernel and fields.pop("path")["cpml"] == (case.abc == "cpml")
    for what, (worst, T) in pw.judge(case, fields, R).items():
        print("%s %s: err / (u M) = %.2f of T = %.1f" % (pw.case_id(case), what, worst, T))
