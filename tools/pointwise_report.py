#!/usr/bin/env python
"""Regenerate profiles/pointwise_margins.json: for every case of tests/test_gpu_pointwise.py the largest err / (u M) the
engine reaches against the fp64 oracle, the factor T the case is held to, the rigorous factor and what the fp32 oracle
itself reaches (tests/_pointwise.py).  Needs a GPU.  A case beyond its T is recorded ("failed"), not hidden; one context
lives at a time and the run stops at the first error that is not a comparison.

    python tools/pointwise_report.py [out.json]
    python tools/pointwise_report.py --table [in.json]     the table of DESIGN.md from that file (no GPU)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import _pointwise as pw  # noqa: E402
from test_gpu_parity import poison_device_memory  # noqa: E402


def main(path):
    rows = []
    for case in pw.CASES:
        R = pw.reference(pw.problem_key(case))
        pw.coverage(R)
        poison_device_memory(64)
        fields = pw.engine_fields(case, R["pb"])   # (asserts the kernel's name and the path the case is meant for)
        ctx = fields.pop("path")
        T = pw.factors(R, case.kw.get("update_form", "standard"))
        row = {"case": pw.case_id(case), "path": case.path, "kernel": fields.pop("kernel"), "T_rig": round(T["rig"], 1),
               "context": {k: ctx[k] for k in ("fused2d", "pair3d", "x-in-kernel", "line-axes", "ty", "zchunk")}}
        if case.abc == "cpml" and len(case.shape) == 3:
            row["masked_lane_stores"] = bool(ctx["x-in-kernel"] and pw.xpml_masked(case.shape, case.order, case.npml,
                                                                                     case.tile[2]))
        for what in pw.ALL:
            if what in fields:
                q = {"err_over_uM": round(pw.ratio(fields[what], R["ref"][what], R["maj"][what], R["u"], T[what]), 2),
                     "T": round(T[what], 1)}
                if R["own"] is not None:
                    q["oracle_fp32"] = round(R["own"][what], 2)
                try:
                    pw.check(fields[what], R["ref"][what], R["maj"][what], R["u"], T[what], what, case.shape, case.tile)
                except AssertionError as e:
                    q["failed"] = str(e)
                row[what] = q
        rows.append(row)
        print(json.dumps(row), flush=True)
    with open(path, "w") as f:
        json.dump({"u": {"float32": "2^-24", "float64": "2^-53"}, "margin_over_oracle_fp32": pw.MARGIN, "cases": rows},
                  f, indent=1)
        f.write("\n")


def table(path):
    """Per path: the cases, the largest err / (u M) of each quantity and the smallest T it was held to."""
    with open(path) as f:
        rows = json.load(f)["cases"]
    print("| path | kernel | cases | forward: worst / T | adjoint: worst / T | gradient: worst / T | T_rig |")
    print("|---|---|---|---|---|---|---|")
    for path_ in dict.fromkeys(r["path"] for r in rows):
        rs = [r for r in rows if r["path"] == path_]
        cells = []
        for what in pw.ALL:
            q = [r[what] for r in rs if what in r]
            w = max(q, key=lambda x: x["err_over_uM"] / x["T"]) if q else None
            cells.append("%.1f / %.0f%s" % (w["err_over_uM"], w["T"], " FAILED" if any("failed" in x for x in q) else "")
                         if w else "--")
        print("| %s | %s | %d | %s | %.0f |" % (path_, "/".join(dict.fromkeys(r["kernel"] for r in rs)), len(rs),
                                             " | ".join(cells), min(r["T_rig"] for r in rs)))


if __name__ == "__main__":
    default = os.path.join(ROOT, "profiles", "pointwise_margins.json")
    if len(sys.argv) > 1 and sys.argv[1] == "--table":
        sys.exit(table(sys.argv[2] if len(sys.argv) > 2 else default))
    main(sys.argv[1] if len(sys.argv) > 1 else default)
