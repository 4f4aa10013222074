#!/usr/bin/env python
"""Regenerate profiles/pointwise_margins.json: for every case of tests/test_gpu_pointwise.py the largest err / (u M) the
engine reaches against the fp64 oracle, the factor T the case is held to, the rigorous factor and what the fp32 oracle
itself reaches (tests/_pointwise.py).  Needs a GPU.  A case beyond its T is recorded ("failed"), not hidden; one context
lives at a time and the run stops at the first error that is not a comparison.

    python tools/pointwise_report.py [out.json]
    python tools/pointwise_report.py --table [in.json]     the table of DESIGN.md from that file (no GPU)

``--born`` does the same for the cases of tests/test_gpu_pointwise_born.py (Born sweeps by every path, the bf16 store's two
paths against each other, the illumination) into profiles/pointwise_born_margins.json:

    python tools/pointwise_report.py --born [out.json]
    python tools/pointwise_report.py --born --table [in.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import _pointwise as pw  # noqa: E402
import _pointwise_born as pb_  # noqa: E402
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


def _context(path):
    return {k: path[k] for k in ("fused2d", "pair3d", "x-in-kernel", "line-axes", "ty", "zchunk")}


def _attempt(q, f):
    """Run the comparison ``f``; a failed one is recorded in ``q``, not hidden."""
    try:
        return f()
    except AssertionError as e:
        q["failed"] = str(e)


def born_main(path):
    rows = []
    for b in pb_.BORN_CASES:
        case = b.case
        R = pb_.born_reference(pw.problem_key(case))
        pb_.born_coverage(R)
        poison_device_memory(64)
        fields, ctx = pb_.engine_born(b, R)   # (asserts kernel, path, born_path, clean padding)
        T = pb_.born_factors(R, case.kw.get("update_form", "standard"))
        row = {"case": pb_.born_case_id(b), "quantity": "born", "path": case.path, "kernel": case.kernel,
               "operator": b.operator, "T_rig_born": round(T["rig"], 1), "context": _context(ctx), "sweeps": {}}
        for (wrt, mode), x in fields.items():
            q = {"born_path": mode, "err_over_uM": round(pw.ratio(x, R["ref"][wrt], R["maj"][wrt], R["u"], T[wrt]), 2),
                 "T": round(T[wrt], 1)}
            if R["own"] is not None:
                q["oracle_fp32"] = round(R["own"][wrt], 2)
            _attempt(q, lambda: pw.check(x, R["ref"][wrt], R["maj"][wrt], R["u"], T[wrt], wrt + " " + mode, case.shape,
                                         case.tile))
            row["sweeps"]["%s/%s" % (wrt, mode)] = q
        rows.append(row)
        print(json.dumps(row), flush=True)
    for b in pb_.BF16_CASES:
        case = b.case
        R = pb_.born_reference(pw.problem_key(case))
        poison_device_memory(64)
        out, ctx = pb_.engine_bf16_paths(b, R)
        T = 2.0 * pb_.born_factors(R)["velocity"]
        M = R["maj"]["velocity"]
        q = {"err_over_uM": round(pw.ratio(out["fused"], out["scatter"], M, R["u"], T), 2), "T": round(T, 1),
             "oracle_fp32": round(R["own"]["velocity"], 2)}
        _attempt(q, lambda: pw.check(out["fused"], out["scatter"], M, R["u"], T, "fused against scatter", case.shape,
                                     case.tile))
        row = {"case": pb_.born_case_id(b), "quantity": "bf16 fused - scatter", "path": case.path, "kernel": case.kernel,
               "context": _context(ctx), "sweeps": {"velocity/fused-scatter": q}}
        rows.append(row)
        print(json.dumps(row), flush=True)
    for case in pb_.ILLUM_CASES:
        key = pw.problem_key(case)
        R = pb_.born_reference(key)
        T_fwd = pw.factors(pw.reference(key), case.kw.get("update_form", "standard"))["forward"]
        poison_device_memory(64)
        hm, hc, hv, ctx = pb_.engine_illumination(case, R)
        Hm, E = pb_.illumination_reference(R)
        bound = pb_.illumination_bound(R, T_fwd, Hm, E)
        err = abs(hm.reshape(-1).astype("float64") - Hm)
        q = {"err_over_bound": round(float((err / bound).max()), 3), "err_over_uE": round(float((err / (R["u"] * E)).max()), 2),
             "T_fwd": round(T_fwd, 1), "illumination_vec_bitwise": bool((hv == hc).all())}
        _attempt(q, lambda: pb_.check_illumination(hm, R, T_fwd, "illumination", case.shape))
        w = _attempt(q, lambda: pb_.check_conversion(hm, hc, R["pb"], R["u"], "conversion"))
        if w is not None:
            q["conversion_rel_err_in_u"] = round(w, 2)
        row = {"case": pw.case_id(case), "quantity": "illumination", "path": case.path, "kernel": case.kernel,
               "context": _context(ctx), "illumination": q}
        rows.append(row)
        print(json.dumps(row), flush=True)
    with open(path, "w") as f:
        json.dump({"u": {"float32": "2^-24", "float64": "2^-53"}, "margin_over_oracle_fp32": pw.MARGIN, "cases": rows},
                  f, indent=1)
        f.write("\n")


def born_table(path):
    """Per path: the cases, the sweep that uses the largest share of its factor, the fp32 oracle's own ratio there and
    the path's smallest rigorous factor; then the illumination's rows."""
    with open(path) as f:
        rows = json.load(f)["cases"]
    print("| path | kernel | cases | born_path: worst err/(u·M_B) / T | fp32 oracle there | T_rig_born |")
    print("|---|---|---|---|---|---|")
    born = [r for r in rows if "sweeps" in r]
    for path_ in dict.fromkeys(r["path"] for r in born):
        rs = [r for r in born if r["path"] == path_]
        cells = []
        for mode in ("scatter", "fused", "fused-scatter"):
            q = [v for r in rs for k, v in r["sweeps"].items() if k.endswith("/" + mode)]
            if q:
                w = max(q, key=lambda x: x["err_over_uM"] / x["T"])
                cells.append(("%s: %.1f / %.0f%s" % (mode, w["err_over_uM"], w["T"],
                                                     " FAILED" if any("failed" in x for x in q) else ""),
                              "%.1f" % w["oracle_fp32"] if "oracle_fp32" in w else "--"))
        rig = [r["T_rig_born"] for r in rs if "T_rig_born" in r]
        print("| %s | %s | %d | %s | %s | %s |" % (path_, "/".join(dict.fromkeys(r["kernel"] for r in rs)), len(rs),
                                                 "; ".join(c[0] for c in cells), "; ".join(c[1] for c in cells),
                                                 "%.0f" % min(rig) if rig else "--"))
    print()
    print("| illumination case | kernel | err / bound | err / (u·E) | T_fwd | velocity conversion (u of 8) |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        if "illumination" in r:
            q = r["illumination"]
            print("| %s | %s | %.3f%s | %.2f | %.1f | %s |" % (r["case"], r["kernel"], q["err_over_bound"],
                                                             " FAILED" if "failed" in q else "", q["err_over_uE"], q["T_fwd"],
                                                             q.get("conversion_rel_err_in_u", "--")))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--born":
        default = os.path.join(ROOT, "profiles", "pointwise_born_margins.json")
        if len(sys.argv) > 2 and sys.argv[2] == "--table":
            sys.exit(born_table(sys.argv[3] if len(sys.argv) > 3 else default))
        sys.exit(born_main(sys.argv[2] if len(sys.argv) > 2 else default))
    default = os.path.join(ROOT, "profiles", "pointwise_margins.json")
    if len(sys.argv) > 1 and sys.argv[1] == "--table":
        sys.exit(table(sys.argv[2] if len(sys.argv) > 2 else default))
    main(sys.argv[1] if len(sys.argv) > 1 else default)
