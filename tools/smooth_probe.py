"""Time of the Gaussian smoothing operator (fwi_vec_smooth) against its floor: medians of the time per call at
256^3 and 1024^2 (fp32) for sigma = 2 (R = 6) and sigma = 8 (R = 24), of each axis alone, and -- on the same context
and vector -- of fwi_vec_axpby, which moves the algorithmic bytes of one pass (one read, one write).  Writes one JSON
document (default profiles/r07_smooth.json).  Calls are timed in batches of 16 between two synchronisations of the
context's stream, so a call shorter than the host's ~5 us per launch reads as that; run the tool under
`rocprofv3 --kernel-trace --stats` for the kernels' own durations."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from full_waveform_inversion_amd import Engine  # noqa: E402


def median_us(e, fn, reps=25, warm=3, calls=16):
    """Median over `reps` batches of the time per call of `calls` stream-ordered calls between two synchronisations
    (the context's stream is its own and non-blocking: events of another stream do not bracket it)."""
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        e.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        e.synchronize()
        ts.append((time.perf_counter() - t0) / calls * 1e6)
    return float(np.median(ts))


def probe(shape, sigmas=(2.0, 8.0)):
    nd = len(shape)
    out = {"shape": list(shape), "dtype": "float32", "vector_MiB": round(int(np.prod(shape)) * 4 / 2 ** 20, 1), "rows": []}
    with Engine(shape, 10.0, 1e-3, 4) as e:
        e.vec_create(2)
        e.vec_upload(0, np.random.default_rng(0).standard_normal(shape).astype(np.float32))
        e.vec_upload(1, np.ones(shape, np.float32))
        axpby = median_us(e, lambda: e.vec_axpby(0, 0.5, 0, 0.5))  # x = y: one read, one write, values unchanged
        out["axpby_us"] = round(axpby, 2)
        out["copy_us"] = round(median_us(e, lambda: e.vec_copy(1, 0)), 2)
        for sg in sigmas:
            row = {"sigma": sg, "R": int(3 * sg + 0.5)}
            for ax in range(nd):
                w = [0.0] * nd
                w[ax] = sg
                row["axis%d_us" % ax] = round(median_us(e, lambda: e.vec_smooth(0, w)), 2)
            row["all_axes_us"] = round(median_us(e, lambda: e.vec_smooth(0, sg)), 2)
            row["axpby_x%d_us" % nd] = round(nd * axpby, 2)
            row["ratio_to_axpby"] = round(row["all_axes_us"] / (nd * axpby), 2)
            out["rows"].append(row)
    return out


def trace_case(shape, sigma, n=20):
    """The dispatches of one case in a fixed order, for a kernel trace: n x axpby, then n x each axis alone (grid
    order), then n x all axes."""
    nd = len(shape)
    with Engine(shape, 10.0, 1e-3, 4) as e:
        e.vec_create(1)
        e.vec_upload(0, np.random.default_rng(0).standard_normal(shape).astype(np.float32))
        for _ in range(n):
            e.vec_axpby(0, 0.5, 0, 0.5)
        for ax in range(nd):
            w = [0.0] * nd
            w[ax] = sigma
            for _ in range(n):
                e.vec_smooth(0, w)
        for _ in range(n):
            e.vec_smooth(0, sigma)
        e.synchronize()


def summarize_trace(csv_path, n=20):
    """Median duration (us) of every run of >= n consecutive dispatches of one kernel in a rocprofv3 kernel trace of
    :func:`trace_case`, in dispatch order, then the per-kernel medians of the remaining (all-axes) dispatches."""
    import csv
    rows = sorted(csv.DictReader(open(csv_path)), key=lambda r: int(r["Start_Timestamp"]))
    rows = [(r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3) for r in rows]
    out, rest, i = [], {}, 0
    while i < len(rows):
        j = i
        while j < len(rows) and rows[j][0] == rows[i][0]:
            j += 1
        if j - i >= n:
            out.append({"kernel": rows[i][0].split("(")[0][:60], "calls": j - i,
                        "median_us": round(float(np.median([d for _, d in rows[i:j]][2:])), 2)})
        else:
            for k, d in rows[i:j]:
                rest.setdefault(k.split("(")[0][:60], []).append(d)
        i = j
    return {"runs": out, "others": {k: {"calls": len(v), "median_us": round(float(np.median(v)), 2)} for k, v in rest.items()}}


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "case":  # case 256,256,256 8.0   (under rocprofv3 --kernel-trace)
        trace_case(tuple(int(v) for v in sys.argv[2].split(",")), float(sys.argv[3]))
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "summarize":  # summarize <kernel_trace.csv>
        print(json.dumps(summarize_trace(sys.argv[2])))
        sys.exit(0)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "r07_smooth.json")
    res = [probe((256, 256, 256)), probe((1024, 1024))]
    for r in res:
        print(json.dumps(r), flush=True)
    with open(path, "w") as f:
        json.dump({"tool": "tools/smooth_probe.py", "unit": "us per call, median of 25 batches of 16 stream-ordered calls", "cases": res},
                  f, indent=1)
        f.write("\n")
