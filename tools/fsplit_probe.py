"""Cost of one part of the tomographic / migration split on the Fourier store (fwi_fourier_split_image_vec) beside the
call whose bytes it moves and more, fwi_fourier_gradient_vec.  The workload and the method of tools/feximage_probe.py:
256^3 O(8), sponge npml 16, increment form, fp32, nt = 1000, image stride 4, F = 8 bins next to the wavelet's peak, batch
8.  One engine runs forward(save) and adjoint_spectral once; every row is then timed on that context: a host clock around
`calls` consecutive calls, each of which ends in a device synchronise, one warm-up round and `reps` timed rounds with the
rows taken in turn inside every round (so a drift of the machine falls on all of them); per call the median, the least
and the largest round are written.  THESE ARE CALL TIMES, NOT KERNEL TIMES: each holds the upload of the weights and
taps, the split launch, the scaling launch and the synchronise.

Rows: the gradient call (existing code, the baseline) and one `same` pass along z, y and x with datafit.hilbert_taps(15)
and (31).  Accounting per cell: a pass along z or y stages CHUNK + 2 R rows for CHUNK = 64 cells, so
it requests 4 F e (1 + 2 R / 64) bytes of coefficients, of which 4 F e are first reads and the halo re-reads are other
workgroups' cells, plus 3 e for the image and its scaling; it issues 4 F times the non-zero taps fp64 FMAs for the filters
(and as many fp64 subtractions).  A z or y pass is accepted when its median is no larger than the larger of (a) its
requested bytes at the baseline's achieved rate, taken at the baseline's largest round plus 10 %, and (b) its FMA count
at the fp64 vector rate (half the 157.3 TFLOPS fp32 vector rate, 39.3e12 FMA/s).  The x rows are reported without a bound.
Writes one JSON document (default profiles/fsplit_probe.json) and prints it."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from full_waveform_inversion_amd import Engine, datafit, fourier, workloads  # noqa: E402

STRIDE, E, NF, BATCH, CHUNK = 4, 4, 8, 8, 64
FP64_FMA_PER_S = 157.3e12 / 2 / 2  # the fp32 vector rate in FLOP/s, halved for fp64, two FLOP per FMA


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "fsplit_probe.json")
    calls = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    if reps < 5:
        raise SystemExit("the baseline's spread needs at least 5 timed rounds")
    w = workloads.cfg4(1.0, npml=16)
    wav, src, rec = w.wavelet(), w.src_idx[:1], w.rec_idx
    bins = fourier.fourier_bins(w.nt, w.dt, STRIDE, 0.0, np.inf)
    f = np.sort(bins[np.argsort(np.abs(bins - w.f0), kind="stable")[:NF]])
    cells = int(np.prod(w.shape))
    base_bytes = (4 * NF + 3) * E
    doc = {"config": w.name, "shape": list(w.shape), "nt": w.nt, "npml": w.npml, "dtype": "float32",
           "update_form": "increment", "image_stride": STRIDE, "F": NF, "B": BATCH, "reps": reps, "calls_per_round": calls,
           "times_are": "host clock around calls that end in a device synchronise: call times, not kernel times",
           "chunk": CHUNK, "fp64_fma_per_s": FP64_FMA_PER_S, "gradient_bytes_per_cell": base_bytes, "rows": {}}
    taps = {R: datafit.hilbert_taps(R) for R in (15, 31)}
    with Engine(w.shape, w.h, w.dt, w.nt, order=w.order, npml=w.npml, update_form="increment", image_stride=STRIDE,
                fourier=f, fourier_batch=BATCH) as e:
        e.set_model(w.c.astype(np.float32))
        d = e.forward(None, (src, wav), rec, save=True)
        e.adjoint_spectral(d * 0.5, image=False)
        e.vec_create(1)
        rows = {"fourier_gradient_vec": lambda: e.fourier_gradient_vec(0, None, "slowness2")}
        for axis in "zyx":
            for R in (15, 31):
                rows["same_%s_R%d" % (axis, R)] = (
                    lambda axis=axis, R=R: e.fourier_split_image_vec(0, "same", axis, taps[R], None, "slowness2"))
        times = {k: [] for k in rows}
        for r in range(reps + 1):
            for k, fn in rows.items():
                e.synchronize()
                t0 = time.perf_counter()
                for _ in range(calls):
                    fn()
                e.synchronize()
                if r >= 1:  # (the first round warms up)
                    times[k].append((time.perf_counter() - t0) * 1e3 / calls)
        doc["kernel"] = e.kernel_name
    for k, t in times.items():
        doc["rows"][k] = {"ms": round(float(np.median(t)), 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4)}
    base = doc["rows"]["fourier_gradient_vec"]
    base["model_TBps"] = round(base_bytes * cells / (base["ms"] * 1e9), 2)
    doc["baseline_spread_max_over_min"] = round(base["ms_max"] / base["ms_min"], 3)
    for axis in "zyx":
        for R in (15, 31):
            row = doc["rows"]["same_%s_R%d" % (axis, R)]
            nz = int(np.count_nonzero(taps[R]))
            row["nonzero_taps"] = nz
            row["fma_per_cell"] = 4 * NF * nz
            row["first_read_bytes_per_cell"] = base_bytes
            row["over_gradient_call"] = round(row["ms"] / base["ms"], 2)
            if axis == "x":
                continue
            row["requested_bytes_per_cell"] = round(4 * NF * E * (1 + 2 * R / CHUNK) + 3 * E, 1)
            row["bytes_bound_ms"] = round(1.10 * base["ms_max"] * row["requested_bytes_per_cell"] / base_bytes, 4)
            row["fma_bound_ms"] = round(row["fma_per_cell"] * cells / FP64_FMA_PER_S * 1e3, 4)
            row["within_bound"] = bool(row["ms"] <= max(row["bytes_bound_ms"], row["fma_bound_ms"]))
    with open(out_path, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
