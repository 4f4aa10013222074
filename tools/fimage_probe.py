"""Cost of spectral imaging on the Fourier store (fwi_adjoint_spectral + fwi_fourier_image) per shot-gradient, beside the
two paths it is measured against: the same store's synthesis plus time-domain imaging (fwi_adjoint(image)), and the native
store.  The workload of tools/fourier_probe.py: 256^3 O(8), sponge npml 16, increment form, fp32, nt = 1000, image stride 4,
with (F, B) in {(4, 8), (8, 8), (16, 8), (8, 1)}.  Per (F, B) ONE engine runs both Fourier paths in turn, forward(save) +
the adjoint of one shot, one warm-up pair and then `reps` timed pairs each, wall clock around work that ends in a device
synchronise; median, least and largest are written.  The native store is timed in the same process, on the last context
with its Fourier store switched off.  The byte model of DESIGN.md s.4p is written beside the measurement, per shot and
cell (e = 4 bytes, N = 250 samples): over the native store the spectral path adds the forward analysis, N (e + 4 e F / B),
the pack and the adjoint analysis, N (3 e + 4 e F / B), and the image pass, (4 F + 2) e, and drops the step kernel's slot
read and its read-modify-write of g, N 3 e; against the time-domain Fourier path it differs by N (2 e F / B - e) +
(4 F + 2) e.  Nothing is asserted about which path is faster.  Writes one JSON document (default
profiles/fimage_probe.json) and prints it."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from full_waveform_inversion_amd import Engine, fourier, workloads  # noqa: E402

STRIDE, E = 4, 4
CONFIGS = ((4, 8), (8, 8), (16, 8), (8, 1))


def timed(e, src, wav, rec, res, adjoint, reps):
    times = []
    for r in range(reps + 1):
        e.reset_gradient()
        e.synchronize()
        t0 = time.perf_counter()
        d = e.forward(None, (src, wav), rec, save=True)
        if res[0] is None:
            res[0] = d * 0.5
        adjoint(res[0])
        e.synchronize()
        if r >= 1:  # (the first pair allocates and warms up)
            times.append((time.perf_counter() - t0) * 1e3)
    return {"shot_gradient_ms": round(float(np.median(times)), 2), "ms_min": round(min(times), 2),
            "ms_max": round(max(times), 2), "store_bytes": e.store_bytes()}


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "fimage_probe.json")
    w = workloads.cfg4(1.0, npml=16)
    wav, src, rec = w.wavelet(), w.src_idx[:1], w.rec_idx
    bins = fourier.fourier_bins(w.nt, w.dt, STRIDE, 0.0, np.inf)
    near = np.argsort(np.abs(bins - w.f0), kind="stable")
    N = fourier.n_samples(w.nt, STRIDE)
    cells = int(np.prod(w.shape))
    doc = {"config": w.name, "shape": list(w.shape), "nt": w.nt, "npml": w.npml, "dtype": "float32",
           "update_form": "increment", "image_stride": STRIDE, "reps": reps, "rows": []}
    res = [None]
    for i, (nf, B) in enumerate(CONFIGS):
        f = np.sort(bins[near[:nf]])
        with Engine(w.shape, w.h, w.dt, w.nt, order=w.order, npml=w.npml, update_form="increment", image_stride=STRIDE,
                    fourier=f, fourier_batch=B) as e:
            e.set_model(w.c.astype(np.float32))
            row = {"F": nf, "B": B, "kernel": e.kernel_name,
                   "time_domain": timed(e, src, wav, rec, res, e.adjoint, reps),
                   "spectral": timed(e, src, wav, rec, res, e.adjoint_spectral, reps),
                   "model_bytes_per_cell_over_native": N * (E + 8 * E * nf / B) + (4 * nf + 2) * E,
                   "model_bytes_per_cell_over_time_domain": N * (2 * E * nf / B - E) + (4 * nf + 2) * E}
            if i == len(CONFIGS) - 1:  # the native store, same process, same context
                e.set_fourier_store(None)
                doc["native"] = timed(e, src, wav, rec, res, e.adjoint, reps)
            doc["rows"].append(row)
            print(json.dumps(row), flush=True)
    t_nat = doc["native"]["shot_gradient_ms"]
    for row in doc["rows"]:
        ts, tt = row["spectral"]["shot_gradient_ms"], row["time_domain"]["shot_gradient_ms"]
        row["spectral_over_native_ms"] = round(ts - t_nat, 2)
        row["spectral_over_time_domain_ms"] = round(ts - tt, 2)
        # the rate the model's added traffic would have to run at to explain the added time
        row["implied_TBps_over_native"] = round(row["model_bytes_per_cell_over_native"] * cells / ((ts - t_nat) * 1e9), 2)
    with open(out_path, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
