"""Cost of one lag of an extended image on the Fourier store (fwi_fourier_offset_image_vec, fwi_fourier_lag_image_vec)
beside the call it moves the bytes of, fwi_fourier_gradient_vec, and beside one model-sized download.  The workload of
tools/fimage_probe.py: 256^3 O(8), sponge npml 16, increment form, fp32, nt = 1000, image stride 4, F = 8 bins next to the
wavelet's peak, batch 8.  One engine runs forward(save) and adjoint_spectral once; every row is then timed on that
context: a host clock around `calls` consecutive calls, each of which ends in a device synchronise, one warm-up round and
`reps` timed rounds with the rows taken in turn inside every round (so a drift of the machine falls on all of them);
per call the median, the least and the largest round are written.  A lag reads the 4 F coefficient volumes and writes
one, then the scaling pass reads and writes that one: (4 F + 3) e bytes per cell, exactly those of the gradient call, so
the passes whose reads stay aligned vectors (z, y, x with h = 4, time) are expected at its time.  They are accepted when
their median lies within the gradient call's own largest round plus 10 % (the two half-shifted address streams share
cache lines differently); the element-read pass (x with h = 1) is reported without a bound.  The last lines compare a
17-lag gather's device time with the time to download its 17 images.  Writes one JSON document (default
profiles/feximage_probe.json) and prints it."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from full_waveform_inversion_amd import Engine, fourier, workloads  # noqa: E402

STRIDE, E, NF, BATCH, LAGS = 4, 4, 8, 8, 17


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "feximage_probe.json")
    calls = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    if reps < 5:
        raise SystemExit("the baseline's spread needs at least 5 timed rounds")
    w = workloads.cfg4(1.0, npml=16)
    wav, src, rec = w.wavelet(), w.src_idx[:1], w.rec_idx
    bins = fourier.fourier_bins(w.nt, w.dt, STRIDE, 0.0, np.inf)
    f = np.sort(bins[np.argsort(np.abs(bins - w.f0), kind="stable")[:NF]])
    cells = int(np.prod(w.shape))
    tau = STRIDE * w.dt
    doc = {"config": w.name, "shape": list(w.shape), "nt": w.nt, "npml": w.npml, "dtype": "float32",
           "update_form": "increment", "image_stride": STRIDE, "F": NF, "B": BATCH, "reps": reps, "calls_per_round": calls,
           "model_bytes_per_cell_per_lag": (4 * NF + 3) * E, "rows": {}}
    with Engine(w.shape, w.h, w.dt, w.nt, order=w.order, npml=w.npml, update_form="increment", image_stride=STRIDE,
                fourier=f, fourier_batch=BATCH) as e:
        e.set_model(w.c.astype(np.float32))
        d = e.forward(None, (src, wav), rec, save=True)
        e.adjoint_spectral(d * 0.5, image=False)
        e.vec_create(1)
        rows = {
            "fourier_gradient_vec": lambda: e.fourier_gradient_vec(0, None, "slowness2"),
            "offset_x_h4": lambda: e.fourier_offset_image_vec(0, "x", 4),
            "offset_x_h1": lambda: e.fourier_offset_image_vec(0, "x", 1),
            "offset_y_h1": lambda: e.fourier_offset_image_vec(0, "y", 1),
            "offset_z_h1": lambda: e.fourier_offset_image_vec(0, "z", 1),
            "time_lag": lambda: e.fourier_lag_image_vec(0, tau),
            "download": lambda: e.vec_download(0),
        }
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
        if k != "download":
            doc["rows"][k]["model_TBps"] = round(doc["model_bytes_per_cell_per_lag"] * cells / (np.median(t) * 1e9), 2)
    base = doc["rows"]["fourier_gradient_vec"]
    doc["baseline_spread_max_over_min"] = round(base["ms_max"] / base["ms_min"], 3)
    doc["aligned_bound_ms"] = round(1.10 * base["ms_max"], 4)
    for k in ("offset_x_h4", "offset_y_h1", "offset_z_h1", "time_lag"):
        doc["rows"][k]["within_bound"] = bool(doc["rows"][k]["ms"] <= doc["aligned_bound_ms"])
    slowest = max(doc["rows"][k]["ms"] for k in rows if k not in ("fourier_gradient_vec", "download"))
    doc["gather_lags"] = LAGS
    doc["gather_device_ms_slowest_row"] = round(LAGS * slowest, 3)
    doc["gather_download_ms"] = round(LAGS * doc["rows"]["download"]["ms"], 3)
    with open(out_path, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
