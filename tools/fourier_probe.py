"""Cost and memory of the Fourier-compressed forward-term store (fwi_set_fourier_store) per shot-gradient, beside the
two modes a user has without it.  Shape: 256^3 O(8), sponge border, increment form, fp32, nt = 1000, image stride 4.  Per
row one engine: forward(save) + adjoint(image) of one shot, one warm-up pair and then `reps` timed pairs, wall clock
around work that ends in a device synchronise; median, least and largest are written so that the spread is on record.
Rows: the Fourier store with F in {4, 8, 16} frequencies (the bins next to the wavelet's peak frequency; the times do not
depend on their values) and batch B in {1, 2, 4, 8}; the native store at the same image stride; checkpointing with
ckpt_interval = 45 (image stride 1: the two do not combine).  `store_bytes` is what fwi_store_bytes reports after the
forward.  The byte model of DESIGN.md s.4n is written beside the measurement (`model_added_bytes_per_step_and_cell`, over
the native store); nothing is asserted about which mode is faster.  Writes one JSON document (default
profiles/fourier_probe.json) and prints it."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from full_waveform_inversion_amd import Engine, fourier, workloads  # noqa: E402

STRIDE = 4


def shot_gradient(w, reps, **kw):
    wav = w.wavelet()
    src, rec = w.src_idx[:1], w.rec_idx
    with Engine(w.shape, w.h, w.dt, w.nt, order=w.order, npml=w.npml, update_form="increment", **kw) as e:
        e.set_model(w.c.astype(np.float32))
        times, res, held = [], None, 0
        for r in range(reps + 1):
            e.reset_gradient()
            e.synchronize()
            t0 = time.perf_counter()
            d = e.forward(None, (src, wav), rec, save=True)
            if res is None:
                res, held = d * 0.5, e.store_bytes()
            e.adjoint(res)
            e.synchronize()
            if r >= 1:  # (the first pair allocates and warms up)
                times.append((time.perf_counter() - t0) * 1e3)
        return {"kernel": e.kernel_name, "shot_gradient_ms": round(float(np.median(times)), 2),
                "ms_min": round(min(times), 2), "ms_max": round(max(times), 2), "store_bytes": held, "reps": reps}


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "fourier_probe.json")
    w = workloads.cfg4(1.0, npml=16)
    bins = fourier.fourier_bins(w.nt, w.dt, STRIDE, 0.0, np.inf)
    near = np.argsort(np.abs(bins - w.f0), kind="stable")
    doc = {"config": w.name, "shape": list(w.shape), "nt": w.nt, "npml": w.npml, "dtype": "float32",
           "update_form": "increment", "image_stride": STRIDE, "rows": []}
    doc["rows"].append({"mode": "native", "image_stride": STRIDE, **shot_gradient(w, reps, image_stride=STRIDE)})
    doc["rows"].append({"mode": "checkpoint", "ckpt_interval": 45, "image_stride": 1,
                        **shot_gradient(w, reps, ckpt_interval=45)})
    for nf in (4, 8, 16):
        f = np.sort(bins[near[:nf]])
        for B in (1, 2, 4, 8):
            row = {"mode": "fourier", "F": nf, "B": B, "image_stride": STRIDE,
                   # analysis e + 4 e F / B and synthesis e + 2 e F / B per SAMPLED step, e = 4 bytes, one step in STRIDE
                   "model_added_bytes_per_step_and_cell": round((2 * 4 + 6 * 4 * nf / B) / STRIDE, 2),
                   **shot_gradient(w, reps, image_stride=STRIDE, fourier=f, fourier_batch=B)}
            doc["rows"].append(row)
            print(json.dumps(row), flush=True)
    with open(out_path, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
