"""Cost of the slant stack over vector slots (fwi_vec_shift_sum) against the bytes it must move, at the rate
fwi_fourier_gradient_vec reaches on the same context in the same run.  The workload of tools/feximage_probe.py: 256^3
O(8), sponge npml 16, increment form, fp32, nt = 1000, image stride 4, F = 8 bins next to the wavelet's peak, batch 8.
One engine runs forward(save) and adjoint_spectral once, so that the gradient call has its coefficients; 33 vector slots
hold standard-normal volumes.  Every row is then timed on that context: a host clock around `calls` consecutive calls
and one device synchronise, one warm-up round and `reps` timed rounds with the rows taken in turn inside every round (so
a drift of the machine falls on all of them); per call the median, the least and the largest round are written.

A call with nsrc sources must read each of them once and write dst: (nsrc + 1) e bytes per cell, + e with beta != 0.
The second tap of a source is the next plane of the same volume, which the thread one plane further reads as its first
tap: it should come from cache.  `ratio_to_bytes` is the call's time over the time its bytes take at the gradient call's
rate; the rows `whole` shift by whole cells (one tap), the rows `frac` by p h with p = tan 30 degrees (two taps, except
at h = 0), so their difference is what the second tap costs.  The last lines give a 17-lag, 33-angle gather (33 calls
of 17 sources) beside the download of its 33 angle images and of the 17 lag images it no longer downloads per shot.
Nothing is asserted.  Writes one JSON document (default profiles/slant_probe.json) and prints it."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from full_waveform_inversion_amd import Engine, fourier, workloads  # noqa: E402

STRIDE, E, NF, BATCH, NSRC, LAGS, ANGLES = 4, 4, 8, 8, (1, 9, 17, 33), 17, 33


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "slant_probe.json")
    calls = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    if reps < 5:
        raise SystemExit("the baseline's spread needs at least 5 timed rounds")
    w = workloads.cfg4(1.0, npml=16)
    wav, src, rec = w.wavelet(), w.src_idx[:1], w.rec_idx
    bins = fourier.fourier_bins(w.nt, w.dt, STRIDE, 0.0, np.inf)
    f = np.sort(bins[np.argsort(np.abs(bins - w.f0), kind="stable")[:NF]])
    cells = int(np.prod(w.shape))
    p = float(fourier.tangents(30.0)[0])
    doc = {"config": w.name, "shape": list(w.shape), "nt": w.nt, "npml": w.npml, "dtype": "float32",
           "update_form": "increment", "image_stride": STRIDE, "F": NF, "B": BATCH, "reps": reps, "calls_per_round": calls,
           "tangent": round(p, 6), "rows": {}}
    nmax = max(NSRC)
    dst, gslot = nmax, nmax + 1
    with Engine(w.shape, w.h, w.dt, w.nt, order=w.order, npml=w.npml, update_form="increment", image_stride=STRIDE,
                fourier=f, fourier_batch=BATCH) as e:
        e.set_model(w.c.astype(np.float32))
        d = e.forward(None, (src, wav), rec, save=True)
        e.adjoint_spectral(d * 0.5, image=False)
        e.vec_create(nmax + 2)
        rng = np.random.default_rng(0)
        for k in range(nmax):
            e.vec_upload(k, rng.standard_normal(w.shape, dtype=np.float32))
        rows = {"fourier_gradient_vec": (lambda: e.fourier_gradient_vec(gslot, None, "slowness2"), (4 * NF + 3) * E)}
        for n in NSRC:
            h = np.arange(n) - n // 2
            slots = list(range(n))
            rows["whole_%d" % n] = (lambda s=slots, h=h: e.vec_shift_sum(dst, s, h.astype(np.float64)), (n + 1) * E)
            rows["frac_%d" % n] = (lambda s=slots, h=h: e.vec_shift_sum(dst, s, p * h), (n + 1) * E)
        h = np.arange(LAGS) - LAGS // 2
        rows["frac_%d_beta" % LAGS] = (lambda: e.vec_shift_sum(dst, list(range(LAGS)), p * h, None, 1.0), (LAGS + 2) * E)
        rows["download"] = (lambda: e.vec_download(dst), None)
        times = {k: [] for k in rows}
        for r in range(reps + 1):
            for k, (fn, _) in rows.items():
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
        if rows[k][1] is not None:
            doc["rows"][k]["bytes_per_cell"] = rows[k][1]
            doc["rows"][k]["model_TBps"] = round(rows[k][1] * cells / (np.median(t) * 1e9), 2)
    base = doc["rows"]["fourier_gradient_vec"]
    doc["baseline_spread_max_over_min"] = round(base["ms_max"] / base["ms_min"], 3)
    for k, row in doc["rows"].items():
        if k not in ("fourier_gradient_vec", "download"):
            row["ratio_to_bytes"] = round(row["ms"] / (base["ms"] * row["bytes_per_cell"] / base["bytes_per_cell"]), 3)
    doc["gather_lags"], doc["gather_angles"] = LAGS, ANGLES
    doc["gather_transform_ms"] = round(ANGLES * doc["rows"]["frac_%d" % LAGS]["ms"], 3)
    doc["gather_angle_download_ms"] = round(ANGLES * doc["rows"]["download"]["ms"], 3)
    doc["gather_lag_download_ms_per_shot"] = round(LAGS * doc["rows"]["download"]["ms"], 3)
    with open(out_path, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
