"""Cost of Born modelling on the Fourier store (fwi_fourier_born_vec) and of one lag of the extended scattering spectrum
(fwi_fbornx.hip, through fwi_fourier_born_extended_vec).  The workload of tools/fimage_probe.py: 256^3 O(8), sponge
npml 16, increment form, fp32, nt = 1000, image stride 4, batch 8, F = 4, 8, 16 bins next to the wavelet's peak.

Per F, on one Fourier-store engine after one forward(save): the time loop of `fourier_born_vec` (fwi_last_loop_ms, the
median of `reps` sweeps) beside the loop of `adjoint(image=True)` on the same context -- a sweep that already pays one
synthesis per batch -- and beside `born_vec(operator="imaging")` on a native-store engine with the same stride, which
pays none.

One lag of the extended source cannot be called on its own; it is timed on the same context after a forward of 8 steps
(two samples, so the sweep behind the lags is a few launches): the host clock around an extended call with 17 lags minus
the same call with one lag, over 16.  That is the cost of an ACCUMULATING lag (it reads and writes P_k); the first lag
only writes.  Rows: z, y, x with even h (vector reads of Q_k), x with odd h (element reads), time lag, beside
`fourier_gradient_vec`, the call that moves the most similar bytes ((4 F + 3) e per cell against (4 F + 1) e read and
2 F e written here).  Nothing is asserted.  Writes one JSON document (default profiles/fborn_probe.json) and prints it."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from full_waveform_inversion_amd import Engine, fourier, workloads  # noqa: E402

STRIDE, E, BATCH, LAGS, SHORT_NT = 4, 4, 8, 17, 8


def _median_loop(e, fn, reps):
    ms = []
    for r in range(reps + 1):
        fn()
        e.synchronize()
        if r >= 1:  # (the first sweep warms up)
            ms.append(e.last_loop_ms())
    return round(float(np.median(ms)), 3), round(min(ms), 3), round(max(ms), 3)


def _wall(e, fn, reps, calls=5):
    ms = []
    for r in range(reps + 1):
        e.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        e.synchronize()
        if r >= 1:
            ms.append((time.perf_counter() - t0) * 1e3 / calls)
    return float(np.median(ms))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "fborn_probe.json")
    w = workloads.cfg4(1.0, npml=16)
    wav, src, rec = w.wavelet(), w.src_idx[:1], w.rec_idx
    bins = fourier.fourier_bins(w.nt, w.dt, STRIDE, 0.0, np.inf)
    c = w.c.astype(np.float32)
    cells = int(np.prod(w.shape))
    kw = dict(order=w.order, npml=w.npml, update_form="increment", image_stride=STRIDE)
    doc = {"config": w.name, "shape": list(w.shape), "nt": w.nt, "npml": w.npml, "dtype": "float32",
           "update_form": "increment", "image_stride": STRIDE, "B": BATCH, "reps": reps, "gather_lags": LAGS,
           "short_nt": SHORT_NT, "rows": {}}
    with Engine(w.shape, w.h, w.dt, w.nt, **kw) as n:
        n.set_model(c)
        n.forward(None, (src, wav), rec, save=True)
        n.vec_create(1)
        n.vec_upload(0, np.full(w.shape, 10.0, np.float32))
        doc["native_born_imaging_loop_ms"] = _median_loop(
            n, lambda: n.born_vec(0, download=False, operator="imaging"), reps)
        doc["native_born_path"] = n.born_path
    for nf in (4, 8, 16):
        f = np.sort(bins[np.argsort(np.abs(bins - w.f0), kind="stable")[:nf]])
        row = {}
        with Engine(w.shape, w.h, w.dt, w.nt, fourier=f, fourier_batch=BATCH, **kw) as e:
            e.set_model(c)
            d0 = e.forward(None, (src, wav), rec, save=True)
            e.vec_create(1)
            e.vec_upload(0, np.full(w.shape, 10.0, np.float32))
            row["fourier_born_loop_ms"] = _median_loop(e, lambda: e.fourier_born_vec(0, download=False), reps)
            row["born_path"] = e.born_path
            row["adjoint_image_loop_ms"] = _median_loop(e, lambda: e.adjoint(d0), reps)
            row["fourier_born_over_native"] = round(row["fourier_born_loop_ms"][0] / doc["native_born_imaging_loop_ms"][0], 3)
            row["fourier_born_over_adjoint_image"] = round(row["fourier_born_loop_ms"][0] / row["adjoint_image_loop_ms"][0], 3)
            # one accumulating lag of the extended source, behind a sweep of SHORT_NT steps
            d = e.forward(None, (src, wav[:SHORT_NT]), rec, save=True)
            e.adjoint_spectral(d, image=False)
            row["fourier_gradient_vec_ms"] = round(_wall(e, lambda: e.fourier_gradient_vec(0, None, "slowness2"), reps, 20), 4)
            e.vec_upload(0, np.full(w.shape, 1e-3, np.float32))
            sets = {"z": ("offset", np.arange(1, LAGS + 1), "z"), "y": ("offset", np.arange(1, LAGS + 1), "y"),
                    "x_even_h": ("offset", 2 * np.arange(1, LAGS + 1), "x"),
                    "x_odd_h": ("offset", 2 * np.arange(1, LAGS + 1) - 1, "x"),
                    "time": ("timelag", STRIDE * w.dt * np.arange(1, LAGS + 1), None)}
            for k, (kind, lags, axis) in sets.items():
                many = _wall(e, lambda: e.fourier_born_extended_vec(kind, lags, [0] * LAGS, axis, download=False), reps)
                one = _wall(e, lambda: e.fourier_born_extended_vec(kind, lags[:1], [0], axis, download=False), reps)
                ms = (many - one) / (LAGS - 1)
                row["lag_" + k] = {"ms": round(ms, 4), "one_lag_call_ms": round(one, 3),
                                   "model_TBps": round((6 * nf + 1) * E * cells / (ms * 1e9), 2),
                                   "over_fourier_gradient_vec": round(ms / row["fourier_gradient_vec_ms"], 3)}
            doc["kernel"] = e.kernel_name
        doc["rows"]["F%d" % nf] = row
    with open(out_path, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
