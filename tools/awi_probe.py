"""Time of the adaptive (per-trace matching-filter) misfit on the device (fwi_misfit_adaptive) against its neighbours: per
case one forward sweep, then `Engine.misfit_adaptive(d_obs, L, lam, weights)` -- the upload of d_obs and of the weights,
the correlations of both kinds, the per-trace solves, the adjoint source, the copy of g into place and the download of J
-- timed between two HIP events recorded on the null stream around the (synchronous) call, after two warm-up calls of the
same shape, 9 repeats: median, least and largest are written, so that the spread is on record.  Beside it, timed the same
way on the same gather, `Engine.misfit_traveltime(d_obs, 2 L, weights)`, whose correlations over 4 L + 1 lags are the
larger of this misfit's two correlation launches; the three phases of the call from the library's own HIP events
(`Engine.misfit_adaptive_ms`: correlations, solves with the sum of J, adjoint source; median of the 9 repeats); and the
host path in the same process: the download of the (nt, ntr) synthetics and the upload of the residual (plain hipMemcpy
between a device buffer and a NumPy array of the data's size, each timed on its own) plus the fp64 NumPy twin
`datafit.AdaptiveMatching`, wall clock, median of 3.  Nothing is asserted about which side wins.  Cases: a 2-D 1024^2
grid with 1000 receivers, nt = 1000, fp32 and fp64, L in {8, 32, 64}.  The fp64 FMAs are counted from the shapes and
written beside the times: nt (6 L + 2) per trace for the correlations as launched (both signs of the autocorrelation's
lags), K^3 / 6 for the factor, nt K for the source.  Writes one JSON document (default profiles/awi_probe.json)."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import match_probe as mp  # noqa: E402
from traveltime_probe import event_times  # noqa: E402
from full_waveform_inversion_amd import Engine, cfl_dt, datafit as df, ricker  # noqa: E402


def probe(dtype, nt=1000, ntr=1000, halves=(8, 32, 64), lam=1e-2, shape=(1024, 1024), order=8):
    h, c = 10.0, 2000.0
    dt = 0.6 * cfl_dt(c, h, len(shape), order)
    es = np.dtype(dtype).itemsize
    rec = np.array([[8, 12 + x] for x in range(ntr)], np.int32)
    out = {"shape": list(shape), "nt": nt, "ntr": ntr, "dtype": dtype, "lam": lam, "rows": []}
    rng = np.random.default_rng(0)
    n = nt * ntr
    down, up = mp.copies_ms(n * es)
    with Engine(shape, h, dt, nt, order=order, dtype=dtype) as e:
        src = (np.array([[128, shape[1] // 2]], np.int32), ricker(nt, dt, 15.0))
        d = e.forward(np.full(shape, c, dtype), src, rec, save=False)
        # the data: the synthetics 7 samples early (the synthetics arrive late), another gain, a little noise
        d_obs = (1.3 * np.roll(d, -7, axis=0) + 1e-3 * np.abs(d).max() * rng.standard_normal(d.shape)).astype(dtype)
        M = (0.5 + 0.5 * rng.random(d.shape)).astype(dtype)
        for L in halves:
            K = 2 * L + 1
            phases = []
            ts = event_times(lambda: (e.misfit_adaptive(d_obs, L, lam, M), phases.append(e.misfit_adaptive_ms())))
            phases = np.median(np.array(phases[-len(ts):]), axis=0)
            tt = event_times(lambda: e.misfit_traveltime(d_obs, 2 * L, M))
            dev, trav = float(np.median(ts)), float(np.median(tt))
            J, W, counts, _ = e.misfit_adaptive(d_obs, L, lam, M, per_trace=True)
            twin = df.AdaptiveMatching(dt, L, lam, dtype=dtype)
            host_fn = mp.wall_ms(lambda: twin(d, d_obs, M))
            Jt = twin(d, d_obs, M)[0]
            assert Jt > 0.0, "no trace counts"
            host = down + host_fn + up
            out["rows"].append({"L": L, "device_ms": round(dev, 3), "device_ms_min": round(min(ts), 3),
                                "device_ms_max": round(max(ts), 3), "repeats": len(ts),
                                "correlations_ms": round(float(phases[0]), 3), "solve_ms": round(float(phases[1]), 3),
                                "source_ms": round(float(phases[2]), 3),
                                "traveltime_max_lag_2L_ms": round(trav, 3), "device_over_traveltime": round(dev / trav, 2),
                                "host_path_ms": round(host, 1), "host_download_ms": round(down, 2),
                                "host_twin_ms": round(host_fn, 1), "host_upload_ms": round(up, 2),
                                "host_over_device": round(host / dev, 1), "device_faster": bool(dev < host),
                                "J_rel_diff_to_twin": abs(J - Jt) / Jt,
                                "counts_equal_to_twin": bool(np.array_equal(counts != 0, twin.counts)),
                                "traces_that_count": int(twin.counts.sum()),
                                "median_sqrt_W_over_dt": float(np.sqrt(np.median(W)) / dt), "pcie_bytes": 2 * n * es,
                                "correlation_fp64_fmas": n * (2 * min(L, nt - 1) + 1 + 2 * min(2 * L, nt - 1) + 1),
                                "factor_fp64_fmas": ntr * K ** 3 // 6, "source_fp64_fmas": n * K})
            print(json.dumps(out["rows"][-1]), flush=True)
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "awi_probe.json")
    res = [probe("float32"), probe("float64")]
    with open(path, "w") as fh:
        json.dump({"tool": "tools/awi_probe.py",
                   "unit": "device: ms per Engine.misfit_adaptive call (weights, no taps), HIP events, median / least / "
                           "largest of 9 after 2 warm-up calls; correlations / solve / source: ms of the call's three phases "
                           "from the library's HIP events (Engine.misfit_adaptive_ms), median of the same 9 calls; "
                           "traveltime_max_lag_2L_ms: Engine.misfit_traveltime at max_lag = 2 L on the same gather, timed the "
                           "same way; host: ms of download + datafit.AdaptiveMatching + upload (16 CPU threads), wall clock, "
                           "median of 3",
                   "cases": res}, fh, indent=1)
        fh.write("\n")
