"""Time of the trace-normalised correlation misfit on the device (fwi_misfit_correlation) against what a user had for
this objective without it: per case one forward sweep, then `Engine.misfit_correlation(d_obs, eps, weights, taps)` -- the
upload of d_obs and of the weights, with taps the two passes of B before and the one after, the three kernels (per-trace
sums, coefficients, adjoint source) and the download of J -- timed between two HIP events recorded on the null stream
around the (synchronous) call, after a warm-up, median of 5; and the host path: the download of the (nt, ntr)
synthetics, `objectives.correlation` (which takes neither weights nor taps nor a floor) and the upload of the residual,
each timed on its own (the two copies as plain hipMemcpy between a device buffer and a NumPy array of the data's size)
and added.  Nothing is asserted about which side wins: a row whose device time is not below the host path's says
`"device_faster": false`.  Cases: a 2-D 1024^2 grid with 1000 receivers, nt = 1000, fp32 and fp64, without taps and with
`datafit.bandpass_taps(dt, 4, 30, R=64)`.  Writes one JSON document (default profiles/correlation_probe.json)."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from match_probe import copies_ms, event_ms, wall_ms  # noqa: E402
from full_waveform_inversion_amd import Engine, cfl_dt, datafit as df, objectives, ricker  # noqa: E402


def probe(dtype, nt=1000, ntr=1000, R=64, shape=(1024, 1024), order=8):
    h, c = 10.0, 2000.0
    dt = 0.6 * cfl_dt(c, h, len(shape), order)
    es = np.dtype(dtype).itemsize
    rec = np.array([[8, 12 + x] for x in range(ntr)], np.int32)
    out = {"shape": list(shape), "nt": nt, "ntr": ntr, "dtype": dtype, "rows": []}
    rng = np.random.default_rng(0)
    n = nt * ntr
    down, up = copies_ms(n * es)
    with Engine(shape, h, dt, nt, order=order, dtype=dtype) as e:
        src = (np.array([[128, shape[1] // 2]], np.int32), ricker(nt, dt, 15.0))
        d = e.forward(np.full(shape, c, dtype), src, rec, save=False)
        d_obs = (1.3 * np.roll(d, 20, axis=0) + 1e-3 * np.abs(d).max() * rng.standard_normal(d.shape)).astype(dtype)
        M = rng.random(d.shape).astype(dtype)
        eps = df.correlation_floor(d_obs, 1.0)
        host_fn = wall_ms(lambda: objectives.correlation(d, d_obs, per_trace=True))
        host = down + host_fn + up
        for taps in (None, df.bandpass_taps(dt, 4.0, 30.0, R)):
            dev = event_ms(lambda: e.misfit_correlation(d_obs, eps, M, taps))
            J = e.misfit_correlation(d_obs, eps, M, taps)
            Jt = df.NormalizedCorrelation(eps, taps, dtype=dtype)(d, d_obs, M)[0]
            assert Jt > 0.0, "no signal at the receivers"
            out["rows"].append({"taps_R": None if taps is None else R, "device_ms": round(dev, 3),
                                "host_path_ms": round(host, 1), "host_download_ms": round(down, 2),
                                "host_objective_ms": round(host_fn, 1), "host_upload_ms": round(up, 2),
                                "host_over_device": round(host / dev, 1), "device_faster": bool(dev < host),
                                "J_rel_diff_to_twin": abs(J - Jt) / Jt, "pcie_bytes": 2 * n * es,
                                "kernel_bytes_without_B": 7 * n * es})
            print(json.dumps(out["rows"][-1]), flush=True)
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "correlation_probe.json")
    res = [probe("float32"), probe("float64")]
    with open(path, "w") as fh:
        json.dump({"tool": "tools/correlation_probe.py",
                   "unit": "device: ms per Engine.misfit_correlation call (weights; without and with taps), HIP events, "
                           "median of 5 after a warm-up; host: ms of download + objectives.correlation + upload (16 CPU "
                           "threads)",
                   "cases": res}, fh, indent=1)
        fh.write("\n")
