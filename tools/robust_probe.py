"""Time of the robust misfits and of the median of |e| on the device (fwi_misfit_robust, fwi_residual_median) against
the call whose passes they share: per case one forward sweep, then `Engine.misfit_robust(d_obs, kind, thresh, weights,
taps)` per kind -- the upload of d_obs, of the weights and of the thresholds, the filter pass that forms e, the
elementwise robust source with its sums, the sum of the tiles per trace, the filter pass that forms r and the download
of J -- timed between two HIP events recorded on the null stream around the (synchronous) call, after two warm-up calls
of the same shape, 9 repeats: median, least and largest are written, so that the spread is on record.  Beside it, timed
the same way on the same gather in the same run: `Engine.misfit_weighted(d_obs, weights, taps)`, which is the two filter
passes alone, and `Engine.residual_median(d_obs, weights, taps)` per trace and of the whole gather (one filter pass and
the radix select, 4 passes over e and the weights in fp32, 8 in fp64).  The expectation from the bytes is
misfit_weighted's two passes plus one elementwise pass over four arrays (e and g, the weights only where W is kept);
nothing is asserted.  Cases: a 2-D 1024^2 grid with 1000 receivers, nt = 1000, fp32 and fp64, weights, taps of half-width
16.  Writes one JSON document (default profiles/robust_probe.json)."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from traveltime_probe import event_times  # noqa: E402
from full_waveform_inversion_amd import Engine, cfl_dt, datafit as df, ricker  # noqa: E402


def _row(name, ts, **more):
    row = {"call": name, "device_ms": round(float(np.median(ts)), 3), "device_ms_min": round(min(ts), 3),
           "device_ms_max": round(max(ts), 3), "repeats": len(ts)}
    row.update(more)
    print(json.dumps(row), flush=True)
    return row


def probe(dtype, nt=1000, ntr=1000, R=16, shape=(1024, 1024), order=8):
    h, c = 10.0, 2000.0
    dt = 0.6 * cfl_dt(c, h, len(shape), order)
    rec = np.array([[8, 12 + x] for x in range(ntr)], np.int32)
    out = {"shape": list(shape), "nt": nt, "ntr": ntr, "dtype": dtype, "taps_halfwidth": R, "rows": []}
    rng = np.random.default_rng(0)
    with Engine(shape, h, dt, nt, order=order, dtype=dtype) as e:
        src = (np.array([[128, shape[1] // 2]], np.int32), ricker(nt, dt, 15.0))
        d = e.forward(np.full(shape, c, dtype), src, rec, save=False)
        # the data: the synthetics plus 1 % noise plus sparse spikes
        amp = 0.01 * np.abs(d).max()
        spikes = (rng.random(d.shape) < 0.02) * 30.0 * rng.choice([-1.0, 1.0], d.shape)
        d_obs = (d + amp * (rng.standard_normal(d.shape) + spikes)).astype(dtype)
        M = (0.5 + 0.5 * rng.random(d.shape)).astype(dtype)
        taps = df.lowpass_taps(dt, 60.0, R)
        med, count = e.residual_median(d_obs, M, taps)
        sigma = df.MAD_TO_SIGMA * med
        assert np.all(sigma > 0.0)
        tw = event_times(lambda: e.misfit_weighted(d_obs, M, taps))
        weighted = float(np.median(tw))
        out["rows"].append(_row("misfit_weighted", tw))
        for kind in df.ROBUST_KINDS:
            a = df.ROBUST_C[kind] * sigma
            for keep in (False, True):
                ts = event_times(lambda: e.misfit_robust(d_obs, kind, a, M, taps, keep_irls=keep))
                J, _, nout = e.misfit_robust(d_obs, kind, a, M, taps, per_trace=True)
                out["rows"].append(_row("misfit_robust", ts, kind=kind, keep_irls=keep,
                                        over_misfit_weighted=round(float(np.median(ts)) / weighted, 2),
                                        share_beyond_threshold=float(nout.sum()) / float(count.sum()), J=J))
        for per_trace in (True, False):
            ts = event_times(lambda: e.residual_median(d_obs, M, taps, per_trace))
            out["rows"].append(_row("residual_median", ts, segment="trace" if per_trace else "gather",
                                    over_misfit_weighted=round(float(np.median(ts)) / weighted, 2)))
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "robust_probe.json")
    res = [probe("float32"), probe("float64")]
    with open(path, "w") as fh:
        json.dump({"tool": "tools/robust_probe.py",
                   "unit": "device: ms per Engine call (weights and taps), HIP events on the null stream around the "
                           "synchronous call, uploads and the download of J included, median / least / largest of 9 after "
                           "2 warm-up calls",
                   "cases": res}, fh, indent=1)
        fh.write("\n")
