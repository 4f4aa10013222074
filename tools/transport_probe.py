"""Time of the optimal-transport misfit on the device (fwi_misfit_transport) against what a user has for this objective
without it, and against its sibling: per case one forward sweep, then `Engine.misfit_transport(d_obs, transform, param,
weights, taps)` -- the upload of d_obs and of the weights, the filter passes where there are taps, the nine launches of
fwi_ot.hip, the copy or filter of g into place and the download of J -- timed between two HIP events recorded on the null
stream around the (synchronous) call, after two warm-up calls of the same shape, 9 repeats: median, least and largest are
written, so that the spread is on record; `Engine.misfit_traveltime` at max_lag = 64 on the same gather, timed the same
way, as the yardstick; and the host path in the same process: the download of the (nt, ntr) synthetics and the upload of
the residual (plain hipMemcpy between a device buffer and a NumPy array of the data's size, each timed on its own) plus
the fp64 NumPy twin `datafit.TransportW2`, wall clock, median of 3.  Nothing is asserted about which side wins: a row whose
device time is not below the host path's says `"device_faster": false`.  Cases: a 2-D 1024^2 grid with 1000 receivers,
nt = 1000, fp32 and fp64, both transforms, with and without taps (R = 32).  The bytes the kernels move, counted from the
shapes, are written beside the times; no kernel-only time is taken here, so no rate is derived from them.  Writes one
JSON document (default profiles/transport_probe.json)."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import match_probe as mp  # noqa: E402
from traveltime_probe import event_times  # noqa: E402
from full_waveform_inversion_amd import Engine, cfl_dt, datafit as df, ricker  # noqa: E402


def kernel_bytes(nt, ntr, es):
    """what the nine launches read and write in the (nt, ntr) gathers (the slice sums and per-trace arrays are a few per
    cent of that): ot_density 3 T in, 2 fp64 out; ot_cdf 2 in, 2 out; ot_search 2 in and the walk over 2 more, 2 out;
    ot_dual 4 in, 1 out; ot_source 2 T and 1 fp64 in, 1 T out"""
    n = nt * ntr
    return n * (6 * es + 18 * 8)


def probe(dtype, nt=1000, ntr=1000, shape=(1024, 1024), order=8, R=32):
    h, c = 10.0, 2000.0
    dt = 0.6 * cfl_dt(c, h, len(shape), order)
    es = np.dtype(dtype).itemsize
    rec = np.array([[8, 12 + x] for x in range(ntr)], np.int32)
    out = {"shape": list(shape), "nt": nt, "ntr": ntr, "dtype": dtype, "rows": []}
    rng = np.random.default_rng(0)
    n = nt * ntr
    down, up = mp.copies_ms(n * es)
    with Engine(shape, h, dt, nt, order=order, dtype=dtype) as e:
        src = (np.array([[128, shape[1] // 2]], np.int32), ricker(nt, dt, 15.0))
        d = e.forward(np.full(shape, c, dtype), src, rec, save=False)
        # the data: the synthetics 7 samples early (the synthetics arrive late), another gain, a little noise
        d_obs = (1.3 * np.roll(d, -7, axis=0) + 1e-3 * np.abs(d).max() * rng.standard_normal(d.shape)).astype(dtype)
        M = (0.5 + 0.5 * rng.random(d.shape)).astype(dtype)
        tt = event_times(lambda: e.misfit_traveltime(d_obs, 64, M))
        out["traveltime_max_lag_64_ms"] = round(float(np.median(tt)), 3)
        for transform in ("softplus", "linear"):
            for taps in (None, df.lowpass_taps(dt, 30.0, R)):
                twin = df.TransportW2(dt, transform, None, taps, dtype=dtype)
                p = twin.param_of(d_obs)
                ts = event_times(lambda: e.misfit_transport(d_obs, transform, p, M, taps))
                dev = float(np.median(ts))
                J, W, counts = e.misfit_transport(d_obs, transform, p, M, taps, per_trace=True)
                host_fn = mp.wall_ms(lambda: twin(d, d_obs, M))
                Jt = twin(d, d_obs, M)[0]
                assert Jt > 0.0 and twin.counts.all(), "a trace does not count"
                host = down + host_fn + up
                out["rows"].append({"transform": transform, "param": p, "taps": None if taps is None else R,
                                    "device_ms": round(dev, 3), "device_ms_min": round(min(ts), 3),
                                    "device_ms_max": round(max(ts), 3), "repeats": len(ts),
                                    "host_path_ms": round(host, 1), "host_download_ms": round(down, 2),
                                    "host_twin_ms": round(host_fn, 1), "host_upload_ms": round(up, 2),
                                    "host_over_device": round(host / dev, 1), "device_faster": bool(dev < host),
                                    "device_over_traveltime": round(dev / out["traveltime_max_lag_64_ms"], 2),
                                    "J_rel_diff_to_twin": abs(J - Jt) / Jt,
                                    "traces_that_count": int(counts.sum()), "pcie_bytes": 2 * n * es,
                                    "kernel_gather_bytes": kernel_bytes(nt, ntr, es)})
                print(json.dumps(out["rows"][-1]), flush=True)
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "transport_probe.json")
    res = [probe("float32"), probe("float64")]
    with open(path, "w") as fh:
        json.dump({"tool": "tools/transport_probe.py",
                   "unit": "device: ms per Engine.misfit_transport call (weights; with and without taps), HIP events, median "
                           "/ least / largest of 9 after 2 warm-up calls; traveltime_max_lag_64_ms: Engine.misfit_traveltime "
                           "on the same gather, timed the same way; host: ms of download + datafit.TransportW2 + upload (16 "
                           "CPU threads), wall clock, median of 3",
                   "cases": res}, fh, indent=1)
        fh.write("\n")
