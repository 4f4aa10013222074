"""Time of the cross-correlation traveltime misfit on the device (fwi_misfit_traveltime) against what a user has for this
objective without it: per case one forward sweep, then `Engine.misfit_traveltime(d_obs, max_lag, weights)` -- the upload
of d_obs and of the weights, the three kernels (correlations over 2 max_lag + 1 lags, pick, adjoint source), the copy of g
into place and the download of J -- timed between two HIP events recorded on the null stream around the (synchronous)
call, after two warm-up calls of the same shape, 9 repeats: median, least and largest are written, so that the spread is
on record; and the host path in the same process: the download of the (nt, ntr) synthetics and the upload of the residual
(plain hipMemcpy between a device buffer and a NumPy array of the data's size, each timed on its own) plus the fp64 NumPy
twin `datafit.TraveltimeL2`, wall clock, median of 3.  Nothing is asserted about which side wins: a row whose device time
is not below the host path's says `"device_faster": false`.  Cases: a 2-D 1024^2 grid with 1000 receivers, nt = 1000,
fp32 and fp64, max_lag in {16, 64, 256}.  The fp64 FMAs of tt_xcorr, nt ntr (2 Ke + 1), are counted from the shapes and
written beside the times; no kernel-only time is taken here, so no rate is derived from them.  Writes one JSON document
(default profiles/traveltime_probe.json)."""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import match_probe as mp  # noqa: E402
from full_waveform_inversion_amd import Engine, cfl_dt, datafit as df, ricker  # noqa: E402


def event_times(fn, reps=9, warm=2):
    """the times in ms of `reps` synchronous calls `fn()` between two events on the null stream, after `warm` calls"""
    hip = mp._hip
    a, b = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(a)) == 0 and hip.hipEventCreate(C.byref(b)) == 0
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        ms = C.c_float(0.0)
        assert hip.hipEventRecord(a, None) == 0
        fn()
        assert hip.hipEventRecord(b, None) == 0 and hip.hipEventSynchronize(b) == 0
        assert hip.hipEventElapsedTime(C.byref(ms), a, b) == 0
        ts.append(ms.value)
    hip.hipEventDestroy(a)
    hip.hipEventDestroy(b)
    return ts


def probe(dtype, nt=1000, ntr=1000, lags=(16, 64, 256), shape=(1024, 1024), order=8):
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
        for K in lags:
            ts = event_times(lambda: e.misfit_traveltime(d_obs, K, M))
            dev = float(np.median(ts))
            J, tau, lag = e.misfit_traveltime(d_obs, K, M, per_trace=True)
            twin = df.TraveltimeL2(dt, K, dtype=dtype)
            host_fn = mp.wall_ms(lambda: twin(d, d_obs, M))
            Jt = twin(d, d_obs, M)[0]
            assert Jt > 0.0, "no trace counts"
            host = down + host_fn + up
            out["rows"].append({"max_lag": K, "device_ms": round(dev, 3), "device_ms_min": round(min(ts), 3),
                                "device_ms_max": round(max(ts), 3), "repeats": len(ts),
                                "host_path_ms": round(host, 1), "host_download_ms": round(down, 2),
                                "host_twin_ms": round(host_fn, 1), "host_upload_ms": round(up, 2),
                                "host_over_device": round(host / dev, 1), "device_faster": bool(dev < host),
                                "J_rel_diff_to_twin": abs(J - Jt) / Jt, "lags_equal_to_twin": bool(np.array_equal(lag, twin.lags)),
                                "traces_that_count": int(twin.counts.sum()), "pcie_bytes": 2 * n * es,
                                "xcorr_fp64_fmas": n * (2 * min(K, nt - 1) + 1)})
            print(json.dumps(out["rows"][-1]), flush=True)
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "traveltime_probe.json")
    res = [probe("float32"), probe("float64")]
    with open(path, "w") as fh:
        json.dump({"tool": "tools/traveltime_probe.py",
                   "unit": "device: ms per Engine.misfit_traveltime call (weights, no taps), HIP events, median / least / "
                           "largest of 9 after 2 warm-up calls; host: ms of download + datafit.TraveltimeL2 + upload (16 CPU "
                           "threads), wall clock, median of 3",
                   "cases": res}, fh, indent=1)
        fh.write("\n")
