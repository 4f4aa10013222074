"""Time of the frequency-domain (spectral) misfit on the device (fwi_misfit_spectral) against what a user has for this
objective without it: per case one forward sweep, then `Engine.misfit_spectral(d_obs, freqs, kind, eps, weights)` -- the
upload of d_obs and of the weights, the three kernels (analysis, coefficients, adjoint source) and the download of J --
timed between two HIP events recorded on the null stream around the (synchronous) call, after a warm-up (which also
forms and uploads the table of twiddles: the timed calls reuse it), median of 5 with the least and the largest beside
it; and the host path: the download of the (nt, ntr) synthetics, the NumPy twin `datafit.SpectralMisfit` on them (wall
clock, median of 3) and the upload of the residual, each timed on its own (the two copies as plain hipMemcpy between a
device buffer and a NumPy array of the data's size) and added.  Nothing is asserted about which side wins: a row whose
device time is not below the host path's says `"device_faster": false`.  Cases: a 2-D 1024^2 grid with 1000 receivers,
nt = 1000, fp32 and fp64, F in {8, 16, 64} bins from 5 Hz up, kind `log` at F = 8 and 16 and `logamp` at 64, with weights,
no taps.  Writes one JSON document (default profiles/spectral_probe.json)."""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import match_probe as mp  # noqa: E402
from full_waveform_inversion_amd import Engine, cfl_dt, datafit as df, fourier, ricker  # noqa: E402


def event_ms3(fn, reps=5, warm=1):
    """(median, least, largest) over `reps` of the time of the synchronous call `fn()` between two events on the null
    stream, after `warm` calls"""
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
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def probe(dtype, nt=1000, ntr=1000, Fs=(8, 16, 64), shape=(1024, 1024), order=8):
    h, c = 10.0, 2000.0
    dt = 0.6 * cfl_dt(c, h, len(shape), order)
    es = np.dtype(dtype).itemsize
    rec = np.array([[8, 12 + x] for x in range(ntr)], np.int32)
    out = {"shape": list(shape), "nt": nt, "ntr": ntr, "dtype": dtype, "dt": dt, "rows": []}
    rng = np.random.default_rng(0)
    n = nt * ntr
    down, up = mp.copies_ms(n * es)
    with Engine(shape, h, dt, nt, order=order, dtype=dtype) as e:
        src = (np.array([[128, shape[1] // 2]], np.int32), ricker(nt, dt, 15.0))
        d = e.forward(np.full(shape, c, dtype), src, rec, save=False)
        d_obs = (1.3 * np.roll(d, 2, axis=0) + 1e-3 * np.abs(d).max() * rng.standard_normal(d.shape)).astype(dtype)
        M = (0.5 + 0.5 * rng.random(d.shape)).astype(dtype)
        for F in Fs:
            kind = "logamp" if F == 64 else "log"
            f = fourier.fourier_bins(nt, dt, 1, 5.0, 1e9)[:F]
            eps = df.spectral_floor(d_obs, dt, f, 1.0, M)
            twin = df.SpectralMisfit(dt, f, kind, eps, dtype=dtype)
            host_fn = mp.wall_ms(lambda: twin(d, d_obs, M))
            host = down + host_fn + up
            dev, lo, hi = event_ms3(lambda: e.misfit_spectral(d_obs, f, kind, eps, M))
            J = e.misfit_spectral(d_obs, f, kind, eps, M)
            Jt = twin(d, d_obs, M)[0]
            assert Jt > 0.0, "no signal at the receivers"
            out["rows"].append({"F": F, "kind": kind, "device_ms": round(dev, 3), "device_ms_min": round(lo, 3),
                                "device_ms_max": round(hi, 3), "host_path_ms": round(host, 1),
                                "host_download_ms": round(down, 2), "host_twin_ms": round(host_fn, 1),
                                "host_upload_ms": round(up, 2), "host_over_device": round(host / dev, 1),
                                "device_faster": bool(dev < host), "J_rel_diff_to_twin": abs(J - Jt) / Jt,
                                "pcie_bytes": 2 * n * es, "fp64_fma": 6 * F * n,
                                "kernel_bytes": 5 * n * es + 64 * F * ((nt + 255) // 256) * ntr + 57 * F * ntr})
            print(json.dumps(out["rows"][-1]), flush=True)
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "spectral_probe.json")
    res = [probe("float32"), probe("float64")]
    with open(path, "w") as fh:
        json.dump({"tool": "tools/spectral_probe.py",
                   "unit": "device: ms per Engine.misfit_spectral call (weights, no taps; uploads included), HIP events, "
                           "median of 5 after a warm-up with the least and the largest; host: ms of download + "
                           "datafit.SpectralMisfit + upload (16 CPU threads)",
                   "cases": res}, fh, indent=1)
        fh.write("\n")
