"""Time of the band-limited, weighted least-squares misfit on the device (fwi_misfit_weighted) against the host path it
replaces: per case one forward sweep, then `Engine.misfit_weighted(d_obs, weights, taps)` -- the upload of d_obs and of
the weights, the two filter passes, the sum and the download of J -- timed between two HIP events recorded on the null
stream around the (synchronous) call, after a warm-up, median of 5; and the host path that `objective=` ran before:
the download of the (nt, ntr) synthetics, the NumPy twin (`datafit.WeightedL2`) and the upload of the residual, each
timed on its own (the two copies as plain hipMemcpy between a device buffer and a NumPy array of the data's size) and
added.  A row whose device time is not below the host path's is marked `"device_faster": false` and the tool then exits
with status 1.  Cases: 3-D 256^3 with a 128 x 128 receiver plane and 2-D 1024^2 with 1024 receivers, nt = 1000, fp32, for
R = 0, 64 and 1024 (low-pass taps).  Writes one JSON document (default profiles/datafit_probe.json)."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from full_waveform_inversion_amd import Engine, cfl_dt, datafit as df, ricker  # noqa: E402

_hip = C.CDLL("libamdhip64.so")


def event_ms(fn, reps=5, warm=1):
    """Median over `reps` of the time of the synchronous call `fn()` between two events on the null stream."""
    a, b = C.c_void_p(), C.c_void_p()
    assert _hip.hipEventCreate(C.byref(a)) == 0 and _hip.hipEventCreate(C.byref(b)) == 0
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        ms = C.c_float(0.0)
        assert _hip.hipEventRecord(a, None) == 0
        fn()
        assert _hip.hipEventRecord(b, None) == 0 and _hip.hipEventSynchronize(b) == 0
        assert _hip.hipEventElapsedTime(C.byref(ms), a, b) == 0
        ts.append(ms.value)
    _hip.hipEventDestroy(a)
    _hip.hipEventDestroy(b)
    return float(np.median(ts))


def wall_ms(fn, reps=3):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def copies_ms(nbytes):
    """(download ms, upload ms) of `nbytes` between the device and a NumPy array, median of 3 each"""
    _hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    _hip.hipFree.argtypes = [C.c_void_p]
    dev, host = C.c_void_p(), np.zeros(nbytes, np.uint8)
    assert _hip.hipMalloc(C.byref(dev), nbytes) == 0
    hp = host.ctypes.data_as(C.c_void_p)
    try:
        assert _hip.hipMemcpy(dev, hp, nbytes, 1) == 0  # (the first copy also maps the pages)
        down = wall_ms(lambda: _hip.hipMemcpy(hp, dev, nbytes, 2))
        up = wall_ms(lambda: _hip.hipMemcpy(dev, hp, nbytes, 1))
    finally:
        _hip.hipFree(dev)
    return down, up


def probe(shape, rec, nt=1000, Rs=(0, 64, 1024), order=8):
    h, c = 10.0, 2000.0
    dt = 0.6 * cfl_dt(c, h, len(shape), order)
    ntr = len(rec)
    out = {"shape": list(shape), "nt": nt, "ntr": ntr, "dtype": "float32", "rows": []}
    rng = np.random.default_rng(0)
    down, up = copies_ms(nt * ntr * 4)
    with Engine(shape, h, dt, nt, order=order) as e:
        # (no deeper than 128 cells: the wave has to reach the receivers at depth 8 well within nt steps)
        src = (np.array([[min(shape[0] // 2, 128)] + [s // 2 for s in shape[1:]]], np.int32), ricker(nt, dt, 15.0))
        d = e.forward(np.full(shape, c, np.float32), src, rec, save=False)
        d_obs = (d + 1e-3 * np.abs(d).max() * rng.standard_normal(d.shape)).astype(np.float32)
        M = rng.random(d.shape).astype(np.float32)
        for R in Rs:
            taps = df.lowpass_taps(dt, 20.0, R)
            Re = min(R, nt - 1)
            dev = event_ms(lambda: e.misfit_weighted(d_obs, M, taps))
            J = e.misfit_weighted(d_obs, M, taps)
            obj = df.WeightedL2(taps)
            twin = wall_ms(lambda: obj(d, d_obs, M))
            host = down + twin + up
            Jt = obj(d, d_obs, M)[0]
            assert Jt > 0.0, "no signal at the receivers"
            n = nt * ntr
            # per output the kernel adds the taps that meet a sample: sum_n (min(n + R, nt - 1) - max(n - R, 0) + 1)
            k = np.arange(nt)
            fma = 2 * ntr * int(np.sum(np.minimum(k + Re, nt - 1) - np.maximum(k - Re, 0) + 1))
            out["rows"].append({"R": R, "device_ms": round(dev, 3), "host_path_ms": round(host, 1),
                                "host_download_ms": round(down, 2), "host_twin_ms": round(twin, 1),
                                "host_upload_ms": round(up, 2), "host_over_device": round(host / dev, 1),
                                "device_faster": bool(dev < host), "J_rel_diff": abs(J - Jt) / Jt,
                                "device_bytes": 7 * n * 4, "pcie_bytes": 2 * n * 4, "fp64_fma": fma,
                                "fp64_Gfma_per_s_of_the_call": round(fma / dev / 1e6, 1)})
            print(json.dumps(out["rows"][-1]), flush=True)
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "datafit_probe.json")
    plane = np.array([[8, y, x] for y in range(0, 256, 2) for x in range(0, 256, 2)], np.int32)
    line = np.array([[8, x] for x in range(1024)], np.int32)
    res = [probe((256, 256, 256), plane), probe((1024, 1024), line)]
    with open(path, "w") as f:
        json.dump({"tool": "tools/datafit_probe.py",
                   "unit": "device: ms per Engine.misfit_weighted call, HIP events, median of 5 after a warm-up; "
                           "host: ms of download + NumPy twin + upload, median of 3 each (16 CPU threads)",
                   "cases": res}, f, indent=1)
        f.write("\n")
    slower = [(c["shape"], r["R"]) for c in res for r in c["rows"] if not r["device_faster"]]
    if slower:
        sys.exit("the device path is not faster than the host path at %s" % slower)
