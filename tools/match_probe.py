"""Time of the matching-filter misfit on the device (fwi_misfit_matched) against the host path a user has without it:
per case one forward sweep, then `Engine.misfit_matched(d_obs, L, mu, weights)` with the filter estimated -- the upload
of d_obs and of the weights, the normal equations, their download, the host solve, the two filter applications, the sum
and the download of J -- timed between two HIP events recorded on the null stream around the (synchronous) call, after
a warm-up, median of 5; and the host path: the download of the (nt, ntr) synthetics, the NumPy twin
(`datafit.MatchedL2`) and the upload of the residual, each timed on its own (the two copies as plain hipMemcpy between
a device buffer and a NumPy array of the data's size) and added.  Nothing is asserted about which side wins: a row
whose device time is not below the host path's says `"device_faster": false`.  Cases: a 2-D 1024^2 grid with 1000
receivers, nt = 1000, for L = 8, 32, 64 in fp32 and fp64, without taps.  Writes one JSON document (default
profiles/match_probe.json)."""
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


def probe(dtype, nt=1000, ntr=1000, Ls=(8, 32, 64), shape=(1024, 1024), order=8):
    h, c = 10.0, 2000.0
    dt = 0.6 * cfl_dt(c, h, len(shape), order)
    es = np.dtype(dtype).itemsize
    rec = np.array([[8, 12 + x] for x in range(ntr)], np.int32)
    out = {"shape": list(shape), "nt": nt, "ntr": ntr, "dtype": dtype, "rows": []}
    rng = np.random.default_rng(0)
    down, up = copies_ms(nt * ntr * es)
    with Engine(shape, h, dt, nt, order=order, dtype=dtype) as e:
        src = (np.array([[128, shape[1] // 2]], np.int32), ricker(nt, dt, 15.0))
        d = e.forward(np.full(shape, c, dtype), src, rec, save=False)
        d_obs = (1.3 * np.roll(d, 2, axis=0) + 1e-3 * np.abs(d).max() * rng.standard_normal(d.shape)).astype(dtype)
        M = rng.random(d.shape).astype(dtype)
        mu = df.prewhitening(d_obs, M, percent=0.1)
        n = nt * ntr
        for L in Ls:
            K = 2 * L + 1
            dev = event_ms(lambda: e.misfit_matched(d_obs, L, mu, M))
            J, f = e.misfit_matched(d_obs, L, mu, M)
            obj = df.MatchedL2(L, mu)
            twin = wall_ms(lambda: obj(d, d_obs, M), reps=1 if L > 8 else 3)
            Jt = obj(d, d_obs, M, shot=0)[0]
            ft = obj.filters[0]
            assert Jt > 0.0, "no signal at the receivers"
            host = down + twin + up
            nT = (K + 7) // 8
            fma_normal = n * (64 * nT * (nT + 1) // 2 + 8 * nT)  # as the kernel forms them: whole 8 x 8 tiles
            fma_apply = 2 * n * ((K + 7) // 8 * 8)
            out["rows"].append({"L": L, "K": K, "device_ms": round(dev, 3), "host_path_ms": round(host, 1),
                                "host_download_ms": round(down, 2), "host_twin_ms": round(twin, 1),
                                "host_upload_ms": round(up, 2), "host_over_device": round(host / dev, 1),
                                "device_faster": bool(dev < host), "J_rel_diff": abs(J - Jt) / Jt,
                                "f_rel_diff": float(np.linalg.norm(f - ft) / np.linalg.norm(ft)),
                                "pcie_bytes": 2 * n * es + (K * K + 2 * K + 1) * 8,
                                "fp64_fma_normal": fma_normal, "fp64_fma_apply": fma_apply,
                                "fp64_Gfma_per_s_of_the_call": round((fma_normal + fma_apply) / dev / 1e6, 1)})
            print(json.dumps(out["rows"][-1]), flush=True)
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "match_probe.json")
    res = [probe("float32"), probe("float64")]
    with open(path, "w") as fh:
        json.dump({"tool": "tools/match_probe.py",
                   "unit": "device: ms per Engine.misfit_matched call (filter estimated, weights, no taps), HIP events, "
                           "median of 5 after a warm-up; host: ms of download + NumPy twin + upload (16 CPU threads)",
                   "cases": res}, fh, indent=1)
        fh.write("\n")
