"""Time of the envelope misfit on the device (fwi_misfit_envelope) against the host path a user has without it: per case
one forward sweep, then `Engine.misfit_envelope(d_obs, hilbert, power, eps, weights)` -- the upload of d_obs and of the
weights, the forward kernel (H s, H d, the envelopes, e, g1, g2, the sum of e^2), the adjoint kernel (g1 - H g2) and the
download of J -- timed between two HIP events recorded on the null stream around the (synchronous) call, after a
warm-up, median of 5; and the host path: the download of the (nt, ntr) synthetics, the NumPy twin
(`datafit.EnvelopeL2`) and the upload of the residual, each timed on its own (the two copies as plain hipMemcpy between
a device buffer and a NumPy array of the data's size) and added.  Nothing is asserted about which side wins: a row
whose device time is not below the host path's says `"device_faster": false`.  Cases: a 2-D 1024^2 grid with 1000
receivers, nt = 1000, for Q = 128, 512, 2048 (datafit.hilbert_taps; 999 of the 2048 taps meet a sample) and both
powers in fp32 and fp64, without taps.  Writes one JSON document (default profiles/envelope_probe.json)."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from match_probe import copies_ms, event_ms, wall_ms  # noqa: E402
from full_waveform_inversion_amd import Engine, cfl_dt, datafit as df, ricker  # noqa: E402

PEAK_FMA_PER_S = 78.6e12 / 2.0  # fp64 vector peak of one MI355X as quoted at 2.4 GHz


def fma_count(nt, ntr, Q, odd_only=True):
    """fp64 FMAs per lane-complete call as the two kernels form them (csrc/fwi_envelope.hip): per block of 64 traces x
    32 times and per wave of 8 outputs, every group of 8 staged rows that can pair a tap with an output costs 64
    products per signal (32 where only the odd taps are formed), two signals forward and one in the adjoint."""
    Q = min(Q, nt - 1)
    groups = 0
    for t0 in range(0, nt, 32):
        lo, hi = max(t0 - Q, 0), min(t0 + 32 + Q, nt)
        for tn0 in range(t0, t0 + 32, 8):
            for m in range(lo, hi, 8):  # (chunks of 16 rows are two groups of 8)
                d0 = m - tn0
                groups += not (d0 + 7 < -Q or d0 - 7 > Q)
    lanes = (ntr + 63) // 64 * 64
    return 3 * groups * (32 if odd_only else 64) * lanes


def probe(dtype, nt=1000, ntr=1000, Qs=(128, 512, 2048), shape=(1024, 1024), order=8):
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
        d_obs = (1.3 * np.roll(d, 20, axis=0) + 1e-3 * np.abs(d).max() * rng.standard_normal(d.shape)).astype(dtype)
        M = rng.random(d.shape).astype(dtype)
        eps = df.envelope_floor(d_obs, 1.0)
        n = nt * ntr
        for Q in Qs:
            taps = df.hilbert_taps(Q)
            for power in (1, 2):
                dev = event_ms(lambda: e.misfit_envelope(d_obs, taps, power, eps, M))
                J = e.misfit_envelope(d_obs, taps, power, eps, M)
                obj = df.EnvelopeL2(taps, power, eps)
                twin = wall_ms(lambda: obj(d, d_obs, M))
                Jt = obj(d, d_obs, M)[0]
                assert Jt > 0.0, "no signal at the receivers"
                host = down + twin + up
                fma = fma_count(nt, ntr, Q)
                out["rows"].append({"Q": Q, "Q_used": min(Q, nt - 1), "power": power, "device_ms": round(dev, 3),
                                    "host_path_ms": round(host, 1), "host_download_ms": round(down, 2),
                                    "host_twin_ms": round(twin, 1), "host_upload_ms": round(up, 2),
                                    "host_over_device": round(host / dev, 1), "device_faster": bool(dev < host),
                                    "J_rel_diff": abs(J - Jt) / Jt, "pcie_bytes": 2 * n * es + 8 * min(Q, nt - 1),
                                    "fp64_fma": fma, "fp64_Gfma_per_s_of_the_call": round(fma / dev / 1e6, 1),
                                    "share_of_fp64_vector_peak": round(fma / (dev * 1e-3) / PEAK_FMA_PER_S, 4)})
                print(json.dumps(out["rows"][-1]), flush=True)
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "envelope_probe.json")
    res = [probe("float32"), probe("float64")]
    with open(path, "w") as fh:
        json.dump({"tool": "tools/envelope_probe.py",
                   "unit": "device: ms per Engine.misfit_envelope call (weights, no taps), HIP events, median of 5 after a "
                           "warm-up; host: ms of download + NumPy twin + upload (16 CPU threads)",
                   "cases": res}, fh, indent=1)
        fh.write("\n")
