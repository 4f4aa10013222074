#!/usr/bin/env python3
"""What the eikonal solver and its adjoint cost on the device: writes profiles/eikonal_probe.json.

Per grid (1024^2 and 256^3, fp32) and source position (a corner, the centre): the launches and the wall time (a host
clock around calls that end in a device synchronise, best of --repeats after one warm-up call) of ``Engine.eikonal``
and ``Engine.eikonal_adjoint`` with one inner sweep per launch (FWI_EIKONAL_K=1) and with the built-in number, and
beside each the time that launch count's two model-sized streams (one read, one write of a vector per launch) would
take at the rate ``vec_axpby`` reaches in the same run -- the floor of a launch that moved nothing else.

``--twin``: the wall time of the NumPy twin on the CPU for the 2-D grid (the 3-D one takes the better part of an hour in
NumPy and is left out), merged into the same file; needs no GPU.  A record, not a bar: nothing is asserted.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "eikonal_probe.json")
GRIDS = [(1024, 1024), (256, 256, 256)]
H = 10.0


def model(shape):
    """1500 m/s at the top to 3500 m/s at the bottom with a smooth lateral undulation: no symmetry to help"""
    ax = np.meshgrid(*[np.linspace(0.0, 1.0, n) for n in shape], indexing="ij")
    return (1500.0 + 2000.0 * ax[0] + 200.0 * np.sin(6.0 * ax[-1]) * ax[0]).astype(np.float32)


def positions(shape):
    return {"corner": tuple(0 for _ in shape), "centre": tuple(n // 2 for n in shape)}


def timed(fn, repeats):
    fn()
    best = float("inf")
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best


def device(repeats):
    from full_waveform_inversion_amd import Engine, _lib
    rows = []
    for shape in GRIDS:
        c = model(shape)
        with Engine(shape, H, 1e-3, 2, order=4, npml=0, dtype="float32") as e:
            e.set_model(c)
            e.vec_create(4)
            n = 50

            def axpby():
                for _ in range(n):
                    e.vec_axpby(1, 0.5, 0, 0.5)
                e.synchronize()
            nbytes = 3 * c.size * 4  # y = a x + b y: two reads and a write
            rate = n * nbytes / timed(axpby, repeats)
            for where, src in positions(shape).items():
                for K in (1, _lib.EIKONAL_K[len(shape)]):
                    os.environ["FWI_EIKONAL_K"] = str(K)
                    t_fwd = timed(lambda: e.eikonal(src, 0, 1, radius=3.0), repeats)
                    n_fwd = e.last_eikonal_launches
                    rec = np.array([[m - 1 for m in shape], [m // 3 for m in shape]])
                    e.vec_scatter_points(2, rec, [1.0, -0.5])
                    t_adj = timed(lambda: e.eikonal_adjoint(0, 2, 3, 1), repeats)
                    n_adj = e.last_eikonal_launches
                    del os.environ["FWI_EIKONAL_K"]
                    stream = 2 * c.size * 4 / rate
                    rows.append({"shape": list(shape), "source": where, "K": K,
                                 "eikonal_launches": n_fwd, "eikonal_ms": round(1e3 * t_fwd, 3),
                                 "eikonal_stream_floor_ms": round(1e3 * n_fwd * stream, 3),
                                 "adjoint_launches": n_adj, "adjoint_ms": round(1e3 * t_adj, 3),
                                 "adjoint_stream_floor_ms": round(1e3 * n_adj * stream, 3),
                                 "vec_axpby_GBps": round(rate / 1e9, 1)})
                    print(json.dumps(rows[-1]), flush=True)
    return rows


def twin():
    from full_waveform_inversion_amd import eikonal as ek
    shape = GRIDS[0]
    c = model(shape)
    rows = []
    for where, src in positions(shape).items():
        t0 = time.perf_counter()
        T, sweeps = ek.solve(c, H, src, radius=3.0, dtype="float32", return_sweeps=True)
        rows.append({"shape": list(shape), "source": where, "what": "eikonal.solve (NumPy, Jacobi, fp32)", "sweeps": sweeps,
                     "seconds": round(time.perf_counter() - t0, 2)})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--twin", action="store_true", help="time the NumPy twin on the CPU instead (merged into the file)")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    rec = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            rec = json.load(f)
    if a.twin:
        rec["cpu_twin"] = twin()
    else:
        rec["device"] = device(a.repeats)
        rec["note"] = ("fp32; wall time around calls that synchronise, best of %d after a warm-up; stream floor = launches x "
                       "(one read + one write of a vector) at the vec_axpby rate of the same run" % a.repeats)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
