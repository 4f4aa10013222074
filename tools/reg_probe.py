"""Time of the regularisation kernel (fwi_vec_regularizer) against its yardsticks: medians of the time per call at
256^3 and 1024^2 (fp32) for both kinds, with and without a prior x0, gradient form (v = d, out := alpha L + out) --
and, on the same context and vectors, of fwi_vec_axpby with x != y, which moves 12 B per cell (two reads, one write).
The byte floor of a call is one read of each input vector and one write (and, beta != 0, one read) of out, at the
6.29 TB/s copy ceiling the repository uses.  The C call is made with value_out = NULL, so that it stays stream-ordered;
`with_value_us` is the Python method, which waits for R.  `shot` adds the time of one 256^3 shot gradient (cfg5).
Writes one JSON document (default profiles/r08_regularizer.json).  Calls are timed in batches of 16 between two
synchronisations of the context's stream."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from full_waveform_inversion_amd import Engine, _lib, shots as sh, workloads  # noqa: E402

COPY_CEILING = 6.29e12  # B/s


def median_us(e, fn, reps=25, warm=3, calls=16):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        e.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        e.synchronize()
        ts.append((time.perf_counter() - t0) / calls * 1e6)
    return float(np.median(ts))


def probe(shape, eps=0.3):
    nd, n = len(shape), int(np.prod(shape))
    out = {"shape": list(shape), "dtype": "float32", "vector_MiB": round(n * 4 / 2 ** 20, 1), "rows": []}
    rng = np.random.default_rng(0)
    with Engine(shape, 10.0, 1e-3, 4) as e:
        e.vec_create(4)
        e.vec_upload(0, (2000.0 + rng.standard_normal(shape)).astype(np.float32))
        e.vec_upload(1, (2000.0 + 0.5 * rng.standard_normal(shape)).astype(np.float32))
        e.vec_upload(2, rng.standard_normal(shape).astype(np.float32))
        axpby = median_us(e, lambda: e.vec_axpby(3, 0.5, 2, 0.5))  # x != y: 12 B per cell
        out["axpby_us"] = round(axpby, 2)
        out["axpby_floor_us"] = round(12.0 * n / COPY_CEILING * 1e6, 2)
        w = np.ones(nd)
        wp = w.ctypes.data_as(C.POINTER(C.c_double))
        raw, ctx = e._lib.fwi_vec_regularizer, e._c
        for kind in ("tikhonov", "tv"):
            for x0 in (-1, 1):
                for v, beta in ((-1, 1.0), (-1, 0.0), (2, 0.0)):
                    def fn():
                        _lib.check(e._ctx, raw(ctx, _lib.REG_KINDS[kind], 0, x0, v, 3, 1e-3, beta, wp, eps, None))
                    vectors = 1 + (x0 >= 0) + (v >= 0) + 1 + (beta != 0.0)  # reads of x, x0, v, write (and read) of out
                    floor = 4.0 * n * vectors / COPY_CEILING * 1e6
                    t = median_us(e, fn)
                    row = {"kind": kind, "x0": x0 >= 0, "v": v >= 0, "beta": beta, "us": round(t, 2),
                           "bytes_per_cell_floor": 4 * vectors, "floor_us": round(floor, 2),
                           "ratio_to_floor": round(t / floor, 2), "ratio_to_axpby": round(t / axpby, 2),
                           "ratio_to_axpby_per_byte": round(t / axpby * 12.0 / (4 * vectors), 2)}
                    if v < 0 and beta == 1.0:
                        row["with_value_us"] = round(median_us(
                            e, lambda: e.vec_regularizer(0, out=3, kind=kind, x0=None if x0 < 0 else x0, alpha=1e-3,
                                                         beta=1.0, weight=1.0, eps=eps), calls=4), 2)
                    out["rows"].append(row)
    return out


def shot_gradient_seconds():
    """One forward + adjoint + gradient of one cfg5 shot at 256^3, the second of two evaluations."""
    w = workloads.cfg5(1.0, nshots=1)
    shots = [sh.Shot(w.src_idx[:1], w.wavelet(), w.rec_idx)]
    from full_waveform_inversion_amd import default_sigma_max
    with sh.inversion_engine(w.shape, w.h, w.dt, w.nt, order=w.order, npml=w.npml,
                             sigma_max=default_sigma_max(float(w.c.max()), w.h, w.npml)) as e:
        sh.model_data(e, w.c.astype(np.float32), shots)
        e.vec_create(2)
        e.vec_upload(0, w.c_init.astype(np.float32))
        ts = []
        for _ in range(2):
            t0 = time.perf_counter()
            sh.misfit_and_gradient_device(e, 0, 1, shots)
            e.synchronize()
            ts.append(time.perf_counter() - t0)
    return {"shape": list(w.shape), "nt": w.nt, "seconds": [round(t, 4) for t in ts]}


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "shot"]
    path = args[0] if args else os.path.join("profiles", "r08_regularizer.json")
    res = [probe((256, 256, 256)), probe((1024, 1024))]
    for r in res:
        print(json.dumps(r), flush=True)
    doc = {"tool": "tools/reg_probe.py", "unit": "us per call, median of 25 batches of 16 stream-ordered calls",
           "copy_ceiling_TB_s": COPY_CEILING / 1e12, "cases": res}
    if "shot" in sys.argv[1:]:
        doc["shot_gradient_256"] = shot_gradient_seconds()
        print(json.dumps(doc["shot_gradient_256"]), flush=True)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
