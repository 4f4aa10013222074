#!/usr/bin/env python3
"""What the walled and slot-started eikonal solves cost on the device: writes profiles/eikonal_stage_probe.json.

In ONE run, per grid of tools/eikonal_probe.py (1024^2 and 256^3, fp32, its model, a source near the top centre with a
ball of 3 cells): the wall time (a host clock around calls that end in a device synchronise; one warm-up call, then
--repeats calls: the median, the fastest and the slowest) and the launches of

  * ``fwi_eikonal``                                        -- the yardstick of every ratio below, timed in this same run;
  * ``fwi_eikonal_stage`` with the same list and no wall   -- the same launches, the same bits (checked here);
  * ``fwi_eikonal_stage`` with a wall that walls nothing   -- the same iterates through the walled sweep: one more 4-byte
    read per cell beside the 12 bytes a launch moves (T in, T out, c), so 1.33 times is what its bytes explain;
  * a two-stage reflection off a flat reflector at 0.6 of the depth (``shots.Reflector.solve``: stage 1, the
    interface's values gathered and scattered, stage 2) and its adjoint chain (adjoint, handover, adjoint, two gradient
    passes).

A record, not a bar: nothing is asserted but the equality of the bits.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
from eikonal_probe import GRIDS, H, model  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "eikonal_stage_probe.json")
W, S0, T1, T2, SC, B, L2, HO, L1, G = range(10)


def timed(fn, repeats):
    """(median, fastest, slowest) seconds of `repeats` calls after one warm-up call"""
    fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), min(t), max(t)


def ms(t):
    return {"median_ms": round(1e3 * t[0], 3), "min_ms": round(1e3 * t[1], 3), "max_ms": round(1e3 * t[2], 3)}


def device(repeats):
    from full_waveform_inversion_amd import Engine, _lib, eikonal as ek, shots as sh
    rows = []
    for shape in GRIDS:
        c = model(shape)
        src = (2.3,) + tuple(0.5 * n + 0.4 for n in shape[1:])
        init = ek.ball(src, shape, H, 3.0)
        refl = sh.Reflector.at_depth(shape, float(int(0.6 * shape[0])))
        with Engine(shape, H, 1e-3, 2, order=4, npml=0, dtype="float32") as e:
            e.set_model(c)
            e.vec_create(10)
            _, args = e._init_args(init)
            n = C.c_int32(0)

            def stage(wall_slot):
                _lib.check(e._ctx, e._lib.fwi_eikonal_stage(e._c, T2, SC, wall_slot, *args, 0, C.byref(n)))

            t_plain = timed(lambda: e.eikonal(init, T1, SC), repeats)
            n_plain = e.last_eikonal_launches
            t_ref = e.vec_download(T1)
            t_stage = timed(lambda: stage(-1), repeats)
            n_stage = int(n.value)
            same = bool(np.array_equal(e.vec_download(T2), t_ref))
            e.vec_upload(W, np.zeros(shape, np.float32))
            t_wall = timed(lambda: stage(W), repeats)
            n_wall = int(n.value)
            same_wall = bool(np.array_equal(e.vec_download(T2), t_ref))
            assert same and same_wall and n_stage == n_plain == n_wall, (same, same_wall, n_plain, n_stage, n_wall)

            refl.upload(e, W, S0)
            launches = {}

            def forward():
                refl.solve(e, src, 3.0, W, S0, T1, T2, SC)

            t_fwd = timed(forward, repeats)
            e.eikonal(init, T1, SC, wall_slot=W)
            launches["stage 1"] = e.last_eikonal_launches
            forward()
            launches["stage 2"] = e.last_eikonal_launches
            rec = np.array([[1] + [m // 3 for m in shape[1:]], [1] + [m - 2 for m in shape[1:]]])
            e.vec_scatter_points(B, rec, [1.0, -0.5])

            def backward():
                sh._reflection_vjp(e, T1, T2, B, L2, HO, L1, G, SC, init, 0.0, "velocity")
                e.synchronize()

            t_bwd = timed(backward, repeats)
            row = {"shape": list(shape), "K": _lib.EIKONAL_K[len(shape)], "interface_nodes": int(refl.gamma.sum()),
                   "fwi_eikonal": dict(ms(t_plain), launches=n_plain),
                   "fwi_eikonal_stage, list, no wall": dict(ms(t_stage), launches=n_stage, same_bits=same,
                                                            ratio_to_fwi_eikonal=round(t_stage[0] / t_plain[0], 3)),
                   "fwi_eikonal_stage, list, a wall that walls nothing": dict(
                       ms(t_wall), launches=n_wall, same_bits=same_wall,
                       ratio_to_fwi_eikonal=round(t_wall[0] / t_plain[0], 3), ratio_its_bytes_explain=round(16 / 12, 3)),
                   "reflection, both stages": dict(ms(t_fwd), launches=launches,
                                                   ratio_to_fwi_eikonal=round(t_fwd[0] / t_plain[0], 3)),
                   "reflection, adjoint chain and gradient": dict(ms(t_bwd),
                                                                  ratio_to_fwi_eikonal=round(t_bwd[0] / t_plain[0], 3))}
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    rec = {"device": device(a.repeats),
           "note": "fp32; wall time around calls that synchronise: one warm-up call, then the median, the fastest and the "
                   "slowest of %d; every ratio is against fwi_eikonal's median in this same run" % a.repeats}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
