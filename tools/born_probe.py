#!/usr/bin/env python3
"""Per-step device time of the two Born paths beside the forward store sweep and the adjoint imaging sweep.

One process, one MI355X.  Per size and update form: one 3-D O(8) fp32 context with a 16-cell sponge, a random
heterogeneous model and dc a random field that is non-zero everywhere (so the Born field is populated wherever the
forward field is: zero data steps faster).  After a warm-up of every sweep, fwi_last_loop_ms / nt of

    forward(save)   adjoint(image)   born SCATTER   born FUSED        (the two Born modes alternating, --reps each)

Both Born modes read the same store and the same w.  The absolute times belong to the fill state of the field after
nt steps from one source (the wave has covered only part of the larger grids) and are labelled so.  The rule for
FWI_BORN_AUTO: FUSED iff its median is <= 0.90 x SCATTER's at every size in both forms and the gap
exceeds the min-max spread of both.

    python tools/born_probe.py --out profiles/r05_born.json                      # 256^3 x 400 and 512^3 x 100
    FWI_HIP_LIB=.../libfwi_hip_bornab.so python tools/born_probe.py --label ...  # an A/B build of the library
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from full_waveform_inversion_amd import Engine, cfl_dt, default_sigma_max, ricker  # noqa: E402


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def probe(n, nt, form, reps):
    shape = (n, n, n)
    rng = np.random.default_rng(n)
    c = (2000.0 + 600.0 * rng.random(shape, dtype=np.float32)).astype(np.float32)
    dc = (30.0 * rng.standard_normal(shape, dtype=np.float32)).astype(np.float32)
    dc[dc == 0.0] = 30.0
    h, npml = 10.0, 16
    dt = 0.6 * cfl_dt(2600.0, h, 3, 8)
    wav = ricker(nt, dt, 0.12 / dt / 8)
    src = np.array([[n // 2, n // 2, n // 2]])
    rec = np.stack([np.full(16, n // 2), np.full(16, n // 2), np.linspace(npml, n - npml - 1, 16).astype(int)], 1)
    out = {"shape": shape, "nt": nt, "update_form": form, "store_gib": nt * n ** 3 * 4 / 2 ** 30}
    with Engine(shape, h, dt, nt, order=8, npml=npml, sigma_max=default_sigma_max(2600.0, h, npml),
                update_form=form) as e:
        us = lambda: 1e3 * e.last_loop_ms() / nt  # noqa: E731
        d = e.forward(c, (src, wav), rec, save=True)
        out["kernel"] = e.kernel_name
        for mode in ("scatter", "fused"):  # warm-up of both paths (and of the adjoint)
            e.born(dc, mode=mode, download=False)
        e.adjoint(d)
        t = {"forward_store": [], "adjoint_image": [], "born_scatter": [], "born_fused": []}
        for _ in range(3):
            e.forward(None, (src, wav), rec, save=True)
            t["forward_store"].append(us())
            e.adjoint(d)
            t["adjoint_image"].append(us())
        e.forward(None, (src, wav), rec, save=True)
        for _ in range(reps):
            for mode in ("scatter", "fused"):
                J = e.born(dc, mode=mode)
                assert e.born_path == mode
                t["born_" + mode].append(us())
        out["dd_over_d"] = float(np.linalg.norm(J.astype(np.float64)) / np.linalg.norm(d.astype(np.float64)))
        # how much of the grid the forward field has reached (the fill state the times belong to)
        out["us_per_step"] = {k: stats(v) for k, v in t.items()}
    s, f = out["us_per_step"]["born_scatter"], out["us_per_step"]["born_fused"]
    out["fused_over_scatter"] = f["median"] / s["median"]
    out["fused_over_adjoint_image"] = f["median"] / out["us_per_step"]["adjoint_image"]["median"]
    spread = max(s["max"] - s["min"], f["max"] - f["min"])
    out["gate"] = bool(f["median"] <= 0.90 * s["median"] and s["median"] - f["median"] > spread)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256:400,512:100", help="n:nt,... (cubes of n^3 points, nt steps)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--label", default="default build")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    runs = []
    for item in a.sizes.split(","):
        n, nt = (int(v) for v in item.split(":"))
        for form in ("standard", "increment"):
            r = probe(n, nt, form, a.reps)
            runs.append(r)
            u = r["us_per_step"]
            print("%d^3 x %d %-9s forward %.1f  adjoint %.1f  scatter %.1f [%.1f .. %.1f]  fused %.1f [%.1f .. %.1f]  "
                  "fused/scatter %.3f  fused/adjoint %.3f  gate %s" % (
                      n, nt, form, u["forward_store"]["median"], u["adjoint_image"]["median"],
                      u["born_scatter"]["median"], u["born_scatter"]["min"], u["born_scatter"]["max"],
                      u["born_fused"]["median"], u["born_fused"]["min"], u["born_fused"]["max"],
                      r["fused_over_scatter"], r["fused_over_adjoint_image"], r["gate"]), flush=True)
    res = {"label": a.label, "library": os.environ.get("FWI_HIP_LIB", "libfwi_hip.so"),
           "note": "us per time step, device time of the sweep's time loop / nt; field after nt steps from one source "
                   "(partly filled grid at the larger sizes): absolute times belong to that fill state",
           "auto_is_fused": bool(all(r["gate"] for r in runs)), "runs": runs}
    print("AUTO = %s" % ("FUSED" if res["auto_is_fused"] else "SCATTER"))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
