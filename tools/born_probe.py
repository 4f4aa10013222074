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

Store modes (the imaging Born operator, fwi_born_imaging): --store, --image-stride and --ckpt each take a comma list;
the plain context (native store, stride 1, no checkpointing) is always measured first, in the same process, as the
baseline, then every other value of each flag on its own.  The bf16 store exists in standard form only.  A
checkpointed Born sweep recomputes the forward as it goes: its cost in forward sweeps is recorded
(born_over_forward_plain, against the store-free forward sweep of the same context).

    python tools/born_probe.py --store native,bf16 --image-stride 1,4 --ckpt 0,32 --forms standard \
        --out profiles/r06_born_modes.json
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


def probe(n, nt, form, reps, store="native", stride=1, ckpt=0):
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
    slots = (ckpt + 1) if ckpt else -(-nt // stride)
    out = {"shape": shape, "nt": nt, "update_form": form, "store_dtype": store, "image_stride": stride,
           "ckpt_interval": ckpt, "store_gib": slots * n ** 3 * (2 if store == "bf16" else 4) / 2 ** 30}
    with Engine(shape, h, dt, nt, order=8, npml=npml, sigma_max=default_sigma_max(2600.0, h, npml),
                update_form=form, store_dtype=store, image_stride=stride, ckpt_interval=ckpt) as e:
        us = lambda: 1e3 * e.last_loop_ms() / nt  # noqa: E731
        d = e.forward(c, (src, wav), rec, save=True)
        out["kernel"] = e.kernel_name
        for mode in ("scatter", "fused"):  # warm-up of both paths (and of the adjoint)
            e.born(dc, mode=mode, download=False, operator="imaging")
        e.adjoint(d)
        t = {"forward_plain": [], "forward_store": [], "adjoint_image": [], "born_scatter": [], "born_fused": []}
        for _ in range(3):
            e.forward(None, (src, wav), rec, save=False)
            t["forward_plain"].append(us())
            e.forward(None, (src, wav), rec, save=True)
            t["forward_store"].append(us())
            e.adjoint(d)
            t["adjoint_image"].append(us())
        e.forward(None, (src, wav), rec, save=True)
        for _ in range(reps):
            for mode in ("scatter", "fused"):
                J = e.born(dc, mode=mode, operator="imaging")
                assert e.born_path == mode
                t["born_" + mode].append(us())
        out["dd_over_d"] = float(np.linalg.norm(J.astype(np.float64)) / np.linalg.norm(d.astype(np.float64)))
        # how much of the grid the forward field has reached (the fill state the times belong to)
        out["us_per_step"] = {k: stats(v) for k, v in t.items()}
    s, f = out["us_per_step"]["born_scatter"], out["us_per_step"]["born_fused"]
    out["fused_over_scatter"] = f["median"] / s["median"]
    out["fused_over_adjoint_image"] = f["median"] / out["us_per_step"]["adjoint_image"]["median"]
    fp = out["us_per_step"]["forward_plain"]["median"]
    out["born_over_forward_plain"] = {"scatter": s["median"] / fp, "fused": f["median"] / fp}
    spread = max(s["max"] - s["min"], f["max"] - f["min"])
    out["gate"] = bool(f["median"] <= 0.90 * s["median"] and s["median"] - f["median"] > spread)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256:400,512:100", help="n:nt,... (cubes of n^3 points, nt steps)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--label", default="default build")
    ap.add_argument("--out", default="")
    ap.add_argument("--store", default="native", help="comma list of native, bf16")
    ap.add_argument("--image-stride", default="1", help="comma list of imaging strides")
    ap.add_argument("--ckpt", default="0", help="comma list of checkpoint intervals (0 = store every step)")
    ap.add_argument("--forms", default="standard,increment")
    a = ap.parse_args()
    configs = [("native", 1, 0)]  # the baseline first, then every other value of each flag on its own
    configs += [(v, 1, 0) for v in a.store.split(",") if v != "native"]
    configs += [("native", int(v), 0) for v in a.image_stride.split(",") if int(v) > 1]
    configs += [("native", 1, int(v)) for v in a.ckpt.split(",") if int(v) > 0]
    runs = []
    for item in a.sizes.split(","):
        n, nt = (int(v) for v in item.split(":"))
        for form, (store, stride, ckpt) in [(f, k) for k in configs for f in a.forms.split(",")]:
            if store == "bf16" and form != "standard":
                continue
            r = probe(n, nt, form, a.reps, store, stride, ckpt)
            runs.append(r)
            u = r["us_per_step"]
            print("%d^3 x %d %-9s %s S=%d K=%d  forward %.1f  adjoint %.1f  scatter %.1f [%.1f .. %.1f]  "
                  "fused %.1f [%.1f .. %.1f]  fused/scatter %.3f  fused/adjoint %.3f  gate %s" % (
                      n, nt, form, store, stride, ckpt, u["forward_store"]["median"], u["adjoint_image"]["median"],
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
