#!/usr/bin/env python3
"""What the eikonal tangent costs on the device, beside the adjoint: writes profiles/eikonal_tangent_probe.json.

The grids, source positions and K values of tools/eikonal_probe.py (1024^2 and 256^3, fp32; a corner and the centre;
FWI_EIKONAL_K=1 and the built-in number).  Per row, in one process and on one context: the launches and the wall time
(a host clock around calls that end in a device synchronise, best of --repeats after one warm-up call) of
``Engine.eikonal_tangent`` and of ``Engine.eikonal_adjoint`` on the same times -- the adjoint is the reference: the
same structure with one more cell of halo and twice the local-solver evaluations.  Then, at the built-in K, one
``shots.TraveltimeOperator.hvp`` of a single shot with and without ``keep_times`` (two solves against three).
The rows above give the tangent a dense perturbation and the adjoint the two-point right-hand side of
tools/eikonal_probe.py; ``input_density`` times both on a two-point and both on a dense input (corner source, built-in
K): a field that is non-zero everywhere changes in every workgroup of nearly every launch, and both iterations pay for it.
``--under-trace {dense,two-points}``: no timing and no file; three tangent and three adjoint solves per grid on that
input (corner source, built-in K), to be run under a kernel trace for kernel-only times, e.g.
``rocprofv3 --kernel-trace --stats --output-format csv -- python tools/eikonal_tangent_probe.py --under-trace dense``;
the figures of such a run are kept by hand under ``kernel_only`` in the file, which a later probe run leaves in place.
A record, not a bar: nothing is asserted.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

from eikonal_probe import GRIDS, H, model, positions, timed  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "eikonal_tangent_probe.json")


def device(repeats):
    from full_waveform_inversion_amd import Engine, _lib, shots as sh
    rows, products, density = [], [], []
    for shape in GRIDS:
        c = model(shape)
        dm = np.random.default_rng(0).standard_normal(shape).astype(np.float32)
        rec = np.array([[m - 1 for m in shape], [m // 3 for m in shape]])
        with Engine(shape, H, 1e-3, 2, order=4, npml=0, dtype="float32") as e:
            e.set_model(c)
            e.vec_create(8)
            T, SC, D, X, B, L = range(6)
            e.vec_upload(D, dm)
            for where, src in positions(shape).items():
                for K in (1, _lib.EIKONAL_K[len(shape)]):
                    os.environ["FWI_EIKONAL_K"] = str(K)
                    init = e.eikonal(src, T, SC, radius=3.0)
                    t_tan = timed(lambda: e.eikonal_tangent(T, D, X, SC, init), repeats)
                    n_tan = e.last_eikonal_launches
                    e.vec_scatter_points(B, rec, [1.0, -0.5])
                    t_adj = timed(lambda: e.eikonal_adjoint(T, B, L, SC), repeats)
                    n_adj = e.last_eikonal_launches
                    del os.environ["FWI_EIKONAL_K"]
                    rows.append({"shape": list(shape), "source": where, "K": K,
                                 "tangent_launches": n_tan, "tangent_ms": round(1e3 * t_tan, 3),
                                 "adjoint_launches": n_adj, "adjoint_ms": round(1e3 * t_adj, 3),
                                 "tangent_over_adjoint_per_launch": round((t_tan / n_tan) / (t_adj / n_adj), 3)})
                    print(json.dumps(rows[-1]), flush=True)
                    if K > 1 and where == "corner":  # both with a two-point and both with a dense input
                        for name in ("two points", "dense"):
                            if name == "dense":
                                e.vec_upload(6, dm)
                                e.vec_upload(B, dm)
                            else:
                                e.vec_scatter_points(6, rec, [1.0, -0.5])
                            tt = timed(lambda: e.eikonal_tangent(T, 6, X, SC, init), repeats)
                            nt = e.last_eikonal_launches
                            ta = timed(lambda: e.eikonal_adjoint(T, B, L, SC), repeats)
                            density.append({"shape": list(shape), "source": where, "K": K, "input": name,
                                            "tangent_launches": nt, "tangent_ms": round(1e3 * tt, 3),
                                            "adjoint_launches": e.last_eikonal_launches,
                                            "adjoint_ms": round(1e3 * ta, 3)})
                            print(json.dumps(density[-1]), flush=True)
                shot = [sh.Shot(np.array([src]), np.zeros(2, np.float32), rec)]
                row = {"shape": list(shape), "source": where}
                for keep in (True, False):
                    op = sh.TraveltimeOperator(e, None, shot, radius=3.0, keep_times=keep)
                    row["hvp_ms_keep_times" if keep else "hvp_ms_resolved"] = round(
                        1e3 * timed(lambda: op.hvp(dm), repeats), 3)
                products.append(row)
                print(json.dumps(row), flush=True)
    return rows, products, density


def under_trace(name):
    from full_waveform_inversion_amd import Engine
    for shape in GRIDS:
        rec = np.array([[m - 1 for m in shape], [m // 3 for m in shape]])
        with Engine(shape, H, 1e-3, 2, order=4, npml=0, dtype="float32") as e:
            e.set_model(model(shape))
            e.vec_create(6)
            T, SC, D, X, B, L = range(6)
            init = e.eikonal(positions(shape)["corner"], T, SC, radius=3.0)
            for slot in (D, B):
                if name == "dense":
                    e.vec_upload(slot, np.random.default_rng(0).standard_normal(shape).astype(np.float32))
                else:
                    e.vec_scatter_points(slot, rec, [1.0, -0.5])
            for _ in range(3):
                e.eikonal_tangent(T, D, X, SC, init)
            n_tan = e.last_eikonal_launches
            for _ in range(3):
                e.eikonal_adjoint(T, B, L, SC)
            print(name, shape, "launches per solve: tangent %d, adjoint %d" % (n_tan, e.last_eikonal_launches), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--under-trace", choices=["dense", "two-points"], default=None,
                    help="run the solves only, for a kernel trace (see the module's text)")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if a.under_trace:
        return under_trace(a.under_trace)
    rows, products, density = device(a.repeats)
    rec = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            rec = json.load(f)
    rec.update({"device": rows, "input_density": density, "hvp_one_shot": products,
                "note": "fp32; wall time around calls that synchronise, best of %d after a warm-up; tangent and adjoint in "
                        "the same process, context and times; hvp includes the upload of v and the download of the product"
                        % a.repeats})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
