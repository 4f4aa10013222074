#!/usr/bin/env python3
"""Records which path the library gives every configuration of tests/_plan_cases.py, into tests/golden/plan_paths.json.

    python tools/plan_table.py --parent <commit>            on a GPU: one process, creation and destruction only
    python tools/plan_table.py --tuning                     no GPU: the launch shapes of the large grids (below)

The record is a statement about ONE commit -- the one the library was built from, named by --parent -- and is what
tests/test_plan_host.py (csrc/fwi_plan.cpp on the CPU) and tests/test_gpu_plan.py (a live context) are held to.  FWI_HIP_LIB
chooses the library as it does everywhere (full_waveform_inversion_amd/_lib.py).  Per case, with FWI_DEBUG_PML=1:

  rc, error    what fwi_create returned and, where it refused, fwi_last_error(NULL)
  line         the context's report of its path on stderr ("fwi: cpml=...")
  kernel       fwi_kernel_name
  offsets      the eight shifts of fwi_placement_info with FWI_PLACEMENT_TUNE=fixed:1,3,5,7,2 -- which arrays the context
               places and in which order; for a case that sets FWI_PLACEMENT_TUNE itself, the shifts under its own value
               (null under "force": the search times kernels, and what it finds is no property of the configuration)

--tuning: stream_default_tuning on grids too large to create cheaply, through tests/plan_host.cpp built with g++
(256^3, 384^3, 512^3, 768^3 fp32; 256^3 with a 16-cell CPML; 256^3 in increment form), under the key "tuning".
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_paths.json")

TUNING = [  # (name, shape, npml, abc, update_form)
    ("256^3", (256, 256, 256), 0, "sponge", "standard"), ("384^3", (384, 384, 384), 0, "sponge", "standard"),
    ("512^3", (512, 512, 512), 0, "sponge", "standard"), ("768^3", (768, 768, 768), 0, "sponge", "standard"),
    ("256^3 cpml 16", (256, 256, 256), 16, "cpml", "standard"), ("256^3 increment", (256, 256, 256), 0, "sponge", "increment"),
]


def config_ints(case, fixed):
    """The fifteen integers of tests/plan_host.cpp's input line (fwi_config from ndim to store_dtype, without device)."""
    from full_waveform_inversion_amd import _lib
    shape, kw = case["shape"], case["kw"]
    nz, nx, ny = shape[0], shape[-1], (shape[1] if len(shape) == 3 else 1)
    return [len(shape), nz, ny, nx, case["order"], fixed["nt_max"], case["npml"],
            _lib.F32 if case["dtype"] == "float32" else _lib.F64,
            {"auto": _lib.KERNEL_AUTO, "point": _lib.KERNEL_POINT, "stream": _lib.KERNEL_STREAM}[kw.get("kernel", "auto")],
            int(kw.get("zchunk", 0)), int(kw.get("ckpt_interval", 0)), int(kw.get("image_stride", 1)),
            _lib.UPDATE_FORMS[kw.get("update_form", "standard")], _lib.ABCS[case["abc"]],
            _lib.STORE_DTYPES[kw.get("store_dtype", "native")]]


def create(lib, case, env):
    """(rc, error, report line, kernel name, offsets) of one fwi_create + fwi_destroy under ``env``."""
    import _pointwise as pw
    import _plan_cases as pc
    from full_waveform_inversion_amd import _lib
    v = config_ints(case, pc.FIXED)
    cfg = _lib.Config(C.sizeof(_lib.Config), v[0], v[1], v[2], v[3], v[4], v[5], v[6], 0, v[7], v[8], v[9], v[10], v[11],
                      v[12], v[13], v[14], 0, pc.FIXED["h"], pc.FIXED["dt"], pc.FIXED["sigma_max"], pc.FIXED["pml_alpha_max"])
    ctx, lines = C.c_void_p(), []
    with pw.environment(dict(env, FWI_DEBUG_PML="1")):
        with pw.context_report(lines):
            rc = lib.fwi_create(C.byref(cfg), C.byref(ctx))
    line = next((ln for ln in lines if ln.startswith("fwi: cpml=")), None)
    if rc:
        return rc, (lib.fwi_last_error(None) or b"").decode(), line, None, None
    name = lib.fwi_kernel_name(ctx).decode()
    shifts = (C.c_int64 * 8)()
    assert lib.fwi_placement_info(ctx, None, None, shifts) == 0
    lib.fwi_destroy(ctx)
    return rc, None, line, name, [int(s) for s in shifts]


def record(case, lib):
    import _plan_cases as pc
    rc, error, line, name, offsets = create(lib, case, case["env"])
    if "FWI_PLACEMENT_TUNE" in case["env"]:
        if pc.searches(case):
            offsets = None
    elif rc == 0:
        offsets = create(lib, case, dict(case["env"], FWI_PLACEMENT_TUNE=pc.DISTINCT))[4]
    return dict(rc=rc, error=error, line=line, kernel=name, offsets=offsets)


def build_host_program(out_dir, name="plan_host", units=("fwi_plan.cpp",)):
    """tests/<name>.cpp over the host-only ``units`` of csrc/, with the address and undefined-behaviour sanitizers."""
    exe = os.path.join(out_dir, name)
    csrc = os.path.join(ROOT, "full_waveform_inversion_amd", "csrc")
    # (the sanitizers' runtimes inside the program: it then runs as it is, whatever else the loader brings along)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-static-libasan",
                           "-static-libubsan", "-g", "-I", csrc, os.path.join(ROOT, "tests", name + ".cpp")] +
                          [os.path.join(csrc, u) for u in units] + ["-o", exe])
    return exe


def build_points_program(out_dir):
    """tests/points_host.cpp: a shot's point tables (csrc/fwi_points.cpp) on the CPU; tests/test_points_host.py runs it."""
    return build_host_program(out_dir, "points_host", ("fwi_plan.cpp", "fwi_points.cpp"))


def run_host_program(exe, cases, env, fixed):
    """plan_host's answer for ``cases`` under the hooks ``env``, one dict per case."""
    text = "".join(" ".join(map(str, config_ints(c, fixed))) + "\n" for c in cases)
    clean = {k: v for k, v in os.environ.items() if not k.startswith("FWI_")}
    run = subprocess.run([exe, "plan"], input=text, capture_output=True, text=True, timeout=120, env=dict(clean, **env))
    assert run.returncode == 0, run.stderr
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    rows = [ln.split("\t") for ln in run.stdout.split("\n")[:-1]]
    assert len(rows) == len(cases), (len(rows), len(cases))
    keys = ("rc", "error", "line", "kernel", "place_kind", "place_mode", "fixed_k", "inc", "tune", "ptot", "esize")
    out = []
    for r in rows:
        d = dict(zip(keys, r))
        for k in ("rc", "place_kind", "place_mode", "inc", "ptot", "esize"):
            d[k] = int(d[k])
        d["fixed_k"] = [int(x) for x in d["fixed_k"].split(",")]
        d["tune"] = dict(zip(("ty", "zchunk", "pf", "tile_x"), map(int, d["tune"].split())))
        out.append(d)
    return out


def tuning_cases():
    return [dict(id=name, shape=list(shape), order=8, npml=npml, dtype="float32", abc=abc, kw={"update_form": form}, env={})
            for name, shape, npml, abc, form in TUNING]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", help="the commit the loaded library was built from")
    ap.add_argument("--tuning", action="store_true", help="record the large grids' launch shapes (no GPU)")
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    import _plan_cases as pc
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    if a.tuning:
        with tempfile.TemporaryDirectory() as tmp:
            got = run_host_program(build_host_program(tmp), tuning_cases(), {}, pc.FIXED)
        doc["tuning"] = {c["id"]: g["tune"] for c, g in zip(tuning_cases(), got)}
    else:
        if not a.parent:
            ap.error("--parent: say which commit the library was built from")
        from full_waveform_inversion_amd import _lib
        lib = _lib.load()
        doc["parent"] = a.parent
        doc["entries"] = {c["id"]: record(c, lib) for c in pc.CASES}
        print("%d entries recorded on %s (library %s)" % (len(doc["entries"]), a.parent, _lib.LIB_PATH))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
