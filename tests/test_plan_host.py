"""Which path a context takes (csrc/fwi_plan.cpp: plan_context), decided and checked where there is no GPU.
tests/plan_host.cpp is a program of its own over fwi_plan.cpp, built with the address and undefined-behaviour sanitizers;
the hooks reach it through its environment, and the cases that share a hook setting run in one process.  It is held to
tests/golden/plan_paths.json (tools/plan_table.py: what the library of the commit named there said of every case of
tests/_plan_cases.py on the GPU), to what the pointwise tables say their cases are meant for, to the recorded launch
shapes of the large grids, and to the size threshold of the placement search."""
import json
import os
import shutil
import subprocess
import sys

import pytest

import _plan_cases as pc
import _pointwise as pw
import _pointwise_born as pwb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import plan_table  # noqa: E402

MIB = 1 << 20
PLACE_SEARCH, PLACE_FIXED = 2, 3   # fwi::PlaceMode


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/plan_host.cpp")
    return plan_table.build_host_program(str(tmp_path_factory.mktemp("plan_host")))


@pytest.fixture(scope="module")
def golden():
    with open(plan_table.GOLDEN) as f:
        return json.load(f)


def plans(exe, cases, extra_env=None):
    """{id: plan_host's answer} for ``cases``, one process per distinct hook setting."""
    groups = {}
    for c in cases:
        groups.setdefault(tuple(sorted(dict(c["env"], **(extra_env or {})).items())), []).append(c)
    out = {}
    for env, group in groups.items():
        for c, got in zip(group, plan_table.run_host_program(exe, group, dict(env), pc.FIXED)):
            out[c["id"]] = got
    return out


def placed_offsets(plan):
    """The shifts fwi_placement_info reports for a plan whose layout is not timed: the movable arrays in search order
    (fwi_api.hip create_impl / fwi_create: ty, zeta_x, tz, psi_x and, in increment form, v; or v and C) sit fixed_k x 2 MiB
    into their allocations under "fixed:", at their start otherwise."""
    nmov = {0: 0, 1: 4 + plan["inc"], 2: 2}[plan["place_kind"]]
    k = plan["fixed_k"] if plan["place_mode"] == PLACE_FIXED else [0] * 8
    return [2 * MIB * k[i] if i < nmov else 0 for i in range(8)]


def test_every_recorded_case_plans_as_the_library_did(exe, golden):
    entries = golden["entries"]
    assert sorted(entries) == sorted(c["id"] for c in pc.CASES), "tests/golden/plan_paths.json is not of these cases"
    own = plans(exe, pc.CASES)
    asked = plans(exe, [c for c in pc.CASES if "FWI_PLACEMENT_TUNE" not in c["env"]], {"FWI_PLACEMENT_TUNE": pc.DISTINCT})
    for c in pc.CASES:
        want, got = entries[c["id"]], own[c["id"]]
        assert got["rc"] == want["rc"], (c["id"], got, want)
        assert ("fwi_create: " + got["error"] if got["rc"] else None) == want["error"], (c["id"], got, want)
        assert (got["line"] or None) == want["line"], (c["id"], got, want)
        assert (got["kernel"] or None) == want["kernel"], (c["id"], got, want)
        if got["place_mode"] == PLACE_SEARCH:   # (grids below the threshold: the layout is timed only when forced)
            assert pc.searches(c), (c["id"], got)
        if want["offsets"] is not None:
            plan = got if "FWI_PLACEMENT_TUNE" in c["env"] else asked[c["id"]]
            assert plan["rc"] == 0 and placed_offsets(plan) == want["offsets"], (c["id"], plan, want)


TABLE = ([("pointwise:", c, c.path == "pair3d") for c in pw.CASES] +
         [(p, c, False) for p, t in (("born:", [b.case for b in pwb.BORN_CASES]), ("bf16:", [b.case for b in pwb.BF16_CASES]),
                                     ("illum:", pwb.ILLUM_CASES)) for c in t])


def test_the_pointwise_tables_take_the_paths_they_are_meant_for(exe):
    """What _pointwise.engine_fields asserts of a live context about its path, without one."""
    got = plans(exe, [pc.from_table(p, c) for p, c, _ in TABLE])
    for prefix, c, pair in TABLE:
        g = got[pc.from_table(prefix, c)["id"]]
        assert g["rc"] == 0, (c, g)
        path = pw.context_path([g["line"]])
        assert g["kernel"] == c.kernel, (pw.case_id(c), g["kernel"], c.kernel)
        for k, v in c.ctx.items():
            assert path[k] == v, "%s: the plan has %s = %d, the case is meant for %d (%s)" % (pw.case_id(c), k, path[k], v, path)
        assert path["pair3d"] == int(pair), (pw.case_id(c), path)
        assert path["fused2d"] == int(c.kernel == "step2d_fused"), (pw.case_id(c), path)
        if "FWI_STREAM_TY" in c.env:
            assert path["ty"] == int(c.env["FWI_STREAM_TY"]), (pw.case_id(c), path)
        if len(c.shape) == 3 and c.kernel == "step3d_stream":
            assert not c.kw.get("zchunk") or path["zchunk"] == c.kw["zchunk"], (pw.case_id(c), path)


def test_large_grids_keep_their_recorded_launch_shapes(exe, golden):
    cases = plan_table.tuning_cases()
    assert sorted(golden["tuning"]) == sorted(c["id"] for c in cases)
    got = plans(exe, cases)
    for c in cases:
        assert got[c["id"]]["rc"] == 0 and got[c["id"]]["tune"] == golden["tuning"][c["id"]], (c["id"], got[c["id"]])
    # (the choices stream_default_tuning's comment states)
    shape = {k: (v["ty"], v["zchunk"]) for k, v in golden["tuning"].items()}
    assert (shape["256^3"], shape["512^3"], shape["256^3 cpml 16"]) == ((4, 64), (8, 256), (8, 32))


def test_placement_search_threshold_on_both_sides(exe):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("FWI_")}
    run = subprocess.run([exe, "threshold"], capture_output=True, text=True, timeout=120, env=clean)
    assert run.returncode == 0, run.stderr
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
