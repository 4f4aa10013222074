"""A shot's point tables (csrc/fwi_points.cpp), built and checked where there is no GPU.  tests/points_host.cpp is a program
of its own over fwi_plan.cpp and fwi_points.cpp, built with the address and undefined-behaviour sanitizers; it plans a
configuration under the hooks of its environment, builds every table the plan calls for and prints them.  They are compared
EXACTLY with tests/_point_tables.py, a restatement from the definitions (every tile asked, entries sorted on the stated
key), never with anything the C++ produced.  The shapes are the smallest at which each table can go wrong: several tiles on
every axis, tiles cut by the grid's edge, halo = tile edge, the CPML's overlap seam on both axes, a non-zero xbase."""
import itertools
import os
import random
import subprocess
import sys

import pytest

import _plan_cases as pc
import _point_tables as pt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import plan_table  # noqa: E402

PLAN_KEYS = ("kernel", "ty", "zchunk", "tile_x", "fused2d", "fused_ft", "cpml", "pair3d", "pair_zc", "pair_tw", "r", "cx",
             "sy", "sz", "off0")


def cfg(ident, shape, order=8, npml=0, dtype="float32", abc="sponge", kw=None, env=None, path="stream"):
    return dict(id=ident, shape=shape, order=order, npml=npml, dtype=dtype, abc=abc, kw=kw or {}, env=env or {}, path=path)


CONFIGS = (
    # the 3-D stream kernel: rows of 4 and 8, several z chunks; two equal x tiles (nx > 256) with short chunks
    [cfg("stream3d-o%d-ty%s" % (o, ty), (22, 19, 30), order=o, npml=4, env={"FWI_STREAM_TY": ty})
     for o in (2, 8) for ty in ("4", "8")] +
    [cfg("stream3d-two-x-tiles", (9, 9, 300), kw={"zchunk": 2}),
     cfg("stream3d-f64", (22, 19, 30), dtype="float64", npml=4),
     cfg("point2d-f64", (70, 90), dtype="float64", npml=4, path="point"),
     cfg("point3d", (22, 19, 30), npml=4, kw={"kernel": "point"}, path="point"),
     cfg("tile2d", (70, 300), npml=4, env={"FWI_NO_FUSED2D": "1"})] +
    # the fused 2-D kernel: halo 4, 8, 16 against tiles of 64, 32, 16 (halo = tile at 16 / O(8)), plain tiling
    [cfg("fused2d-ft%s-o%d" % (ft, o), (70, 90), order=o, npml=4, env={"FWI_FUSED2D_TILE": ft}, path="fused")
     for ft in ("64", "32", "16") for o in (2, 4, 8)] +
    [cfg("fused2d-130x150", (130, 150), npml=4, env={"FWI_FUSED2D_TILE": "64"}, path="fused"),
     # ... and with the CPML inside the launch (whole 64-cell tiles, one overlap seam per axis; O(8) is what exists)
     cfg("fused2d-cpml-130x150", (130, 150), npml=8, abc="cpml", path="fused-cpml"),
     cfg("fused2d-cpml-200x131", (200, 131), npml=12, abc="cpml", path="fused-cpml")] +
    # the two-step 3-D kernel: one x tile; two x tiles (xbase != 0) and two z chunks
    [cfg("pair3d", (22, 19, 30), env={"FWI_STREAM_PAIR": "1"}, path="pair"),
     cfg("pair3d-o4-zchunk5", (22, 19, 30), order=4, env={"FWI_STREAM_PAIR": "1", "FWI_PAIR_ZCHUNK": "5"}, path="pair"),
     cfg("pair3d-two-x-tiles", (20, 9, 300), env={"FWI_STREAM_PAIR": "1"}, path="pair")])


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return plan_table.build_points_program(str(tmp_path_factory.mktemp("points_host")))


def run(exe, mode, text, env=None):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("FWI_")}
    got = subprocess.run([exe, mode], input=text, capture_output=True, text=True, timeout=120, env=dict(clean, **(env or {})))
    assert got.returncode == 0, (got.returncode, got.stderr)
    assert "Sanitizer" not in got.stderr and "runtime error" not in got.stderr, got.stderr
    return got.stdout


def tables(exe, c, lists):
    """points_host's answer for configuration ``c`` and each point list: one dict of name -> integers per list"""
    head = " ".join(map(str, plan_table.config_ints(c, pc.FIXED)))
    text = "".join("%s\n%d %s\n" % (head, len(p), " ".join(str(v) for q in p for v in q)) for p in lists)
    out = []
    for block in run(exe, "tables", text, c["env"]).split("end\n")[:-1]:
        rows = [ln.split(" ") for ln in block.split("\n")[:-1]]
        d = {r[0]: [int(v) for v in r[1:]] for r in rows}
        assert d.pop("rc") == [0], (c["id"], d)
        d["plan"] = dict(zip(PLAN_KEYS, d["plan"]))
        out.append(d)
    assert len(out) == len(lists)
    return out


def expected(plan, shape, pts):
    outside, pidx, cidx = pt.flatten(plan, shape, pts)
    want = {"plan": plan, "outside": [outside]}
    if outside < 0:
        want.update({"pidx": pidx, "cidx": cidx}, **pt.step_table(plan, shape, pts))
        if plan["fused2d"]:
            want.update(pt.fused2d_tables(plan, shape, pts))
        if plan["pair3d"]:
            want.update(pt.pair3d_table(plan, shape, pts))
    return want


def edges(plan, shape):
    """Per axis the coordinates at which a table can go wrong: the ends of the axis; the first cell of every region a
    workgroup writes, owns or (fused, two-step kernel) reads from, the cell before it, and the cell behind its end."""
    nd = len(shape)
    out = [{0, n - 1} for n in shape]

    def add(axis, lo, hi):
        out[axis] |= {lo - 1, lo, hi - 1, hi}

    for box in pt.step_boxes(plan, shape):
        for axis, (lo, hi) in enumerate(box if nd == 3 else (box[0], box[2])):
            add(axis, lo, hi)
    if plan["fused2d"]:
        hl = pt.fused2d_halo(plan)
        for axis, n in enumerate(shape):
            for (lo, hi), (olo, ohi) in pt.fused2d_axis(n, plan["fused_ft"], plan["cpml"], hl):
                add(axis, lo, hi), add(axis, olo, ohi), add(axis, lo + hl, hi - hl)
                add(axis, lo - hl, hi + hl)     # (the cells a halo's width outside the extended region)
    if plan["pair3d"]:
        for box, _ in pt.pair3d_boxes(plan, shape):
            for axis, (lo, hi) in enumerate(box):
                add(axis, lo, hi), add(axis, lo - plan["r"], hi + plan["r"])
    return [sorted(c for c in s if 0 <= c < n) for s, n in zip(out, shape)]


def point_lists(plan, shape):
    """[(name, points)]: none, one, and the list that holds every edge, a node three times and a random set"""
    rng = random.Random(20261021)
    ax = edges(plan, shape)
    grid = list(itertools.product(*ax))
    if len(grid) > 700:     # (3-D: every edge of every axis still occurs, in ~700 of the combinations)
        keep = set(itertools.product(*[(a[0], a[-1]) for a in ax]))
        keep |= {tuple(a[(i + s) % len(a)] for a, s in zip(ax, shift)) for i in range(max(map(len, ax)))
                 for shift in ((0, 0, 0), (0, 1, 2), (0, 2, 5), (0, 3, 1))}
        grid = sorted(keep | set(rng.sample(grid, 500)))
    corners = list(itertools.product(*[(0, n - 1) for n in shape]))
    assert set(corners) <= set(grid) and all(set(a) == {p[i] for p in grid} for i, a in enumerate(ax))
    rng.shuffle(grid)
    cloud = [tuple(rng.randrange(n) for n in shape) for _ in range(200)]
    node = tuple(n // 2 for n in shape)
    full = [node] + grid[:len(grid) // 2] + [node] + cloud + grid[len(grid) // 2:] + [node]
    return [("none", []), ("one", [node]), ("full", full)]


@pytest.mark.parametrize("c", CONFIGS, ids=[c["id"] for c in CONFIGS])
def test_tables_are_what_the_definitions_say(exe, c):
    shape = tuple(c["shape"])
    plan = tables(exe, c, [[]])[0]["plan"]
    # the configuration takes the path it is meant for
    assert (plan["kernel"], plan["fused2d"], plan["cpml"] and plan["fused2d"], plan["pair3d"]) == {
        "stream": (pt.K_STREAM, 0, 0, 0), "point": (pt.K_POINT, 0, 0, 0), "fused": (pt.K_STREAM, 1, 0, 0),
        "fused-cpml": (pt.K_STREAM, 1, 1, 0), "pair": (pt.K_STREAM, 0, 0, 1)}[c["path"]], plan
    if "FWI_FUSED2D_TILE" in c["env"]:
        assert plan["fused_ft"] == int(c["env"]["FWI_FUSED2D_TILE"])
    if "FWI_STREAM_TY" in c["env"]:
        assert plan["ty"] == int(c["env"]["FWI_STREAM_TY"])
    lists = point_lists(plan, shape)
    for (name, pts), got in zip(lists, tables(exe, c, [p for _, p in lists])):
        want = expected(plan, shape, pts)
        assert sorted(got) == sorted(want), (name, sorted(got), sorted(want))
        for k in want:
            assert got[k] == want[k], "%s, %s points: %s differs" % (c["id"], name, k)
    full = expected(plan, shape, lists[2][1])   # (what the shape is there for: several tiles; a node listed three times)
    assert sum(a != b for a, b in zip(full["step.start"], full["step.start"][1:])) > 1 and max(full["step.run"]) >= 3


@pytest.mark.parametrize("c", [CONFIGS[0], CONFIGS[6], CONFIGS[9], CONFIGS[-1]], ids=lambda c: c["id"])
def test_the_first_point_outside_the_grid_is_named(exe, c):
    shape = tuple(c["shape"])
    rng = random.Random(7)
    ok = [tuple(rng.randrange(n) for n in shape) for _ in range(12)]
    lists = []
    for k, (axis, bad) in enumerate((a, v) for a, n in enumerate(shape) for v in (-1, n)):
        first = tuple(bad if i == axis else 0 for i in range(len(shape)))
        later = tuple(n if i != axis else 0 for i, n in enumerate(shape))     # (outside on the other axes)
        lists.append((k, ok[:k] + [first] + ok[k:] + [later]))
    lists.append((0, [tuple(-1 for _ in shape)]))
    for (k, pts), got in zip(lists, tables(exe, c, [p for _, p in lists])):
        assert got["outside"] == [k] and sorted(got) == ["outside", "plan"], (c["id"], pts[k], got)
        assert pt.flatten(got["plan"], shape, pts)[0] == k


SPREAD = [  # (npts, nnodes, pt_start, have_weight)
    (5, 10, [0, 0, 1, 9, 9, 10], True),           # points of 0, 1 and 8 nodes
    (1, 0, [0, 0], True), (0, 0, None, False), (3, 24, [0, 8, 16, 24], True),
    (-1, 0, [0], True), (2, 2, None, True), (2, 2, [0, 1, 2], False),      # bad set
    (0, 3, None, True),                                                   # nodes without points
    (2, 4, [1, 2, 4], True), (2, 4, [0, 2, 5], True),                      # does not run from 0 to the node count
    (2, 9, [0, 9, 9], True), (3, 3, [0, 5, 1, 3], True), (3, 4, [0, -1, 2, 4], True),   # a count outside 0 .. 8
    # ... found before any owner is written: the counts before it run past the node count
    (4, 3, [0, 8, 16, 2, 3], True),
]


def test_spread_owner_table_and_its_refusals(exe):
    text = "".join("%d %d %d %d %d %s\n" % (npts, nnodes, start is not None, w, len(start or []), " ".join(map(str, start or [])))
                   for npts, nnodes, start, w in SPREAD)
    rows = [[int(v) for v in ln.split(" ")[1:]] for ln in run(exe, "spread", text).split("\n")[:-1]]
    assert len(rows) == len(SPREAD)
    seen = set()
    for (npts, nnodes, start, w), got in zip(SPREAD, rows):
        check, point, count, owner = pt.spread_owners(npts, nnodes, start, w)
        assert got == [check, point, count] + owner, ((npts, nnodes, start, w), got)
        seen.add(check)
    assert seen == set(range(5))
    assert rows[0][3:] == [1, 2, 2, 2, 2, 2, 2, 2, 2, 4]      # (written out once, by hand)


def test_no_cpml_width_puts_the_small_grid_into_the_fused_launch(exe):
    """(70, 90) is the fused kernel's small shape, but one 64-cell tile of a 70-cell axis sees both borders: whatever the
    width, its CPML runs as slab launches around the tile kernel, and the seam tiling is tested on the larger shapes."""
    for npml in (1, 4, 10, 24, 48):
        plan = tables(exe, cfg("", (70, 90), npml=npml, abc="cpml"), [[]])[0]["plan"]
        assert (plan["cpml"], plan["fused2d"]) == (1, 0), (npml, plan)
