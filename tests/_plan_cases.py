"""Configurations x creation-time hooks whose path through fwi_create is on record (tests only; no test in this file).

``CASES`` is plain data: ``{"id", "shape", "order", "npml", "dtype", "abc", "kw", "env"}`` with ``kw`` the Engine options
that reach fwi_config (kernel, zchunk, ckpt_interval, image_stride, update_form, store_dtype) and ``env`` the hooks.
tools/plan_table.py creates each of them once on the GPU and writes what the context says of itself into
tests/golden/plan_paths.json; tests/test_plan_host.py holds csrc/fwi_plan.cpp to that record on the CPU,
tests/test_gpu_plan.py a live context of the small ones.  Nothing here says what a case is expected to do: the record does.

h, dt, nt_max, sigma_max and pml_alpha_max are the same for every case (``FIXED``): no decision depends on them, and an
explicit sigma_max lets creation happen without a model.

The cases of the pointwise tables keep their own grids (up to 300 columns in 3-D, 260 in 2-D); every other 3-D grid is at
most 48 cells per axis, save the ones whose point is an x extent above 256, and every other 2-D grid at most 160.
"""
import _pointwise as pw
import _pointwise_born as pwb

FIXED = dict(h=10.0, dt=1e-3, nt_max=8, sigma_max=900.0, pml_alpha_max=0.0)
PLAN_KW = ("kernel", "zchunk", "ckpt_interval", "image_stride", "update_form", "store_dtype")
# the layout under which the placed arrays of every case are recorded (tests/test_gpu_placement.py DISTINCT)
DISTINCT = "fixed:1,3,5,7,2"


def _mk(ident, shape, order=8, npml=4, dtype="float32", abc="sponge", kw=None, env=None):
    kw = dict(kw or {})
    assert set(kw) <= set(PLAN_KW), kw
    return dict(id=ident, shape=list(shape), order=order, npml=npml, dtype=dtype, abc=abc, kw=kw, env=dict(env or {}))


def from_table(prefix, c):
    """The plan case of a _pointwise.Case: its shape, order, npml, dtype, abc, kw and env."""
    inc = c.kw.get("update_form") == "increment" and "increment" not in c.path   # (as _pointwise_born.born_case_id)
    return _mk(prefix + pw.case_id(c) + ("-increment" if inc else ""), c.shape, c.order, c.npml, c.dtype, c.abc,
               {k: v for k, v in c.kw.items() if k in PLAN_KW}, c.env)


def _suffix(kw, env):
    return "".join("-%s=%s" % (k.replace("FWI_", "").lower(), v) for k, v in sorted(list(kw.items()) + list(env.items())))


def _cases():
    out = []
    for c in pw.CASES:
        out.append(from_table("pointwise:", c))
    for prefix, table in (("born:", [b.case for b in pwb.BORN_CASES]), ("bf16:", [b.case for b in pwb.BF16_CASES]),
                          ("illum:", pwb.ILLUM_CASES)):
        for c in table:
            out.append(from_table(prefix, c))

    def add(group, shape, order=8, npml=4, dtype="float32", abc="sponge", kw=None, env=None):
        kw, env = dict(kw or {}), dict(env or {})
        out.append(_mk("%s:%s-O%d-npml%d-%s-%s%s" % (group, "x".join(map(str, shape)), order, npml, dtype[-2:], abc,
                                                      _suffix(kw, env)), shape, order, npml, dtype, abc, kw, env))

    # tests/test_gpu_placement.py: the three placed kinds and the contexts that place nothing, under the hook values there
    kinds = [{"abc": "cpml"}, {"abc": "cpml", "kw": {"update_form": "increment"}}, {"kw": {"update_form": "increment"}}]
    values = ("fixed:1,3,5,7,2", "fixed:7", "fixed:0,4", "fixed:2,0,6,1,3,5,7,4", "0", "fixed:8", "fixed:1,3,9",
                              "fixed:-1", "fixed:", "fixed:1,,2", "fixed:1,2,", "fixed:x", "fixed:1 ,2",
                              "fixed:0,1,2,3,4,5,6,7,0", "fixed:2.5", "fixed:100000000000000000000")
    for k in kinds:
        for v in values:
            add("placement-suite", (40, 36, 64), npml=8, env={"FWI_PLACEMENT_TUNE": v}, **k)
    for shape, k in [((40, 36, 64), {}), ((72, 96), {}), ((72, 96), {"abc": "cpml", "kw": {"update_form": "increment"}}),
                     ((40, 36, 64), {"dtype": "float64", "abc": "cpml"}),
                     ((40, 36, 64), {"kw": {"kernel": "point", "update_form": "increment"}}), ((30, 26, 45), {"abc": "cpml"})]:
        for v in ("fixed:3", "fixed:9"):
            add("placement-suite", shape, npml=8, env={"FWI_PLACEMENT_TUNE": v}, **k)
    for shape in ((72, 64, 96), (40, 36, 45), (96, 96, 128)):
        for k in kinds:
            for env in ({}, {"FWI_STREAM_TY": "8"}):
                add("placement-suite", shape, npml=8, env=env, **k)

    # x border in the kernel: 3-D fp32 O(8) CPML, npml 4, 24^3, and one step off it in every direction
    X = (24, 24, 24)
    add("xpml", X, abc="cpml")
    add("xpml", X, npml=5, abc="cpml")
    add("xpml", (24, 24, 26), abc="cpml")
    add("xpml", X, order=4, abc="cpml")
    add("xpml", X, dtype="float64", abc="cpml")
    add("xpml", X, abc="cpml", env={"FWI_NO_STREAM_XPML": "1"})
    add("xpml", X, abc="cpml", env={"FWI_NO_PML_LINES": "1"})
    add("xpml", (24, 24, 2 * (4 + 4) - 4), abc="cpml")   # nx = 2 (npml + 4) - 4: the two borders' reaches meet
    add("xpml", (24, 24, 2 * (4 + 4)), abc="cpml")
    for nx in (260, 264, 516):                          # two and three equal x tiles
        add("xpml", (8, 8, nx), abc="cpml")
    for npml in (124, 126):   # nx 260 = tiles of 132 and 128 columns: the last one holds npml + 4 cells, or is narrower
        add("xpml", (8, 8, 260), npml=npml, abc="cpml")

    # fused 2-D
    add("fused2d", (96, 96), npml=6)
    add("fused2d", (96, 96), npml=6, dtype="float64")
    add("fused2d", (96, 96), npml=6, kw={"kernel": "point"})
    add("fused2d", (96, 96), npml=6, kw={"kernel": "stream"})
    add("fused2d", (96, 96), npml=6, env={"FWI_NO_FUSED2D": "1"})
    for n in (65, 64):
        add("fused2d", (n, n), npml=6, abc="cpml")
    for npml in (48, 49):
        add("fused2d", (160, 160), npml=npml, abc="cpml")
    add("fused2d", (150, 152), npml=6, abc="cpml")
    add("fused2d", (150, 152), npml=6, abc="cpml", env={"FWI_NO_FUSED2D_CPML": "1"})
    add("fused2d", (150, 152), npml=6, abc="cpml", env={"FWI_NO_FUSED2D": "1"})
    add("fused2d", (150, 152), order=4, npml=6, abc="cpml")
    add("fused2d", (96, 96), npml=6, kw={"update_form": "increment"})                        # fused; names the point kernel
    add("fused2d", (96, 96), npml=6, kw={"update_form": "increment", "kernel": "stream"})    # refused
    add("fused2d", (96, 96), npml=6, kw={"update_form": "increment", "kernel": "point"})
    add("fused2d", (150, 152), npml=6, abc="cpml", kw={"update_form": "increment"})
    for v in ("16", "32", "64", "48"):
        add("fused2d", (96, 96), npml=6, env={"FWI_FUSED2D_TILE": v})
        add("fused2d", (150, 152), npml=6, abc="cpml", env={"FWI_FUSED2D_TILE": v})        # (the CPML's tiles are 64)
    for v in ("0", "1"):
        add("fused2d", (96, 96), npml=6, env={"FWI_FUSED2D_SKIPD": v})

    # kernel choice
    add("kernel", (40, 44), dtype="float64")
    add("kernel", (40, 44), dtype="float64", kw={"kernel": "stream"})          # refused
    add("kernel", X, dtype="float64", kw={"update_form": "increment"})
    add("kernel", X, dtype="float64", kw={"update_form": "increment", "kernel": "stream"})   # refused
    add("kernel", X, kw={"update_form": "increment", "kernel": "stream"})
    add("kernel", X, kw={"kernel": "point"})
    add("kernel", X, npml=0, kw={"store_dtype": "bf16"})
    for order in (2, 4):
        add("kernel", X, order=order)
        add("kernel", (40, 44), order=order)

    # two steps per pass
    P = {"FWI_STREAM_PAIR": "1"}
    add("pair3d", X, npml=0, env=P)
    add("pair3d", X, npml=4, env=P)
    add("pair3d", X, npml=0, kw={"update_form": "increment"}, env=P)
    add("pair3d", X, npml=4, abc="cpml", env=P)
    add("pair3d", X, npml=0, abc="cpml", env=P)                # (a CPML of no cells is no CPML)
    add("pair3d", X, npml=0, dtype="float64", env=P)
    add("pair3d", (40, 44), npml=0, env=P)
    add("pair3d", X, npml=0, kw={"kernel": "point"}, env=P)
    add("pair3d", X, npml=0, env={"FWI_STREAM_PAIR": "0"})
    add("pair3d", X, npml=0)
    for zc in ("8", "0", "-3"):
        add("pair3d", X, npml=0, env=dict(P, FWI_PAIR_ZCHUNK=zc))
    add("pair3d", (48, 8, 300), npml=0, env=P)                 # x tiles of the two-step kernel

    # launch shape
    add("shape", X, kw={"zchunk": 7})
    add("shape", X, abc="cpml", kw={"zchunk": 7})
    add("shape", (40, 44), kw={"zchunk": 7})
    for v in ("4", "8", "16", "5"):
        add("shape", X, env={"FWI_STREAM_TY": v})
        add("shape", X, abc="cpml", env={"FWI_STREAM_TY": v})
        add("shape", (40, 44), env={"FWI_STREAM_TY": v, "FWI_NO_FUSED2D": "1"})
    for v in ("0", "2", "4"):
        add("shape", X, env={"FWI_STREAM_PF": v})
    for shape in ((48, 48, 48), (17, 9, 31), (48, 3, 5)):
        add("shape", shape)
        add("shape", shape, dtype="float64")

    # placement: every kind of hook value on every kind of context
    for v in ("0", "pad", "force", "fixed:1,3", "fixed:8", "fixed:1,,2"):
        env = {"FWI_PLACEMENT_TUNE": v}
        add("placement", X, abc="cpml", env=env)                                          # x border in the kernel
        add("placement", X, kw={"update_form": "increment"}, env=env)
        add("placement", X, abc="cpml", kw={"update_form": "increment"}, env=env)
        add("placement", X, env=env)                                                      # places nothing
        add("placement", X, dtype="float64", abc="cpml", env=env)
    ids = [c["id"] for c in out]
    assert len(ids) == len(set(ids)), sorted(i for i in ids if ids.count(i) > 1)
    return out


CASES = _cases()


def searches(case):
    """The hook value under which a placed context TIMES its layout: creation launches kernels, the offsets are measured."""
    return case["env"].get("FWI_PLACEMENT_TUNE") == "force"


def small(case):
    """The cases tests/test_gpu_plan.py creates: the edges (not the tables' cases, which the pointwise suites create
    anyway) on 3-D grids of at most 24 cells per axis and 2-D grids of at most 96, where no layout is timed."""
    return (case["id"].split(":")[0] in ("xpml", "fused2d", "kernel", "pair3d", "shape", "placement") and not searches(case)
            and max(case["shape"]) <= (24 if len(case["shape"]) == 3 else 96))
