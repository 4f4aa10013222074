"""Placed 3-D contexts at KNOWN offsets.  A 3-D fp32 stream context with the convolutional PML, or in increment form,
keeps some of its arrays inside padded allocations at the offset a search timed as fastest (fwi_api.hip tune_placement):
which layout a run meets is decided by a stopwatch.  FWI_PLACEMENT_TUNE=fixed:<k0>,<k1>,... asks for a layout instead, and
this file holds "the arithmetic never sees an address" to account with it: the hook itself, every sweep bit for bit
against the unplaced context, a moved layout against the C oracle, the size where the search is on by its own threshold,
and what fwi_destroy gives back."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

from full_waveform_inversion_amd import Engine, FwiError, _lib, workloads
from oracle import fwi_oracle as fo
from oracle.c_oracle import CPropagator

pytestmark = pytest.mark.gpu
TOL32 = 1e-5
MIB = 1 << 20
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_gpu_parity import _band_limited_residual  # noqa: E402  (the residual every full-size comparison shares)

# the three placed kinds: engine options, movable arrays (search order: include/fwi.h fwi_placement_info)
KINDS = {
    "cpml_standard": ({"abc": "cpml", "pml_alpha_max": 20.0}, 4),                               # ty, zeta_x, tz, psi_x
    "cpml_increment": ({"abc": "cpml", "pml_alpha_max": 20.0, "update_form": "increment"}, 5),  # ... and v
    "sponge_increment": ({"update_form": "increment"}, 2),                                      # v, C
}
DISTINCT, FAR_END = "fixed:1,3,5,7,2", "fixed:7"  # all shifts distinct and non-zero; every array's end on its allocation's
LAYOUTS = [DISTINCT, FAR_END]


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / np.linalg.norm(b))


def _expected_shifts(layout, nmov):
    k = [int(v) for v in layout.split(":")[1].split(",")]
    k += [k[-1]] * (8 - len(k))
    return tuple(2 * MIB * v for v in k[:nmov]) + (0,) * (8 - nmov)


def _shot(shape, nt, seed):
    rng = np.random.default_rng(seed)
    c = (1800.0 + 900.0 * rng.random(shape)).astype(np.float32)
    c2 = (2000.0 + 600.0 * rng.random(shape)).astype(np.float32)
    h, order = 10.0, 8
    dt = 0.7 * fo.cfl_dt(2700.0, h, 3, order)
    src = np.array([[s // 2 for s in shape], [1] + [s - 2 for s in shape[1:]]])  # the second one inside the border
    rec = np.stack([rng.integers(0, s, 7) for s in shape], 1)
    wav = np.stack([fo.ricker(nt, dt, 0.12 / dt / 8), 0.5 * fo.ricker(nt, dt, 0.12 / dt / 6)], 1).astype(np.float32)
    r = (rng.standard_normal((nt, len(rec))) * 1e-3).astype(np.float32)  # (a residual no layout can have a hand in)
    return c, c2, h, dt, order, src, rec, wav, r


# ---------------------------------------------------------------------------------------------------------------------
# a. the hook does what it says
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS + ["fixed:0,4", "fixed:2,0,6,1,3,5,7,4"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_fixed_layout_is_reported_exactly_and_no_search_runs(gpu, monkeypatch, kind, layout):
    kw, nmov = KINDS[kind]
    monkeypatch.setenv("FWI_PLACEMENT_TUNE", layout)
    with Engine((40, 36, 64), 10.0, 1e-3, 8, npml=8, sigma_max=900.0, **kw) as e:
        assert e.kernel_name == "step3d_stream"
        before, after, shifts = e.placement_info()
        assert (before, after) == (0.0, 0.0)
        assert shifts == _expected_shifts(layout, nmov)
        assert e.dirty_padding() == 0


@pytest.mark.parametrize("value", ["fixed:8", "fixed:1,3,9", "fixed:-1", "fixed:", "fixed:1,,2", "fixed:1,2,", "fixed:x",
                                   "fixed:1 ,2", "fixed:0,1,2,3,4,5,6,7,0", "fixed:2.5", "fixed:100000000000000000000"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_fixed_layout_out_of_range_or_malformed_is_einval(gpu, monkeypatch, kind, value):
    monkeypatch.setenv("FWI_PLACEMENT_TUNE", value)
    with pytest.raises(FwiError) as ei:
        Engine((40, 36, 64), 10.0, 1e-3, 8, npml=8, sigma_max=900.0, **KINDS[kind][0])
    assert ei.value.code == 1 and "FWI_PLACEMENT_TUNE" in str(ei.value)
    monkeypatch.setenv("FWI_PLACEMENT_TUNE", "fixed:7")  # ... and the next creation on the thread is none the worse
    with Engine((40, 36, 64), 10.0, 1e-3, 8, npml=8, sigma_max=900.0, **KINDS[kind][0]) as e:
        assert e.placement_info()[2][0] == 14 * MIB
    assert _lib.load().fwi_last_error(None) == b""  # (a successful fwi_create clears the creation error)


@pytest.mark.parametrize("shape,kw", [((40, 36, 64), {}),                                          # plain sponge, standard form
                                      ((72, 96), {}), ((72, 96), {"abc": "cpml", "update_form": "increment"}),  # 2-D
                                      ((40, 36, 64), {"dtype": "float64", "abc": "cpml"}),
                                      ((40, 36, 64), {"kernel": "point", "update_form": "increment"}),
                                      ((30, 26, 45), {"abc": "cpml"})])                           # x border in slabs: not placed
def test_contexts_that_place_nothing_ignore_fixed(gpu, monkeypatch, shape, kw):
    for value in ("fixed:3", "fixed:9"):  # (ignored means ignored: not even read)
        monkeypatch.setenv("FWI_PLACEMENT_TUNE", value)
        with Engine(shape, 10.0, 1e-3, 8, npml=8, sigma_max=900.0, **kw) as e:
            assert e.placement_info() == (0.0, 0.0, (0,) * 8)


# ---------------------------------------------------------------------------------------------------------------------
# b. bits do not depend on the layout
# ---------------------------------------------------------------------------------------------------------------------
def _sweeps(shape, nt, kw, env, second_model):
    """Every sweep a context runs, on one context, as a list of (name, array): store-free and storing forward, F^T r,
    gradient and illumination; optionally the same under a second model; then reset_gradient() and the first shot again."""
    c, c2, h, dt, order, src, rec, wav, r = _shot(shape, nt, seed=5)
    out = []
    with Engine(shape, h, dt, nt, order=order, npml=8, sigma_max=900.0, illumination=True, **kw) as e:
        e.set_model(c)
        assert e.kernel_name == "step3d_stream"
        assert e.dirty_padding() == 0
        info = e.placement_info()

        def shot(tag):
            out.append((tag + "/forward", e.forward(None, (src, wav), rec, save=False).copy()))
            out.append((tag + "/forward(save)", e.forward(None, (src, wav), rec, save=True).copy()))
            out.append((tag + "/adjoint", e.adjoint(r).copy()))
            out.append((tag + "/gradient", e.gradient().copy()))
            out.append((tag + "/illumination", e.illumination().copy()))
            assert e.dirty_padding() == 0, (tag, env)

        shot("first")
        if second_model:  # (C is a moved array in the (sponge, increment) kind: the new model must land where the kernels read)
            e.set_model(c2)
            shot("second model")
            e.set_model(c)
        e.reset_gradient()
        shot("repeat")
    first = {k.split("/")[1]: v for k, v in out if k.startswith("first/")}
    for k, v in out:  # the repeated shot on the same context returns the bits of its first run
        if k.startswith("repeat/"):
            assert np.array_equal(v, first[k.split("/")[1]]), (k, env)
    assert all(np.isfinite(v).all() for _, v in out)
    assert np.abs(first["gradient"]).max() > 0 and np.abs(first["illumination"]).max() > 0 and np.abs(first["adjoint"]).max() > 0
    return info, out


# one list, not a full product: every variation at least once per kind (image_stride and ckpt_interval exclude each other)
VARIATIONS = [
    ("stream", {"launch_mode": "stream"}, None, True),
    ("graph", {"launch_mode": "graph"}, None, True),          # the graph captures pointers
    ("ckpt", {"ckpt_interval": 16}, None, False),             # the recomputation pair fwv / pml_*_fw beside moved arrays
    ("stride3", {"image_stride": 3}, None, False),
    ("ty8", {}, "8", False),                                  # FWI_STREAM_TY=8: the 8-row tiles of the HBM-regime grids
    ("graph+ckpt+ty8", {"launch_mode": "graph", "ckpt_interval": 7}, "8", True),
]
LANES, NOT_LANES = (72, 64, 96), (40, 36, 45)  # nx % 4 == 0: the x border runs in the lanes; nx % 4 != 0
BIT_CASES = [(kind, LANES, v) for kind in KINDS for v in VARIATIONS]
BIT_CASES += [("sponge_increment", NOT_LANES, v) for v in VARIATIONS[:3] + VARIATIONS[4:5]]


@pytest.mark.parametrize("kind,shape,variation", BIT_CASES,
                         ids=["%s-%s-%s" % (k, "x".join(map(str, s)), v[0]) for k, s, v in BIT_CASES])
def test_bits_do_not_depend_on_the_layout(gpu, monkeypatch, kind, shape, variation):
    """The statement the placement rests on, at known non-zero offsets: seismograms (store-free and storing forward),
    F^T r, gradient and illumination of the same sequence are bit-identical with every movable array at the start of an
    unpadded allocation (FWI_PLACEMENT_TUNE=0), with all of them at distinct offsets, and with all of them at the far
    end of their allocations."""
    _, opts, stream_ty, second_model = variation
    kw = dict(KINDS[kind][0], **opts)
    nt = 50
    if stream_ty:
        monkeypatch.setenv("FWI_STREAM_TY", stream_ty)
    monkeypatch.setenv("FWI_PLACEMENT_TUNE", "0")
    info, ref = _sweeps(shape, nt, kw, "0", second_model)
    assert info == (0.0, 0.0, (0,) * 8)
    for layout in LAYOUTS:
        monkeypatch.setenv("FWI_PLACEMENT_TUNE", layout)
        info, got = _sweeps(shape, nt, kw, layout, second_model)
        assert info == (0.0, 0.0, _expected_shifts(layout, KINDS[kind][1]))  # (the layout under test is the one asked for)
        assert [k for k, _ in got] == [k for k, _ in ref]
        for (k, a), (_, b) in zip(got, ref):
            assert np.array_equal(a, b), (layout, k, rel(a, b))


# ---------------------------------------------------------------------------------------------------------------------
# c. a moved layout against the C oracle ((cpml, *): the "fixed" rows of
#    tests/test_gpu_cpml.py::test_cpml_3d_lines_and_lanes_at_size_vs_c_oracle)
# ---------------------------------------------------------------------------------------------------------------------
def _sponge_vs_c_oracle(w, nt, kern, **kw):
    wav = w.wavelet(np.float64)[:nt]
    p = CPropagator(w.c, w.h, w.dt, w.order, w.npml)
    d = p.forward(w.src_idx, wav, w.rec_idx, save=True)
    r = 0.7 * d + 0.2 * np.roll(d, 3, axis=0)
    a = p.adjoint(r)
    g = p.gradient("velocity")
    p.q_store = None
    with Engine(w.shape, w.h, w.dt, nt, order=w.order, npml=w.npml, sigma_max=p.sigma_max, **kw) as e:
        dg = e.forward(w.c, (w.src_idx, wav), w.rec_idx, save=True)
        assert e.kernel_name == kern
        shifts = e.placement_info()[2]
        ag = e.adjoint(r)
        gg = e.gradient("velocity")
    print("sponge vs C oracle %s: seis %.3e adjoint %.3e gradient %.3e" % (kw, rel(dg, d), rel(ag, a), rel(gg, g)))
    assert rel(dg, d) < TOL32, rel(dg, d)
    assert rel(ag, a) < TOL32, rel(ag, a)
    assert rel(gg, g) < TOL32, rel(gg, g)
    return shifts


def test_sponge_increment_form_at_fixed_offsets_vs_c_oracle(gpu, monkeypatch):
    """3-D 160^3 heterogeneous model, sponge of 16 cells, 400 steps, increment form with v and C moved 2 and 6 MiB into
    their allocations: seismograms, F^T r and gradient against the C oracle."""
    monkeypatch.setenv("FWI_PLACEMENT_TUNE", "fixed:1,3")
    w = workloads.cfg5(0.625, nshots=1)
    w.npml = 16
    shifts = _sponge_vs_c_oracle(w, 400, "step3d_stream", update_form="increment")
    assert shifts == _expected_shifts("fixed:1,3", 2)


# ---------------------------------------------------------------------------------------------------------------------
# d. the size where the search is on by itself
# ---------------------------------------------------------------------------------------------------------------------
def _record_parity(row, entry):
    """Prints what a 256^3 row measured; profiles/r05_parity_placed.json keeps one such run.  A test run leaves the tree
    alone: the rows are written only on request, into the JSON file FWI_RECORD_PARITY names."""
    print("r05_parity_placed %s: %s" % (row, json.dumps(entry)))
    path = os.environ.get("FWI_RECORD_PARITY")
    if not path:
        return
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc.setdefault("rows", {})[row] = entry
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


@pytest.mark.parametrize("row,abc,kw", [("sponge_increment", "sponge", {"update_form": "increment"}),
                                        ("cpml_standard", "cpml", {})])
def test_full_size_heterogeneous_3d_with_the_search_on_vs_c_oracle(gpu, monkeypatch, row, abc, kw):
    """configs[4]'s heterogeneous model at its own size (256^3, O(8), npml 16), 400 of its 1000 steps, FWI_PLACEMENT_TUNE
    unset: the placement search runs by its own threshold.  (sponge, increment form) is the default engine of a 3-D
    inversion; (cpml, standard) is the other placed border.  Seismograms, F^T r and the gradient of a shared residual
    against the C oracle at the flat 1e-5 of every fp32 comparison here; the shifts the search chose are printed."""
    monkeypatch.delenv("FWI_PLACEMENT_TUNE", raising=False)
    w = workloads.cfg5(1.0, nshots=1)
    nt = 400
    wav = w.wavelet(np.float64)[:nt]
    okw = {"abc": "cpml", "pml_alpha_max": 3.14159 * 10.0} if abc == "cpml" else {}
    p = CPropagator(w.c, w.h, w.dt, w.order, w.npml, **okw)
    d = p.forward(w.src_idx, wav, w.rec_idx, save=True)
    assert np.abs(d).max() > 0
    r = _band_limited_residual(d, 1)
    a = p.adjoint(r)
    g = p.gradient("velocity")
    p.q_store = None
    assert np.abs(g).max() > 0 and np.abs(a).max() > 0
    with Engine(w.shape, w.h, w.dt, nt, order=w.order, npml=w.npml, sigma_max=p.sigma_max, **dict(okw, **kw)) as e:
        dg = e.forward(w.c, (w.src_idx, wav), w.rec_idx, save=True)
        assert e.kernel_name == "step3d_stream"
        before, after, shifts = e.placement_info()
        ag = e.adjoint(r)
        gg = e.gradient("velocity")
        assert e.dirty_padding() == 0
    entry = {"shape": list(w.shape), "nt": nt, "npml": w.npml, "us_per_step_before": before, "us_per_step_after": after,
             "shift_MiB": [s // MIB for s in shifts], "seis": rel(dg, d), "adjoint": rel(ag, a), "gradient": rel(gg, g)}
    _record_parity(row, entry)
    assert before > 0, "the placement search did not run at 256^3"
    assert rel(dg, d) < TOL32, rel(dg, d)
    assert rel(ag, a) < TOL32, rel(ag, a)
    assert rel(gg, g) < TOL32, rel(gg, g)


# ---------------------------------------------------------------------------------------------------------------------
# e. life cycle at placed sizes
# ---------------------------------------------------------------------------------------------------------------------
def _free_bytes():
    hip = C.CDLL("libamdhip64.so")
    fr, tot = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(fr), C.byref(tot)) == 0
    return fr.value


def _cycles(n, shape, kw, shot):
    c, _, h, dt, order, src, rec, wav, r = shot
    lib = _lib.load()
    for i in range(n):
        with Engine(shape, h, dt, wav.shape[0], order=order, npml=8, sigma_max=900.0, **kw) as e:
            e.forward(c, (src, wav), rec, save=True)
            e.adjoint(r)
            e.gradient()
            shifts = e.placement_info()[2]
        msg = lib.fwi_last_error(None) or b""
        assert not msg.startswith(b"fwi_destroy:"), (i, msg.decode())
    return shifts


@pytest.mark.parametrize("kind", list(KINDS))
def test_destroy_gives_back_every_placed_array(gpu, monkeypatch, kind):
    """Six create -> forward(save) -> adjoint -> gradient -> destroy cycles of a 96 x 96 x 128 context with every movable
    array at a different non-zero offset: fwi_destroy reports no refused free, and free device memory ends within 14 MiB
    of where it was after a warm-up cycle.  14 MiB is the pad alone: an array freed through a moved pointer and refused
    leaks its own bytes plus the pad, so ONE such array in six cycles is already over the bound.  The same six cycles
    with FWI_PLACEMENT_TUNE=0 run first as the control: if that moves by more, somebody else on the device did it."""
    kw, nmov = KINDS[kind]
    shape, bound = (96, 96, 128), 14 * MIB
    shot = _shot(shape, 12, seed=3)
    drift = {}
    for env in ("0", DISTINCT):
        monkeypatch.setenv("FWI_PLACEMENT_TUNE", env)
        _cycles(1, shape, kw, shot)  # warm-up: the runtime's own first-use allocations are not leaks
        start = _free_bytes()
        shifts = _cycles(6, shape, kw, shot)
        drift[env] = start - _free_bytes()
        print("life cycle %s %s: free memory fell by %.1f MiB over 6 cycles" % (kind, env, drift[env] / MIB))
        if env == "0":
            assert not any(shifts)
            assert abs(drift[env]) <= bound, (
                "CONTROL: free device memory moved by %.1f MiB over six cycles of an UNPLACED context -- the device's "
                "free memory moves without us (another tenant?); this says nothing about placed contexts"
                % (drift[env] / MIB))
        else:
            assert shifts == _expected_shifts(env, nmov)
            assert abs(drift[env]) <= bound, (
                "six cycles of a PLACED context lost %.1f MiB of device memory (the unplaced control: %.1f MiB): "
                "fwi_destroy does not give back what fwi_create allocated" % (drift[env] / MIB, drift["0"] / MIB))
