"""Walled, slot-started eikonal solves and reflection tomography off a fixed interface on the CPU: the NumPy twin that
defines ``fwi_eikonal_stage``, ``fwi_eikonal_handover`` and ``fwi_eikonal_tangent_stage``
(full_waveform_inversion_amd/eikonal.py), and ``shots.reflection_fg`` / ``shots.ReflectionOperator`` on
``eikonal.TwinEngine``.  DESIGN.md s.4y.

Bounds.

* Bit for bit: ``solve_from`` on the list's ``T_init`` against ``solve``; ``wall=None``; one more sweep.
* Walled block Jacobi against plain Jacobi: 1e-13 of max T, the bound of the unwalled pair in test_eikonal_host.py.
* Flat reflector against the image source, constant medium, source ball of 3 cells at (2.3, 0.3 nx + 0.4), receivers
  on the top row: the committed twin gives 1.37 %, 0.82 % and 0.48 % of the largest exact time on 41 x 61, 81 x 121
  and 161 x 241 with the reflector at 30, 60 and 120 cells.  Held to those plus a quarter, the convention of
  test_eikonal_host.py: 1.71 %, 1.03 %, 0.61 %.
* The wall example ((21, 61), 2000 over 6000 m/s at z = 8): the twin gives 0.28162 s walled against 0.27893 s exact
  (0.97 %; bound: plus a quarter, 1.21 %) and 0.16338 s with the lower layer open, 42 % of the reflection earlier
  (bound: more than 30 %).
* Gradient against central differences, relative step 1e-5 along three random directions: 1e-6, the bound of the
  first arrivals (the twin gives at most 4.8e-9 on these models); without the handover term more than 1e-2 (the twin:
  at least 4.0e-2).  ``<w, J v>`` against ``<J^T w, v>`` and the symmetry of the operator's ``hvp``: 1e-12.
* Five L-BFGS iterations of ``reflection_fg`` from a constant model: J falls by a factor of 87.6 on the test's survey; half
  of that, 43.8, is asserted.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from _eikonal import smooth_model  # noqa: E402
from _eikonal_stage import H, curved_reflector, source, survey  # noqa: E402
from full_waveform_inversion_amd import eikonal as ek, lbfgs as lb, newton as nw, shots as sh  # noqa: E402

SHAPES = [(37, 41), (19, 22, 27)]
_CASE = {}


def case(shape):
    """(c, src, gamma, wall, T1, T2, init) of the test model on `shape`, computed once"""
    if shape not in _CASE:
        c = smooth_model(shape)
        gamma, wall = ek.interface(shape, curved_reflector(shape))
        T1, T2, init = ek.reflection_solve(c, H, source(shape), gamma, wall, radius=2.0)
        for a in (c, gamma, wall, T1, T2):
            a.setflags(write=False)
        _CASE[shape] = (c, source(shape), gamma, wall, T1, T2, init)
    return _CASE[shape]


@pytest.mark.parametrize("shape", SHAPES)
def test_solve_from_is_solve_and_the_wall_holds(shape):
    c, src, gamma, wall, T1, T2, init = case(shape)
    T, n = ek.solve(c, H, init, return_sweeps=True)
    Tf, nf = ek.solve_from(c, H, ek.init_times(c, H, init), return_sweeps=True)
    assert np.array_equal(T, Tf) and n == nf
    assert np.array_equal(ek.solve(c, H, init, wall=None), T)
    assert np.array_equal(ek.solve(c, H, init, wall=np.zeros(shape, bool)), T)
    for dtype in ("float64", "float32"):
        Tw = ek.solve(c, H, init, wall=wall, dtype=dtype)
        assert Tw.dtype == np.dtype(dtype)
        assert np.all(np.isposinf(Tw[wall])) and np.all(np.isfinite(Tw[~wall]))
        s = ek._slowness(c, np.dtype(dtype))
        assert np.array_equal(ek.sweep(Tw, s, H, wall), Tw)           # one more sweep changes no bit
        T2w = ek.solve_from(c, H, np.where(gamma, Tw, np.inf), wall, dtype=dtype)
        assert np.array_equal(ek.sweep(T2w, s, H, wall), T2w) and np.all(np.isposinf(T2w[wall]))
        assert not np.any(np.isnan(Tw)) and not np.any(np.isnan(T2w))
    # the wall only ever delays
    assert np.all(T1[~wall] >= T[~wall])
    # a start the solve refuses
    for bad in (np.full(shape, np.inf), np.where(gamma, -1.0, np.inf), np.where(gamma, np.nan, np.inf)):
        with pytest.raises(ValueError):
            ek.solve_from(c, H, bad, wall)
    ok = np.where(gamma, 0.0, np.inf)
    ok[wall] = np.nan  # whatever T_init says inside the wall
    assert np.all(np.isposinf(ek.solve_from(c, H, ok, wall)[wall]))


@pytest.mark.parametrize("shape", SHAPES)
def test_walled_block_jacobi_matches_plain_jacobi(shape):
    c, src, gamma, wall, T1, T2, init = case(shape)
    tile, inner = (16, 8) if len(shape) == 2 else (8, 4)
    B1, n1 = ek.solve_blocks(c, H, init, tile=tile, inner=inner, wall=wall)
    B2, n2 = ek.solve_blocks(c, H, None, tile=tile, inner=inner, wall=wall, T_init=np.where(gamma, B1, np.inf))
    for B, T in ((B1, T1), (B2, T2)):
        assert np.all(np.isposinf(B[wall]))
        err = float(np.abs(B[~wall] - T[~wall]).max() / T[~wall].max())
        print("walled block Jacobi %s: against plain Jacobi %.1e of max T (bound 1e-13)" % (shape, err))
        assert err <= 1e-13
    assert n1 >= 2 and n2 >= 2


@pytest.mark.parametrize("shape,Z,bound", [((41, 61), 30, 1.71e-2), ((81, 121), 60, 1.03e-2), ((161, 241), 120, 0.61e-2)])
def test_flat_reflector_matches_the_image_source(shape, Z, bound):
    c0 = 2000.0
    src = (2.3, 0.3 * shape[1] + 0.4)
    gamma, wall = ek.interface(shape, float(Z))
    assert gamma[Z].all() and gamma.sum() == shape[1] and wall[Z + 1:].all() and not wall[:Z + 1].any()
    _, T2, _ = ek.reflection_solve(np.full(shape, c0), H, src, gamma, wall, radius=3.0)
    rec = np.array([[0, x] for x in range(0, shape[1], 4)])
    exact = ek.exact_reflection_constant(shape, H, c0, src, rec, Z)
    err = float(np.abs(ek.times_at(T2, rec) - exact).max() / exact.max())
    print("flat reflector %s at %d cells: error %.2f %% of max T (bound %.2f %%)" % (shape, Z, 100 * err, 100 * bound))
    assert err <= bound


def test_the_wall_keeps_the_head_wave_out():
    shape = (21, 61)
    c = np.where(np.arange(shape[0])[:, None] <= 8, 2000.0, 6000.0) * np.ones(shape)
    gamma, wall = ek.interface(shape, 8.0)
    src, rec = (1.0, 3.0), np.array([[1, 57]])
    exact = float(ek.exact_reflection_constant(shape, H, 2000.0, src, rec, 8)[0])
    _, T2, _ = ek.reflection_solve(c, H, src, gamma, wall)
    walled = float(ek.times_at(T2, rec)[0])
    T1o = ek.solve(c, H, src)
    opened = float(ek.times_at(ek.solve_from(c, H, np.where(gamma, T1o, np.inf)), rec)[0])
    print("wall example: walled %.5f s, open %.5f s, exact reflection %.5f s" % (walled, opened, exact))
    assert abs(walled - exact) <= 1.21e-2 * exact
    assert walled - opened > 0.30 * exact  # the open one is the head wave through the fast layer: the wall leaks if not


def test_interface_rounds_to_the_nearest_node_the_lower_on_a_tie():
    gamma, wall = ek.interface((9, 5), np.array([2.0, 2.4, 2.5, 2.6, 8.0]))
    assert np.array_equal(np.argmax(gamma, axis=0), [2, 2, 2, 3, 8]) and np.all(gamma.sum(axis=0) == 1)
    assert np.array_equal(wall.sum(axis=0), [6, 6, 6, 5, 0]) and not (gamma & wall).any()
    assert all(wall[k + 1:, j].all() for j, k in enumerate([2, 2, 2, 3, 8]))
    g3, w3 = ek.interface((9, 4, 5), 3.0)
    assert g3[3].all() and g3.sum() == 20 and w3[4:].all() and not w3[:4].any()
    with pytest.raises(ValueError):
        ek.interface((9, 5), 8.5)


@pytest.mark.parametrize("shape", SHAPES)
def test_handover_selects_the_interface_and_only_source_determined_nodes(shape):
    c, src, gamma, wall, T1, T2, init = case(shape)
    x = np.random.default_rng(3).standard_normal(shape)
    sd = ek.source_determined(T2, c, H)
    assert sd[gamma].all()                       # every interface node is source-determined in stage 2
    assert np.array_equal(T2[gamma], T1[gamma])  # ... and then holds its start
    got = ek.handover(T2, c, H, x)
    assert np.array_equal(got, np.where(sd, x, 0.0)) and np.array_equal(got[gamma], x[gamma])
    assert not sd[wall].any() and not got[wall].any()
    # by hand: of two neighbours in the start, the late one is reached earlier through the early one
    start = np.full(shape, np.inf)
    a = tuple(n // 2 for n in shape)
    b = a[:-1] + (a[-1] + 1,)
    start[a], start[b] = 0.0, 1.0  # one second against a cell's h / c = 5 ms
    T = ek.solve_from(c, H, start)
    assert T[a] == 0.0 and T[b] < 1.0
    sd = ek.source_determined(T, c, H)
    assert sd[a] and not sd[b] and sd.sum() == 1
    assert np.count_nonzero(ek.handover(T, c, H, np.ones(shape))) == 1


def _directional(shape, wrt, with_handover=True):
    """the largest relative error of <g, v> against central differences of J = <b2, T2> over three directions"""
    c, src, gamma, wall, T1, T2, init = case(shape)
    rng = np.random.default_rng(11)
    b2 = np.zeros(shape)
    b2[1] = rng.standard_normal(shape[1:])  # "receivers" on the plane z = 1
    g = ek.reflection_gradient(T1, T2, c, H, init, b2, wrt, with_handover=with_handover)
    m = c if wrt == "velocity" else 1.0 / c ** 2

    def J(mm):
        cc = mm if wrt == "velocity" else 1.0 / np.sqrt(mm)
        return float(np.sum(b2[1] * ek.reflection_solve(cc, H, src, gamma, wall, radius=2.0)[1][1]))

    worst, least = 0.0, np.inf
    for _ in range(3):
        v = rng.standard_normal(shape)
        v /= np.abs(v).max()
        eps = 1e-5 * float(np.abs(m).max())
        fd = (J(m + eps * v) - J(m - eps * v)) / (2.0 * eps)
        err = abs(fd - float(np.sum(g * v))) / abs(fd)
        worst, least = max(worst, err), min(least, err)
    return worst, least


@pytest.mark.parametrize("wrt", ek.WRT)
@pytest.mark.parametrize("shape", SHAPES)
def test_gradient_matches_central_differences_and_needs_the_handover(shape, wrt):
    worst, _ = _directional(shape, wrt)
    _, least = _directional(shape, wrt, with_handover=False)
    print("reflection gradient %s %s: against central differences %.1e (bound 1e-6); without the handover at least "
          "%.1e (must exceed 1e-2)" % (shape, wrt, worst, least))
    assert worst <= 1e-6
    assert least > 1e-2


@pytest.mark.parametrize("wrt", ek.WRT)
@pytest.mark.parametrize("shape", SHAPES)
def test_tangent_and_gradient_are_transposes(shape, wrt):
    c, src, gamma, wall, T1, T2, init = case(shape)
    rng = np.random.default_rng(5)
    v, w = rng.standard_normal(shape), np.where(wall, 0.0, rng.standard_normal(shape))
    x = ek.reflection_tangent(T1, T2, c, H, init, v, wrt)
    g = ek.reflection_gradient(T1, T2, c, H, init, w, wrt)
    a, b = float(np.sum(w * x)), float(np.sum(g * v))
    print("reflection transposition %s %s: %.1e (bound 1e-12)" % (shape, wrt, abs(a - b) / max(abs(a), abs(b))))
    assert abs(a - b) <= 1e-12 * max(abs(a), abs(b))
    # b0 is added where the twin says: with b0 = 0 the stage tangent is the plain one without a source term
    x0 = ek.tangent(T2, c, H, v, None, wrt)
    assert np.array_equal(ek.tangent(T2, c, H, v, None, wrt, b0=np.zeros(shape)), x0)
    assert np.array_equal(ek.tangent(T1, c, H, v, init, wrt, b0=None), ek.tangent(T1, c, H, v, init, wrt))


@pytest.mark.parametrize("shape", [(37, 41), (9, 10, 11)])
def test_operator_is_symmetric_and_matches_reflection_fg(shape):
    c = smooth_model(shape)
    refl = sh.Reflector.at_depth(shape, curved_reflector(shape) if len(shape) == 2 else 6.0)
    shots = survey(shape)
    tw = ek.TwinEngine(shape, H)
    tw.vec_create(sh.ReflectionOperator.WORK_SLOTS + 2 * len(shots))
    picks = sh.reflection_times(tw, 1.03 * c, shots, refl, radius=2.0)
    w = [np.linspace(0.5, 1.5, len(p)) for p in picks]
    picks[0][2] = np.nan
    rng = np.random.default_rng(7)
    u, v = rng.standard_normal(shape), rng.standard_normal(shape)
    for wrt in ek.WRT:
        for keep in (True, False):
            op = sh.ReflectionOperator(tw, c, shots, refl, radius=2.0, wrt=wrt, pick_weights=w, picks=picks,
                                       keep_times=keep)
            assert op.slots_needed(len(shots)) == 11 + (2 * len(shots) if keep else 2)
            a, b = float(np.sum(u * op.hvp(v))), float(np.sum(v * op.hvp(u)))
            assert abs(a - b) <= 1e-12 * max(abs(a), abs(b)), (wrt, keep, a, b)
            assert a != 0.0
        # J^T W (times - picks) is reflection_fg's gradient, and the solves are counted two per shot
        n0 = dict(op.solves)
        r = [np.where(np.isnan(p), 0.0, ww * (t - np.where(np.isnan(p), 0.0, p))) for t, p, ww in zip(op.times(), picks, w)]
        g_op = op.vjp(r)
        J, g = sh.reflection_fg(tw, c, shots, picks, refl, pick_weights=w, radius=2.0, wrt=wrt)
        assert J > 0.0 and np.abs(g_op - g).max() <= 1e-12 * np.abs(g).max()
        assert op.solves["adjoint"] - n0["adjoint"] == 2 * len(shots)
        assert op.solves["eikonal"] - n0["eikonal"] == 2 * 2 * len(shots)  # keep_times=False: times() and vjp() solve
    # a Newton step runs on it and descends
    op = sh.ReflectionOperator(tw, c, shots, refl, radius=2.0, pick_weights=w, picks=picks)
    J, g = sh.reflection_fg(tw, c, shots, picks, refl, pick_weights=w, radius=2.0)
    p, _ = nw.traveltime_newton_step(op, g, damping=1e-3 * float(np.vdot(g, op.hvp(g)) / np.vdot(g, g)), maxiter=4)
    assert float(np.sum(p * g)) < 0.0
    # refusals of the stand-in are ValueErrors
    with pytest.raises(ValueError):
        tw.eikonal_restart(0, 0)
    with pytest.raises(ValueError):
        tw.eikonal_handover(0, 1, 1)
    tw.vec_upload(0, np.full(shape, np.inf))
    with pytest.raises(ValueError):
        tw.eikonal_restart(0, 1)


def test_reflection_tomography_reduces_the_misfit():
    shape = (25, 41)
    z = np.arange(shape[0])[:, None] * np.ones(shape)
    x = np.arange(shape[1])[None, :] * np.ones(shape)
    c_true = 2000.0 + 150.0 * np.exp(-((z - 9.0) ** 2 + (x - 20.0) ** 2) / 40.0)
    refl = sh.Reflector.at_depth(shape, 18.0)
    wav = np.zeros(4)
    rec = np.array([[1, k] for k in range(1, shape[1], 2)])
    shots = [sh.Shot(np.array([[1, s]]), wav, rec) for s in (4, 20, 36)]
    tw = ek.TwinEngine(shape, H)
    tw.vec_create(sh.REFLECTION_SLOTS)
    picks = sh.reflection_times(tw, c_true, shots, refl, radius=2.0)
    c0 = np.full(shape, 2000.0)
    fg = lambda m: sh.reflection_fg(tw, m, shots, picks, refl, radius=2.0)  # noqa: E731
    J0, _ = fg(c0)
    m, J, log = lb.lbfgs(fg, c0, maxiter=5, first_step=50.0, bounds=(1500.0, 3000.0))
    print("reflection tomography: J %.3e -> %.3e after five L-BFGS iterations, a factor of %.1f" % (J0, J, J0 / J))
    assert J0 / J >= 43.8


def test_run_config_knows_the_reflector_flag_and_refuses_bad_combinations():
    """tools/run_config.py --tomography-reflector DEPTH_CELLS: checked before any engine exists"""
    import subprocess
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "run_config.py")
    out = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--tomography-reflector DEPTH_CELLS" in out.stdout
    for bad in (["--tomography-reflector", "20"],                                              # needs --tomography
                ["--tomography", "2", "--tomography-newton", "3", "--tomography-reflector", "20"],  # L-BFGS only
                ["--tomography", "2", "--tomography-reflector", "-1"]):
        out = subprocess.run([sys.executable, tool] + bad, capture_output=True, text=True)
        assert out.returncode == 2 and "--tomography-reflector" in out.stderr, (bad, out.stderr[-400:])
