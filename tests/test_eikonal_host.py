"""First-arrival traveltimes without a GPU: the NumPy twin that defines them (full_waveform_inversion_amd/eikonal.py),
``shots.traveltime_fg`` on the twin-backed stand-in ``eikonal.TwinEngine``, and the two pick helpers of datafit.

Bounds that are not set by the scheme's own definition, and where they come from:

* Closed forms.  The first-order error measured by the prototype of the scheme against ``s r`` with the source at the
  top centre is 1.2 % of max T on 101^2 and 0.69 % on 201^2 at radius 0, 0.45 % on 201^2 at radius 8, and 0.9 % on
  201^2 in ``c = c0 + g z`` with g = 1 / s.  The tests hold the twin to 1.5 %, 0.85 %, 0.6 % and 1.2 %: those numbers plus
  a quarter, which leaves room for a different but equivalent rounding and none for a wrong stencil (a missing case of
  the local solver costs several per cent).  The ratio 101^2 : 201^2 must be at least 1.5 (prototype: 1.70; first order
  would be 2 without the logarithmic term of the point source).  3-D has no prototype figure, so no absolute error
  is asserted there: the solution is held between the straight ray and the path along the axes (G <= a + f), must be
  exact on the axes through the source and equal to the 2-D solution on the coordinate planes through it (the third
  axis is inactive there), and its error must fall by the same 1.5 from 21^3 to 41^3 (seen: 8.4 % -> 5.2 %, 1.62).
* Finite differences: relative step 1e-5 along a random direction, central, asserted at 1e-6 (the project's
  convention: the truncation term is ~1e-10 and the roundoff of J, ~1e-16 J / 1e-5, stays below 1e-9).
* Block Jacobi against plain Jacobi: 1e-13 of max T.  Dense solve against the Jacobi adjoint: 1e-12 of max |lambda|
  (a 990 x 990 triangular system in fp64).

Largest figures seen: gradient against central differences 5.7e-8 (bound 1e-6); dense adjoint 2.5e-16 (1e-12); block
against plain Jacobi 0 (1e-13); five L-BFGS iterations reduce J by 4.4 (asserted: 2)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from _eikonal import layered_model, smooth_model  # noqa: E402
from full_waveform_inversion_amd import datafit as df, eikonal as ek, shots as sh  # noqa: E402
from full_waveform_inversion_amd.engine import ricker  # noqa: E402
from full_waveform_inversion_amd.lbfgs import lbfgs  # noqa: E402

H = 10.0


# ---- closed forms ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def constant_errors():
    """relative errors against s r, source at the top centre: {(n, radius): error / max T}"""
    out = {}
    for n, radius in ((101, 0.0), (201, 0.0), (201, 8.0)):
        src = (0.0, (n - 1) / 2.0)
        T = ek.solve(np.full((n, n), 2000.0), H, src, radius=radius)
        ex = ek.exact_constant((n, n), H, 2000.0, src)
        out[n, radius] = float(np.abs(T - ex).max() / ex.max())
    print("eikonal: error / max T against s r:", out)
    return out


def test_constant_velocity_2d_is_first_order(constant_errors):
    e = constant_errors
    assert e[101, 0.0] < 0.015 and e[201, 0.0] < 0.0085 and e[201, 8.0] < 0.006, e
    assert e[101, 0.0] / e[201, 0.0] >= 1.5, e
    assert e[201, 8.0] < e[201, 0.0], e


def test_error_shrinks_with_radius():
    n, src = 101, (0.0, 50.0)
    ex = ek.exact_constant((n, n), H, 2000.0, src)
    err = [float(np.abs(ek.solve(np.full((n, n), 2000.0), H, src, radius=r) - ex).max()) for r in (0.0, 3.0, 8.0)]
    print("eikonal: 101^2 error by radius 0, 3, 8:", err)
    assert err[0] > err[1] > err[2], err


def test_constant_velocity_3d():
    err, c0 = {}, 2500.0
    for n in (21, 41):
        m = (n - 1) // 2
        src = (float(m),) * 3
        T = ek.solve(np.full((n, n, n), c0), H, src)
        ex = ek.exact_constant((n, n, n), H, c0, src)
        err[n] = float(np.abs(T - ex).max() / ex.max())
        # never faster than the straight ray, never slower than the path along the axes (G <= a + f)
        man = ek.exact_constant((n,), H, c0, src[:1])
        man = man[:, None, None] + man[None, :, None] + man[None, None, :]
        assert np.all(T >= ex * (1.0 - 1e-12)) and np.all(T <= man * (1.0 + 1e-12))
        # exact along the axes through the source; the coordinate planes through it carry the 2-D solution
        assert np.abs(T[m, m] - ex[m, m]).max() <= 1e-14 * ex.max()
        T2 = ek.solve(np.full((n, n), c0), H, src[:2])
        assert np.abs(T[m] - T2).max() <= 1e-14 * ex.max() and np.abs(T[:, :, m] - T2).max() <= 1e-14 * ex.max()
    print("eikonal: 3-D error / max T, source in the centre:", err)
    assert err[21] / err[41] >= 1.5, err


def test_constant_gradient_medium():
    n, c0, g = 201, 1500.0, 1.0
    src = (0.0, (n - 1) / 2.0)
    c = c0 + g * H * np.arange(n, dtype=np.float64)[:, None] * np.ones((1, n))
    T = ek.solve(c, H, src)
    ex = ek.exact_gradient((n, n), H, c0, g, src)
    err = float(np.abs(T - ex).max() / ex.max())
    print("eikonal: 201^2, g = 1 / s: error / max T:", err)
    assert err < 0.012, err


def test_off_grid_ball_and_reference():
    idx, dist, ref = ek.ball((5.3, 30.6), (37, 41), H, 2.0)
    assert tuple(ref) == (5, 31)
    r = np.sqrt(((idx - np.array([5.3, 30.6])) ** 2).sum(axis=1))
    assert np.all(r <= 2.0) and np.allclose(dist, r * H) and len(idx) == 13
    flat = idx[:, 0] * 41 + idx[:, 1]
    assert np.all(np.diff(flat) > 0)
    idx0, dist0, ref0 = ek.ball((5.5, 30.5), (37, 41), H, 0.0)  # four nodes equally near: the lowest index
    assert idx0.tolist() == [[5, 30]] and tuple(ref0) == (5, 30) and np.isclose(dist0[0], H * np.sqrt(0.5))
    idx1, dist1, _ = ek.ball((4, 7), (37, 41), H, 0.0)
    assert idx1.tolist() == [[4, 7]] and dist1[0] == 0.0


# ---- fixed point and determinism ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, src, radius", [((37, 41), (5, 30), 0.0), ((19, 22, 27), (3.4, 15.2, 8.7), 2.0)])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_fixed_point_is_bit_exact_and_blocks_agree(shape, src, radius, dtype):
    c = layered_model(shape)
    T = ek.solve(c, H, src, radius=radius, dtype=dtype)
    assert T.dtype == np.dtype(dtype) and np.all(np.isfinite(T))
    s = (T.dtype.type(1) / c.astype(dtype))
    assert np.array_equal(ek.sweep(T, s, H), T)  # one more sweep changes no bit
    if dtype == "float64":
        Tb, outer = ek.solve_blocks(c, H, src, radius=radius, tile=8, inner=4)
        plain = ek.solve(c, H, src, radius=radius, return_sweeps=True)[1]
        err = float(np.abs(Tb - T).max() / T.max())
        print("eikonal: blocks of 8, 4 inner sweeps: %d outer steps (plain Jacobi: %d sweeps), difference %.1e" % (outer, plain, err))
        assert err <= 1e-13 and outer < plain


def test_listed_nodes_are_source_determined_only_where_below_G():
    shape, src = (37, 41), (5.3, 30.6)
    c = smooth_model(shape)
    init = ek.ball(src, shape, H, 2.0)
    T = ek.solve(c, H, init)
    W, _, dGds = ek.derivatives(T, c, H)
    listed = np.zeros(shape, bool)
    listed[tuple(init[0].T)] = True
    dead = dGds == 0
    assert np.all(listed[dead]) and dead.sum() >= 1  # only listed nodes have no dependence on their own slowness
    assert np.allclose(sum(W)[~dead], 1.0, rtol=0, atol=1e-14)  # the weights of a live cell sum to one


# ---- adjoint -----------------------------------------------------------------------------------------------------
def test_jacobi_adjoint_stops_and_matches_the_dense_solve():
    shape = (9, 10, 11)
    rng = np.random.default_rng(3)
    c = 2000.0 + 200.0 * rng.standard_normal(shape)
    T = ek.solve(c, H, (2, 3, 4))
    b = rng.standard_normal(shape)
    lam, n = ek.adjoint(T, c, H, b, return_sweeps=True)
    W, lower, _ = ek.derivatives(T, c, H)
    assert np.array_equal(ek.adjoint_sweep(lam, b, W, lower), lam)  # bit-exact stop
    A = ek.adjoint_matrix(T, c, H)
    assert np.all(np.linalg.matrix_power((A != 0).astype(np.float64), sum(shape)) == 0)  # nilpotent
    ref = np.linalg.solve(np.eye(T.size) - A.T, b.ravel())
    err = float(np.abs(lam.ravel() - ref).max() / np.abs(ref).max())
    print("eikonal: Jacobi adjoint, %d sweeps, against the dense solve: %.1e" % (n, err))
    assert err <= 1e-12


# ---- gradient against central differences --------------------------------------------------------------------------
_BASE = {}


def _problem(shape, model, src, radius):
    key = (shape, model, src, radius)
    if key not in _BASE:
        rng = np.random.default_rng(11)
        c = smooth_model(shape) if model == "smooth" else layered_model(shape)
        init = ek.ball(src, shape, H, radius)
        rec = np.array([[int(rng.integers(0, n)) for n in shape] for _ in range(12)])
        T = ek.solve(c, H, init)
        tobs = ek.times_at(T, rec) * (1.0 + 0.2 * rng.uniform(-1.0, 1.0, len(rec)))
        b = np.zeros(shape)
        np.add.at(b, tuple(rec.T), ek.times_at(T, rec) - tobs)
        _BASE[key] = (c, init, rec, tobs, T, ek.adjoint(T, c, H, b))
    return _BASE[key]


def _fd_error(shape, model, src, radius, wrt, ball_term=True):
    c, init, rec, tobs, T, lam = _problem(shape, model, src, radius)
    g = ek.gradient(T, lam, c, H, init, wrt, ball_term=ball_term)
    d = np.random.default_rng(5).standard_normal(shape)

    def J(cm):
        return 0.5 * float(np.sum((ek.times_at(ek.solve(cm, H, init), rec) - tobs) ** 2))
    if wrt == "velocity":
        eps = 1e-5 * np.abs(c).max() / np.abs(d).max()
        fd = (J(c + eps * d) - J(c - eps * d)) / (2.0 * eps)
    else:
        m = 1.0 / c ** 2
        eps = 1e-5 * np.abs(m).max() / np.abs(d).max()
        fd = (J((m + eps * d) ** -0.5) - J((m - eps * d) ** -0.5)) / (2.0 * eps)
    return abs(fd - float(np.sum(g * d))) / abs(fd)


@pytest.mark.parametrize("wrt", ek.WRT)
@pytest.mark.parametrize("model", ["smooth", "layered"])
@pytest.mark.parametrize("shape, src, radius", [((37, 41), (5, 30), 0.0), ((37, 41), (5.3, 30.6), 2.0),
                                                ((19, 22, 27), (3, 15, 8), 0.0), ((19, 22, 27), (3.4, 15.2, 8.7), 2.0)])
def test_gradient_against_central_differences(shape, src, radius, model, wrt):
    err = _fd_error(shape, model, src, radius, wrt)
    print("eikonal: gradient against central differences, %s %s %s: %.1e" % (shape, model, wrt, err))
    assert err < 1e-6
    if radius > 0.0:  # the source term must matter: without it the same check fails
        assert _fd_error(shape, model, src, radius, wrt, ball_term=False) > 1e-6


# ---- traveltime_fg on the twin-backed stand-in -------------------------------------------------------------------------
SHAPE = (21, 31)


def _survey():
    c_true = np.where(np.arange(SHAPE[0])[:, None] < 10, 1500.0, 3000.0) * np.ones(SHAPE)
    rec = np.array([[1, k] for k in range(0, 31, 2)] + [[19, k] for k in range(0, 31, 3)])
    shots = [sh.Shot(np.array([[1, x]]), np.zeros(4), rec) for x in (2, 15, 28)]
    shots.append(sh.Shot.at_coordinates([[1.5, 7.3]], np.zeros(4), [[18.2, 3.3], [17.5, 20.1], [1.2, 29.5], [17.9, 3.6]], SHAPE))
    e = ek.TwinEngine(SHAPE, H)
    e.vec_create(sh.TRAVELTIME_SLOTS)
    return c_true, shots, e, sh.traveltime_times(e, c_true, shots, radius=2.0)


class _Share(sh.NoExchange):
    """one rank of a host-summed job, recording instead of summing: the test adds the ranks' results itself"""

    def __init__(self, rank, world):
        self.rank, self.world = rank, world


def test_traveltime_fg_zero_at_the_true_model_nan_picks_and_ranks():
    c_true, shots, e, picks = _survey()
    J, g = sh.traveltime_fg(e, c_true, shots, picks, radius=2.0)
    assert J == 0.0 and not g.any()
    c0 = np.full(SHAPE, 2000.0)
    w = [np.linspace(0.5, 1.5, len(p)) for p in picks]
    J0, g0 = sh.traveltime_fg(e, c0, shots, picks, w, radius=2.0)
    assert J0 > 0.0 and g0.shape == SHAPE and np.all(np.isfinite(g0))
    # a NaN pick does not count: the same as weight zero there
    holes = [p.copy() for p in picks]
    w_zero = [x.copy() for x in w]
    for p, x in zip(holes, w_zero):
        p[1::4] = np.nan
        x[1::4] = 0.0
    Jn, gn = sh.traveltime_fg(e, c0, shots, holes, w, radius=2.0)
    Jz, gz = sh.traveltime_fg(e, c0, shots, picks, w_zero, radius=2.0)
    assert Jn == Jz and np.array_equal(gn, gz) and 0.0 < Jn < J0
    # two ranks, summed on the host, give the serial result
    parts = [sh.traveltime_fg(e, c0, shots, picks, w, radius=2.0, exchange=_Share(r, 2)) for r in (0, 1)]
    Js, gs = parts[0][0] + parts[1][0], parts[0][1] + parts[1][1]
    assert abs(Js - J0) <= 1e-14 * J0 and np.abs(gs - g0).max() <= 1e-13 * np.abs(g0).max()
    # both parametrisations describe the same functional
    Jm, gm = sh.traveltime_fg(e, c0, shots, picks, w, radius=2.0, wrt="slowness2")
    assert Jm == J0 and np.allclose(gm, g0 * (-(c0 ** 3) / 2.0), rtol=1e-12, atol=0)


def test_traveltime_tomography_reduces_the_misfit():
    c_true, shots, e, picks = _survey()
    log = lbfgs(lambda m: sh.traveltime_fg(e, m, shots, picks, radius=2.0), np.full(SHAPE, 2000.0), maxiter=5,
                first_step=100.0, bounds=(1000.0, 4000.0))[2]
    J = [l["f"] for l in log]
    print("eikonal: J over five L-BFGS iterations:", J, "factor %.2f" % (J[0] / J[-1]))
    assert len(J) == 6 and all(b < a for a, b in zip(J, J[1:])) and J[-1] < J[0] / 2.0


# ---- picks and mutes ---------------------------------------------------------------------------------------------
def test_first_breaks_follow_the_shift():
    dt, nt, f0 = 1e-3, 400, 25.0
    t = np.arange(nt) * dt
    shifts = np.array([0.0, 50.0, 123.4, 17.75])  # samples

    def wavelet(tt):
        a = (np.pi * f0 * (tt - 0.06)) ** 2
        return (1.0 - 2.0 * a) * np.exp(-a)
    d = np.stack([wavelet(t - s * dt) for s in shifts] + [np.zeros(nt)], axis=1)
    assert np.allclose(d[:, 0], ricker(nt, dt, f0, t0=0.06, dtype=np.float64))
    p = df.first_breaks(d, dt, 0.05)
    assert np.isnan(p[-1]) and np.all(np.isfinite(p[:-1]))
    assert np.all(np.abs((p[1:-1] - p[0]) / dt - shifts[1:]) <= 1.0), (p[:-1] - p[0]) / dt
    assert 0.0 < p[0] < 0.06  # before the peak
    assert np.array_equal(df.first_breaks(3.0 * d, dt, 0.05)[:-1], p[:-1])  # blind to the gain of a trace


def test_first_arrival_mute_is_the_offset_mute_with_times():
    shot = sh.Shot(np.array([[2, 5]]), np.zeros(60), np.array([[2, k] for k in range(0, 30, 3)]))
    dt, v = 2e-3, 1800.0
    off = H * np.abs(np.arange(0, 30, 3) - 5.0)
    for t_pad, taper in ((0.0, 0), (0.004, 7)):
        assert np.array_equal(df.first_arrival_mute(off / v, 60, dt, t_pad, taper),
                              df.offset_time_mute(shot, H, dt, v, t_pad, taper))
    w = df.first_arrival_mute([0.01, np.nan], 30, 1e-3, taper=4)
    assert w[:10, 0].sum() == 0.0 and w[14:, 0].min() == 1.0 and not w[:, 1].any()
