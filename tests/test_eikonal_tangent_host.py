"""The tangent of the first-arrival traveltimes without a GPU: ``eikonal.tangent`` (the definition of
``fwi_eikonal_tangent``), ``shots.TraveltimeOperator`` on the twin-backed stand-in ``eikonal.TwinEngine`` and
``newton.traveltime_gauss_newton``.

Bounds and where they come from:

* Central differences of ``eikonal.solve``, relative step 1e-5, asserted at 1e-6 of max |dT| (the project's convention,
  tests/test_eikonal_host.py: truncation ~1e-10, roundoff of T / step below 1e-9).  Seen: at most 2.3e-8.  With a ball
  the same check FAILS (seen 2.5e-2 ... 2.7e-1) when the source-determined nodes' b_i is left out.
* Transposition: |<w, J v> - <J^T w, v>| <= 1e-12 max(|.|), J^T = gradient(adjoint(.)); both sides sum a few
  thousand fp64 products of the same quantities in another order.  Seen: at most 1.8e-14.
  Both on an on-grid and an off-grid source, each with radius 0 and with radius 2.
* Dense solve (990 x 990, fp64): 1e-12 of max |dT|.
* The operator: symmetry of hvp and the two-rank sum at 1e-12 (sums of the same terms in another order); keep_times on
  and off, a NaN pick and a zero weight, bit for bit.
* Gauss-Newton: J must fall in each of three iterations and by at least 3 in all (seen 7.0)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from _eikonal import layered_model, smooth_model  # noqa: E402
from full_waveform_inversion_amd import eikonal as ek, newton as nw, shots as sh  # noqa: E402

H = 10.0
CASES = [(shape, src, radius)  # on- and off-grid sources, each with the nearest node alone and with a ball of 2 cells
         for shape, on, off in (((37, 41), (5, 30), (5.3, 30.6)), ((19, 22, 27), (3, 15, 8), (3.4, 15.2, 8.7)))
         for src in (on, off) for radius in (0.0, 2.0)]
MODELS = {"smooth": smooth_model, "layered": layered_model}

_BASE = {}


def _problem(shape, model, src, radius):
    """(c, init, T, d, w) of a case, computed once and left unchanged"""
    key = (shape, model, src, radius)
    if key not in _BASE:
        c = MODELS[model](shape)
        init = ek.ball(src, shape, H, radius)
        rng = np.random.default_rng(5)
        _BASE[key] = (c, init, ek.solve(c, H, init), rng.standard_normal(shape), rng.standard_normal(shape))
    return _BASE[key]


def _central_differences(c, init, d, wrt):
    if wrt == "velocity":
        eps = 1e-5 * np.abs(c).max() / np.abs(d).max()
        return (ek.solve(c + eps * d, H, init) - ek.solve(c - eps * d, H, init)) / (2.0 * eps)
    m = 1.0 / c ** 2
    eps = 1e-5 * np.abs(m).max() / np.abs(d).max()
    return (ek.solve((m + eps * d) ** -0.5, H, init) - ek.solve((m - eps * d) ** -0.5, H, init)) / (2.0 * eps)


@pytest.mark.parametrize("wrt", ek.WRT)
@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("shape, src, radius", CASES)
def test_tangent_against_central_differences_and_its_transpose(shape, src, radius, model, wrt):
    c, init, T, d, w = _problem(shape, model, src, radius)
    fd = _central_differences(c, init, d, wrt)
    x, n = ek.tangent(T, c, H, d, init, wrt, return_sweeps=True)
    scale = float(np.abs(fd).max())
    err = float(np.abs(x - fd).max()) / scale
    assert x.dtype == T.dtype and 2 <= n <= 4 * sum(shape)
    # <w, J v> against <J^T w, v>, J^T = gradient(adjoint(.))
    a = float(np.sum(w * x))
    b = float(np.sum(ek.gradient(T, ek.adjoint(T, c, H, w), c, H, init, wrt) * d))
    defect = abs(a - b) / max(abs(a), abs(b))
    print("eikonal tangent %s %s %s radius %g: %d sweeps, central differences %.1e (bound 1e-6), transpose %.1e "
          "(bound 1e-12)" % (shape, model, wrt, radius, n, err, defect))
    assert err <= 1e-6
    assert defect <= 1e-12
    if radius > 0.0:  # the ball's term must matter: without it the same check fails
        x0 = ek.tangent(T, c, H, d, init, wrt, ball_term=False)
        assert float(np.abs(x0 - fd).max()) / scale > 1e-6


def test_tangent_matches_the_dense_solve():
    shape = (9, 10, 11)
    rng = np.random.default_rng(3)
    c = 2000.0 + 200.0 * rng.standard_normal(shape)
    for src, radius, wrt in (((2, 3, 4), 0.0, "velocity"), ((2.4, 3.3, 4.6), 2.0, "slowness2")):
        init = ek.ball(src, shape, H, radius)
        T = ek.solve(c, H, init)
        d = rng.standard_normal(shape)
        x, n = ek.tangent(T, c, H, d, init, wrt, return_sweeps=True)
        b, _, _ = ek.tangent_rhs(T, c, H, d, init, wrt)
        A = ek.adjoint_matrix(T, c, H)
        ref = np.linalg.solve(np.eye(T.size) - A, b.ravel())
        err = float(np.abs(x.ravel() - ref).max() / np.abs(ref).max())
        print("eikonal tangent: Jacobi, %d sweeps, against the dense solve: %.1e" % (n, err))
        assert err <= 1e-12


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("shape, src, radius", [((37, 41), (5.3, 30.6), 2.0), ((19, 22, 27), (3.4, 15.2, 8.7), 2.0)])
def test_one_more_sweep_changes_no_bit(shape, src, radius, dtype):
    c = layered_model(shape).astype(dtype)
    init = ek.ball(src, shape, H, radius)
    T = ek.solve(c, H, init, dtype=dtype)
    d = np.random.default_rng(5).standard_normal(shape).astype(dtype)
    for wrt in ek.WRT:
        x = ek.tangent(T, c, H, d, init, wrt)
        b, W, lower = ek.tangent_rhs(T, c, H, d, init, wrt)
        assert x.dtype == np.dtype(dtype) and np.all(np.isfinite(x))
        assert np.array_equal(ek.tangent_sweep(x, b, W, lower), x)
        # a cell that is not live keeps its right-hand side
        dead = ~(sum(W) > 0)
        assert dead.any() and np.array_equal(x[dead], b[dead])


# ---- the operator on the twin-backed stand-in ----------------------------------------------------------------------
SHAPE = (21, 31)
RADIUS = 2.0


def _survey(off_grid=True):
    """the survey of tests/test_eikonal_host.py: two layers, three on-grid shots and one with off-grid points"""
    c_true = np.where(np.arange(SHAPE[0])[:, None] < 10, 1500.0, 3000.0) * np.ones(SHAPE)
    rec = np.array([[1, k] for k in range(0, 31, 2)] + [[19, k] for k in range(0, 31, 3)])
    shots = [sh.Shot(np.array([[1, x]]), np.zeros(4), rec) for x in (2, 15, 28)]
    if off_grid:
        shots.append(sh.Shot.at_coordinates([[1.5, 7.3]], np.zeros(4),
                                            [[18.2, 3.3], [17.5, 20.1], [1.2, 29.5], [17.9, 3.6]], SHAPE))
    e = ek.TwinEngine(SHAPE, H)
    e.vec_create(16)
    return c_true, shots, e, sh.traveltime_times(e, c_true, shots, radius=RADIUS)


class _Share(sh.NoExchange):
    """one rank of a host-summed job, recording instead of summing: the test adds the ranks' results itself"""

    def __init__(self, rank, world):
        self.rank, self.world = rank, world


@pytest.fixture(scope="module")
def survey():
    c_true, shots, e, picks = _survey()
    c0 = smooth_model(SHAPE)  # no symmetry: the times have no exact ties, where T is not differentiable
    w = [np.linspace(0.5, 1.5, len(p)) for p in picks]
    rng = np.random.default_rng(8)
    return e, shots, picks, c0, w, rng.standard_normal(SHAPE), rng.standard_normal(SHAPE)


@pytest.mark.parametrize("wrt", ek.WRT)
def test_operator_hvp_is_symmetric_positive_and_ranks_add_up(survey, wrt):
    e, shots, picks, c0, w, u, v = survey
    op = sh.TraveltimeOperator(e, c0, shots, radius=RADIUS, wrt=wrt, pick_weights=w)
    assert op.slots_needed(len(shots)) == 6 + len(shots) <= len(e.vecs)
    Hu, Hv = op.hvp(u), op.hvp(v)
    assert Hu.shape == SHAPE and Hu.dtype == np.float64
    a, b = float(np.vdot(v, Hu)), float(np.vdot(u, Hv))
    print("traveltime operator %s: symmetry defect %.1e, v.Hv %.3e" % (wrt, abs(a - b) / max(abs(a), abs(b)),
                                                                        float(np.vdot(v, Hv))))
    assert abs(a - b) <= 1e-12 * max(abs(a), abs(b))
    assert float(np.vdot(v, Hv)) >= 0.0 and float(np.vdot(u, Hu)) > 0.0
    # hvp is vjp of the weighted jvp, and the kept times are the times
    Jv = op.jvp(v)
    assert [len(x) for x in Jv] == [len(p) for p in picks]
    assert np.abs(op.vjp([wi * x for wi, x in zip(w, Jv)]) - Hv).max() <= 1e-12 * np.abs(Hv).max()
    assert all(np.array_equal(x, y) for x, y in zip(op.times(), sh.traveltime_times(e, c0, shots, radius=RADIUS)))
    assert op.solves == {"eikonal": len(shots), "tangent": 3 * len(shots), "adjoint": 3 * len(shots)}
    # two ranks, summed on the host, give the serial result
    # (both ranks on the one stand-in: each keeps its times in slots of its own)
    parts = [sh.TraveltimeOperator(e, c0, shots, radius=RADIUS, wrt=wrt, pick_weights=w, exchange=_Share(r, 2),
                                   slot0=8 * r) for r in (0, 1)]
    assert all(p.slots_needed(2) == 8 for p in parts)
    Hs = parts[0].hvp(v) + parts[1].hvp(v)
    assert np.abs(Hs - Hv).max() <= 1e-12 * np.abs(Hv).max()
    Js = [x + y for x, y in zip(parts[0].jvp(v), parts[1].jvp(v))]
    assert all(np.array_equal(x, y) for x, y in zip(Js, Jv))


def test_operator_keep_times_nan_picks_and_spread_receivers(survey):
    e, shots, picks, c0, w, u, v = survey
    op = sh.TraveltimeOperator(e, c0, shots, radius=RADIUS, pick_weights=w)
    Hv, Jv = op.hvp(v), op.jvp(v)
    # times solved again in every product: the same arrays, three solves per shot and product instead of two
    again = sh.TraveltimeOperator(e, c0, shots, radius=RADIUS, pick_weights=w, keep_times=False)
    assert again.slots_needed(len(shots)) == 7
    assert np.array_equal(again.hvp(v), Hv) and all(np.array_equal(x, y) for x, y in zip(again.jvp(v), Jv))
    assert again.solves == {"eikonal": 2 * len(shots), "tangent": 2 * len(shots), "adjoint": len(shots)}
    # a NaN pick does not count: the same as weight zero there
    holes = [p.copy() for p in picks]
    w_zero = [x.copy() for x in w]
    for p, x in zip(holes, w_zero):
        p[1::4] = np.nan
        x[1::4] = 0.0
    Hn = sh.TraveltimeOperator(e, c0, shots, radius=RADIUS, pick_weights=w, picks=holes).hvp(v)
    Hz = sh.TraveltimeOperator(e, c0, shots, radius=RADIUS, pick_weights=w_zero).hvp(v)
    assert np.array_equal(Hn, Hz) and not np.array_equal(Hn, Hv)
    # off-grid receivers: the Spread-weighted nodes of the tangent field
    s = shots[3]
    init = ek.ball(s.src_spread.coords[0], SHAPE, H, RADIUS)
    x = ek.tangent(ek.solve(c0, H, init), c0, H, v, init)
    sp = s.rec_spread
    want = np.add.reduceat(x[tuple(np.asarray(sp.idx).T)] * sp.weights, sp.pt_start[:-1])
    assert len(Jv[3]) == 4 and np.array_equal(Jv[3], want)
    # jvp predicts the change of the picks
    eps = 1e-5 * np.abs(c0).max() / np.abs(v).max()
    fd = [(a - b) / (2.0 * eps) for a, b in zip(sh.traveltime_times(e, c0 + eps * v, shots, radius=RADIUS),
                                                sh.traveltime_times(e, c0 - eps * v, shots, radius=RADIUS))]
    scale = max(float(np.abs(f).max()) for f in fd)
    assert max(float(np.abs(a - b).max()) for a, b in zip(Jv, fd)) <= 1e-6 * scale


def test_gauss_newton_tomography_reduces_the_misfit():
    c_true, shots, e, picks = _survey(off_grid=False)
    model, log = nw.traveltime_gauss_newton(e, np.full(SHAPE, 2000.0), shots, picks, iters=3, cg_iters=6,
                                            radius=RADIUS, bounds=(1000.0, 4000.0))
    J = [entry["J"] for entry in log]
    print("traveltime Gauss-Newton: J", J, "factor %.2f" % (J[0] / J[-1]))
    for entry in log:
        print("  iteration %d: t %s, mu %s, cg products %d, solves %r" % (
            entry["iter"], entry.get("t"), entry.get("mu"), len(entry.get("cg", [1])) - 1, entry["solves"]))
    assert len(J) == 4 and all(b < a for a, b in zip(J, J[1:])) and J[-1] <= J[0] / 3.0
    assert model.shape == SHAPE and model.min() >= 1000.0 and model.max() <= 4000.0
    assert all(set(entry["solves"]) == {"eikonal", "tangent", "adjoint"} for entry in log)
    assert all(entry["t"] == 1.0 and entry["mu"] > 0.0 and entry["cg"][-1]["stop"] for entry in log[1:])
    # the step alone: cg on the operator reduces the residual of the damped normal equations
    J0, g = sh.traveltime_fg(e, np.full(SHAPE, 2000.0), shots, picks, radius=RADIUS)
    op = sh.TraveltimeOperator(e, np.full(SHAPE, 2000.0), shots, radius=RADIUS, picks=picks)
    p, cglog = nw.traveltime_newton_step(op, g, damping=log[1]["mu"], maxiter=6)
    assert J0 == J[0] and cglog[-1]["rnorm"] < cglog[0]["rnorm"] and float(np.vdot(p, g)) < 0.0


def test_refused_arguments():
    shape = (9, 12)
    e = ek.TwinEngine(shape, H)
    e.vec_create(4)
    T, D, X, SC = range(4)
    init = ek.ball((4, 5), shape, H, 1.0)
    bad = [
        lambda: e.eikonal_tangent(T, D, X, SC, init),                                        # no model
    ]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    e.set_model(np.full(shape, 2000.0))
    e.eikonal(init, T, SC)
    e.vec_upload(D, np.ones(shape))
    node = np.array([[4, 5]])
    bad = [
        lambda: e.eikonal_tangent(T, D, X, 4, init),                                          # no such slot
        lambda: e.eikonal_tangent(T, D, X, -1, init),
        lambda: e.eikonal_tangent(T, T, X, SC, init),                                         # two slots equal
        lambda: e.eikonal_tangent(T, D, D, SC, init),
        lambda: e.eikonal_tangent(T, D, X, X, init),
        lambda: e.eikonal_tangent(T, D, X, T, init),
        lambda: e.eikonal_tangent(T, D, X, SC, (np.zeros((0, 2), np.int32), np.zeros(0), node[0])),  # empty list
        lambda: e.eikonal_tangent(T, D, X, SC, (np.array([[9, 5]]), np.zeros(1), node[0])),   # outside the grid
        lambda: e.eikonal_tangent(T, D, X, SC, (node, np.zeros(1), np.array([4, 12]))),
        lambda: e.eikonal_tangent(T, D, X, SC, (np.concatenate([node, node]), np.zeros(2), node[0])),  # twice
        lambda: e.eikonal_tangent(T, D, X, SC, (node, np.array([-1.0]), node[0])),            # a negative distance
        lambda: e.eikonal_tangent(T, D, X, SC, (node, np.array([np.inf]), node[0])),
        lambda: e.eikonal_tangent(T, D, X, SC, init, wrt="impedance"),                        # an unknown wrt
        lambda: ek.tangent(e.vecs[T], e.c, H, np.ones(shape), init, wrt="impedance"),
        lambda: ek.tangent(e.vecs[T], e.c, H, np.ones((3, 3)), init),
        lambda: sh.TraveltimeOperator(e, None, [], wrt="impedance"),
    ]
    before = [v.copy() for v in e.vecs]
    for n, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
        assert all(np.array_equal(a, b) for a, b in zip(before, e.vecs)), n
    e.eikonal_tangent(T, D, X, SC, init)
    assert e.last_eikonal_launches >= 2 and np.all(np.isfinite(e.vecs[X])) and e.vecs[X].any()
