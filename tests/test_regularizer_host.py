"""Tikhonov / total-variation regularisation without a GPU: the library's fp64 NumPy twin (regularizers.py) against the
restatement of tests/_regularizer.py, the properties of the definition (gradient of the value, symmetry, positivity,
null space, prior, weights), the exported symbol, and the wrappers around fg and the Gauss-Newton products."""
import ctypes as C
import os

import numpy as np
import pytest

import _born
import _regularizer as tr
from full_waveform_inversion_amd import _lib, newton, regularizers as rg, shots as sh
from oracle import fwi_oracle as fo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWI_EINVAL = 1
U = 2.0 ** -53
SHAPES = [(37, 23), (19, 21, 23), (9, 6, 1), (1, 9)]
KINDS = [("tikhonov", None), ("tv", 0.3)]


def _fields(shape, seed=0):
    rng = np.random.default_rng(seed + sum(shape))
    return 2000.0 + rng.standard_normal(shape), 2000.0 + 0.5 * rng.standard_normal(shape), rng.standard_normal(shape)


def _w(shape):
    return [1.0, 0.25, 2.0][:len(shape)]


@pytest.mark.parametrize("kind,eps", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_the_library_twin_equals_the_restatement(shape, kind, eps):
    x, x0, v = _fields(shape)
    for w in (1.0, _w(shape)):
        for prior in (None, x0):
            for vv in (None, v):
                got = rg.apply(x, vv, kind, w, eps, prior)
                ref = tr.apply(x, vv, kind, w, eps, prior)
                M = tr.majorant(x, vv, kind, w, eps, prior)
                err = np.abs(got - ref)
                assert got.shape == ref.shape and (err <= 64 * U * M).all(), (err.max(), M.max())
            r, r_ref = rg.value(x, kind, w, eps, prior), tr.value(x, kind, w, eps, prior)
            assert abs(r - r_ref) <= (x.size + 16) * U * r_ref, (r, r_ref)
            r2, g2 = rg.value_and_gradient(x, kind, w, eps, prior)
            assert r2 == r and np.array_equal(g2, rg.apply(x, None, kind, w, eps, prior))


@pytest.mark.parametrize("shape", SHAPES[:2], ids=str)
def test_tikhonov_is_the_quadratic_its_gradient_and_operator_describe(shape):
    _, _, v = _fields(shape, 1)
    x = _fields(shape, 2)[2]
    w, t = _w(shape), 0.37
    r0, g = rg.value_and_gradient(x, "tikhonov", w)
    r1 = rg.value(x + t * v, "tikhonov", w)
    gv, vLv = float(np.vdot(g, v)), float(np.vdot(v, rg.apply(x, v, "tikhonov", w)))
    lhs, rhs = r1 - r0 - t * gv, 0.5 * t * t * vLv
    assert abs(lhs - rhs) <= 64 * U * (r1 + r0 + abs(t * gv) + rhs), (lhs, rhs)


@pytest.mark.parametrize("shape", SHAPES[:2], ids=str)
def test_the_tv_gradient_is_the_derivative_of_the_value(shape):
    x, x0, v = _fields(shape, 3)
    w, eps, t = _w(shape), 0.3, 1e-2  # remainder ~ t^2 N / eps ~ 1e-1: thirteen digits above the round-off of R ~ N
    r0, g = rg.value_and_gradient(x, "tv", w, eps, x0)
    gv = float(np.vdot(g, v))
    rem = [rg.value(x + s * v, "tv", w, eps, x0) - r0 - s * gv for s in (t, 0.5 * t)]
    assert rem[1] > 0.0 and 3.0 <= rem[0] / rem[1] <= 5.0, rem


@pytest.mark.parametrize("kind,eps", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_the_operator_is_symmetric_positive_semidefinite_with_constants_in_its_null_space(shape, kind, eps):
    x, x0, v = _fields(shape, 4)
    u = np.random.default_rng(5).standard_normal(shape)
    w = _w(shape)
    Lv, Lu = rg.apply(x, v, kind, w, eps, x0), rg.apply(x, u, kind, w, eps, x0)
    a, b = float(np.vdot(u, Lv)), float(np.vdot(v, Lu))
    assert abs(a - b) <= 64 * U * float(np.sum(np.abs(u * Lv)) + np.sum(np.abs(v * Lu)))
    assert float(np.vdot(v, Lv)) >= 0.0 and float(np.vdot(u, Lu)) >= 0.0
    c = np.full(shape, 1234.5)
    r, g = rg.value_and_gradient(c, kind, w, eps)
    assert r == 0.0 and not g.any()
    assert not rg.apply(x, c, kind, w, eps, x0).any()  # L(d; const) = 0 exactly, whatever d
    r, g = rg.value_and_gradient(x, kind, w, eps, x)   # prior = model
    assert r == 0.0 and not g.any()


@pytest.mark.parametrize("kind,eps", KINDS)
def test_a_zero_weight_switches_its_axis_off(kind, eps):
    shape = (7, 8, 9)
    x, x0, v = _fields(shape, 6)
    rng = np.random.default_rng(7)
    for ax in range(3):
        w = [1.0, 0.5, 2.0]
        w[ax] = 0.0
        line = [1] * 3
        line[ax] = shape[ax]
        bump = rng.standard_normal(line)  # varies along the switched-off axis only
        d = np.broadcast_to(bump, shape)
        r, g = rg.value_and_gradient(d, kind, w, eps)
        assert r == 0.0 and not g.any()
        # and the other axes do not see it: every line along the axis is treated alone
        sl = [slice(None)] * 3
        sl[ax] = 3
        keep = [k for k in range(3) if k != ax]
        got = rg.apply(x, v, kind, w, eps, x0)[tuple(sl)]
        if kind == "tikhonov":
            want = rg.apply(x[tuple(sl)], v[tuple(sl)], kind, [w[k] for k in keep], eps, x0[tuple(sl)])
            assert np.array_equal(got, want)
    assert rg.value(x, kind, 0.0, eps) == 0.0
    with pytest.raises(ValueError):
        rg.value(x, kind, [1.0, 1.0], eps)
    with pytest.raises(ValueError):
        rg.value(x, kind, [1.0, -1.0, 1.0], eps)
    with pytest.raises(ValueError):
        rg.value(x, "tv", 1.0, None)
    with pytest.raises(ValueError):
        rg.value(x, "huber", 1.0, 0.1)


def test_the_library_exports_fwi_vec_regularizer_at_abi_14():
    lib = _lib.load()
    assert lib.fwi_abi_version() == _lib.ABI_VERSION == 14
    header = open(os.path.join(ROOT, "include", "fwi.h")).read()
    assert "fwi_vec_regularizer" in _lib.SIGNATURES and hasattr(lib, "fwi_vec_regularizer")
    assert "fwi_vec_regularizer(" in header and "FWI_REG_TIKHONOV = 0, FWI_REG_TV = 1" in header
    assert _lib.REG_KINDS == {"tikhonov": 0, "tv": 1}
    w = np.ones(3).ctypes.data_as(C.POINTER(C.c_double))
    val = C.c_double(0.0)
    assert lib.fwi_vec_regularizer(None, 1, 0, -1, -1, 1, 1.0, 0.0, w, 0.1, C.byref(val)) == FWI_EINVAL
    assert lib.fwi_vec_regularizer(None, 0, 0, -1, -1, -1, 1.0, 0.0, None, 0.0, None) == FWI_EINVAL


def _quadratic(shape=(11, 13)):
    rng = np.random.default_rng(8)
    x_star = rng.standard_normal(shape)

    def fg(x):
        r = np.asarray(x, np.float64) - x_star
        return 0.5 * float(np.vdot(r, r)), r

    return x_star, fg


def test_regularized_fg_adds_the_term_and_is_fg_itself_without_a_weight():
    x_star, fg = _quadratic()
    x0 = 0.5 * x_star
    assert rg.regularized_fg(fg, 0.0, "tv", 1.0, 0.1) is fg
    assert rg.regularized_fg_device(None, fg, 0.0) is fg
    x = np.random.default_rng(9).standard_normal(x_star.shape)
    for kind, eps in KINDS:
        f, g = rg.regularized_fg(fg, 0.7, kind, [1.0, 2.0], eps, x0)(x)
        r, gr = tr.value(x, kind, [1.0, 2.0], eps, x0), tr.apply(x, None, kind, [1.0, 2.0], eps, x0)
        f0, g0 = fg(x)
        assert abs(f - (f0 + 0.7 * r)) <= 1e-13 * abs(f) and np.allclose(g, g0 + 0.7 * gr, rtol=0, atol=1e-13)
    g32 = rg.regularized_fg(lambda m: (1.0, np.zeros(m.shape, np.float32)), 0.7, "tikhonov")(x)[1]
    assert g32.dtype == np.float32
    with pytest.raises(ValueError):
        rg.regularized_fg(fg, -1.0, "tikhonov")
    with pytest.raises(ValueError):
        rg.regularized_fg(fg, 1.0, "tv")


def test_cg_with_the_tikhonov_term_solves_the_normal_equations():
    """1/2 |x - x*|^2 + lam R(x - x0) is quadratic: one exact Newton step from any model lands on
    (I + lam L) x = x* + lam L x0."""
    x_star, fg = _quadratic()
    x0 = np.zeros_like(x_star) + 0.3
    reg = rg.Regularizer(2.5, "tikhonov", [1.0, 0.5], x0=x0)
    m = np.random.default_rng(10).standard_normal(x_star.shape)
    f, g = rg.regularized_fg(fg, reg.lam, reg.kind, reg.weight, reg.eps, reg.x0)(m)
    p, log = newton.cg(lambda v: v + reg.hvp(m, v), -g, maxiter=400, rtol=1e-13)
    assert log[-1]["stop"] == "converged"
    x = m + p
    L = lambda v: rg.apply(v, v, "tikhonov", [1.0, 0.5])  # noqa: E731  (Tikhonov: L does not depend on its first argument)
    res = x + 2.5 * L(x) - (x_star + 2.5 * L(x0))
    assert np.abs(res).max() <= 1e-11 * np.abs(x_star).max(), np.abs(res).max()
    assert np.linalg.norm(x - x_star) > 1e-2  # the term pulled the answer


def _survey(seed=2):  # the host fake of tests/test_born_host.py
    shape, order, npml, nt = (36, 44), 4, 6, 70
    rng = np.random.default_rng(seed)
    c = 2000.0 + 500.0 * rng.random(shape)
    h = 10.0
    dt = 0.6 * fo.cfl_dt(c.max(), h, 2, order)
    wav = fo.ricker(nt, dt, 0.12 / dt / 8)
    rec = np.stack([np.full(10, 8), np.arange(4, 44, 4)], 1)
    shots = [sh.Shot(np.array([[7, x]]), wav, rec) for x in (8, 20, 34)]
    v = 30.0 * rng.standard_normal(shape)
    mk = lambda: _born.BornOracleEngine(shape, h, dt, nt, order=order, npml=npml)  # noqa: E731
    return c, shots, v, mk


def test_gauss_newton_step_without_a_regularizer_is_unchanged_and_with_one_adds_its_term():
    c, shots, v, mk = _survey()
    e = mk()
    H = lambda x: sh.gauss_newton_hvp(e, c, shots, x)  # noqa: E731
    g = -H(v)
    p0, log0 = newton.gauss_newton_step(e, c, shots, g, maxiter=3, rtol=1e-8)
    p1, log1 = newton.gauss_newton_step(e, c, shots, g, maxiter=3, rtol=1e-8, regularizer=None)
    pc, logc = newton.cg(lambda x: np.asarray(H(np.asarray(x, np.float64)), np.float64), -g, maxiter=3, rtol=1e-8)
    assert np.array_equal(p0, p1) and log0 == log1
    assert np.array_equal(p0, pc) and log0 == logc  # what the function was before it took the argument
    lam = float(np.abs(H(v)).max() / np.abs(rg.apply(c, v, "tv", 1.0, 5.0)).max())
    reg = rg.Regularizer(lam, "tv", 1.0, 5.0)
    pr, logr = newton.gauss_newton_step(e, c, shots, g, maxiter=3, rtol=1e-8, regularizer=reg)
    pe, loge = newton.cg(lambda x: H(x) + lam * tr.apply(c, x, "tv", 1.0, 5.0), -g, maxiter=3, rtol=1e-8)
    assert np.allclose(pr, pe, rtol=1e-9, atol=1e-9 * np.abs(pe).max()) and not np.allclose(pr, p0, rtol=1e-3)
    assert all(r["curvature"] > 0.0 for r in logr[1:])
