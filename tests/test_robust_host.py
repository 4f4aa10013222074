"""The robust (Huber, hybrid L1/L2, Cauchy) misfits without a GPU: the NumPy twin alone (datafit.RobustMisfit,
datafit.median_abs, datafit.mad_scale), the binding, the shot loop and the Gauss-Newton product on the CPU oracle, and an
outlier experiment: with 2 % of the observed samples replaced by spikes of 50 times the largest amplitude, the gradient
of every robust kind stays closer (in cosine) to its own clean gradient than least squares' does."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from _born import BornOracleEngine  # noqa: E402
from _oracle_engine import OracleEngine  # noqa: E402
from full_waveform_inversion_amd import _lib, datafit as df, shots as sh  # noqa: E402
from oracle import fwi_oracle as fo  # noqa: E402

FWI_EINVAL = 1
DT = 2e-3
KINDS = list(df.ROBUST_KINDS)
FLAGS = [(False, False, False), (True, False, True), (False, True, False), (True, True, True)]


def _random(nt, ntr, seed):
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((nt, ntr))
    d = s + 0.3 * rng.standard_normal((nt, ntr))
    d[rng.random((nt, ntr)) < 0.05] += 8.0
    return rng, s, d


def _options(rng, nt, ntr, flags):
    weighted, with_taps, trace_weighted = flags
    M = None
    if weighted:
        M = 0.25 + 0.75 * rng.random((nt, ntr))
        M[nt // 3] = 0.0
    taps = df.lowpass_taps(DT, 60.0, 5) if with_taps else None
    tw = None
    if trace_weighted:
        tw = 0.25 + rng.random(ntr)
        tw[ntr // 3] = 0.0
    return M, taps, tw


@pytest.mark.parametrize("flags", FLAGS, ids=["---", "M-w", "-B-", "MBw"])
@pytest.mark.parametrize("kind", KINDS)
def test_twin_gradient_matches_central_differences(kind, flags):
    """dJ/ds . v against (J(s + h v) - J(s - h v)) / 2 h along random directions.  hybrid and cauchy are smooth: the
    error falls like h^2 between two step sizes (a ratio of 4, taken as within [3, 5]).  huber is C^1 with a kink in its
    second derivative: on inputs with no |e| within 10 h |de/dh| of its threshold (asserted) J is quadratic along the line
    on every sample, and central differences are exact to the round-off of J over the step, taken as 64 * 2^-52 J / h"""
    nt, ntr = 41, 7
    rng, s, d = _random(nt, ntr, 3)
    M, taps, tw = _options(rng, nt, ntr, flags)
    obj = df.RobustMisfit(kind, scale=0.4, taps=taps)
    a = obj.thresh_of(None, d, M)
    J, r = obj(s, d, M, tw)
    assert J > 0.0 and 0 < np.sum(obj.nout) < nt * ntr  # both branches
    for trial in range(3):
        v = rng.standard_normal((nt, ntr))
        exact = float(np.sum(r * v))
        h1, h2 = (1e-5, 5e-6) if kind == "huber" else (1e-3, 5e-4)
        de = obj.residuals(v, np.zeros_like(v), M)[0]  # e is linear in s
        if kind == "huber":
            e0 = obj.residuals(s, d, M)[0]
            assert np.all(np.abs(np.abs(e0) - a) > 10.0 * h1 * np.abs(de))  # a condition on the inputs
        err = [abs((obj(s + h * v, d, M, tw)[0] - obj(s - h * v, d, M, tw)[0]) / (2.0 * h) - exact) for h in (h1, h2)]
        print(kind, flags, "errors", err, "of", abs(exact))
        if kind == "huber":  # (what is left is the round-off of the two sums of J over the step)
            assert max(err) <= 64.0 * 2.0 ** -52 * J / h2
        else:
            # (Taylor: h^2 / 6 times the third derivative along the line; the third derivative of rho is at most 3 / a)
            third = float(np.sum((1.0 if tw is None else tw) * np.abs(de) ** 3 * 3.0 / a))
            assert err[0] <= h1 * h1 / 6.0 * third and 3.0 <= err[0] / err[1] <= 5.0


@pytest.mark.parametrize("kind", KINDS)
def test_equal_data_give_exact_zeros_and_the_shape_of_psi(kind):
    rng, s, d = _random(30, 5, 4)
    M, taps, tw = _options(rng, 30, 5, (True, True, True))
    obj = df.RobustMisfit(kind, scale=0.4, taps=taps)
    J, r = obj(s, s, M, tw)
    assert J == 0.0 and not np.any(r) and not np.any(obj.nout) and not np.any(obj.J_trace)
    # |d(psi e)/de| <= 1 everywhere; cauchy's reaches -1/8 at v = 3 (not convex), the others' stays >= 0
    e = np.linspace(-30.0, 30.0, 200001)[:, None]
    psi, rho = obj.psi_rho(e, np.array([1.0]))
    slope = np.diff((psi * e)[:, 0]) / np.diff(e[:, 0])
    assert np.all(np.abs(slope) <= 1.0 + 1e-9) and np.all(psi > 0.0) and np.all(psi <= 1.0) and np.all(rho >= 0.0)
    if kind == "cauchy":
        assert abs(slope.min() + 0.125) < 1e-6 and abs(abs(e[np.argmin(slope), 0]) - np.sqrt(3.0)) < 1e-3
    else:
        assert slope.min() >= -1e-12
    # rho is the integral of psi e
    mid = 0.5 * (e[1:, 0] + e[:-1, 0])
    pm = obj.psi_rho(mid[:, None], np.array([1.0]))[0][:, 0]
    # (the midpoint rule, whose error is h^3 / 24 per step where psi e is smooth and below h^2 at huber's kink)
    assert np.allclose(np.diff(rho[:, 0]), pm * mid * np.diff(e[:, 0]), rtol=0.0, atol=(e[1, 0] - e[0, 0]) ** 2)


@pytest.mark.parametrize("flags", FLAGS, ids=["---", "M-w", "-B-", "MBw"])
def test_huber_at_an_infinite_threshold_is_weighted_l2_exactly(flags):
    rng, s, d = _random(37, 6, 5)
    M, taps, _ = _options(rng, 37, 6, flags)
    for obj in (df.RobustMisfit("huber", scale=np.inf, taps=taps), df.RobustMisfit("huber", c=np.inf, scale=1.0, taps=taps)):
        J, r = obj(s, d, M)
        Jw, rw = df.WeightedL2(taps)(s, d, M)
        assert J == Jw and np.array_equal(r, rw) and not np.any(obj.nout) and np.all(obj.psi == 1.0)


def _by_sort(a, keep):
    vals = np.abs(a)[keep]
    return (np.sort(vals)[(vals.size - 1) // 2], vals.size) if vals.size else (0.0, 0)


def test_median_abs_is_the_lower_median_of_np_sort():
    rng = np.random.default_rng(6)
    for dtype in (np.float32, np.float64):
        e = rng.standard_normal((12, 9)).astype(dtype)   # even count
        e[:, 1] = np.round(e[:, 1])                      # ties
        e[:7, 2] = 0.0                                   # more than half exact zeros
        e[3, 3], e[4, 3], e[5, 3] = np.nan, np.inf, -np.inf
        e[:, 4] = np.nan
        e[:, 5] = -0.75                                  # all equal
        M = (rng.random(e.shape) < 0.7).astype(dtype)
        M[:, 6] = 0.0                                    # a dead-weight row of the gather's transpose: nothing counts
        M[5] = 0.0                                       # a dead time row: odd counts where all else counts
        for W in (None, M, 0.5 * M):
            keep = np.ones(e.shape, bool) if W is None else W > 0
            med, count = df.median_abs(e, W)
            assert med.dtype == np.float64 and count.dtype == np.int64 and med.shape == count.shape == (9,)
            for j in range(9):
                m, n = _by_sort(e[:, j], keep[:, j])
                assert count[j] == n and (med[j] == m or (np.isnan(med[j]) and np.isnan(m))), (j, med[j], m)
            m, n = _by_sort(e, keep)
            assert df.median_abs(e, W, per_trace=False) == (m, n)
            assert np.array_equal(df.mad_scale(e, W), df.MAD_TO_SIGMA * med, equal_nan=True)
        assert df.median_abs(e)[0][2] == 0.0 and df.median_abs(e)[0][5] == 0.75 and np.isfinite(df.median_abs(e)[0][3])
        assert df.median_abs(e, M)[1][6] == 0 and df.median_abs(e, M)[0][6] == 0.0
        odd = e[:11]
        assert np.array_equal(df.median_abs(odd)[0][:1], [np.sort(np.abs(odd[:, 0]))[5]])
    assert df.median_abs(np.zeros((0, 3)))[0].tolist() == [0.0, 0.0, 0.0]
    assert df.median_abs(np.zeros((4, 3)), np.zeros((4, 3)), per_trace=False) == (0.0, 0)
    with pytest.raises(ValueError):
        df.median_abs(np.zeros(4))
    with pytest.raises(ValueError):
        df.median_abs(np.zeros((4, 3)), np.ones((4, 2)))


@pytest.mark.parametrize("kind", KINDS)
def test_normal_is_symmetric_positive_semidefinite(kind):
    nt, ntr = 23, 4
    rng, s, d = _random(nt, ntr, 7)
    M, taps, tw = _options(rng, nt, ntr, (True, True, True))
    obj = df.RobustMisfit(kind, scale=0.4, taps=taps)
    obj(s, d, M, tw)
    n = nt * ntr
    A = np.stack([obj.normal(col.reshape(nt, ntr), M, tw).ravel() for col in np.eye(n)], 1)
    assert np.allclose(A, A.T, rtol=0.0, atol=1e-14 * np.abs(A).max())
    assert np.linalg.eigvalsh(0.5 * (A + A.T)).min() >= -1e-12 * np.abs(A).max()
    x = rng.standard_normal((nt, ntr))
    assert np.array_equal(obj.normal(x, M, tw), obj.normal(x, M, tw, obj.psi))
    # at an infinite threshold it is WeightedL2's
    inf = df.RobustMisfit("huber", scale=np.inf, taps=taps)
    inf(s, d, M)
    assert np.array_equal(inf.normal(x, M), df.WeightedL2(taps).normal(x, M))
    with pytest.raises(ValueError):
        df.RobustMisfit(kind, scale=0.4).normal(x)  # no psi yet


def test_argument_refusals():
    rng, s, d = _random(20, 3, 8)
    for bad in (dict(kind="l1"), dict(c=0.0), dict(c=-1.0), dict(c=np.nan), dict(scale=0.0), dict(scale=-1.0),
                dict(kind="hybrid", c=np.inf), dict(kind="cauchy", c=np.inf), dict(taps=np.ones((2, 2)))):
        with pytest.raises(ValueError):
            df.RobustMisfit(**bad)
    obj = df.RobustMisfit("hybrid", scale=0.5)
    for bad in (dict(thresh=0.0), dict(thresh=np.array([1.0, np.nan, 1.0])), dict(thresh=np.inf),
                dict(weights=-np.ones((20, 3))), dict(weights=np.ones((20, 2))), dict(trace_weights=np.ones(2)),
                dict(trace_weights=np.array([1.0, -1.0, 1.0]))):
        with pytest.raises(ValueError):
            obj(s, d, **bad)
    with pytest.raises(ValueError):
        obj(s, d[:, :2])
    with pytest.raises(ValueError):
        df.RobustMisfit("hybrid", scale=[0.5, 0.5])(s, d)  # a scale per shot needs the shot
    with pytest.raises(ValueError):
        df.RobustMisfit("hybrid", scale=[np.inf])(s, d, shot=0)
    assert df.RobustMisfit("huber", scale=[np.inf])(s, d, shot=0)[0] == df.WeightedL2()(s, d)[0]
    # defaults: c per kind; the data-only scale, crude, with a dead trace taking the gather's largest threshold
    assert [df.RobustMisfit(k).c for k in KINDS] == [1.345, 1.0, 2.385]
    d2 = d.copy()
    d2[:, 1] = 0.0
    a = df.RobustMisfit("huber").thresh_of(0, d2)
    ref = 1.345 * (df.MAD_TO_SIGMA * np.sort(np.abs(d2), axis=0)[(20 - 1) // 2])
    assert np.array_equal(a[[0, 2]], ref[[0, 2]]) and a[1] == max(ref[0], ref[2])


class _StandIn:
    def misfit_robust(self, *args, **kw):
        self.args, self.kw = args, kw
        return 1.5


def test_objective_protocol_and_binding():
    taps = df.lowpass_taps(DT, 60.0, 3)
    _, s, d = _random(30, 4, 9)
    scales = [np.full(4, 0.5), np.array([0.1, 0.2, 0.3, 0.4])]
    obj = df.RobustMisfit("cauchy", c=2.0, scale=scales, taps=taps)
    assert obj.engine_method == "misfit_robust" and hasattr(obj, "host") and hasattr(obj, "normal")
    ragged = df.RobustMisfit("huber", scale=[np.full(4, 0.5), np.full(3, 0.25), 2.0])  # shots of different trace counts
    assert np.array_equal(ragged.thresh_of(1, np.zeros((5, 3))), np.full(3, 1.345 * 0.25))
    assert np.array_equal(ragged.thresh_of(2, np.zeros((5, 3))), np.full(3, 1.345 * 2.0))
    shot = sh.Shot(np.array([[1, 1]], np.int32), np.zeros(30), np.array([[1, 2]] * 4, np.int32))
    shot.d_obs, shot.weights, shot.trace_weights = d, np.ones(d.shape), np.arange(4.0)
    e = _StandIn()
    assert obj.device(e, shot, 1) == 1.5
    assert e.args[0] is d and e.args[1] == "cauchy" and np.array_equal(e.args[2], 2.0 * scales[1])
    assert e.args[3] is shot.weights and e.args[4] is obj.taps and e.args[5] is shot.trace_weights
    assert e.kw == {"keep_irls": False}
    obj.device(e, shot, 0, keep_irls=True)
    assert e.kw == {"keep_irls": True} and np.array_equal(e.args[2], 2.0 * scales[0])
    J, r = obj.host(s, shot, 1)
    J2, r2 = obj(s, d, shot.weights, shot.trace_weights, thresh=2.0 * scales[1])
    assert J == J2 and np.array_equal(r, r2)
    assert np.array_equal(obj.irls(s, shot, 1), obj.psi)
    assert not isinstance(obj, df.WeightedL2)
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fwi.h")).read()
    for name in ("fwi_misfit_robust", "fwi_residual_weight_robust", "fwi_residual_median"):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and name + "(" in header
    assert _lib.ROBUST_KINDS == {k: i for i, k in enumerate(df.ROBUST_KINDS)}
    assert lib.fwi_abi_version() == _lib.ABI_VERSION == 14
    J = C.c_double(0.0)
    assert lib.fwi_misfit_robust(None, None, None, None, 0, 0, None, None, 0, None, None, C.byref(J)) == FWI_EINVAL
    assert lib.fwi_residual_weight_robust(None, None, 0) == FWI_EINVAL
    assert lib.fwi_residual_median(None, None, None, None, 0, 0, None, None) == FWI_EINVAL


def _problem(nshots=2, seed=5):
    rng = np.random.default_rng(seed)
    shape, h, order, nt = (24, 28), 10.0, 4, 60
    c_true = 2000.0 + 200.0 * rng.random(shape)
    c0 = np.full(shape, 2100.0)
    dt = 0.6 * fo.cfl_dt(c_true.max(), h, 2, order)
    wav = fo.ricker(nt, dt, 30.0)
    rec = np.array([[10, x] for x in range(4, 24, 3)], np.int32)
    shots = [sh.Shot(np.array([[12, 8 + 6 * k]], np.int32), wav, rec) for k in range(nshots)]
    return rng, shape, h, order, nt, dt, c_true, c0, shots


def test_shot_loop_and_residual_scales_run_the_twin_on_an_engine_without_the_device_calls():
    rng, shape, h, order, nt, dt, c_true, c0, shots = _problem()
    e = OracleEngine(shape, h, dt, nt, order=order, npml=4)
    sh.model_data(e, c_true, shots)
    assert not hasattr(e, "misfit_robust") and not hasattr(e, "residual_median")
    shots[1].weights = 0.5 + 0.5 * rng.random(shots[1].d_obs.shape)
    shots[1].trace_weights = rng.random(shots[1].d_obs.shape[1])
    taps = df.lowpass_taps(dt, 60.0, 5)
    probe = df.RobustMisfit("huber", taps=taps)
    scales = sh.residual_scales(e, c0, shots, probe)
    gathers = sh.residual_scales(e, None, shots, probe, per_trace=False)
    e.set_model(c0)
    for i, s in enumerate(shots):
        ei = probe.residuals(s.forward(e, save=False), s.d_obs, s.weights)[0]
        assert np.array_equal(scales[i], df.mad_scale(ei, s.weights)) and np.all(scales[i] > 0.0)
        assert gathers[i] == df.mad_scale(ei, s.weights, per_trace=False) and isinstance(gathers[i], float)
    obj = df.RobustMisfit("huber", scale=scales, taps=taps)
    J, g = sh.misfit_and_gradient(e, c0, shots, objective=obj)
    e.set_model(c0)
    e.reset_gradient()
    Jh = 0.0
    for i, s in enumerate(shots):
        j, r = obj(s.forward(e, save=True), s.d_obs, s.weights, s.trace_weights, shot=i)
        assert 0 < np.sum(obj.nout) < r.size
        s.adjoint(e, r)
        Jh += j
    assert J > 0.0 and J == Jh and np.any(g != 0.0) and np.array_equal(g, e.gradient())


@pytest.mark.parametrize("kind", KINDS)
def test_gauss_newton_product_is_symmetric_positive_semidefinite_on_the_oracle(kind):
    """gauss_newton_hvp(objective=RobustMisfit) on the CPU oracle with Born modelling (tests/_born.py's engine over
    the oracle: tests/_oracle_engine.py's has no born): <H v, w> = <v, H w> and v^T H v >= 0, cauchy included"""
    rng, shape, h, order, nt, dt, c_true, c0, shots = _problem()
    e = BornOracleEngine(shape, h, dt, nt, order=order, npml=4)
    sh.model_data(e, c_true, shots)
    shots[1].weights = 0.5 + 0.5 * rng.random(shots[1].d_obs.shape)
    shots[1].trace_weights = 0.25 + rng.random(shots[1].d_obs.shape[1])
    taps = df.lowpass_taps(dt, 60.0, 5)
    obj = df.RobustMisfit(kind, scale=sh.residual_scales(e, c0, shots, df.RobustMisfit(taps=taps)), taps=taps)
    v, w = (30.0 * rng.standard_normal(shape) for _ in range(2))
    Hv = sh.gauss_newton_hvp(e, c0, shots, v, objective=obj)
    Hw = sh.gauss_newton_hvp(e, None, shots, w, objective=obj)
    a, b, q = float(np.vdot(w, Hv)), float(np.vdot(v, Hw)), float(np.vdot(v, Hv))
    print(kind, "<w, H v> - <v, H w> relative", abs(a - b) / abs(a), "v^T H v", q)
    assert abs(a - b) <= 1e-10 * abs(a) and q > 0.0
    plain = sh.gauss_newton_hvp(e, c0, shots, v)
    assert np.linalg.norm(Hv - plain) > 0.05 * np.linalg.norm(plain)  # the weight is not a no-op
    shots[0].d_obs = None
    with pytest.raises(ValueError, match="no observed data"):
        sh.gauss_newton_hvp(e, c0, shots, v, objective=obj)
    with pytest.raises(ValueError, match="WeightedL2"):
        sh.gauss_newton_hvp(e, c0, shots, v, objective=df.NormalizedCorrelation())


def _cos(a, b):
    return float(np.vdot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)))


def test_outliers_turn_the_least_squares_gradient_further_than_any_robust_one():
    """2 % of the observed samples replaced by spikes of 50 times the largest amplitude; the scale is mad_scale of the
    contaminated residuals at the starting model, per trace (shots.residual_scales), with each kind's default c.  Only
    the ordering is asserted: cos(contaminated, clean) under each robust kind > the same under least squares.  Measured
    (printed): see README.md and DESIGN.md."""
    rng, shape, h, order, nt, dt, c_true, c0, shots = _problem(nshots=3)
    e = OracleEngine(shape, h, dt, nt, order=order, npml=4)
    sh.model_data(e, c_true, shots)
    clean = [s.d_obs.copy() for s in shots]
    dirty = []
    for d in clean:
        x = d.copy()
        hit = rng.random(d.shape) < 0.02
        x[hit] = 50.0 * np.max(np.abs(d)) * rng.choice([-1.0, 1.0], int(hit.sum()))
        dirty.append(x)

    def gradient(objective, data):
        for s, d in zip(shots, data):
            s.d_obs = d
        return sh.misfit_and_gradient(e, c0, shots, objective=objective)[1]

    cos = {"l2": _cos(gradient(df.WeightedL2(), dirty), gradient(df.WeightedL2(), clean))}
    for s, d in zip(shots, dirty):
        s.d_obs = d
    scales = sh.residual_scales(e, c0, shots, df.RobustMisfit())
    g_l2_clean = gradient(df.WeightedL2(), clean)
    against_l2 = {}
    for kind in KINDS:
        obj = df.RobustMisfit(kind, scale=scales)
        g_dirty = gradient(obj, dirty)
        cos[kind] = _cos(g_dirty, gradient(obj, clean))
        against_l2[kind] = _cos(g_dirty, g_l2_clean)
    print("cosine of the contaminated with the clean gradient:", {k: round(v, 4) for k, v in cos.items()},
          "; of the contaminated robust with the clean least-squares gradient:",
          {k: round(v, 4) for k, v in against_l2.items()})
    for kind in KINDS:
        assert cos[kind] > cos["l2"]


def test_run_config_knows_the_robust_flags_and_refuses_bad_combinations():
    """tools/run_config.py --robust KIND [--robust-c C] [--robust-scale S]: checked before any engine exists"""
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "run_config.py")
    out = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and all(f in out.stdout for f in ("--robust", "--robust-c", "--robust-scale"))
    for bad, word in ((["--robust", "huber", "--traveltime", "8"], "--robust"),
                      (["--robust", "huber", "--correlation"], "--robust"),
                      (["--robust", "hybrid", "--transport", "softplus"], "--robust"),
                      (["--robust", "cauchy", "--envelope", "--hilbert-fmin", "5"], "--robust"),
                      (["--robust", "huber", "--match-source", "4"], "--robust"),
                      (["--robust", "huber", "--adaptive", "8"], "--robust"),
                      (["--robust", "huber", "--spectral", "l2", "--spectral-band", "5,10"], "--robust"),
                      (["--robust", "l1"], "--robust"),
                      (["--robust-c", "1.5"], "--robust-c"),
                      (["--robust-scale", "gather"], "--robust-scale"),
                      (["--robust", "huber", "--robust-c", "0"], "--robust-c"),
                      (["--robust", "huber", "--robust-c", "nan"], "--robust-c"),
                      (["--robust", "huber", "--robust-scale", "shot"], "--robust-scale"),
                      (["--robust", "huber", "--robust-scale", "-1"], "--robust-scale"),
                      (["--robust", "huber", "--bands", "5,10", "--iters", "0"], "--bands")):
        out = subprocess.run([sys.executable, tool] + bad, capture_output=True, text=True)
        assert out.returncode == 2 and word in out.stderr, (bad, out.stderr[-300:])
