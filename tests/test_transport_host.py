"""The trace-by-trace optimal-transport (W2) misfit without a GPU (full_waveform_inversion_amd/datafit.py TransportW2,
include/fwi.h fwi_misfit_transport): the NumPy twin's dual value against its primal formula and against
the optimum of the transport linear programme, the exact zero at d_obs == d_syn, a density moved by whole samples, central
differences, the property the misfit exists for (it keeps growing where least squares turns round), the traces that do
not count, the twin through the shot loop on the CPU oracle engine, the binding and the new flags of tools/run_config.py.

The roundoff of W and J between two fp64 evaluations that add in different orders: roundoff_bounds of
tests/_transport.py, derived there and shared with tests/test_gpu_transport.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from _oracle_engine import OracleEngine  # noqa: E402
from _transport import U2, level_gap, roundoff_bounds  # noqa: E402
from full_waveform_inversion_amd import _lib, datafit as df, shots as sh  # noqa: E402
from oracle import fwi_oracle as fo  # noqa: E402

FWI_EINVAL = 1
DT = 1e-3
TRANSFORMS = [("softplus", 2.0), ("linear", 8.0)]  # (transform, param) for traces of unit variance
SCAN = (0, 5, 10, 20, 30, 40, 60)


def ricker(shift=0.0, nt=400, t0=0.12, f0=25.0):
    """the wavelet delayed by `shift` samples, exactly (evaluated, not interpolated)"""
    a = (np.pi * f0 * (np.arange(nt) * DT - t0 - shift * DT)) ** 2
    return (1.0 - 2.0 * a) * np.exp(-a)


def _random(nt, ntr, seed):
    rng = np.random.default_rng(seed)
    return rng, rng.standard_normal((nt, ntr)), rng.standard_normal((nt, ntr))


@pytest.mark.parametrize("transform,param", TRANSFORMS)
def test_dual_value_equals_the_primal_formula(transform, param):
    """W by the potentials against W by the quantile functions over the merged breakpoints, random traces.  The primal
    formula adds at most 2 nt - 1 widths, each the difference of two levels that carry (nt + 8) 2^-53 each
    (tests/_transport.py), times a squared distance of at most (nt - 1)^2 samples; the dual side has its own bound"""
    nt, ntr = 50, 40
    _, s, d = _random(nt, ntr, 1)
    obj = df.TransportW2(DT, transform, param)
    J, _ = obj(s, d)
    F, G = obj.cdfs(s, d)[:2]
    Wp = obj.primal(F, G)
    tol = roundoff_bounds(obj, s, d)[0] + DT * DT * (2 * nt - 1) * (nt + 8) * U2 * (nt - 1) ** 2
    print("max |dual - primal| / tol", float(np.max(np.abs(obj.distances - Wp) / tol)), "W", obj.distances[:4] / DT ** 2)
    assert obj.counts.all() and np.all(obj.distances > 0.0) and np.all(np.abs(obj.distances - Wp) <= tol)
    assert J == float(np.sum(0.5 * obj.distances))


@pytest.mark.parametrize("nt", [2, 3, 9, 16])
def test_dual_value_equals_the_optimum_of_the_transport_lp(nt):
    """min sum_nm T_nm (n - m)^2 dt^2 over T >= 0 with the marginals f and g.  The solver stops at a relative optimality
    and feasibility tolerance of 1e-7 at worst (HiGHS's default); a vertex it returns is exact to roundoff, so what is
    asserted is 1e-9 relative, and the figure is printed"""
    opt = pytest.importorskip("scipy.optimize")
    for transform, param in TRANSFORMS:
        _, s, d = _random(nt, 6, 2 + nt)
        obj = df.TransportW2(DT, transform, param)
        obj(s, d)
        f, g = obj.cdfs(s, d)[2:4]
        cost = ((np.arange(nt)[:, None] - np.arange(nt)[None, :]) ** 2).astype(np.float64).ravel() * DT * DT
        A = np.zeros((2 * nt, nt * nt))
        for n in range(nt):
            A[n, n * nt:(n + 1) * nt] = 1.0  # sum_m T_nm = f_n
            A[nt + n, n::nt] = 1.0           # sum_n T_nm = g_m
        for j in range(f.shape[1]):
            res = opt.linprog(cost, A_eq=A, b_eq=np.concatenate([f[:, j], g[:, j]]), bounds=(0, None), method="highs")
            assert res.status == 0, res.message
            print(transform, "nt", nt, "W", obj.distances[j], "lp", res.fun, "rel", abs(obj.distances[j] - res.fun) / res.fun)
            assert abs(obj.distances[j] - res.fun) <= 1e-9 * res.fun


@pytest.mark.parametrize("weighted", [False, True], ids=["no_weights", "weights"])
@pytest.mark.parametrize("with_taps", [False, True], ids=["no_taps", "taps"])
@pytest.mark.parametrize("transform,param", TRANSFORMS)
def test_equal_data_give_exactly_zero(transform, param, with_taps, weighted):
    """d_obs == d_syn: every level of F ties with a level of G, the two-sided count gives phi = psi = 0, J = 0, r = 0"""
    rng, s, _ = _random(64, 7, 3)
    taps = df.bandpass_taps(DT, 5.0, 60.0, 16) if with_taps else None
    M = 0.5 + 0.5 * rng.random(s.shape) if weighted else None
    w = 0.25 + rng.random(7) if weighted else None
    obj = df.TransportW2(DT, transform, param, taps)
    J, r = obj(s, s.copy(), M, w)
    F, G = obj.cdfs(s, s, M)[:2]
    phi, psi = obj.potentials(F, G)
    assert obj.counts.all() and not phi.any() and not psi.any()
    assert J == 0.0 and not np.any(r) and not np.any(obj.distances)


@pytest.mark.parametrize("k", [1, 7, 30])
def test_a_density_moved_by_k_samples_is_k_dt_squared_away(k):
    """at the level of f and g: g_n = f_{n-k} with both supports inside the record (zero-mass atoms outside: ties), so
    that the optimal plan moves every atom by k samples and W = (k dt)^2.  Every level of G equals a level of F bit for
    bit (leading zeros add nothing to a running sum): this is the tie rule at work.  Tolerance: the bound of
    tests/_transport.py evaluated on these f, g, phi, psi"""
    nt = 96
    rng = np.random.default_rng(4)
    p = np.zeros((nt, 3))
    p[10:50] = rng.random((40, 3)) + 0.1
    q = np.roll(p, k, axis=0)
    S = np.sum(p, axis=0)
    F, G = np.cumsum(p, axis=0) / S, np.cumsum(q, axis=0) / np.sum(q, axis=0)
    assert np.array_equal(G[k:], F[:nt - k])
    obj = df.TransportW2(DT, "linear", 1.0)
    phi, psi = (x.astype(np.float64) for x in obj.potentials(F, G))
    f, g = p / S, q / np.sum(q, axis=0)
    W = DT * DT * (np.sum(phi * f, axis=0) + np.sum(psi * g, axis=0))
    rng_ = (phi.max(axis=0) - phi.min(axis=0)) + (psi.max(axis=0) - psi.min(axis=0))
    mag = np.sum(np.abs(phi) * f, axis=0) + np.sum(np.abs(psi) * g, axis=0)
    tol = DT * DT * ((nt + 8) * U2 * rng_ + (2 * nt + 4) * U2 * mag)
    print("k", k, "W / dt^2", W / DT ** 2, "tol / dt^2", tol / DT ** 2)
    assert np.all(np.abs(W - (k * DT) ** 2) <= tol)
    assert np.all(np.abs(obj.primal(F, G) - (k * DT) ** 2) <= tol + DT * DT * (2 * nt - 1) * (nt + 8) * U2 * k * k)


@pytest.mark.parametrize("transform,param", TRANSFORMS)
def test_twin_gradient_matches_central_differences(transform, param):
    """<r, v> against D(t) = (J(s + t v) - J(s - t v)) / (2 t) with M, B and w.  Where the four index arrays do not
    change J is smooth, D(t) = J' + t^2 J''' / 6 + O(t^4), so D(2 t) - D(t) = t^2 J''' / 2 is three times the truncation
    term of D(t): the tolerance is twice that term (the factor for the next order) plus the roundoff of the quotient,
    two evaluations of J at roundoff_bounds each over 2 t.  All four index arrays are equal at s, s +- t v and
    s +- 2 t v: asserted, no case skipped"""
    nt, ntr = 50, 5
    rng, s, d = _random(nt, ntr, 5)
    taps = df.bandpass_taps(DT, 5.0, 200.0, 8)
    M = 0.5 + 0.5 * rng.random(s.shape)
    w = 0.25 + rng.random(ntr)
    obj = df.TransportW2(DT, transform, param, taps)
    J, r = obj(s, d, M, w)
    v = rng.standard_normal(s.shape)
    t = 1e-6

    def at(x):
        F, G = obj.cdfs(x, d, M)[:2]
        return obj.indices(F, G), obj(x, d, M, w)[0]

    idx, _ = at(s)
    vals = {}
    for c in (-2.0, -1.0, 1.0, 2.0):
        i, vals[c] = at(s + c * t * v)
        assert all(np.array_equal(a, b) for a, b in zip(i, idx)), "a level of F crossed a level of G within the step"
    D1, D2 = (vals[1.0] - vals[-1.0]) / (2.0 * t), (vals[2.0] - vals[-2.0]) / (4.0 * t)
    an = float(np.sum(r * v))
    trunc = abs(D2 - D1) / 3.0
    Jb = roundoff_bounds(obj, s, d, M, w)[1]
    tol = 2.0 * trunc + 2.0 * (2.0 * Jb / (2.0 * t))  # (D2 - D1 carries the same roundoff: the second factor 2)
    print(transform, "J", J, "<r, v>", an, "D(t)", D1, "|diff|", abs(an - D1), "truncation", trunc, "roundoff", Jb / t)
    assert obj.counts.all() and J > 0.0 and abs(an) > 1e-3 * J and abs(an - D1) <= tol
    assert tol <= 1e-3 * abs(an)  # ... and the tolerance means something: a worst-case roundoff bound, far below <r, v>


def test_w2_grows_with_the_shift_where_least_squares_turns_round():
    """25 Hz Ricker, dt = 1 ms, nt = 400, the default softplus parameter b = 4 / max|d|: least squares falls between 20
    and 30 samples of shift (18.6 -> 11.8), W^2 rises through 60 samples, sample by sample; its values at the scanned
    shifts are DESIGN.md s.4m's to the digits given there.  The default linear offset c = 10 max|d| is monotone too"""
    d = ricker()[:, None]
    soft, lin = df.TransportW2(DT), df.TransportW2(DT, "linear")
    assert soft.param_of(d) == 4.0 / np.max(np.abs(d)) and lin.param_of(d) == 10.0 * np.max(np.abs(d))
    W, Wl, ls = [], [], []
    for k in range(61):
        s = ricker(k)[:, None]
        W.append(2.0 * soft(s, d)[0])
        Wl.append(2.0 * lin(s, d)[0])
        ls.append(0.5 * float(np.sum((s - d) ** 2)))
    print("shift", SCAN, "least squares", [round(ls[k], 2) for k in SCAN], "W2^2", ["%.2g" % W[k] for k in SCAN],
          "linear", ["%.2g" % Wl[k] for k in SCAN])
    assert ls[20] > ls[30] and ls[20] > ls[60]  # cycle skipped
    assert [round(ls[k], 1) for k in (20, 30)] == [18.6, 11.8]
    assert W[0] == 0.0 and np.all(np.diff(W) > 0.0) and np.all(np.diff(Wl) > 0.0)
    assert ["%.1e" % W[k] for k in SCAN[1:]] == ["3.8e-06", "1.2e-05", "3.5e-05", "6.3e-05", "9.1e-05", "1.4e-04"]


def test_a_trace_below_minus_c_does_not_count_and_adds_nothing():
    rng, s, d = _random(40, 6, 7)
    M = 0.5 + 0.5 * rng.random(s.shape)
    w = 0.25 + rng.random(6)
    c = 6.0
    obj = df.TransportW2(DT, "linear", c)
    J0, r0 = obj(s, d, M, w)
    W0 = obj.distances.copy()
    assert obj.counts.all()
    s2 = s.copy()
    s2[11, 2] = -2.0 * c / M[11, 2]  # M . s < -c at one sample
    J1, r1 = obj(s2, d, M, w)
    keep = np.arange(6) != 2
    assert list(obj.counts) == [True, True, False, True, True, True]
    assert obj.distances[2] == 0.0 and not np.any(r1[:, 2])
    assert np.array_equal(obj.distances[keep], W0[keep]) and np.array_equal(r1[:, keep], r0[:, keep])
    assert 0.0 < J1 < J0 and J1 == float(np.sum(0.5 * w * np.where(keep, W0, 0.0)))
    # the data side drops a trace as well; softplus only fails on non-finite samples
    d2 = d.copy()
    d2[3, 4] = -2.0 * c / M[3, 4]
    obj(s, d2, M, w)
    assert not obj.counts[4] and obj.counts[keep & (np.arange(6) != 4)].all()
    soft = df.TransportW2(DT, "softplus", 2.0)
    J2, r2 = soft(s2, d2, M, w)
    assert soft.counts.all() and np.isfinite(J2) and np.all(np.isfinite(r2))
    s2[0, 0] = np.nan
    J3, r3 = soft(s2, d2, M, w)
    assert not soft.counts[0] and soft.counts[1:].all() and np.isfinite(J3) and not np.any(r3[:, 0])
    assert np.all(np.isfinite(r3))


def test_edge_shapes_and_argument_errors():
    obj = df.TransportW2(DT, "softplus", 2.0)
    J, r = obj(np.ones((1, 3)), 2.0 * np.ones((1, 3)))  # nt = 1
    assert J == 0.0 and r.shape == (1, 3) and not np.any(r) and obj.counts.all()
    J, r = obj(np.zeros((5, 0)), np.zeros((5, 0)))  # no traces
    assert J == 0.0 and r.shape == (5, 0)
    for bad in (dict(dt=0.0), dict(transform="sigmoid"), dict(param=0.0), dict(param=-1.0), dict(param=np.inf),
                dict(sharpness=0.0), dict(factor=np.nan)):
        with pytest.raises(ValueError):
            df.TransportW2(**{"dt": DT, **bad})
    with pytest.raises(ValueError):
        obj(np.ones((4, 2)), np.ones((4, 3)))
    with pytest.raises(ValueError):
        obj(np.ones((4, 2)), np.ones((4, 2)), None, np.array([1.0, -1.0]))
    with pytest.raises(ValueError):
        df.TransportW2(DT).param_of(np.zeros((4, 2)))
    # dtype=: B s, B d and g are rounded to it
    _, a, b = _random(40, 3, 8)
    r32 = df.TransportW2(DT, "softplus", 2.0, dtype="float32")(a.astype("f4"), b.astype("f4"))[1]
    assert np.any(r32) and np.array_equal(r32, r32.astype("f4").astype("f8"))
    o32 = df.TransportW2(DT, "softplus", 2.0, df.lowpass_taps(DT, 80.0, 2), dtype="float32")
    f = o32.filter(a)
    assert np.array_equal(f, f.astype("f4").astype("f8")) and not np.array_equal(f, df.fir_time(a, o32.taps))


def _setup_2d(nt=60):
    rng = np.random.default_rng(5)
    shape, h, order = (24, 28), 10.0, 4
    c_true = 2000.0 + 200.0 * rng.random(shape)
    c0 = np.full(shape, 2100.0)
    dt = 0.6 * fo.cfl_dt(c_true.max(), h, 2, order)
    wav = fo.ricker(nt, dt, 30.0)
    rec = np.array([[10, x] for x in range(4, 24, 3)], np.int32)
    shots = [sh.Shot(np.array([[12, 8]], np.int32), wav, rec), sh.Shot(np.array([[14, 20]], np.int32), wav, rec)]
    e = OracleEngine(shape, h, dt, nt, order=order, npml=4)
    sh.model_data(e, c_true, shots)
    return rng, e, c0, shots, dt


@pytest.mark.parametrize("transform", ["softplus", "linear"])
def test_shot_loop_runs_the_twin_on_an_engine_without_misfit_transport(transform):
    rng, e, c0, shots, dt = _setup_2d()
    assert not hasattr(e, "misfit_transport")
    shots[1].weights = 0.5 + 0.5 * rng.random(shots[1].d_obs.shape)
    shots[1].trace_weights = rng.random(shots[1].d_obs.shape[1])
    obj = df.TransportW2(dt, transform, None, df.lowpass_taps(dt, 60.0, 5))
    J, g = sh.misfit_and_gradient(e, c0, shots, objective=obj)
    # the same by hand: the twin per shot with the shot's own parameter, its r through adjoint()
    e.set_model(c0)
    e.reset_gradient()
    Jh = 0.0
    for s in shots:
        d = s.forward(e, save=True)
        ref = df.TransportW2(dt, transform, obj.param_of(s.d_obs), obj.taps)
        j, r = ref(d, s.d_obs, s.weights, s.trace_weights)
        assert ref.counts.all()
        s.adjoint(e, r)
        Jh += j
    assert J > 0.0 and J == Jh and np.any(g != 0.0) and np.array_equal(g, e.gradient())
    with pytest.raises(ValueError, match="WeightedL2"):
        sh.gauss_newton_hvp(e, c0, shots, np.ones(c0.shape), objective=obj)


def test_binding_is_declared_and_refuses_a_null_context():
    lib = _lib.load()
    assert "fwi_misfit_transport" in _lib.SIGNATURES and _lib.OT_TRANSFORMS == df.OT_TRANSFORMS
    assert lib.fwi_abi_version() == _lib.ABI_VERSION == 14
    J = C.c_double(0.0)
    assert lib.fwi_misfit_transport(None, None, None, None, 0, None, 1, 1.0, C.byref(J), None, None) == FWI_EINVAL


def test_run_config_knows_the_transport_flags_and_refuses_bad_combinations():
    """tools/run_config.py --transport {softplus,linear} [--transport-param X]: checked before any engine exists"""
    import subprocess
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "run_config.py")
    out = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--transport" in out.stdout and "--transport-param" in out.stdout
    for bad, word in ((["--transport", "softplus", "--traveltime", "8"], "--transport"),
                      (["--transport", "softplus", "--correlation"], "--transport"),
                      (["--transport", "linear", "--envelope", "--hilbert-fmin", "5"], "--transport"),
                      (["--transport", "linear", "--match-source", "4"], "--transport"),
                      (["--transport", "sigmoid"], "--transport"),
                      (["--transport-param", "2.0"], "--transport-param"),
                      (["--transport", "softplus", "--transport-param", "0"], "--transport-param"),
                      (["--transport", "softplus", "--transport-param", "-1"], "--transport-param"),
                      (["--transport", "softplus", "--transport-param", "nan"], "--transport-param"),
                      (["--transport", "softplus", "--bands", "5,10", "--iters", "0"], "--bands")):
        out = subprocess.run([sys.executable, tool] + bad, capture_output=True, text=True)
        assert out.returncode == 2 and word in out.stderr, (bad, out.stderr[-300:])
