"""The trace-normalised correlation misfit without a GPU (full_waveform_inversion_amd/datafit.py NormalizedCorrelation,
include/fwi.h fwi_misfit_correlation): the NumPy twin against central differences, against the
reference's CC measure (objectives.correlation), its invariance under a gain, the traces that do not count, the property
the misfit exists for (a gain per trace is no misfit), the twin through the shot loop on the CPU oracle engine, the
binding and the new flag of tools/run_config.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from _oracle_engine import OracleEngine  # noqa: E402
from full_waveform_inversion_amd import _lib, datafit as df, objectives, shots as sh  # noqa: E402
from oracle import fwi_oracle as fo  # noqa: E402

FWI_EINVAL = 1
NT, NTR = 40, 5


def _gathers(seed=3):
    rng = np.random.default_rng(seed)
    s, d = rng.standard_normal((NT, NTR)), rng.standard_normal((NT, NTR))
    M = rng.random((NT, NTR))
    w = 0.25 + rng.random(NTR)
    w[1] = 0.0
    return rng, s, d, M, w


def test_correlation_floor_by_hand():
    d = np.array([[3.0, 0.0], [4.0, -2.0]])
    assert df.correlation_floor(d) == 0.05 and df.correlation_floor(d, 50.0) == 2.5 and df.correlation_floor(d, 0.0) == 0.0
    assert df.correlation_floor(np.zeros((0, 3))) == 0.0
    for bad in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            df.correlation_floor(d, bad)
    with pytest.raises(ValueError):
        df.correlation_floor(np.ones(4))


@pytest.mark.parametrize("trace_weighted", [False, True], ids=["no_tw", "tw"])
@pytest.mark.parametrize("weighted", [False, True], ids=["no_weights", "weights"])
@pytest.mark.parametrize("with_taps", [False, True], ids=["no_taps", "taps"])
@pytest.mark.parametrize("floor", [False, True], ids=["eps0", "floor"])
def test_twin_gradient_matches_central_differences(floor, with_taps, weighted, trace_weighted):
    """<r, v> against (J(s + t v) - J(s - t v)) / (2 t), t = 1e-6.  The bound is the roundoff of the difference: each J
    is an (nt + ntr)-term fp64 sum of terms of size <= 2 w_j, so it carries at most (nt + ntr + 10) 2^-53 * 2 sum w
    ~ 7e-14, the difference of two twice that, divided by 2 t = 2e-6: 7e-8 absolute on a derivative of order 1 (printed),
    hence 1e-6 relative with a margin for a small |fd|; the truncation error t^2 J''' / 6 ~ 1e-12 is far below.  Measured
    with these inputs: 6e-11 .. 6e-9."""
    rng, s, d, M, w = _gathers()
    taps = df.bandpass_taps(2e-3, 8.0, 90.0, 7) if with_taps else None
    eps = df.correlation_floor(d) if floor else 0.0
    obj = df.NormalizedCorrelation(eps, taps)
    M, w = (M if weighted else None), (w if trace_weighted else None)
    J, r = obj(s, d, M, w)
    v = rng.standard_normal(s.shape)
    t = 1e-6
    fd = (obj(s + t * v, d, M, w)[0] - obj(s - t * v, d, M, w)[0]) / (2.0 * t)
    err = abs(float(np.sum(r * v)) - fd) / abs(fd)
    print("eps", eps, "taps", with_taps, "J", J, "<r, v>", float(np.sum(r * v)), "fd", fd, "rel", err)
    assert J > 0.0 and abs(fd) > 1e-2 and err <= 1e-6


def test_twin_is_the_reference_cc_measure_on_mean_free_traces():
    """eps = 0, no weights, no taps, mean-free traces: J / ntr and r / ntr are objectives.correlation(per_trace=True), to
    the roundoff of two fp64 evaluation orders (a few 2^-53 of values of order 1; measured 0 and 3.5e-18)"""
    _, s, d, _, _ = _gathers()
    s, d = s - s.mean(0), d - d.mean(0)
    obj = df.NormalizedCorrelation(0.0)
    J, r = obj(s, d)
    Jr, rr = objectives.correlation(s, d, per_trace=True)
    print("J / ntr - J_ref", J / NTR - Jr, "max |r / ntr - r_ref|", float(np.max(np.abs(r / NTR - rr))))
    assert abs(J / NTR - Jr) <= 8 * 2.0 ** -53 and np.max(np.abs(r / NTR - rr)) <= 8 * 2.0 ** -53
    assert obj.correlations.shape == (NTR,) and abs(float(np.sum(1.0 - obj.correlations)) - J) <= 8 * 2.0 ** -53


def test_a_gain_changes_nothing_at_eps_zero_and_equal_gathers_have_no_misfit():
    _, s, d, M, w = _gathers()
    obj = df.NormalizedCorrelation(0.0, df.lowpass_taps(2e-3, 80.0, 5))
    J, r = obj(s, d, M, w)
    for k in (3.0, 0.125, 1e3):
        Jk, rk = obj(k * s, d, M, w)
        assert abs(Jk - J) <= 16 * 2.0 ** -53 * NTR  # rho_j is a ratio of sums that scale alike: roundoff only
        assert np.linalg.norm(k * rk - r) <= 1e-13 * np.linalg.norm(r)  # ... and r is homogeneous of degree -1
    J0, r0 = obj(d, d, M, w)
    assert abs(J0) <= 4 * 2.0 ** -53 * NTR and np.linalg.norm(r0) <= 1e-14 * np.linalg.norm(r)


def test_traces_that_do_not_count():
    """a trace killed by its weights and a trace whose data are zero: J_j = 0, rho_j = 0 and a zero column of the adjoint
    source, with and without a floor; with eps = 0 a zero SYNTHETIC trace does not count either"""
    _, s, d, M, w = _gathers()
    M = M.copy()
    M[:, 2] = 0.0
    d = d.copy()
    d[:, 3] = 0.0
    for eps in (0.0, 0.3):
        obj = df.NormalizedCorrelation(eps)
        J, r = obj(s, d, M)
        rho = obj.correlations
        assert rho[2] == 0.0 and rho[3] == 0.0 and not np.any(r[:, 2]) and not np.any(r[:, 3])
        live = [0, 1, 4]
        assert J == float(np.sum(1.0 - rho[live])) and all(np.any(r[:, j]) for j in live)
    s0 = s.copy()
    s0[:, 0] = 0.0
    obj = df.NormalizedCorrelation(0.0)
    J, r = obj(s0, d)
    assert obj.correlations[0] == 0.0 and not np.any(r[:, 0]) and np.isfinite(J) and np.all(np.isfinite(r))
    obj = df.NormalizedCorrelation(0.3)  # with a floor the zero synthetic trace counts: rho = 0, J_j = 1, r = -d / (eps nd)
    J, r = obj(s0, d)
    assert obj.correlations[0] == 0.0 and np.any(r[:, 0]) and np.all(np.isfinite(r))
    # a trace weight of zero: the trace keeps its rho but adds nothing to J or to r
    obj = df.NormalizedCorrelation(0.0)
    J, r = obj(s, d, None, np.array([1.0, 0.0, 1.0, 1.0, 1.0]))
    assert obj.correlations[1] != 0.0 and not np.any(r[:, 1])
    assert J == float(np.sum(1.0 - obj.correlations[[0, 2, 4]]))


def test_twin_checks_its_arguments_and_is_no_weighted_l2():
    for bad in (dict(eps=-1.0), dict(eps=np.nan), dict(eps=np.inf), dict(floor_percent=-1.0), dict(taps=np.ones((2, 2))),
                dict(taps=[1.0, np.inf])):
        with pytest.raises(ValueError):
            df.NormalizedCorrelation(**bad)
    obj = df.NormalizedCorrelation()
    assert not isinstance(obj, df.WeightedL2) and obj.correlations is None
    assert obj.eps_of(np.full((4, 2), -5.0)) == 0.1 and df.NormalizedCorrelation(0.25).eps_of(np.ones((3, 2))) == 0.25
    assert df.NormalizedCorrelation(floor_percent=10.0).eps_of(np.full((4, 2), -5.0)) == 1.0
    s = np.ones((6, 2))
    with pytest.raises(ValueError):
        obj(s, np.ones((6, 3)))
    with pytest.raises(ValueError):
        obj(s, s, -s)
    for bad_tw in (np.ones(3), [1.0, -1.0], [1.0, np.nan]):
        with pytest.raises(ValueError):
            obj(s, s, None, bad_tw)
    # dtype=: B s, B d and g are rounded to it
    rng = np.random.default_rng(0)
    a, b = rng.standard_normal((6, 2)), rng.standard_normal((6, 2))
    r32 = df.NormalizedCorrelation(0.1, dtype="float32")(a.astype("f4"), b.astype("f4"))[1]
    assert np.array_equal(r32, r32.astype("f4").astype("f8"))
    o32 = df.NormalizedCorrelation(0.1, df.lowpass_taps(2e-3, 80.0, 2), dtype="float32")
    f = o32.filter(a)
    assert np.array_equal(f, f.astype("f4").astype("f8")) and not np.array_equal(f, df.fir_time(a, o32.taps))


def test_a_gain_per_trace_is_a_large_least_squares_misfit_and_no_correlation_misfit():
    """d_obs = gain_j * s with gains in [0.2, 5]: what an acoustic engine cannot model.  WeightedL2 sees a large J and a
    non-zero residual; the correlation sees J <= 1e-12 ntr and |r| <= 1e-10 |r_L2| (the issue's bounds)."""
    rng = np.random.default_rng(7)
    nt, ntr = 200, 12
    t = np.arange(nt)[:, None] * 2e-3
    s = np.sin(2.0 * np.pi * 12.0 * t + rng.random(ntr) * 6.0) * np.exp(-((t - 0.2) / 0.08) ** 2)
    gain = 0.2 * 25.0 ** rng.random(ntr)
    assert gain.min() >= 0.2 and gain.max() <= 5.0
    d = gain * s
    M = df.offset_time_mute(sh.Shot(np.array([[0, 0]]), np.zeros(nt), np.array([[0, 3 * j] for j in range(ntr)])),
                            10.0, 2e-3, 3000.0, 0.0, 5)
    for taps in (None, df.bandpass_taps(2e-3, 4.0, 40.0, 16)):
        J2, r2 = df.WeightedL2(taps)(s, d, M)
        J, r = df.NormalizedCorrelation(0.0, taps)(s, d, M)
        print("taps", taps is not None, "J_L2", J2, "J", J, "|r| / |r_L2|", np.linalg.norm(r) / np.linalg.norm(r2))
        assert J2 > 1.0 and np.linalg.norm(r2) > 1.0
        assert abs(J) <= 1e-12 * ntr and np.linalg.norm(r) <= 1e-10 * np.linalg.norm(r2)


def _setup_2d(nt=40):
    rng = np.random.default_rng(5)
    shape, h, order = (24, 28), 10.0, 4
    c_true = 2000.0 + 200.0 * rng.random(shape)
    c0 = np.full(shape, 2100.0)
    dt = 0.6 * fo.cfl_dt(c_true.max(), h, 2, order)
    wav = fo.ricker(nt, dt, 30.0)
    rec = np.array([[3, x] for x in range(2, 26, 3)], np.int32)
    shots = [sh.Shot(np.array([[12, 8]], np.int32), wav, rec), sh.Shot(np.array([[14, 20]], np.int32), wav, rec)]
    e = OracleEngine(shape, h, dt, nt, order=order, npml=4)
    sh.model_data(e, c_true, shots)
    return rng, e, c0, shots, dt


def test_shot_loop_runs_the_twin_on_an_engine_without_misfit_correlation():
    rng, e, c0, shots, dt = _setup_2d()
    assert not hasattr(e, "misfit_correlation") and shots[0].trace_weights is None
    shots[1].weights = rng.random(shots[1].d_obs.shape)
    shots[1].trace_weights = rng.random(shots[1].d_obs.shape[1])
    obj = df.NormalizedCorrelation(None, df.lowpass_taps(dt, 60.0, 5))
    J, g = sh.misfit_and_gradient(e, c0, shots, objective=obj)
    # the same by hand: the twin per shot with the shot's own floor, its r through adjoint()
    e.set_model(c0)
    e.reset_gradient()
    Jh = 0.0
    for s in shots:
        d = s.forward(e, save=True)
        ref = df.NormalizedCorrelation(df.correlation_floor(s.d_obs), obj.taps)
        j, r = ref(d, s.d_obs, s.weights, s.trace_weights)
        s.adjoint(e, r)
        Jh += j
    assert J > 0.0 and J == Jh and np.any(g != 0.0) and np.array_equal(g, e.gradient())
    with pytest.raises(ValueError, match="WeightedL2"):
        sh.gauss_newton_hvp(e, c0, shots, np.ones(c0.shape), objective=obj)


def test_binding_is_declared_and_refuses_a_null_context():
    lib = _lib.load()
    assert "fwi_misfit_correlation" in _lib.SIGNATURES
    assert lib.fwi_abi_version() == _lib.ABI_VERSION == 14
    J = C.c_double(0.0)
    assert lib.fwi_misfit_correlation(None, None, None, None, 0, None, 1.0, C.byref(J), None) == FWI_EINVAL


def test_run_config_knows_the_correlation_flag_and_refuses_bad_combinations():
    """tools/run_config.py --correlation [FLOOR_PERCENT]: checked before any engine exists"""
    import subprocess
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "run_config.py")
    out = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--correlation" in out.stdout and "FLOOR_PERCENT" in out.stdout
    for bad, word in ((["--correlation", "--envelope", "--hilbert-fmin", "5"], "--correlation"),
                      (["--correlation", "2", "--match-source", "4"], "--correlation"),
                      (["--correlation", "-1"], "FLOOR_PERCENT"),
                      (["--correlation", "nan"], "FLOOR_PERCENT"),
                      (["--correlation", "--bands", "5,10", "--iters", "0"], "--bands")):
        out = subprocess.run([sys.executable, tool] + bad, capture_output=True, text=True)
        assert out.returncode == 2 and word in out.stderr, (bad, out.stderr[-300:])
