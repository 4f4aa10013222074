"""The matching-filter (source-independent) misfit without a GPU (full_waveform_inversion_amd/datafit.py MatchedL2,
include/fwi.h fwi_match_solve): the NumPy twin against finite differences and against WeightedL2, the
recovery of a known filter, the host Cholesky solve of the C-ABI against numpy.linalg, the two helpers on hand-computed
cases and the twin through the shot loop on the CPU oracle engine."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from _oracle_engine import OracleEngine  # noqa: E402
from full_waveform_inversion_amd import _lib, datafit as df, shots as sh  # noqa: E402
from oracle import fwi_oracle as fo  # noqa: E402

NT, NTR = 40, 5
FWI_EINVAL = 1


def _gathers(seed=0, nt=NT, ntr=NTR):
    rng = np.random.default_rng(seed)
    s, d = rng.standard_normal((nt, ntr)), rng.standard_normal((nt, ntr))
    M = rng.random((nt, ntr))
    M[nt // 3] = 0.0     # a dead row
    M[:, ntr // 2] = 0.0  # a dead trace
    return rng, s, d, M


@pytest.mark.parametrize("with_taps", [False, True], ids=["no_taps", "taps"])
@pytest.mark.parametrize("L", [0, 1, 4, 8])
def test_twin_gradient_of_the_reduced_objective_matches_finite_differences(L, with_taps):
    """dJ/ds of the REDUCED objective (f* re-estimated at s +- eps ds) is r = B C_f*^T (M . e): the envelope theorem.
    Bound: the issue's 1e-6 relative at step 1e-6, mu = 1e-3 sum d^2 (measured there: 1e-8 or better)."""
    rng, s, d, M = _gathers(L)
    taps = df.bandpass_taps(2e-3, 8.0, 90.0, 7) if with_taps else None
    obj = df.MatchedL2(L, 1e-3 * float(np.sum(d * d)), taps)
    _, r = obj(s, d, M)
    ds = rng.standard_normal(s.shape)
    eps = 1e-6
    fd = (obj(s + eps * ds, d, M)[0] - obj(s - eps * ds, d, M)[0]) / (2 * eps)
    an = float(np.sum(r * ds))
    print("L", L, "fd", fd, "analytic", an, "rel", abs(fd - an) / abs(an))
    assert abs(fd - an) <= 1e-6 * abs(an)


def test_twin_recovers_a_causal_three_tap_filter():
    _, s, _, M = _gathers(3)
    g = np.array([0.8, -0.35, 0.15])
    f_true = np.concatenate([np.zeros(2), g])  # f_0, f_1, f_2 = g: d[n] = sum_k g_k s[n - k]
    d = df.matched_wavelet(s, f_true)
    obj = df.MatchedL2(2, 0.0)
    G, b = obj.normal(s, d, M)
    f = obj.solve(G, b)
    J, _ = obj.apply(s, d, f, M)
    print("f", f, "J", J, "sum d^2", float(np.sum(d * d)))
    assert np.max(np.abs(f - f_true)) <= 1e-10
    assert J <= 1e-20 * float(np.sum(d * d))


def test_twin_with_the_unit_filter_is_weighted_l2_bit_for_bit():
    _, s, d, M = _gathers(4)
    for weights in (None, M):
        J, r = df.MatchedL2(0, 0.0).apply(s, d, np.ones(1), weights)
        Jw, rw = df.WeightedL2()(s, d, weights)
        assert J == Jw and np.array_equal(r, rw)
    # with taps B s - B d is not B (s - d) bit for bit: round-off only
    taps = df.bandpass_taps(2e-3, 8.0, 90.0, 7)
    J, r = df.MatchedL2(0, 0.0, taps).apply(s, d, np.ones(1), M)
    Jw, rw = df.WeightedL2(taps)(s, d, M)
    assert abs(J - Jw) <= 1e-13 * Jw and np.max(np.abs(r - rw)) <= 1e-13 * np.max(np.abs(rw))


def test_twin_normal_equations_are_the_definition_written_out():
    """G and b entry by entry from the definition's triple sum, on a gather short enough for L > nt - 1"""
    rng, s, d, M = _gathers(5, nt=6, ntr=3)
    L = 7
    obj = df.MatchedL2(L, 1.0)
    G, b = obj.normal(s, d, M)
    K, nt = 2 * L + 1, 6
    Gd, bd = np.zeros((K, K)), np.zeros(K)
    at = lambda x, n, j: x[n, j] if 0 <= n < nt else 0.0  # noqa: E731
    for k in range(-L, L + 1):
        for n in range(nt):
            for j in range(3):
                bd[k + L] += M[n, j] ** 2 * at(s, n - k, j) * d[n, j]
                for l in range(-L, L + 1):
                    Gd[k + L, l + L] += M[n, j] ** 2 * at(s, n - k, j) * at(s, n - l, j)
    assert np.max(np.abs(G - Gd)) <= 1e-14 * np.max(np.abs(Gd)) and np.max(np.abs(b - bd)) <= 1e-14 * np.max(np.abs(bd))
    assert np.array_equal(G, G.T) and np.all(G[:1] == 0.0)  # the shift -7 meets no sample
    f = obj.solve(G, b)
    assert f[0] == 0.0 and f[-1] == 0.0  # ... and mu carries it


def test_twin_rejects_bad_arguments():
    for bad in (lambda: df.MatchedL2(-1, 0.0), lambda: df.MatchedL2(65, 0.0), lambda: df.MatchedL2(1.5, 0.0),
                lambda: df.MatchedL2(1, -1.0), lambda: df.MatchedL2(1, np.nan), lambda: df.MatchedL2(1, [1.0, -2.0]),
                lambda: df.MatchedL2(1, 0.0, [1.0, np.nan]),
                lambda: df.MatchedL2(1, 0.0).apply(np.zeros((4, 2)), np.zeros((4, 2)), np.ones(1)),
                lambda: df.MatchedL2(1, 0.0)(np.zeros((4, 2)), np.zeros((4, 2))),  # zero matrix, mu = 0
                lambda: df.MatchedL2(1, [1.0, 2.0])(np.ones((4, 2)), np.ones((4, 2))),  # per-shot mu without shot=
                lambda: df.MatchedL2(1, 1.0)(np.ones((4, 2)), np.ones((4, 2)), -np.ones((4, 2))),
                lambda: df.matched_wavelet(np.ones(4), np.ones(2)), lambda: df.prewhitening(np.ones(4), percent=-1.0)):
        with pytest.raises(ValueError):
            bad()
    assert not issubclass(df.MatchedL2, df.WeightedL2)
    obj = df.MatchedL2(1, [1.0, 2.0])
    assert obj.mu_of(1) == 2.0 and df.MatchedL2(1, 3.0).mu_of(7) == 3.0


def _solve(lib, G, b, K, mu):
    f = np.full(max(K, 1), np.nan)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    return lib.fwi_match_solve(vp(G), vp(b), K, mu, vp(f)), f


@pytest.mark.parametrize("K", [1, 2, 17, 129])
def test_fwi_match_solve_against_numpy(K):
    """The library's Cholesky solve on the twin's G + mu I, mu = 1e-3 sum d^2.  Bound: kappa K^2 2^-52 relative, the
    first-order backward-error bound of a Cholesky solve (Higham, Accuracy and Stability, thm 10.4, with its constant
    3 K + 1 <= K^2 for K >= 4 and kappa >= 1 absorbing the rest) against numpy's LU solve, which obeys the same."""
    lib = _lib.load()
    L = (K - 1) // 2 if K % 2 else None
    rng, s, d, M = _gathers(K, nt=80, ntr=7)
    mu = 1e-3 * float(np.sum(d * d))
    if L is None:  # K = 2: a leading block of the L = 1 system
        G, b = df.MatchedL2(1, mu).normal(s, d, M)
        G, b = np.ascontiguousarray(G[:2, :2]), b[:2].copy()
    else:
        G, b = df.MatchedL2(L, mu).normal(s, d, M)
    A = G + mu * np.eye(K)
    kappa = float(np.linalg.cond(A))
    ref = np.linalg.solve(A, b)
    lower_junk = np.triu(G) + np.tril(np.full((K, K), 1e300), -1)  # only the upper triangle is read
    rc, f = _solve(lib, lower_junk, b, K, mu)
    err = float(np.linalg.norm(f - ref) / np.linalg.norm(ref))
    print("K", K, "kappa", kappa, "rel err", err, "bound", kappa * K * K * 2.0 ** -52)
    assert rc == 0 and kappa <= 1e6
    assert err <= kappa * K * K * 2.0 ** -52
    if L is not None:
        assert np.array_equal(df.MatchedL2(L, mu).solve(G, b), ref)  # (the twin solves with numpy)


def test_fwi_match_solve_rejects_bad_arguments():
    lib = _lib.load()
    assert "fwi_match_solve" in _lib.SIGNATURES and "fwi_misfit_matched" in _lib.SIGNATURES
    assert lib.fwi_abi_version() == _lib.ABI_VERSION == 14
    G, b = np.eye(3), np.ones(3)
    assert _solve(lib, G, b, 3, 0.0)[0] == 0
    assert _solve(lib, np.zeros((3, 3)), b, 3, 0.0)[0] == FWI_EINVAL  # not positive definite
    rc, f = _solve(lib, np.zeros((3, 3)), b, 3, 2.0)
    assert rc == 0 and np.array_equal(f, 0.5 * b)                     # ... until mu carries it
    assert _solve(lib, -np.eye(3), b, 3, 0.5)[0] == FWI_EINVAL
    assert _solve(lib, np.full((3, 3), np.nan), b, 3, 1.0)[0] == FWI_EINVAL
    assert _solve(lib, G, b, 3, -1.0)[0] == FWI_EINVAL and _solve(lib, G, b, 3, np.inf)[0] == FWI_EINVAL
    assert _solve(lib, None, b, 3, 1.0)[0] == FWI_EINVAL and _solve(lib, G, None, 3, 1.0)[0] == FWI_EINVAL
    assert lib.fwi_match_solve(G.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), 3, 1.0, None) == FWI_EINVAL
    big = np.eye(131)
    for K in (0, -1, 130, 131):
        assert lib.fwi_match_solve(big.ctypes.data_as(C.c_void_p), np.ones(131).ctypes.data_as(C.c_void_p), K, 1.0,
                                   np.zeros(131).ctypes.data_as(C.c_void_p)) == FWI_EINVAL, K
    assert _solve(lib, np.eye(129), np.ones(129), 129, 0.0)[0] == 0
    # the device entry point refuses a null context before anything else
    J = C.c_double(0.0)
    assert lib.fwi_misfit_matched(None, None, None, None, 0, 0, 0.0, None, None, None, C.byref(J)) == FWI_EINVAL


def test_matched_wavelet_and_prewhitening_by_hand():
    w = np.array([1.0, 2.0, 3.0, 4.0])
    # f_-1 = 10, f_0 = 1, f_1 = 100: w'[n] = 10 w[n + 1] + w[n] + 100 w[n - 1]
    assert np.array_equal(df.matched_wavelet(w, [10.0, 1.0, 100.0]), [21.0, 132.0, 243.0, 304.0])
    w2 = np.stack([w, -w], 1)
    out = df.matched_wavelet(w2, [0.0, 0.0, 0.0, 2.0, 0.0])  # f_1 = 2: a delay by one sample, doubled
    assert out.shape == (4, 2) and np.array_equal(out[:, 0], [0.0, 2.0, 4.0, 6.0]) and np.array_equal(out[:, 1], -out[:, 0])
    assert np.array_equal(df.matched_wavelet(w, [1.0]), w)
    assert np.array_equal(df.matched_wavelet(w, np.r_[1.0, np.zeros(10)]), np.zeros(4))  # f_-5: beyond the trace
    d = np.array([[1.0, 2.0], [3.0, 4.0]])
    assert df.prewhitening(d) == 0.1 / 100.0 * 30.0
    assert df.prewhitening(d, np.array([[1.0, 0.0], [0.5, 1.0]]), percent=50.0) == 0.5 * (1.0 + 2.25 + 16.0)
    assert df.prewhitening(d, percent=0.0) == 0.0


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


def test_shot_loop_takes_the_host_branch_on_an_engine_without_misfit_matched():
    rng, e, c0, shots, dt = _setup_2d()
    assert not hasattr(e, "misfit_matched")
    shots[1].weights = rng.random(shots[1].d_obs.shape)
    mus = [df.prewhitening(s.d_obs, s.weights) for s in shots]
    obj = df.MatchedL2(3, mus, df.lowpass_taps(dt, 60.0, 5))
    J, g = sh.misfit_and_gradient(e, c0, shots, objective=obj)
    assert sorted(obj.filters) == [0, 1] and all(f.shape == (7,) for f in obj.filters.values())
    # the same by hand: the twin per shot, its r through adjoint()
    e.set_model(c0)
    e.reset_gradient()
    Jh = 0.0
    for i, s in enumerate(shots):
        d = s.forward(e, save=True)
        ref = df.MatchedL2(3, mus[i], obj.taps)
        j, r = ref(d, s.d_obs, s.weights)
        assert np.array_equal(ref.solve(*ref.normal(d, s.d_obs, s.weights)), obj.filters[i])
        s.adjoint(e, r)
        Jh += j
    assert J > 0.0 and J == Jh and np.array_equal(g, e.gradient())
    # a scaled, delayed wavelet in the data is taken up by the filter: J falls far below plain least squares
    for s in shots:
        s.d_obs = df.matched_wavelet(s.d_obs, [0.0, 0.0, 0.0, 0.0, 1.7, 0.0, 0.0])
    e2 = OracleEngine(c0.shape, 10.0, dt, 40, order=4, npml=4)
    true_model_shots = [sh.Shot(s.src_idx, s.wavelet, s.rec_idx, s.d_obs) for s in shots]
    c_true = 2000.0 + 200.0 * np.random.default_rng(5).random(c0.shape)
    obj2 = df.MatchedL2(3, 0.0)
    Jm, _ = sh.misfit_and_gradient(e2, c_true, true_model_shots, objective=obj2)
    Jp, _ = sh.misfit_and_gradient(e2, c_true, true_model_shots)
    assert Jm <= 1e-20 * Jp
    # the filter itself to kappa K 2^-52: G of a smooth, oversampled wavefield is ill-conditioned without mu
    s0 = true_model_shots[0]
    kappa = float(np.linalg.cond(obj2.normal(s0.forward(e2, save=False), s0.d_obs)[0]))
    err = float(np.max(np.abs(obj2.filters[0] - [0.0, 0.0, 0.0, 0.0, 1.7, 0.0, 0.0])))
    print("kappa", kappa, "filter error", err, "bound", kappa * 7 * 2.0 ** -52 * 1.7)
    assert err <= kappa * 7 * 2.0 ** -52 * 1.7
    with pytest.raises(ValueError):
        sh.gauss_newton_hvp(e, c0, shots, np.ones(c0.shape), objective=obj)


def test_run_config_knows_the_match_flags_and_refuses_a_bad_length():
    """tools/run_config.py --match-source / --match-mu-percent: the arguments are checked before any engine exists"""
    import subprocess
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "run_config.py")
    out = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--match-source" in out.stdout and "--match-mu-percent" in out.stdout
    for bad in (["--match-source", "65"], ["--match-source", "-1"], ["--match-source", "x"],
                ["--match-source", "4", "--match-mu-percent", "-1"]):
        out = subprocess.run([sys.executable, tool] + bad, capture_output=True, text=True)
        assert out.returncode == 2 and "--match" in out.stderr, (bad, out.stderr[-300:])
