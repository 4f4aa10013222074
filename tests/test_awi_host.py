"""The adaptive (per-trace matching-filter) misfit without a GPU (full_waveform_inversion_amd/datafit.py AdaptiveMatching,
include/fwi.h fwi_misfit_adaptive): the NumPy twin's gradient against central differences of its J, the
Toeplitz normal matrix against the dense one of the full convolution, the property the misfit exists for (sqrt(W) reads
the shift where least squares does not even order the shifts), gain invariance, the bound on W, the traces that do not
count, the conditioning of the systems, the errors, the objective protocol, the binding and the new flags of
tools/run_config.py.

Central differences: J is a smooth rational function of s wherever the set of counting traces does not change, so
D(h) = (J(s + h v) - J(s - h v)) / (2 h) = <r, v> + O(h^2 J''').  With h = 1e-6 of the largest amplitude the truncation
is of relative order 1e-12 and the cancellation in the difference of two J of order 2^-53 J / (h J') ~ 1e-10: the
tolerance of 1e-6 leaves four digits.  The roundoff bound between two evaluations is roundoff_bounds of tests/_awi.py,
derived there and shared with tests/test_gpu_awi.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from _awi import roundoff_bounds  # noqa: E402
from _oracle_engine import OracleEngine  # noqa: E402
from full_waveform_inversion_amd import _lib, datafit as df, shots as sh  # noqa: E402
from oracle import fwi_oracle as fo  # noqa: E402

FWI_EINVAL = 1
DT = 2e-3
CASES = [(16, 1e-2), (7, 1e-3), (40, 1e-2), (64, 1e-2)]  # nt = 45 below: L = 64 exceeds nt - 1
FLAGS = [(wt, tp, tw) for wt in (False, True) for tp in (False, True) for tw in (False, True)]


def ricker(nt=400, t0=0.2, f0=25.0):
    a = (np.pi * f0 * (np.arange(nt) * DT - t0)) ** 2
    return (1.0 - 2.0 * a) * np.exp(-a)


def _random(nt, ntr, seed):
    rng = np.random.default_rng(seed)
    return rng, rng.standard_normal((nt, ntr)), rng.standard_normal((nt, ntr))


def _options(rng, shape, flags):
    weighted, with_taps, trace_weighted = flags
    M = 0.25 + 0.75 * rng.random(shape) if weighted else None
    taps = df.bandpass_taps(DT, 10.0, 120.0, 5) if with_taps else None
    tw = 0.25 + rng.random(shape[1]) if trace_weighted else None
    return M, taps, tw


@pytest.mark.parametrize("flags", FLAGS, ids=["".join(c if f else "-" for c, f in zip("MBw", fl)) for fl in FLAGS])
@pytest.mark.parametrize("L,lam", CASES)
def test_twin_gradient_matches_central_differences(L, lam, flags):
    nt = 45 if L == 64 else 70
    rng, s, d = _random(nt, 3, 10 + L)
    assert L != 64 or L > nt - 1
    M, taps, tw = _options(rng, s.shape, flags)
    obj = df.AdaptiveMatching(DT, L, lam, taps)
    J, r = obj(s, d, M, tw)
    assert J > 0.0 and obj.counts.all() and r.shape == s.shape
    h = 1e-6 * float(np.max(np.abs(s)))
    for _ in range(5):
        v = rng.standard_normal(s.shape)
        fd = (obj(s + h * v, d, M, tw)[0] - obj(s - h * v, d, M, tw)[0]) / (2.0 * h)
        an = float(np.sum(r * v))
        print("L", L, "lam", lam, flags, "central difference", fd, "<r, v>", an, "relative", abs(fd - an) / abs(fd))
        assert abs(fd - an) <= 1e-6 * abs(fd)


@pytest.mark.parametrize("L,nt", [(3, 20), (16, 70), (40, 33)])
def test_toeplitz_matrix_is_the_dense_normal_matrix_of_the_full_convolution(L, nt):
    """C[n, k] = dh[n - k] over the whole output range n = -L .. nt - 1 + L of the convolution w * dh: G = C^T C + lam
    a(0) I and c = C^T (sh zero-extended).  Sums of at most nt products: (nt + 2) 2^-52 times the majorant apart."""
    rng, s, d = _random(nt, 4, 3)
    M = 0.25 + 0.75 * rng.random(s.shape)
    obj = df.AdaptiveMatching(DT, L, 1e-2)
    a, c, (Aa, Ac), sh_, dh = obj.correlations(s, d, M)
    G, alive = obj.normal(a)
    K = 2 * L + 1
    assert alive.all() and G.shape == (4, K, K)
    for j in range(4):
        Cm = np.zeros((nt + 2 * L, K))
        for k in range(-L, L + 1):
            Cm[k + L:k + L + nt, k + L] = dh[:, j]  # row n + L, n = m + k
        spad = np.concatenate([np.zeros(L), sh_[:, j], np.zeros(L)])
        dense = Cm.T @ Cm + 1e-2 * a[0, j] * np.eye(K)
        tol = (nt + 2) * 2.0 ** -52 * Aa[:, j][np.abs(np.arange(K)[:, None] - np.arange(K)[None, :])] + 2.0 ** -51 * a[0, j]
        assert np.all(np.abs(G[j] - dense) <= tol)
        assert np.all(np.abs(c[:, j] - Cm.T @ spad) <= (nt + 2) * 2.0 ** -52 * Ac[:, j])
        assert np.array_equal(G[j], G[j].T) and a[0, j] == Aa[0, j]


def test_moment_reads_the_shift_where_least_squares_does_not_order_it():
    """25 Hz Ricker, dt = 2 ms, nt = 400, L = 64, lam = 1e-2, synthetics = the data circularly shifted"""
    d = ricker()
    obj = df.AdaptiveMatching(DT, 64, 1e-2)
    shifts, width, l2 = (0, 5, 20, 30, 60), [], []
    for k in shifts:
        s = np.roll(d, k)
        obj(s[:, None], d[:, None])
        width.append(float(np.sqrt(obj.moments[0])) / DT)
        l2.append(0.5 * float(np.sum((s - d) ** 2)))
    print("shift", shifts, "sqrt(W) / dt", width, "least squares", l2)
    assert all(b > a for a, b in zip(width, width[1:]))
    assert all(abs(wd - k) <= 0.02 * k for k, wd in zip(shifts, width) if k >= 20)
    assert width[0] > 0.0  # the zero-shift floor: the width of the band-limited delta
    assert not all(b > a for a, b in zip(l2, l2[1:]))


@pytest.mark.parametrize("L,lam", CASES)
def test_gain_invariance_bound_on_w_and_conditioning(L, lam):
    rng, s, d = _random(70, 3, 20 + L)
    obj = df.AdaptiveMatching(DT, L, lam)
    J, r = obj(s, d)
    W = obj.moments.copy()
    Jg, rg = obj(3.7 * s, d)
    print("L", L, "J", J, "with gain", Jg, "relative", abs(Jg - J) / J)
    assert abs(Jg - J) <= 1e-12 * J
    gain = np.array([0.2, 1.0, 5.0])
    assert abs(obj(gain * s, d)[0] - J) <= 1e-12 * J
    assert np.all(W > 0.0) and np.all(W <= (L * DT) ** 2)
    b = roundoff_bounds(obj, s, d)
    print("condition numbers", b.cond, "bound", 1.0 + (2 * L + 1) / lam)
    assert np.all(b.cond <= 1.0 + (2 * L + 1) / lam)
    # two evaluations that differ by roundoff only (the traces in another order of memory) lie inside the bounds
    J2, _ = obj(np.asfortranarray(s), np.asfortranarray(d))
    assert abs(J2 - J) <= b.J and np.all(np.abs(obj.moments - W) <= b.W)


def test_dead_traces_do_not_count_and_leave_no_residual():
    rng, s, d = _random(50, 5, 31)
    d[:, 1] = 0.0  # a dead data trace
    s[:, 3] = 0.0  # a dead synthetic trace: w = 0
    M = np.ones(s.shape)
    M[:, 4] = 0.0  # a trace killed by its weights
    obj = df.AdaptiveMatching(DT, 8, 1e-2)
    J, r = obj(s, d, M)
    assert list(obj.counts) == [True, False, True, False, False]
    assert not np.any(r[:, [1, 3, 4]]) and np.any(r[:, 0]) and np.any(r[:, 2])
    assert not np.any(obj.moments[[1, 3, 4]]) and not np.any(obj.filters[[1, 3, 4]])
    assert J == float(np.sum(0.5 * obj.moments)) and np.all(np.isfinite(r))
    d[7, 0] = np.nan  # not finite: a_j(0) is not
    J, r = obj(s, d, M)
    assert not obj.counts[0] and not np.any(r[:, 0]) and np.isfinite(J)


def test_edge_shapes_and_argument_errors():
    obj = df.AdaptiveMatching(DT, 4)
    assert obj.lam == 1e-2 and obj.L_MAX == 64 and df.AdaptiveMatching.L_MAX == 64
    J, r = obj(np.ones((1, 3)), 2.0 * np.ones((1, 3)))  # nt = 1: w = (0 .. 0, s d / ((1 + lam) d^2), 0 .. 0), W = 0
    assert J == 0.0 and obj.counts.all() and r.shape == (1, 3) and obj.filters.shape == (3, 9)
    J, r = obj(np.zeros((5, 0)), np.zeros((5, 0)))
    assert J == 0.0 and r.shape == (5, 0)
    for bad in (dict(dt=0.0), dict(dt=np.nan), dict(L=0), dict(L=65), dict(L=2.5), dict(lam=0.0), dict(lam=-1.0),
                dict(lam=np.inf), dict(taps=np.ones((2, 2)))):
        with pytest.raises(ValueError):
            df.AdaptiveMatching(**{"dt": DT, "L": 4, **bad})
    _, s, d = _random(20, 3, 2)
    for bad in (dict(weights=np.ones((20, 2))), dict(weights=-np.ones((20, 3))), dict(trace_weights=np.ones(2)),
                dict(trace_weights=np.array([1.0, -1.0, 1.0])), dict(trace_weights=np.array([1.0, np.nan, 1.0]))):
        with pytest.raises(ValueError):
            obj(s, d, **bad)
    with pytest.raises(ValueError):
        obj(s, d[:, :2])
    # dtype=: B s, B d and g are rounded to it
    r32 = df.AdaptiveMatching(DT, 4, dtype="float32")(s.astype("f4"), d.astype("f4"))[1]
    assert np.any(r32) and np.array_equal(r32, r32.astype("f4").astype("f8"))


class _StandIn:
    """an engine that records the call of the objective's device path"""

    def misfit_adaptive(self, *args):
        self.args = args
        return 1.5


def test_objective_protocol_and_binding():
    taps = df.lowpass_taps(DT, 60.0, 3)
    obj = df.AdaptiveMatching(DT, 12, 5e-3, taps)
    assert obj.engine_method == "misfit_adaptive" and hasattr(obj, "host")
    _, s, d = _random(30, 4, 5)
    shot = sh.Shot(np.array([[1, 1]], np.int32), np.zeros(30), np.array([[1, 2]] * 4, np.int32))
    shot.d_obs, shot.weights, shot.trace_weights = d, np.ones(d.shape), np.arange(4.0)
    e = _StandIn()
    assert obj.device(e, shot, 0) == 1.5
    assert e.args[0] is d and e.args[1:3] == (12, 5e-3) and e.args[3] is shot.weights and e.args[4] is obj.taps
    assert e.args[5] is shot.trace_weights
    J, r = obj.host(s, shot, 0)
    J2, r2 = obj(s, d, shot.weights, shot.trace_weights)
    assert J == J2 and np.array_equal(r, r2)
    assert not isinstance(obj, df.WeightedL2)  # gauss_newton_hvp takes a WeightedL2 only
    lib = _lib.load()
    assert "fwi_misfit_adaptive" in _lib.SIGNATURES and _lib.AWI_LMAX == df.AdaptiveMatching.L_MAX
    assert lib.fwi_abi_version() == _lib.ABI_VERSION == 14
    J = C.c_double(0.0)
    assert lib.fwi_misfit_adaptive(None, None, None, None, 0, None, 4, 1e-2, C.byref(J), None, None, None) == FWI_EINVAL


def test_shot_loop_runs_the_twin_on_an_engine_without_misfit_adaptive():
    rng = np.random.default_rng(5)
    shape, h, order, nt = (24, 28), 10.0, 4, 60
    c_true = 2000.0 + 200.0 * rng.random(shape)
    c0 = np.full(shape, 2100.0)
    dt = 0.6 * fo.cfl_dt(c_true.max(), h, 2, order)
    wav = fo.ricker(nt, dt, 30.0)
    rec = np.array([[10, x] for x in range(4, 24, 3)], np.int32)
    shots = [sh.Shot(np.array([[12, 8]], np.int32), wav, rec), sh.Shot(np.array([[14, 20]], np.int32), wav, rec)]
    e = OracleEngine(shape, h, dt, nt, order=order, npml=4)
    sh.model_data(e, c_true, shots)
    assert not hasattr(e, "misfit_adaptive")
    shots[1].weights = 0.5 + 0.5 * rng.random(shots[1].d_obs.shape)
    shots[1].trace_weights = rng.random(shots[1].d_obs.shape[1])
    obj = df.AdaptiveMatching(dt, 10, 1e-2, df.lowpass_taps(dt, 60.0, 5))
    J, g = sh.misfit_and_gradient(e, c0, shots, objective=obj)
    e.set_model(c0)
    e.reset_gradient()
    Jh = 0.0
    for s in shots:
        d = s.forward(e, save=True)
        j, r = obj(d, s.d_obs, s.weights, s.trace_weights)
        assert obj.counts.all()
        s.adjoint(e, r)
        Jh += j
    assert J > 0.0 and J == Jh and np.any(g != 0.0) and np.array_equal(g, e.gradient())
    with pytest.raises(ValueError, match="WeightedL2"):
        sh.gauss_newton_hvp(e, c0, shots, np.ones(c0.shape), objective=obj)


def test_run_config_knows_the_adaptive_flags_and_refuses_bad_combinations():
    """tools/run_config.py --adaptive L [--adaptive-ridge LAM]: checked before any engine exists"""
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "run_config.py")
    out = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--adaptive" in out.stdout and "--adaptive-ridge" in out.stdout
    for bad, word in ((["--adaptive", "8", "--traveltime", "8"], "--adaptive"),
                      (["--adaptive", "8", "--correlation"], "--adaptive"),
                      (["--adaptive", "8", "--transport", "softplus"], "--adaptive"),
                      (["--adaptive", "8", "--envelope", "--hilbert-fmin", "5"], "--adaptive"),
                      (["--adaptive", "8", "--match-source", "4"], "--adaptive"),
                      (["--adaptive", "8", "--spectral", "l2", "--spectral-band", "5,10"], "--adaptive"),
                      (["--adaptive", "0"], "--adaptive"),
                      (["--adaptive", "65"], "--adaptive"),
                      (["--adaptive-ridge", "0.01"], "--adaptive-ridge"),
                      (["--adaptive", "8", "--adaptive-ridge", "0"], "--adaptive-ridge"),
                      (["--adaptive", "8", "--adaptive-ridge", "nan"], "--adaptive-ridge"),
                      (["--adaptive", "8", "--bands", "5,10", "--iters", "0"], "--bands")):
        out = subprocess.run([sys.executable, tool] + bad, capture_output=True, text=True)
        assert out.returncode == 2 and word in out.stderr, (bad, out.stderr[-300:])
