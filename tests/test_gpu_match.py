"""The matching-filter (source-independent) misfit on the GPU (include/fwi.h fwi_misfit_matched, csrc/fwi_match.hip,
DESIGN.md s.4i).  The oracle is the fp64 NumPy twin (datafit.MatchedL2) fed the engine's own downloaded synthetics, and
d_obs and the weights rounded to the engine's dtype; with taps it rounds B s and B d to that dtype as the device does.

Bounds.  With n = nt ntr terms per sum and u = 2^-53, a sum of n products in fp64, in any order, is within about n u of
the sum of the absolute values of its terms; device and twin each are, hence n 2^-52 times the majorant (Ghat, bhat,
Jhat below, which the test forms from absolute values).  The residual is checked through the gradient that adjoint(None)
forms from it, against the gradient of the twin's r handed to adjoint(), with test_gpu_datafit.py's GRAD_TOL: 168
roundings of the dtype, so that the fp64 run pins the arithmetic (one fp32 operation anywhere would leave 1e-8).  An
estimated filter inherits the error of G and b through (G + mu I)^-1 and the K^2 u kappa of the host solve."""
import ctypes as C

import numpy as np
import pytest

from full_waveform_inversion_amd import Engine, FwiError, _lib, datafit as df, shots as sh
from oracle import fwi_oracle as fo

pytestmark = pytest.mark.gpu

SHAPE, H, ORDER, NPML, NT = (24, 28), 10.0, 4, 4, 40
DTYPES = ["float32", "float64"]
ESTATE, EINVAL = 3, 1
GRAD_TOL = {"float32": 1e-5, "float64": 1e-5 * 2.0 ** -29}  # 168 roundings of the dtype (test_gpu_datafit.py)
U2 = 2.0 ** -52


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _models(shape, seed=0):
    rng = np.random.default_rng(seed)
    return 2000.0 + 300.0 * rng.random(shape), np.full(shape, 2150.0)


def _dt(shape, order=ORDER):
    return 0.6 * fo.cfl_dt(2300.0, H, len(shape), order)


def _nodes(ntr, shape=SHAPE, seed=1):
    """ntr distinct interior nodes"""
    rng = np.random.default_rng(seed)
    grids = np.meshgrid(*[np.arange(NPML, n - NPML) for n in shape], indexing="ij")
    allnodes = np.stack([g.ravel() for g in grids], 1)
    return np.ascontiguousarray(allnodes[rng.permutation(len(allnodes))[:ntr]], dtype=np.int32)


def _weights(nt, ntr, seed=2):
    M = np.random.default_rng(seed).random((nt, ntr))
    M[nt // 3] = 0.0  # one dead time row
    if ntr > 1:
        M[:, ntr // 2] = 0.0  # one dead trace
    return M


_ENGINES = {}


@pytest.fixture(scope="module")
def engines(gpu):
    """one 2-D context per dtype for the whole module"""
    def get(dtype):
        if dtype not in _ENGINES:
            _ENGINES[dtype] = Engine(SHAPE, H, _dt(SHAPE), NT, order=ORDER, npml=NPML, dtype=dtype)
        return _ENGINES[dtype]
    yield get
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


_DATA = {}


def _data(e, dtype, nt, ntr):
    """(src, rec, d_obs, d_syn) of the 2-D problem; computed once per (dtype, nt, ntr) and never written to"""
    key = (dtype, nt, ntr)
    if key not in _DATA:
        c_true, c0 = _models(SHAPE)
        src = (np.array([[12, 9]], np.int32), fo.ricker(nt, _dt(SHAPE), 60.0))
        rec = _nodes(ntr)
        d_obs = e.forward(c_true, src, rec, save=False)
        d_syn = e.forward(c0, src, rec, save=True)
        for a in (d_obs, d_syn):
            a.setflags(write=False)
        _DATA[key] = (src, rec, d_obs, d_syn)
    return _DATA[key]


# (name, nt, ntr, L, weighted, taps): 39 = nt - 1, 64 > nt
CASES = ([("ntr%d" % n, NT, n, 7, True, False) for n in (1, 5, 63, 65, 130)]
         + [("L%d" % L, NT, 65, L, True, False) for L in (0, 1, 8, 9, 39, 64)]
         + [("nt37", 37, 65, 7, True, False), ("no_weights", NT, 65, 7, False, False), ("taps", NT, 65, 7, True, True),
            ("taps_no_weights_L1", NT, 65, 1, False, True)])
IDS = [c[0] for c in CASES]


class _Run:
    pass


_RUNS = {}


def _run(e, dtype, case, fixed):
    """One device call (f estimated, or a fixed random f) and the twin's answer to the same inputs, with both gradients;
    once per (dtype, case, fixed)."""
    key = (dtype, case[0], fixed)
    if key in _RUNS:
        return _RUNS[key]
    _, nt, ntr, L, weighted, with_taps = case
    src, rec, d_obs, d_syn = _data(e, dtype, nt, ntr)
    _, c0 = _models(SHAPE)
    K = 2 * L + 1
    r = _Run()
    r.n, r.K = nt * ntr, K
    r.taps = df.bandpass_taps(_dt(SHAPE), 8.0, 90.0, 7) if with_taps else None
    r.M = _weights(nt, ntr).astype(dtype) if weighted else None
    r.mu = 1e-3 * float(np.sum(np.asarray(d_obs, np.float64) ** 2))
    r.f_in = None
    if fixed:
        r.f_in = np.ones(1) if L == 0 else np.random.default_rng(100 + L).standard_normal(K)
    obj = df.MatchedL2(L, r.mu, r.taps, dtype=dtype if with_taps else None)
    d = e.forward(c0, src, rec, save=True)
    assert np.array_equal(d, d_syn)
    e.reset_gradient()
    r.J, r.f, r.G, r.b = e.misfit_matched(d_obs, L, r.mu, r.M, r.taps, f=r.f_in, normal=True)
    e.adjoint(None)
    r.g = e.gradient()
    # the twin, and its majorants from absolute values
    r.Gt, r.bt = obj.normal(d_syn, d_obs, r.M)
    s1, d1 = np.abs(obj.filter(d_syn)), np.abs(obj.filter(d_obs))
    plain = df.MatchedL2(L, r.mu)
    r.Ghat, r.bhat = plain.normal(s1, d1, r.M)
    r.ft = obj.solve(r.Gt, r.bt) if r.f_in is None else r.f_in
    r.Jt, rt = obj.apply(d_syn, d_obs, r.ft, r.M)
    ehat = df.matched_wavelet(s1, np.abs(r.ft)) + d1
    if r.M is not None:
        ehat = ehat * r.M
    r.Jhat = 0.5 * float(np.sum(ehat * ehat)) + 0.5 * r.mu * float(np.sum(r.ft * r.ft))
    A = r.Gt + r.mu * np.eye(K)
    r.kappa = float(np.linalg.cond(A))
    r.inv_norm = float(np.linalg.norm(np.linalg.inv(A), 2))
    e.forward(c0, src, rec, save=True)
    e.reset_gradient()
    e.adjoint(rt.astype(dtype))
    r.gt = e.gradient()
    _RUNS[key] = r
    return r


def _filter_bound(r):
    """||f - f_t||: the error n 2^-52 (Ghat, bhat) of the normal equations through (G + mu I)^-1, to first order and
    doubled, and the kappa K^2 2^-52 of the two solves"""
    nf = float(np.linalg.norm(r.ft))
    return (2.0 * r.inv_norm * r.n * U2 * (float(np.linalg.norm(r.Ghat)) * nf + float(np.linalg.norm(r.bhat)))
            + r.kappa * r.K ** 2 * U2 * nf)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [c for c in CASES if not c[5]], ids=[c[0] for c in CASES if not c[5]])
def test_normal_equations_against_the_twin(engines, dtype, case):
    r = _run(engines(dtype), dtype, case, False)
    dG, db = np.abs(r.G - r.Gt), np.abs(r.b - r.bt)
    with np.errstate(divide="ignore", invalid="ignore"):
        print("max |G - G_t| / Ghat", np.nanmax(np.where(r.Ghat > 0, dG / r.Ghat, 0.0)), "max |b - b_t| / bhat",
              np.nanmax(np.where(r.bhat > 0, db / r.bhat, 0.0)), "bound", r.n * U2)
    assert r.G.shape == (r.K, r.K) and np.any(r.G != 0.0)
    assert np.array_equal(r.G, r.G.T)
    assert np.all(dG <= r.n * U2 * r.Ghat)
    assert np.all(db <= r.n * U2 * r.bhat)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fixed_filter_against_the_twin(engines, dtype, case):
    r = _run(engines(dtype), dtype, case, True)
    bound = (r.n + 2 * r.K) * U2
    if case[5] and dtype == "float32":
        bound = 2.0 ** -23  # B s and B d are rounded to fp32: a rounding boundary may fall differently in the twin
    print("J", r.J, "twin", r.Jt, "|J - J_t| / Jhat", abs(r.J - r.Jt) / r.Jhat, "bound", bound, "gradient rel L2",
          rel(r.g, r.gt))
    assert r.Jt > 0.0 and np.all(np.isfinite(r.g)) and np.array_equal(r.f, r.f_in)
    assert abs(r.J - r.Jt) <= bound * r.Jhat
    assert rel(r.g, r.gt) <= GRAD_TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_estimated_filter_against_the_twin(engines, dtype, case):
    r = _run(engines(dtype), dtype, case, False)
    err, bound = float(np.linalg.norm(r.f - r.ft)), _filter_bound(r)
    print("kappa", r.kappa, "|f - f_t|", err, "bound", bound, "|f_t|", float(np.linalg.norm(r.ft)), "J", r.J, "twin", r.Jt,
          "gradient rel L2", rel(r.g, r.gt), "bound", GRAD_TOL[dtype] + r.kappa * r.n * U2)
    assert r.kappa <= 1e6  # (kappa <= K sum s'^2 / mu + 1: otherwise the inputs are wrong, not the kernel)
    assert np.linalg.norm(r.ft) > 0.0 and r.J > 0.0
    assert err <= bound
    assert rel(r.g, r.gt) <= GRAD_TOL[dtype] + r.kappa * r.n * U2


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_unit_filter_is_misfit_weighted_bit_for_bit_without_taps(engines, dtype):
    """L = 0, f = (1), mu = 0 without taps: e and r are fwi_misfit_weighted's, bit for bit -- the same fp64 operations on
    the same numbers, and the same order of the sum of e^2 (blocks of 64 traces x 32 times, per thread over ascending
    time, the same trees).  With weights J is then equal too; without weights fwi_misfit_weighted sums the squares of the
    residual AS STORED (its plain case, fwi_misfit_l2's rule), so only the gradient is compared."""
    e = engines(dtype)
    src, rec, d_obs, _ = _data(e, dtype, NT, 130)
    _, c0 = _models(SHAPE)
    for M in (_weights(NT, 130).astype(dtype), None):
        out = []
        for call in (lambda: e.misfit_weighted(d_obs, M), lambda: e.misfit_matched(d_obs, 0, 0.0, M, f=np.ones(1))[0]):
            e.forward(c0, src, rec, save=True)
            e.reset_gradient()
            J = call()
            e.adjoint(None)
            out.append((J, e.gradient()))
        (Jw, gw), (Jm, gm) = out
        print("weights", M is not None, "J weighted", Jw, "matched", Jm)
        assert np.any(gw != 0) and np.array_equal(gm, gw)
        if M is not None:
            assert Jm == Jw


def test_source_independence_in_fp64(engines):
    """fp64, the true model, mu = 0, L = 2: d_obs modelled with the wavelet C_(0, 0, g) w, the synthetics with w.  The
    discrete scheme is linear, causal and time-invariant in the wavelet, so d_obs = C_(0, 0, g) d_syn up to fp64
    round-off (about nt 2^-53): the filter is recovered and the misfit vanishes."""
    e = engines("float64")
    c_true, _ = _models(SHAPE)
    g = np.array([0.8, -0.35, 0.15])
    f_true = np.concatenate([np.zeros(2), g])
    w = fo.ricker(NT, _dt(SHAPE), 60.0)
    idx, rec = np.array([[12, 9]], np.int32), _nodes(65)
    d_obs = e.forward(c_true, (idx, df.matched_wavelet(w, f_true)), rec, save=False)
    e.forward(c_true, (idx, w), rec, save=True)
    J_plain = e.misfit_l2(d_obs)
    e.forward(c_true, (idx, w), rec, save=True)
    J, f = e.misfit_matched(d_obs, 2, 0.0)
    print("f", f, "J", J, "J_plain", J_plain)
    assert J_plain > 0.0
    assert np.max(np.abs(f - f_true)) <= 1e-9
    assert J <= 1e-18 * J_plain


def _two_shots(e, dtype, rng):
    """one shot on the nodes, one off the grid, weights rounded to the engine's dtype"""
    c_true, c0 = _models(SHAPE)
    dt = _dt(SHAPE)
    wav = fo.ricker(NT, dt, 60.0).astype(dtype)
    lo, hi = NPML + 0.5, np.array(SHAPE) - NPML - 1.5
    rec = lo + rng.random((9, 2)) * (hi - lo)
    shots = [sh.Shot(_nodes(1, SHAPE, seed=7), wav, _nodes(11, SHAPE)),
             sh.Shot.at_coordinates([lo + rng.random(2) * (hi - lo)], wav, rec, SHAPE)]
    sh.model_data(e, c_true.astype(dtype), shots)
    for s in shots:
        s.weights = (df.offset_time_mute(s, H, dt, 2600.0, 2 * dt, 5) * (0.25 + 0.75 * rng.random(s.d_obs.shape))).astype(dtype)
    return shots, c0.astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_shot_loop_device_branch_against_the_host_branch(engines, dtype):
    e = engines(dtype)
    shots, c0 = _two_shots(e, dtype, np.random.default_rng(21))
    L = 3
    mus = [df.prewhitening(s.d_obs, s.weights, percent=0.1) for s in shots]
    od, oh = df.MatchedL2(L, mus), df.MatchedL2(L, mus)
    calls = []
    raw = e.misfit_matched
    e.misfit_matched = lambda *a, **k: (calls.append(1), raw(*a, **k))[1]
    try:
        Jd, gd = sh.misfit_and_gradient(e, c0, shots, objective=od)
    finally:
        del e.misfit_matched
    assert len(calls) == 2  # the device path ran, once per shot
    Jh, gh = sh.misfit_and_gradient(e, c0, shots, objective=oh, device_l2=False)
    assert sorted(od.filters) == sorted(oh.filters) == [0, 1]
    # per shot the bounds of the estimated-filter check, from the twin's own normal equations and their majorants
    e.set_model(c0)
    jtol, kmax, nmax = 0.0, 0.0, 0
    for i, s in enumerate(shots):
        d = np.asarray(s.forward(e, save=False), np.float64)
        r = _Run()
        r.n, r.K = d.size, 2 * L + 1
        r.Gt, r.bt = oh.normal(d, s.d_obs, s.weights)
        r.Ghat, r.bhat = oh.normal(np.abs(d), np.abs(s.d_obs), s.weights)
        r.ft = oh.filters[i]
        A = r.Gt + mus[i] * np.eye(r.K)
        r.kappa, r.inv_norm = float(np.linalg.cond(A)), float(np.linalg.norm(np.linalg.inv(A), 2))
        err, bound = float(np.linalg.norm(od.filters[i] - r.ft)), _filter_bound(r)
        print("shot", i, "kappa", r.kappa, "|f_device - f_host|", err, "bound", bound)
        assert r.kappa <= 1e6 and err <= bound
        ehat = df.matched_wavelet(np.abs(d), np.abs(r.ft)) + np.abs(s.d_obs)
        Jhat = 0.5 * float(np.sum((ehat * s.weights) ** 2)) + 0.5 * mus[i] * float(np.sum(r.ft ** 2))
        # J at the device's f: the fixed-filter bound, and (f - f_t)^T (G + mu I) (f - f_t) around the minimiser
        jtol += (r.n + 2 * r.K) * U2 * Jhat + float(np.linalg.norm(A, 2)) * bound ** 2
        kmax, nmax = max(kmax, r.kappa), max(nmax, r.n)
    print("J device", Jd, "host", Jh, "diff", abs(Jd - Jh), "bound", jtol, "gradient rel L2", rel(gd, gh))
    assert Jh > 0.0 and abs(Jd - Jh) <= jtol
    assert rel(gd, gh) <= GRAD_TOL[dtype] + kmax * nmax * U2


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_call_is_reproducible_bit_for_bit(engines, dtype):
    e = engines(dtype)
    src, rec, d_obs, _ = _data(e, dtype, NT, 130)
    _, c0 = _models(SHAPE)
    taps, M = df.bandpass_taps(_dt(SHAPE), 8.0, 90.0, 7), _weights(NT, 130)
    mu = 1e-3 * float(np.sum(np.asarray(d_obs, np.float64) ** 2))
    e.forward(c0, src, rec, save=True)
    outs = [e.misfit_matched(d_obs, 9, mu, M, taps, normal=True) for _ in range(3)]
    assert outs[0][0] > 0.0 and np.any(outs[0][1] != 0.0)
    for o in outs[1:]:
        assert o[0] == outs[0][0] and all(np.array_equal(a, b) for a, b in zip(o[1:], outs[0][1:]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_state_and_argument_errors(engines, dtype):
    e = engines(dtype)
    lib, ctx = e._lib, e._c
    src, rec, d_obs, _ = _data(e, dtype, NT, 5)
    _, c0 = _models(SHAPE)
    J = C.c_double(-1.0)
    taps, f3 = np.ones(5000), np.array([0.0, 1.0, 0.0])
    bad_f = np.array([0.0, np.nan, 0.0])
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    tp, dp, jp = vp(taps), vp(d_obs), C.byref(J)

    def call(d=dp, t=None, R=0, L=1, mu=1.0, f=None, j=jp, c=ctx):
        return lib.fwi_misfit_matched(c, d, None, t, R, L, mu, f, None, None, j)

    assert call(c=None) == EINVAL
    with Engine(SHAPE, H, _dt(SHAPE), NT, order=ORDER, npml=NPML, dtype=dtype) as fresh:
        fresh.set_model(c0)
        assert call(c=fresh._c) == ESTATE  # no forward yet
        assert b"fwi_misfit_matched" in lib.fwi_last_error(fresh._c)
    e.forward(c0, src, rec, save=True)
    for kw in (dict(j=None), dict(d=None), dict(L=-1), dict(L=65), dict(mu=-1.0), dict(mu=float("nan")),
               dict(mu=float("inf")), dict(f=vp(bad_f)), dict(t=tp, R=4097), dict(t=tp, R=-1), dict(t=None, R=3)):
        assert call(**kw) == EINVAL, kw
        assert b"fwi_misfit_matched" in lib.fwi_last_error(ctx)
    assert call(t=tp, R=4096, L=64) == 0 and J.value >= 0.0  # R > nt and L > nt: harmless
    assert call(f=vp(f3), mu=0.0) == 0
    e.adjoint(None)
    assert call() == ESTATE  # the synthetics are gone
    with pytest.raises(FwiError) as ei:
        e.misfit_matched(d_obs, 1, 1.0)
    assert ei.value.code == ESTATE
    e.forward(c0, src, rec, save=True)
    e.born(np.ones(SHAPE, dtype), download=False)
    assert call() == ESTATE  # ... after a Born sweep as well
    e.forward(c0, src, rec, save=True)
    for bad in (dict(weights=np.ones((NT, 4))), dict(f=np.ones(2)), dict(taps=np.ones((2, 2)))):
        with pytest.raises(ValueError):
            e.misfit_matched(d_obs, 1, 1.0, **bad)
    with pytest.raises(ValueError):
        e.misfit_matched(d_obs[:, :4], 1, 1.0)
    with pytest.raises(FwiError) as ei:
        e.misfit_matched(d_obs, 65, 1.0)
    assert ei.value.code == EINVAL
    out = e.misfit_matched(d_obs, 1, 1.0)
    assert len(out) == 2 and out[1].shape == (3,) and len(e.misfit_matched(d_obs, 1, 1.0, normal=True)) == 4
    assert "fwi_misfit_matched" in _lib.SIGNATURES and lib.fwi_abi_version() == 14


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_matrix_that_is_not_positive_definite_is_refused_and_a_larger_mu_succeeds(engines, dtype):
    """A zero wavelet gives zero synthetics: G = 0, b = 0.  mu = 0 is FWI_EINVAL naming the call and leaves no residual;
    the forward's synthetics remain, and mu = 1 on the same forward returns f = 0 and J = 1/2 sum (M d')^2."""
    e = engines(dtype)
    lib, ctx = e._lib, e._c
    src, rec, d_obs, _ = _data(e, dtype, NT, 5)
    _, c0 = _models(SHAPE)
    M = _weights(NT, 5).astype(dtype)
    d = e.forward(c0, (src[0], np.zeros(NT)), rec, save=True)
    assert not np.any(d)
    with pytest.raises(FwiError) as ei:
        e.misfit_matched(d_obs, 2, 0.0, M)
    assert ei.value.code == EINVAL and "fwi_misfit_matched" in str(ei.value) and "raise mu" in str(ei.value)
    assert b"fwi_misfit_matched" in lib.fwi_last_error(ctx)
    with pytest.raises(FwiError) as ei:
        e.adjoint(None)  # no residual was left
    assert ei.value.code == EINVAL
    J, f, G, b = e.misfit_matched(d_obs, 2, 1.0, M, normal=True)
    md = np.asarray(M, np.float64) * np.asarray(d_obs, np.float64)
    Jt = 0.5 * float(np.sum(md * md))
    print("J", J, "twin", Jt)
    assert not np.any(f) and not np.any(G) and not np.any(b)
    assert Jt > 0.0 and abs(J - Jt) <= d_obs.size * U2 * Jt
    e.adjoint(None)  # ... and now there is one
