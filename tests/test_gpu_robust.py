"""The robust (Huber, hybrid L1/L2, Cauchy) misfits, their IRLS Gauss-Newton weight and the median of |e| on the GPU
(include/fwi.h fwi_misfit_robust, fwi_residual_weight_robust, fwi_residual_median; csrc/fwi_robust.hip).  The oracle is
the fp64 NumPy twin (datafit.RobustMisfit, datafit.median_abs) fed the engine's own downloaded synthetics, and d_obs and
the weights rounded to the engine's dtype; with dtype= it rounds e and g to that dtype where the device does.

Inputs: the set-up of tests/test_gpu_awi.py.  A 2-D (24, 28) grid, order 4, npml 4; the receivers are the nodes nearest
the source.  d_obs is the synthetics of the starting model plus noise of 1 % of each trace's largest amplitude plus
sparse spikes (3 % of the samples, 20 to 40 times the noise).  The thresholds are datafit.mad_scale of the twin's e per
trace (c = 1: a Gaussian residual puts about a third of its samples beyond it, so that both branches of every kind run).

Conditions, asserted on the TWIN before the device is compared (conditions on the inputs, not tolerances): between 5 %
and 50 % of the counted samples lie beyond their threshold, and no |e| lies within max(4 u_T a_j, the bound on de) of
a_j, so that nout must agree exactly.

Bounds (tests/_robust.py, with the derivation): J and J_trace within (nt + 2) 2^-52 times their terms plus
sum tw (|psi e| |de| + de^2 / 2); nothing in them comes from the device.  The adjoint source g stays on the device (there
is no call that downloads it): its per-sample bound tw (|de| + (u_T + 8 u) |e|) is printed relative to |g|, and g and
r = B (M . g) are checked through the gradient that adjoint(None) forms from r, against the gradient of the twin's r
handed to adjoint(), relative L2, to GRAD_TOL of tests/test_gpu_correlation.py in both dtypes.

Bit for bit: huber at a = inf with tw = 1 against misfit_weighted on the same forward -- the gradient (hence r) in every
option combination and both dtypes; J where misfit_weighted sums its J from e as stored (fp64, or fp32 without taps and
weights), and within the rounding of e otherwise, since there misfit_weighted sums the UNROUNDED e and the definition of
the robust misfits rounds e first (include/fwi.h); d_obs == d_syn gives J == 0 and an all-zero gradient; the median and
its count without taps and with weights in {0, 1}, where e is exact on both sides, for both segmentations.  With taps
the median is compared by rank: it must lie between the twin's order statistics k - 1 and k + 1.

Shapes.  ntr in {1, 5, 63, 65, 130} (either side of a 64-trace tile, three tiles), nt in {33, 37, 70}."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from _robust import UNIT, roundoff_bounds  # noqa: E402
from full_waveform_inversion_amd import Engine, FwiError, _lib, datafit as df, shots as sh  # noqa: E402
from oracle import fwi_oracle as fo  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPE, H, ORDER, NPML, NT_MAX = (24, 28), 10.0, 4, 4, 70
SRC = (12, 9)
DTYPES = ["float32", "float64"]
KINDS = list(df.ROBUST_KINDS)
ESTATE, EINVAL = 3, 1
GRAD_TOL = {"float32": 1e-5, "float64": 1e-5 * 2.0 ** -29}  # tests/test_gpu_correlation.py
TAPS_R = 7
WORST = {}  # the largest observed error / bound per quantity, printed by every comparison


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _c0(shape=SHAPE, seed=0):
    return 2000.0 + 300.0 * np.random.default_rng(seed).random(shape)


def _dt(shape=SHAPE, order=ORDER):
    return 0.6 * fo.cfl_dt(2300.0, H, len(shape), order)


def _nodes(ntr, shape=SHAPE, src=SRC, npml=NPML):
    """the ntr interior nodes nearest the source (the source's own node first)"""
    grids = np.meshgrid(*[np.arange(npml, n - npml) for n in shape], indexing="ij")
    allnodes = np.stack([g.ravel() for g in grids], 1)
    d2 = np.sum((allnodes - np.array(src)) ** 2, axis=1)
    return np.ascontiguousarray(allnodes[np.argsort(d2, kind="stable")[:ntr]], dtype=np.int32)


def _weights(nt, ntr, seed=2):
    M = 0.25 + 0.75 * np.random.default_rng(seed).random((nt, ntr))
    M[nt // 3] = 0.0  # one dead time row
    return M


def _mask(nt, ntr, seed=3):
    M = (np.random.default_rng(seed).random((nt, ntr)) < 0.8).astype(np.float64)  # weights in {0, 1}
    M[nt // 3] = 0.0
    return M


def _trace_weights(ntr, seed=4):
    w = 0.25 + np.random.default_rng(seed).random(ntr)
    if ntr > 1:
        w[ntr // 3] = 0.0  # one trace that counts but adds nothing
    return w


def observed(d_syn, dtype, seed=6):
    """d_obs = d_syn + 1 % noise + sparse spikes"""
    rng = np.random.default_rng(seed)
    d = np.asarray(d_syn, np.float64)
    amp = 0.01 * np.max(np.abs(d), axis=0)
    noise = rng.standard_normal(d.shape)
    spikes = (rng.random(d.shape) < 0.03) * rng.uniform(20.0, 40.0, d.shape) * rng.choice([-1.0, 1.0], d.shape)
    return np.ascontiguousarray((d + amp * (noise + spikes)).astype(dtype))


_ENGINES = {}


@pytest.fixture(scope="module")
def engines(gpu):
    """one 2-D context per dtype for the whole module"""
    def get(dtype):
        if dtype not in _ENGINES:
            _ENGINES[dtype] = Engine(SHAPE, H, _dt(), NT_MAX, order=ORDER, npml=NPML, dtype=dtype)
        return _ENGINES[dtype]
    yield get
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


_DATA = {}


def _shot(e, dtype, nt, ntr):
    """the 2-D shot and the synthetics of the starting model; computed once per key and never written to"""
    key = (dtype, nt, ntr)
    if key not in _DATA:
        s = sh.Shot(np.array([SRC], np.int32), fo.ricker(nt, _dt(), 60.0), _nodes(ntr))
        d_syn = e.forward(_c0(), (s.src_idx, s.wavelet), s.rec_idx, save=True)
        d_syn.setflags(write=False)
        _DATA[key] = (s, d_syn)
    return _DATA[key]


def _inputs(dtype, nt, ntr, flags):
    weighted, with_taps, trace_weighted = flags
    taps = df.bandpass_taps(_dt(), 8.0, 90.0, TAPS_R) if with_taps else None
    M = _weights(nt, ntr).astype(dtype) if weighted else None
    return M, taps, (_trace_weights(ntr) if trace_weighted else None)


def _thresholds(obj, d_syn, d_obs, M):
    """a_j = mad_scale of the twin's e per trace"""
    a = df.mad_scale(obj.residuals(d_syn, d_obs, M)[0], M)
    assert np.all(a > 0.0) and np.all(np.isfinite(a))
    return a


class _Run:
    pass


def _compare(e, dtype, shot, d_obs, c0, M, taps, tw, kind, thresh=None):
    """One device call and the twin's answer to the same inputs, with both gradients and the bounds"""
    r = _Run()
    e.set_model(c0)
    d_syn = shot.forward(e, save=True)
    r.nt, r.ntr = d_syn.shape
    obj = df.RobustMisfit(kind, taps=taps, dtype=dtype)
    r.a = _thresholds(obj, d_syn, d_obs, M) if thresh is None else thresh
    e.reset_gradient()
    r.J, r.J_trace, r.nout = e.misfit_robust(d_obs, kind, r.a, M, taps, tw, per_trace=True)
    e.adjoint(None)
    r.g = e.gradient()
    r.Jt, r.rt = obj(d_syn, d_obs, M, tw, thresh=r.a)
    r.J_trace_t, r.nout_t = obj.J_trace, obj.nout
    r.b = roundoff_bounds(obj, d_syn, d_obs, M, tw, r.a, dtype)
    if np.any(r.rt):
        shot.forward(e, save=True)
        e.reset_gradient()
        shot.adjoint(e, r.rt.astype(dtype))
        r.gt = e.gradient()
    else:
        r.gt = np.zeros_like(r.g)
    return r


def _conditions(r):
    """the conditions on the inputs of the module's docstring, on the twin's values"""
    frac = float(np.sum(r.b.beyond)) / float(np.sum(r.b.counted))
    print("beyond the threshold: %.3f of %d counted samples; margin of the nearest |e| %.3g" %
          (frac, int(np.sum(r.b.counted)), r.b.margin))
    assert 0.05 <= frac <= 0.50
    assert r.b.margin > 0.0


def _ratio(name, err, bound):
    worst = float(np.max(np.asarray(err) / np.where(np.asarray(bound) > 0.0, bound, 1.0))) if np.size(err) else 0.0
    WORST[name] = max(WORST.get(name, 0.0), worst)
    return worst


def _check(r, dtype):
    """the assertions of the module's docstring; prints what it measured first"""
    gt = np.abs(r.b.tw * r.b.psi * r.b.e)
    ratios = (_ratio("J", abs(r.J - r.Jt), r.b.J), _ratio("J_trace", np.abs(r.J_trace - r.J_trace_t), r.b.J_trace),
              _ratio("gradient_" + dtype, rel(r.g, r.gt), GRAD_TOL[dtype]))
    print("J", r.J, "twin", r.Jt, "|J - J_t|", abs(r.J - r.Jt), "bound", r.b.J, "error / bound: J %.3g J_trace %.3g "
          "gradient %.3g" % ratios, "gradient rel L2", rel(r.g, r.gt), "bound", GRAD_TOL[dtype],
          "bound on g / |g|", float(np.linalg.norm(r.b.g) / max(np.linalg.norm(gt), 1e-300)), "worst so far", WORST)
    assert r.Jt > 0.0 and np.all(np.isfinite(r.g)) and np.any(r.gt != 0.0)
    assert r.nout.dtype == np.int32 and np.array_equal(r.nout, r.nout_t)
    assert abs(r.J - r.Jt) <= r.b.J
    assert np.all(np.abs(r.J_trace - r.J_trace_t) <= r.b.J_trace)
    assert rel(r.g, r.gt) <= GRAD_TOL[dtype]


SIZES = [(70, n) for n in (1, 5, 63, 65, 130)] + [(nt, n) for nt in (33, 37) for n in (65, 130)]
FLAGS = [(wt, tp, tw) for wt in (False, True) for tp in (False, True) for tw in (False, True)]
NONE_ON, ALL_ON = (False, False, False), (True, True, True)


def _cases():
    out = [(k, s, f) for k in KINDS for s in SIZES for f in (NONE_ON, ALL_ON)]
    out += [(k, (70, 130), f) for k in KINDS for f in FLAGS]
    out += [(k, (37, 65), f) for k in KINDS for f in ((True, False, False), (False, True, False), (False, False, True))]
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return uniq


def _id(kind, size, flags):
    return "%s_nt%d_ntr%d_%s%s%s" % ((kind,) + size + tuple(c if f else "-" for c, f in zip("MBw", flags)))


CASES = _cases()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES, ids=[_id(*c) for c in CASES])
def test_misfit_and_gradient_against_the_twin(engines, dtype, case):
    kind, (nt, ntr), flags = case
    e = engines(dtype)
    shot, d_syn = _shot(e, dtype, nt, ntr)
    M, taps, tw = _inputs(dtype, nt, ntr, flags)
    r = _compare(e, dtype, shot, observed(d_syn, dtype), _c0(), M, taps, tw, kind)
    _conditions(r)
    _check(r, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_off_grid_receivers(engines, dtype, kind):
    e = engines(dtype)
    nt = 40
    c0 = _c0().astype(dtype)
    rng = np.random.default_rng(11)
    src = np.array(SRC, np.float64) + 0.3
    rec = src + rng.uniform(-3.0, 3.0, (9, 2))
    s = sh.Shot.at_coordinates([src], fo.ricker(nt, _dt(), 60.0).astype(dtype), rec, SHAPE)
    sh.model_data(e, c0, [s])  # the synthetics of the starting model, per point
    assert s._on_device(e) and s.d_obs.shape == (nt, 9)
    d_obs = observed(s.d_obs, dtype)
    taps = df.bandpass_taps(_dt(), 8.0, 90.0, TAPS_R)
    r = _compare(e, dtype, s, d_obs, c0, _weights(nt, 9).astype(dtype), taps, _trace_weights(9), kind)
    assert r.J_trace.shape == (9,) and r.nout.shape == (9,)  # ntr is the number of points
    _conditions(r)
    _check(r, dtype)
    # the median per point, by rank (taps), and exact without them
    s.forward(e, save=True)
    med, count = e.residual_median(d_obs, None, None)
    med_t, count_t = df.median_abs(df.RobustMisfit(dtype=dtype).residuals(s.d_obs, d_obs)[0].astype(dtype))
    assert np.array_equal(med, med_t) and np.array_equal(count, count_t) and np.all(med > 0.0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("flags", [NONE_ON, (True, False, False), (False, True, False), (True, True, False)],
                         ids=["---", "M--", "-B-", "MB-"])
def test_huber_at_an_infinite_threshold_is_misfit_weighted(engines, dtype, flags):
    """r (through the gradient) bit for bit in every combination; J bit for bit where misfit_weighted sums it from e as
    stored, and within the rounding of e where it sums the unrounded e (fp32 with taps or weights: 2 u_T relative for
    the squares of e, plus the sums' (nt + 2) 2^-52)"""
    e = engines(dtype)
    nt, ntr = 70, 130
    shot, d_syn = _shot(e, dtype, nt, ntr)
    M, taps, _ = _inputs(dtype, nt, ntr, flags)
    d_obs = observed(d_syn, dtype)
    c0 = _c0()
    out = {}
    for name in ("weighted", "robust", "robust_ones"):
        e.set_model(c0)
        shot.forward(e, save=True)
        e.reset_gradient()
        if name == "weighted":
            J = e.misfit_weighted(d_obs, M, taps)
        else:
            J = e.misfit_robust(d_obs, "huber", np.inf, M, taps, None if name == "robust" else np.ones(ntr))
        e.adjoint(None)
        out[name] = (J, e.gradient())
    (Jw, gw), (Jr, gr), (Jo, go) = out["weighted"], out["robust"], out["robust_ones"]
    stored = dtype == "float64" or flags == NONE_ON
    print("J weighted", Jw, "robust", Jr, "difference", Jr - Jw, "summed from e as stored:", stored)
    assert Jw > 0.0 and np.any(gw != 0.0)
    assert np.array_equal(gr, gw) and np.array_equal(go, gw) and Jo == Jr
    if stored:
        assert Jr == Jw
    else:
        assert abs(Jr - Jw) <= (2.0 * UNIT[dtype] * (1.0 + UNIT[dtype]) + (nt + 2) * 2.0 ** -52) * Jw


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_equal_data_give_exact_zeros(engines, dtype, kind):
    e = engines(dtype)
    nt, ntr = 70, 65
    shot, d_syn = _shot(e, dtype, nt, ntr)
    M, taps, tw = _inputs(dtype, nt, ntr, ALL_ON)
    for args in ((None, None, None), (M, taps, tw)):
        e.set_model(_c0())
        d = shot.forward(e, save=True)
        e.reset_gradient()
        J, J_trace, nout = e.misfit_robust(d, kind, 1e-3, *args, per_trace=True)
        e.adjoint(None)
        assert J == 0.0 and not np.any(J_trace) and not np.any(nout) and not np.any(e.gradient())


def _median_inputs(dtype, nt, ntr, weighted):
    return _mask(nt, ntr).astype(dtype) if weighted else None


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("weighted", [False, True], ids=["all", "mask"])
@pytest.mark.parametrize("size", SIZES, ids=["nt%d_ntr%d" % s for s in SIZES])
def test_residual_median_is_the_exact_order_statistic(engines, dtype, size, weighted):
    """without taps and with weights in {0, 1} e is exact on both sides: the median and the count equal the twin's bit
    for bit, per trace and for the whole gather; nt = 33, 37 give odd counts per trace, 70 an even one, the dead row of
    the mask changes the parity; the call is repeatable and a misfit call follows on the same forward"""
    nt, ntr = size
    e = engines(dtype)
    shot, d_syn = _shot(e, dtype, nt, ntr)
    d_obs = observed(d_syn, dtype)
    M = _median_inputs(dtype, nt, ntr, weighted)
    e.set_model(_c0())
    shot.forward(e, save=True)
    et = df.RobustMisfit(dtype=dtype).residuals(d_syn, d_obs, M)[0].astype(dtype)
    med_t, count_t = df.median_abs(et, M)
    all_t = df.median_abs(et, M, per_trace=False)
    med, count = e.residual_median(d_obs, M)
    assert med.dtype == np.float64 and count.dtype == np.int64
    assert np.array_equal(count, count_t) and np.array_equal(med, med_t) and np.all(med > 0.0)
    assert e.residual_median(d_obs, M, per_trace=False) == all_t and all_t[0] > 0.0
    med2, count2 = e.residual_median(d_obs, M)
    assert np.array_equal(med, med2) and np.array_equal(count, count2)
    with pytest.raises(FwiError) as ei:
        e.adjoint(None)  # it leaves no residual on the device: fwi_adjoint's "null residual"
    assert ei.value.code == EINVAL
    assert e.misfit_robust(d_obs, "huber", df.MAD_TO_SIGMA * med) > 0.0  # the synthetics are still there
    if not weighted:
        assert set(count) == {nt}


@pytest.mark.parametrize("dtype", DTYPES)
def test_residual_median_with_ties_zeros_and_equal_traces(engines, dtype):
    """d_obs == d_syn on a third of the rows (ties at 0), on more than half of them (the median is 0), traces whose
    |e| are all equal, a trace nothing of which counts (count 0, median 0), +inf and NaN in the data (they sort last)"""
    nt, ntr = 70, 65
    e = engines(dtype)
    shot, d_syn = _shot(e, dtype, nt, ntr)
    e.set_model(_c0())
    shot.forward(e, save=True)
    twin = df.RobustMisfit(dtype=dtype)
    d_obs = observed(d_syn, dtype)
    d_obs[::3] = d_syn[::3]
    d_obs[:, 7] = d_syn[:, 7]
    d_obs[: nt // 2 + 3, 9] = d_syn[: nt // 2 + 3, 9]
    # (a non-finite sample makes the device's e non-finite over its aligned group of 8 times, 0 * inf in the pass that
    # forms e: a whole group is filled, so that both sides put the same eight samples last)
    d_obs[8:16, 13] = [np.inf, np.nan, -np.inf, np.inf, np.nan, -np.inf, np.inf, np.nan]
    d_obs[:, 15] = np.nan
    M = np.ones((nt, ntr), dtype)
    M[:, 17] = 0.0
    for W in (None, M):
        et = twin.residuals(d_syn, d_obs, W)[0].astype(dtype)
        med_t, count_t = df.median_abs(et, W)
        med, count = e.residual_median(d_obs, W)
        assert np.array_equal(count, count_t) and np.array_equal(med, med_t, equal_nan=True)
        assert med[7] == 0.0 and med[9] == 0.0 and np.isnan(med[15]) and np.isfinite(med[13])
        all_t = df.median_abs(et, W, per_trace=False)
        got = e.residual_median(d_obs, W, per_trace=False)
        assert got == all_t and np.isfinite(got[0])
    assert count[17] == 0 and med[17] == 0.0
    # all-equal traces: a wavelet of zeros gives d_syn = 0, so that |e| = |d_obs| exactly
    dead = sh.Shot(shot.src_idx, 0.0 * shot.wavelet, shot.rec_idx)
    assert not np.any(dead.forward(e, save=True))
    d_all = np.where(np.arange(nt)[:, None] % 2, 0.125, -0.125).astype(dtype) * np.ones((1, ntr), dtype)
    d_all[:, 3] *= 3.0
    med, count = e.residual_median(d_all)
    assert np.array_equal(med, np.where(np.arange(ntr) == 3, 0.375, 0.125)) and set(count) == {nt}
    assert e.residual_median(d_all, per_trace=False) == (0.125, nt * ntr)
    shot.forward(e, save=True)
    # nothing counts at all
    med, count = e.residual_median(d_obs, np.zeros((nt, ntr), dtype))
    assert not np.any(med) and not np.any(count)
    assert e.residual_median(d_obs, np.zeros((nt, ntr), dtype), per_trace=False) == (0.0, 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("size", [(70, 130), (37, 65), (33, 5)], ids=["nt70_ntr130", "nt37_ntr65", "nt33_ntr5"])
def test_residual_median_with_taps_by_rank(engines, dtype, size):
    nt, ntr = size
    e = engines(dtype)
    shot, d_syn = _shot(e, dtype, nt, ntr)
    d_obs = observed(d_syn, dtype)
    M, taps, _ = _inputs(dtype, nt, ntr, ALL_ON)
    e.set_model(_c0())
    shot.forward(e, save=True)
    et = np.abs(df.RobustMisfit(taps=taps, dtype=dtype).residuals(d_syn, d_obs, M)[0])
    med, count = e.residual_median(d_obs, M, taps)
    keep = M > 0
    assert np.array_equal(count, np.sum(keep, axis=0))
    for j in range(ntr):
        s = np.sort(et[keep[:, j], j])
        k = (len(s) - 1) // 2
        assert s[max(k - 1, 0)] <= med[j] <= s[min(k + 1, len(s) - 1)], j
    s = np.sort(et[keep])
    k = (len(s) - 1) // 2
    m_all, c_all = e.residual_median(d_obs, M, taps, per_trace=False)
    assert c_all == len(s) and s[k - 1] <= m_all <= s[k + 1]


class _HostOnly:
    """the engine without its device misfit, median and weighting: the shot loop then takes the twin"""

    def __init__(self, e):
        self._e = e

    def __getattr__(self, name):
        if name in ("misfit_robust", "residual_weight_robust", "residual_median"):
            raise AttributeError(name)
        return getattr(self._e, name)


def _two_shots(e, dtype, nt=40):
    """one shot on the nodes and one off the grid, with weights and trace weights, and the data of another model plus
    noise and spikes"""
    rng = np.random.default_rng(21)
    c0 = _c0().astype(dtype)
    wav = fo.ricker(nt, _dt(), 60.0).astype(dtype)
    src = np.array(SRC, np.float64) + 0.3
    shots = [sh.Shot(np.array([SRC], np.int32), wav, _nodes(11)),
             sh.Shot.at_coordinates([src], wav, src + rng.uniform(-3.0, 3.0, (9, 2)), SHAPE)]
    sh.model_data(e, c0, shots)
    for s in shots:
        s.d_obs = observed(s.d_obs, dtype)
        s.weights = (0.25 + 0.75 * rng.random(s.d_obs.shape)).astype(dtype)
    shots[1].trace_weights = _trace_weights(9)
    return shots, c0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_gauss_newton_product_with_the_irls_weight(engines, dtype, kind):
    """gauss_newton_hvp(objective=RobustMisfit) with the weight kept and applied on the device, one shot on the nodes and
    one off the grid: symmetric, v^T H v >= 0, and the host-only path (the twin's psi and normal) to GRAD_TOL; the
    scales come from residual_scales, on the device and through the twin alike"""
    e = engines(dtype)
    shots, c0 = _two_shots(e, dtype)
    taps = df.bandpass_taps(_dt(), 8.0, 90.0, TAPS_R)
    probe = df.RobustMisfit(kind, taps=taps, dtype=dtype)
    scales = sh.residual_scales(e, c0, shots, probe)
    scales_h = sh.residual_scales(_HostOnly(e), c0, shots, probe)
    assert [s.shape for s in scales] == [(11,), (9,)] and all(np.all(s > 0.0) for s in scales)
    for a, b in zip(scales, scales_h):  # (with taps e agrees to its rounding: the same order statistic but for near-ties)
        assert np.allclose(a, b, rtol=8.0 * UNIT[dtype], atol=0.0)
    obj = df.RobustMisfit(kind, c=1.0, scale=scales, taps=taps, dtype=dtype)
    rng = np.random.default_rng(33)
    v, w = (rng.standard_normal(SHAPE).astype(dtype) for _ in range(2))
    calls = []
    raw = e.residual_weight_robust
    e.residual_weight_robust = lambda *a, **k: (calls.append(1), raw(*a, **k))[1]
    try:
        Hv = sh.gauss_newton_hvp(e, c0, shots, v, objective=obj)
        Hw = sh.gauss_newton_hvp(e, c0, shots, w, objective=obj)
    finally:
        del e.residual_weight_robust
    assert len(calls) == 4
    ref = sh.gauss_newton_hvp(_HostOnly(e), c0, shots, v, objective=obj)
    plain = sh.gauss_newton_hvp(e, c0, shots, v)
    a, b = float(np.vdot(w.astype(np.float64), Hv)), float(np.vdot(v.astype(np.float64), Hw))
    vHv = float(np.vdot(v.astype(np.float64), Hv))
    print("Hv rel L2", rel(Hv, ref), "bound", GRAD_TOL[dtype], "symmetry", abs(a - b) / abs(a), "v^T H v", vHv,
          "weighted vs plain", rel(Hv, plain))
    assert rel(Hv, plain) > 0.1  # the weight is not a no-op
    assert vHv >= 0.0
    assert abs(a - b) <= (1e-5 if dtype == "float32" else 1e-11) * abs(a)
    assert rel(Hv, ref) <= GRAD_TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_shot_loop_device_branch_against_the_host_objective_path(engines, dtype):
    """misfit_and_gradient takes the device path once per shot and returns the bits of the same calls made by hand; the
    host-objective path (device_l2=False) agrees within the shots' bounds on J and GRAD_TOL"""
    e = engines(dtype)
    shots, c0 = _two_shots(e, dtype)
    taps = df.bandpass_taps(_dt(), 8.0, 90.0, TAPS_R)
    obj = df.RobustMisfit("hybrid", scale=sh.residual_scales(e, c0, shots, df.RobustMisfit(taps=taps)), taps=taps,
                          dtype=dtype)
    calls = []
    raw = e.misfit_robust
    e.misfit_robust = lambda *a, **k: (calls.append(1), raw(*a, **k))[1]
    try:
        Jd, gd = sh.misfit_and_gradient(e, c0, shots, objective=obj)
    finally:
        del e.misfit_robust
    assert len(calls) == 2
    e.set_model(c0)
    e.reset_gradient()
    Js, Jb = 0.0, 0.0
    for i, s in enumerate(shots):
        d = s.forward(e, save=True)
        a = obj.thresh_of(i, s.d_obs, s.weights)
        Js += e.misfit_robust(s.d_obs, "hybrid", a, s.weights, taps, s.trace_weights)
        e.adjoint(None)
        Jb += roundoff_bounds(obj, d, s.d_obs, s.weights, s.trace_weights, a, dtype).J
    assert Jd > 0.0 and Jd == Js and np.any(gd != 0.0) and np.array_equal(gd, e.gradient())
    Jh, gh = sh.misfit_and_gradient(e, c0, shots, objective=obj, device_l2=False)
    print("J device", Jd, "host", Jh, "|dJ|", abs(Jd - Jh), "bound", Jb, "gradient rel L2", rel(gd, gh))
    assert abs(Jd - Jh) <= Jb and rel(gd, gh) <= GRAD_TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_state_and_argument_errors(engines, dtype):
    e = engines(dtype)
    lib, ctx = e._lib, e._c
    nt = 40
    shot, d_syn = _shot(e, dtype, nt, 5)
    d_obs = observed(d_syn, dtype)
    src, rec, c0 = (shot.src_idx, shot.wavelet), shot.rec_idx, _c0()
    J = C.c_double(-1.0)
    taps = np.ones(5000)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    ok_a = np.full(5, 1e-3)
    bad_tw = [np.array([1.0, 1.0, -0.5, 1.0, 1.0]), np.array([1.0, np.nan, 1.0, 1.0, 1.0]),
              np.array([1.0, 1.0, 1.0, 1.0, np.inf])]
    bad_a = [np.array([1.0, 0.0, 1.0, 1.0, 1.0]), np.array([1.0, 1.0, -1.0, 1.0, 1.0]),
             np.array([1.0, 1.0, 1.0, np.nan, 1.0])]
    inf_a = np.array([1.0, 1.0, 1.0, 1.0, np.inf])
    tp, dp, jp = vp(taps), vp(d_obs), C.byref(J)
    med, cnt = np.zeros(5), np.zeros(5, np.int64)

    def call(d=dp, t=None, R=0, kind=0, a=vp(ok_a), tw=None, keep=0, j=jp, c=ctx):
        return lib.fwi_misfit_robust(c, d, None, t, R, kind, a, tw, keep, None, None, j)

    def median(d=dp, t=None, R=0, seg=0, m=vp(med), n=vp(cnt), c=ctx):
        return lib.fwi_residual_median(c, d, None, t, R, seg, m, n)

    assert call(c=None) == EINVAL and median(c=None) == EINVAL and lib.fwi_residual_weight_robust(None, None, 0) == EINVAL
    with Engine(SHAPE, H, _dt(), nt, order=ORDER, npml=NPML, dtype=dtype) as fresh:
        fresh.set_model(c0)
        assert call(c=fresh._c) == ESTATE and median(c=fresh._c) == ESTATE  # no forward yet
        assert b"fwi_residual_median" in lib.fwi_last_error(fresh._c)
        assert lib.fwi_residual_weight_robust(fresh._c, None, 0) == ESTATE
    e.forward(c0, src, rec, save=True)
    for kw in (dict(j=None), dict(d=None), dict(kind=3), dict(kind=-1), dict(a=None), dict(a=vp(bad_a[0])),
               dict(a=vp(bad_a[1])), dict(a=vp(bad_a[2])), dict(a=vp(inf_a), kind=1), dict(a=vp(inf_a), kind=2),
               dict(t=tp, R=4097), dict(t=tp, R=-1), dict(t=None, R=3), dict(tw=vp(bad_tw[0])), dict(tw=vp(bad_tw[1])),
               dict(tw=vp(bad_tw[2]))):
        assert call(**kw) == EINVAL, kw
        assert b"fwi_misfit_robust" in lib.fwi_last_error(ctx), kw
    for kw in (dict(d=None), dict(m=None), dict(n=None), dict(seg=2), dict(seg=-1), dict(t=tp, R=4097), dict(t=None, R=3)):
        assert median(**kw) == EINVAL, kw
        assert b"fwi_residual_median" in lib.fwi_last_error(ctx), kw
    # after the refused calls the forward's synthetics are still usable
    assert call(a=vp(inf_a)) == 0 and J.value > 0.0  # huber takes +inf
    J_inf = e.misfit_robust(d_obs, "huber", inf_a)
    assert call(t=tp, R=4096) == 0 and np.isfinite(J.value)  # R > nt: harmless
    assert median() == 0 and np.all(med > 0.0) and set(cnt) == {nt}
    # the IRLS weight: none kept yet; kept, it needs a residual; a new forward drops it
    assert call() == 0
    assert lib.fwi_residual_weight_robust(ctx, None, 0) == ESTATE
    assert b"fwi_residual_weight_robust" in lib.fwi_last_error(ctx)
    assert call(keep=1) == 0
    for R, t in ((4097, tp), (-1, tp), (2, None)):
        assert lib.fwi_residual_weight_robust(ctx, t, R) == EINVAL
    assert lib.fwi_residual_weight_robust(ctx, None, 0) == 0  # the misfit's own residual is one
    assert median() == 0  # ... which the median gives up, keeping W
    assert lib.fwi_residual_weight_robust(ctx, None, 0) == ESTATE
    assert call(keep=1) == 0 and call(keep=0) == 0  # a call that keeps none drops the one held
    assert lib.fwi_residual_weight_robust(ctx, None, 0) == ESTATE
    assert call(keep=1) == 0
    e.forward(c0, src, rec, save=True)
    assert e.misfit_l2(d_obs) > 0.0
    assert lib.fwi_residual_weight_robust(ctx, None, 0) == ESTATE  # dropped by the forward
    with pytest.raises(FwiError) as ei:
        e.residual_weight_robust()
    assert ei.value.code == ESTATE
    e.adjoint(None)
    assert call() == ESTATE and median() == ESTATE  # the synthetics are gone
    with pytest.raises(FwiError) as ei:
        e.misfit_robust(d_obs, "huber", 1.0)
    assert ei.value.code == ESTATE
    e.forward(c0, src, rec, save=True)
    e.born(np.ones(SHAPE, dtype), download=False)
    assert call() == ESTATE  # ... after a Born sweep as well
    e.forward(c0, src, rec, save=True)
    for bad in (dict(kind="l1"), dict(thresh=np.ones(4)), dict(thresh=np.ones((5, 1))), dict(weights=np.ones((nt, 4))),
                dict(taps=np.ones((2, 2))), dict(trace_weights=np.ones(4))):
        with pytest.raises(ValueError):
            e.misfit_robust(d_obs, **{"kind": "huber", "thresh": 1.0, **bad})
    for bad in (dict(thresh=0.0), dict(thresh=np.nan), dict(kind="hybrid", thresh=np.inf),
                dict(kind="cauchy", thresh=np.inf), dict(trace_weights=bad_tw[0])):
        with pytest.raises(FwiError) as ei:
            e.misfit_robust(d_obs, **{"kind": "huber", "thresh": 1.0, **bad})
        assert ei.value.code == EINVAL
    assert e.misfit_robust(d_obs, "huber", np.inf) == J_inf  # and still usable
    for name in ("fwi_misfit_robust", "fwi_residual_weight_robust", "fwi_residual_median"):
        assert name in _lib.SIGNATURES
    assert lib.fwi_abi_version() == 14
