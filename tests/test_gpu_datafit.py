"""Band-limited, weighted least squares on the GPU (include/fwi.h fwi_misfit_weighted / fwi_residual_weight,
csrc/fwi_data.hip).  The oracle is the fp64 NumPy twin (datafit.WeightedL2) fed the engine's own
downloaded synthetics and d_obs rounded to the engine's dtype.

The context keeps no accessor to the residual it leaves for fwi_adjoint(NULL): r is checked through the gradient that
adjoint(None) forms from it, against the gradient of the twin's r handed to adjoint(): the project's flat 1e-5 relative
L2 in fp32, which is 168 roundings of 2^-24, and the same 168 roundings of 2^-53 = 1.9e-14 in fp64, so that the fp64 run
pins the arithmetic (one fp32 sum or product anywhere would leave 1e-8).  The J bounds are the issue's, n 2^-52 J, J
being summed from unrounded fp64 values."""
import ctypes as C

import numpy as np
import pytest

from full_waveform_inversion_amd import Engine, FwiError, _lib, datafit as df, shots as sh
from oracle import fwi_oracle as fo

pytestmark = pytest.mark.gpu

SHAPE, H, ORDER, NPML, NT = (24, 28), 10.0, 4, 4, 40
DTYPES = ["float32", "float64"]
ESTATE, EINVAL = 3, 1
GRAD_TOL = {"float32": 1e-5, "float64": 1e-5 * 2.0 ** -29}  # 168 roundings of the dtype


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _models(shape, seed=0):
    rng = np.random.default_rng(seed)
    c_true = 2000.0 + 300.0 * rng.random(shape)
    return c_true, np.full(shape, 2150.0)


def _dt(shape, order=ORDER):
    return 0.6 * fo.cfl_dt(2300.0, H, len(shape), order)


def _nodes(ntr, shape=SHAPE, seed=1):
    """ntr distinct interior nodes"""
    rng = np.random.default_rng(seed)
    grids = np.meshgrid(*[np.arange(NPML, n - NPML) for n in shape], indexing="ij")
    allnodes = np.stack([g.ravel() for g in grids], 1)
    return np.ascontiguousarray(allnodes[rng.permutation(len(allnodes))[:ntr]], dtype=np.int32)


def _taps(R, dt):
    if R is None:
        return None
    return np.array([0.7]) if R == 0 else df.bandpass_taps(dt, 8.0, 90.0, R)


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


def _device_and_twin(e, dtype, nt, ntr, R, weighted):
    """(J, g) of the device path, (J, g) of the twin whose r is handed to adjoint()"""
    src, rec, d_obs, d_syn = _data(e, dtype, nt, ntr)
    _, c0 = _models(SHAPE)
    taps = _taps(R, _dt(SHAPE))
    M = _weights(nt, ntr).astype(dtype) if weighted else None
    obj = df.WeightedL2(taps)
    d = e.forward(c0, src, rec, save=True)
    assert np.array_equal(d, d_syn)
    e.reset_gradient()
    J = e.misfit_weighted(d_obs, M, taps)
    e.adjoint(None)
    g = e.gradient()
    Jt, rt = obj(d_syn, d_obs, M)
    e.forward(c0, src, rec, save=True)
    e.reset_gradient()
    e.adjoint(rt.astype(dtype))
    return (J, g), (Jt, e.gradient())


SHAPE_CASES = ([("ntr%d" % n, NT, n, 7, True) for n in (1, 5, 63, 65, 130)]
               + [("R%d" % R, NT, 65, R, True) for R in (0, 1, 39, 64)]
               + [("nt37", 37, 65, 7, True), ("no_weights", NT, 65, 7, False), ("no_taps", NT, 65, None, True)])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", SHAPE_CASES, ids=[c[0] for c in SHAPE_CASES])
def test_misfit_weighted_against_the_twin(engines, dtype, case):
    _, nt, ntr, R, weighted = case
    e = engines(dtype)
    (J, g), (Jt, gt) = _device_and_twin(e, dtype, nt, ntr, R, weighted)
    n = nt * ntr
    print("J", J, "twin", Jt, "rel", abs(J - Jt) / Jt, "bound", n * 2.0 ** -52, "gradient rel L2", rel(g, gt))
    assert Jt > 0.0 and np.all(np.isfinite(g))
    assert abs(J - Jt) <= n * 2.0 ** -52 * Jt
    assert rel(g, gt) <= GRAD_TOL[dtype]


_L2_PAIR = {}


def _l2_and_weighted(e, dtype):
    """(J, gradient) after misfit_l2 and after misfit_weighted(d_obs) on the same forward problem; once per dtype"""
    if dtype not in _L2_PAIR:
        src, rec, d_obs, _ = _data(e, dtype, NT, 65)
        _, c0 = _models(SHAPE)
        out = []
        for call in (e.misfit_l2, e.misfit_weighted):
            e.forward(c0, src, rec, save=True)
            e.reset_gradient()
            J = call(d_obs)
            e.adjoint(None)
            out.append((J, e.gradient()))
        _L2_PAIR[dtype] = out
    return _L2_PAIR[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_without_taps_and_weights_the_gradient_is_misfit_l2s_bit_for_bit(engines, dtype):
    """taps=None, weights=None: the residual is misfit_l2's, bit for bit (the rounded fp64 difference of two fp32 numbers
    is the correctly rounded fp32 difference), and so is the gradient adjoint(None) forms from it."""
    (_, g2), (_, gw) = _l2_and_weighted(engines(dtype), dtype)
    assert np.any(g2 != 0) and np.array_equal(gw, g2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_without_taps_and_weights_J_is_misfit_l2s(engines, dtype):
    """taps=None, weights=None: J agrees with misfit_l2's to n 2^-52 J.

    Both calls then sum the same numbers, the squares of the residual as stored (each exact in fp64 for an fp32
    residual), in different orders: two fp64 sums of n non-negative terms differ by at most 2 (n - 1) 2^-53 of the sum.
    (The sum over the UNROUNDED fp32 differences, which every call with taps or weights forms, lies 1.6e-09 relative
    away here: 2 x 2^-24 per square.)"""
    (J2, _), (Jw, _) = _l2_and_weighted(engines(dtype), dtype)
    n = NT * 65
    print("J misfit_l2", J2, "misfit_weighted", Jw, "rel", abs(Jw - J2) / J2, "bound", n * 2.0 ** -52)
    assert J2 > 0.0
    assert abs(Jw - J2) <= n * 2.0 ** -52 * J2


@pytest.mark.parametrize("dtype", DTYPES)
def test_without_taps_and_weights_J_against_the_twin(engines, dtype):
    """taps=None, weights=None is the one case whose J is summed from the residual as stored, x (1 + d) with |d| <= u
    (2^-24 or 2^-53), not from the unrounded differences x the twin squares: every square is off by at most 2 u + u^2
    relative, and so is their sum, on top of the n 2^-52 of the summation."""
    e = engines(dtype)
    _, (Jw, _) = _l2_and_weighted(e, dtype)
    _, _, d_obs, d_syn = _data(e, dtype, NT, 65)
    Jt, _ = df.WeightedL2(None)(d_syn, d_obs, None)
    n, u = NT * 65, 2.0 ** (-24 if dtype == "float32" else -53)
    print("J misfit_weighted", Jw, "twin", Jt, "rel", abs(Jw - Jt) / Jt, "bound", 2 * u + u * u + n * 2.0 ** -52)
    assert Jt > 0.0
    assert abs(Jw - Jt) <= (2 * u + u * u + n * 2.0 ** -52) * Jt


def _two_shots(e, shape, dtype, nt, rng, off_grid):
    c_true, c0 = _models(shape)
    dt = _dt(shape)
    wav = fo.ricker(nt, dt, 60.0).astype(dtype)
    nd = len(shape)
    if off_grid:
        lo, hi = NPML + 0.5, np.array(shape) - NPML - 1.5
        rec = lo + rng.random((9, nd)) * (hi - lo)
        shots = [sh.Shot.at_coordinates([lo + rng.random(nd) * (hi - lo)], wav, rec, shape) for _ in range(2)]
    else:
        rec = _nodes(11, shape)
        shots = [sh.Shot(_nodes(1, shape, seed=7 + k), wav, rec) for k in range(2)]
    sh.model_data(e, c_true.astype(dtype), shots)
    for s in shots:
        s.weights = df.offset_time_mute(s, H, dt, 2600.0, 2 * dt, 5) * (0.25 + 0.75 * rng.random(s.d_obs.shape))
    return shots, c0.astype(dtype), dt


class _HostOnly:
    """the engine without its device misfit and weighting: the shot loop then takes the twin"""

    def __init__(self, e):
        self._e = e

    def __getattr__(self, name):
        if name in ("misfit_weighted", "residual_weight"):
            raise AttributeError(name)
        return getattr(self._e, name)


E2E = [("2d", SHAPE, False), ("3d", (12, 14, 16), False), ("2d_off_grid", SHAPE, True)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", E2E, ids=[c[0] for c in E2E])
def test_end_to_end_device_path_against_the_host_path(gpu, engines, dtype, case):
    _, shape, off_grid = case
    rng = np.random.default_rng(21)
    e = engines(dtype) if shape == SHAPE else Engine(shape, H, _dt(shape), NT, order=ORDER, npml=NPML, dtype=dtype)
    try:
        shots, c0, dt = _two_shots(e, shape, dtype, NT, rng, off_grid)
        obj = df.WeightedL2(df.bandpass_taps(dt, 8.0, 90.0, 12))
        calls = []
        raw = e.misfit_weighted
        e.misfit_weighted = lambda *a, **k: (calls.append(1), raw(*a, **k))[1]
        try:
            Jd, gd = sh.misfit_and_gradient(e, c0, shots, objective=obj)
        finally:
            del e.misfit_weighted
        assert len(calls) == 2  # the device path ran, once per shot
        Jh, gh = sh.misfit_and_gradient(e, c0, shots, objective=obj, device_l2=False)
        print("J device", Jd, "host", Jh, "rel", abs(Jd - Jh) / Jh, "gradient rel L2", rel(gd, gh))
        assert Jh > 0.0
        assert abs(Jd - Jh) <= (1e-6 if dtype == "float32" else 1e-12) * Jh
        assert rel(gd, gh) <= 1e-5
    finally:
        if shape != SHAPE:
            e.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_gauss_newton_product_with_the_objectives_weight(engines, dtype):
    """gauss_newton_hvp(objective=) with residual_weight on the device, one shot on the nodes and one off the grid,
    against born -> the twin's W -> adjoint through the host; and its symmetry."""
    e = engines(dtype)
    rng = np.random.default_rng(33)
    on, c0, dt = _two_shots(e, SHAPE, dtype, NT, rng, False)
    off, _, _ = _two_shots(e, SHAPE, dtype, NT, rng, True)
    shots = [on[0], off[0]]
    obj = df.WeightedL2(df.lowpass_taps(dt, 60.0, 9))
    v, w = (rng.standard_normal(SHAPE).astype(dtype) for _ in range(2))
    calls = []
    raw = e.residual_weight
    e.residual_weight = lambda *a, **k: (calls.append(1), raw(*a, **k))[1]
    try:
        Hv = sh.gauss_newton_hvp(e, c0, shots, v, objective=obj)
        Hw = sh.gauss_newton_hvp(e, c0, shots, w, objective=obj)
    finally:
        del e.residual_weight
    assert len(calls) == 4
    ref = sh.gauss_newton_hvp(_HostOnly(e), c0, shots, v, objective=obj)
    plain = sh.gauss_newton_hvp(e, c0, shots, v)
    a, b = float(np.vdot(w.astype(np.float64), Hv)), float(np.vdot(v.astype(np.float64), Hw))
    print("Hv rel L2", rel(Hv, ref), "symmetry", abs(a - b) / abs(a), "weighted vs plain", rel(Hv, plain))
    assert rel(Hv, plain) > 0.1  # the weight is not a no-op
    assert rel(Hv, ref) <= 1e-5
    assert abs(a - b) <= (1e-5 if dtype == "float32" else 1e-11) * abs(a)


@pytest.mark.parametrize("dtype", DTYPES)
def test_state_and_argument_errors(engines, dtype):
    e = engines(dtype)
    lib, ctx = e._lib, e._c
    src, rec, d_obs, _ = _data(e, dtype, NT, 5)
    _, c0 = _models(SHAPE)
    J = C.c_double(-1.0)
    taps = np.ones(5000)
    tp, dp = taps.ctypes.data_as(C.c_void_p), d_obs.ctypes.data_as(C.c_void_p)
    assert lib.fwi_misfit_weighted(None, dp, None, None, 0, C.byref(J)) == EINVAL
    assert lib.fwi_residual_weight(None, None, None, 0) == EINVAL
    e.forward(c0, src, rec, save=True)
    assert lib.fwi_residual_weight(ctx, None, None, 0) == ESTATE  # no residual on the device yet
    assert b"fwi_residual_weight" in lib.fwi_last_error(ctx)
    for bad in ((dp, tp, 4097, C.byref(J)), (dp, tp, -1, C.byref(J)), (dp, None, 3, C.byref(J)), (None, tp, 3, C.byref(J)),
                (dp, tp, 3, None)):
        assert lib.fwi_misfit_weighted(ctx, bad[0], None, bad[1], bad[2], bad[3]) == EINVAL, bad[2]
        assert b"fwi_misfit_weighted" in lib.fwi_last_error(ctx)
    assert lib.fwi_misfit_weighted(ctx, dp, None, tp, 4096, C.byref(J)) == 0 and J.value >= 0.0  # R > nt: harmless
    for R, t in ((4097, tp), (-1, tp), (2, None)):
        assert lib.fwi_residual_weight(ctx, None, t, R) == EINVAL
    assert lib.fwi_residual_weight(ctx, None, tp, 4096) == 0
    e.adjoint(None)
    assert lib.fwi_misfit_weighted(ctx, dp, None, None, 0, C.byref(J)) == ESTATE  # the synthetics are gone
    assert lib.fwi_residual_weight(ctx, None, None, 0) == ESTATE                  # ... and the residual is used up
    with pytest.raises(FwiError) as ei:
        e.misfit_weighted(d_obs)
    assert ei.value.code == ESTATE
    with pytest.raises(ValueError):
        e.misfit_weighted(d_obs, weights=np.ones((NT, 4)))
    assert "fwi_misfit_weighted" in _lib.SIGNATURES and lib.fwi_abi_version() == 14


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_misfit_is_reproducible_bit_for_bit(engines, dtype):
    e = engines(dtype)
    src, rec, d_obs, _ = _data(e, dtype, NT, 130)
    _, c0 = _models(SHAPE)
    taps, M = _taps(7, _dt(SHAPE)), _weights(NT, 130)
    e.forward(c0, src, rec, save=True)
    Js = [e.misfit_weighted(d_obs, M, taps) for _ in range(3)]
    assert Js[0] > 0.0 and Js[0] == Js[1] == Js[2]
