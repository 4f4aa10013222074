"""The frequency-domain (spectral) misfit on the GPU (include/fwi.h fwi_misfit_spectral, csrc/fwi_spec.hip, DESIGN.md
s.4o).  The oracle is the fp64 NumPy twin (datafit.SpectralMisfit) fed the engine's own downloaded synthetics, and d_obs
and the weights rounded to the engine's dtype; with dtype= it rounds B s, B d (with taps) and g to that dtype where the
device does.

Bounds and conditions are those of tests/_spectral.py (its docstring derives them): J within the rounding model's bound,
phi and a of every pair within theirs, the counts equal, and the residual -- which cannot be downloaded -- through the
gradient that adjoint(None) forms from it, against the gradient of the twin's r handed to adjoint(): GRAD_TOL of
test_gpu_datafit.py plus the source's share.  The fp64 run pins the arithmetic: one fp32 operation anywhere in the path
would leave 1e-8.  Before any comparison the conditions are asserted on the twin's values: every counted pair has
|phi| <= pi - 0.2, no |S|^2 or |O|^2 lies within [eps^2 / 4, 4 eps^2], every pair counts (but for the dead traces of the
one test about them).  The receivers lie within 8.5 cells of the source, so that the wave has passed all of them within
70 steps, and the frequencies inside 20 .. 70 Hz, where the spectra of the 60 Hz wavelet's records have no notch."""
import ctypes as C

import numpy as np
import pytest

import _spectral as sp
from full_waveform_inversion_amd import Engine, FwiError, _lib, datafit as df, fourier, shots as sh
from oracle import fwi_oracle as fo

pytestmark = pytest.mark.gpu

SHAPE, H, ORDER, NPML, NT, NT_MAX, SEG = sp.SHAPE, sp.H, sp.ORDER, sp.NPML, sp.NT, sp.NT_MAX, sp.SEG
DTYPES = ["float32", "float64"]
ESTATE, EINVAL = 3, 1
GRAD_TOL = sp.GRAD_TOL


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


_ENGINES = {}


@pytest.fixture(scope="module")
def engines(gpu):
    """one 2-D context per dtype for the whole module"""
    def get(dtype):
        if dtype not in _ENGINES:
            _ENGINES[dtype] = Engine(SHAPE, H, sp.dt_of(), NT_MAX, order=ORDER, npml=NPML, dtype=dtype)
        return _ENGINES[dtype]
    yield get
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


_DATA = {}


def _shot(e, dtype, nt, ntr, scale=1.0):
    """the 2-D shot with its observed data and the synthetics of the starting model; computed once per key and never
    written to.  scale: the factor on the wavelet of the synthetics (the observed data keep theirs)"""
    key = (dtype, nt, ntr, scale)
    if key not in _DATA:
        c_true, c0 = sp.models()
        wav = fo.ricker(nt, sp.dt_of(), 60.0)
        s = sh.Shot(np.array([sp.SRC], np.int32), scale * wav, sp.receivers(ntr))
        s.d_obs = e.forward(c_true, (s.src_idx, wav), s.rec_idx, save=False)
        d_syn = e.forward(c0, (s.src_idx, s.wavelet), s.rec_idx, save=True)
        for a in (s.d_obs, d_syn):
            a.setflags(write=False)
        _DATA[key] = (s, d_syn)
    return _DATA[key]


class _Run:
    pass


def _compare(e, dtype, shot, c0, kind, f, M, taps, fw, tw, eps=None, dead=()):
    """One device call and the twin's answer to the same inputs, with both gradients, the conditions and the bounds"""
    r = _Run()
    dt = e.dt
    e.set_model(c0)
    d_syn = shot.forward(e, save=True)
    r.eps = sp.floor_of(shot.d_obs, dt, f, M) if eps is None else eps
    e.reset_gradient()
    r.J, r.phi, r.a, r.counts = e.misfit_spectral(shot.d_obs, f, kind, r.eps, M, taps, fw, tw, per_pair=True)
    e.adjoint(None)
    r.g = e.gradient()
    obj = df.SpectralMisfit(dt, f, kind, r.eps, taps, dtype=dtype, freq_weights=fw)
    r.Jt, r.rt = obj(d_syn, shot.d_obs, M, tw)
    r.obj = obj
    sp.check_conditions(obj, r.eps, dead)
    r.Jb, r.dphi, r.da, r.rerr = sp.bounds(obj, d_syn, shot.d_obs, M, tw, r.eps, dtype)
    shot.forward(e, save=True)
    e.reset_gradient()
    shot.adjoint(e, r.rt.astype(dtype))
    r.gt = e.gradient()
    return r


def _check(r, dtype):
    """the assertions of the module's docstring; prints what it measured first"""
    obj = r.obj
    gtol = GRAD_TOL[dtype] + 4.0 * r.rerr / float(np.linalg.norm(r.rt))
    ephi, ea = np.abs(r.phi - obj.phases), np.abs(r.a - obj.logamps)
    print("J", r.J, "twin", r.Jt, "|J - J_t|", abs(r.J - r.Jt), "bound", r.Jb,
          "max |phi - phi_t| / bound", float(np.max(ephi / np.where(r.dphi > 0, r.dphi, 1.0))),
          "max |a - a_t| / bound", float(np.max(ea / np.where(r.da > 0, r.da, 1.0))),
          "gradient rel L2", rel(r.g, r.gt), "bound", gtol)
    assert r.Jt > 0.0 and np.all(np.isfinite(r.g)) and np.any(r.gt != 0.0)
    assert abs(r.J - r.Jt) <= r.Jb
    assert np.array_equal(r.counts.astype(bool), obj.counts)
    assert np.all(ephi <= r.dphi) and np.all(ea <= r.da)
    assert rel(r.g, r.gt) <= gtol


CASES = sp.cases()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES, ids=[sp.case_id(c) for c in CASES])
def test_misfit_and_gradient_against_the_twin(engines, dtype, case):
    (nt, ntr), kind, F, flags = case
    e = engines(dtype)
    shot, _ = _shot(e, dtype, nt, ntr)
    M, taps, fw, tw, f = sp.inputs(dtype, nt, ntr, F, flags, e.dt)
    r = _compare(e, dtype, shot, sp.models()[1], kind, f, M, taps, fw, tw)
    assert r.eps > 0.0 and r.phi.shape == (F, ntr)
    _check(r, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", sp.KINDS)
def test_without_a_floor_against_the_twin(engines, dtype, kind):
    e = engines(dtype)
    shot, _ = _shot(e, dtype, NT, 65)
    M, taps, fw, tw, f = sp.inputs(dtype, NT, 65, 9, (True, False, True, True), e.dt)
    _check(_compare(e, dtype, shot, sp.models()[1], kind, f, M, taps, fw, tw, eps=0.0), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["phase", "log"])
def test_a_dead_trace_does_not_count(engines, dtype, kind):
    """two all-zero observed traces: exactly their F pairs do not count and they receive no adjoint source (their columns
    of phi and a are zeros); with and without a floor"""
    e = engines(dtype)
    shot0, _ = _shot(e, dtype, NT, 65)
    dead = (7, 64)
    d_obs = shot0.d_obs.copy()
    d_obs[:, dead] = 0.0
    shot = sh.Shot(shot0.src_idx, shot0.wavelet, shot0.rec_idx)
    shot.d_obs = d_obs
    M, taps, fw, tw, f = sp.inputs(dtype, NT, 65, 8, (True, True, False, True), e.dt)
    for eps in (None, 0.0):
        r = _compare(e, dtype, shot, sp.models()[1], kind, f, M, taps, fw, tw, eps=eps, dead=dead)
        assert not r.counts[:, dead].any() and r.counts.sum() == 8 * 63
        assert not np.any(r.phi[:, dead]) and not np.any(r.a[:, dead])
        _check(r, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", sp.KINDS)
def test_equal_gathers_give_exact_zeros(engines, dtype, kind):
    """d_obs == d_syn: J = 0 and a zero adjoint source exactly, for every kind (the cross term of the phase is formed from
    two rounded products), so the gradient stays exactly zero"""
    e = engines(dtype)
    shot, d_syn = _shot(e, dtype, SEG + 1, 130)
    for flags in ((True, True, True, True), (False, False, False, False)):
        M, taps, fw, tw, f = sp.inputs(dtype, SEG + 1, 130, 9, flags, e.dt)
        for eps in (0.0, sp.floor_of(d_syn, e.dt, f, M)):
            d = e.forward(sp.models()[1], (shot.src_idx, shot.wavelet), shot.rec_idx, save=True)
            assert np.array_equal(d, d_syn)
            e.reset_gradient()
            J, phi, a, counts = e.misfit_spectral(d_syn, f, kind, eps, M, taps, fw, tw, per_pair=True)
            e.adjoint(None)
            assert J == 0.0 and not np.any(phi) and not np.any(a) and counts.all() and not np.any(e.gradient())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_taps", [False, True], ids=["no_taps", "taps"])
def test_a_gain_on_the_synthetics_changes_nothing_under_phase(engines, dtype, with_taps):
    """the same shot with the wavelet times 4 and eps = 0: both runs lie within the bound of the twin, so the two values of
    J within the sum of both bounds, and the gradient within GRAD_TOL (bit equality is not demanded: fp32 denormals can
    break it); the phases of every pair within twice their bound"""
    e = engines(dtype)
    _, c0 = sp.models()
    M, taps, fw, tw, f = sp.inputs(dtype, NT, 130, 8, (True, with_taps, True, True), e.dt)
    r1, r4 = [_compare(e, dtype, _shot(e, dtype, NT, 130, scale)[0], c0, "phase", f, M, taps, fw, tw, eps=0.0)
              for scale in (1.0, 4.0)]
    print("J", r1.J, "J(4 s)", r4.J, "|dJ|", abs(r1.J - r4.J), "bound", r1.Jb + r4.Jb, "gradient rel L2", rel(r4.g, r1.g),
          "bound", GRAD_TOL[dtype])
    assert r1.J > 0.0 and np.any(r1.g != 0.0)
    assert abs(r1.J - r4.J) <= r1.Jb + r4.Jb
    assert np.all(np.abs(r1.phi - r4.phi) <= r1.dphi + r4.dphi)
    assert rel(r4.g, r1.g) <= GRAD_TOL[dtype] + 4.0 * (r1.rerr + r4.rerr) / float(np.linalg.norm(r1.rt))


def test_a_3d_context_with_65_receivers(gpu):
    shape, dtype, src = (12, 12, 12), "float32", (6, 5, 6)
    c_true, c0 = sp.models(shape)
    dt = sp.dt_of(shape)
    with Engine(shape, H, dt, NT, order=ORDER, npml=2, dtype=dtype) as e:
        rec = sp.receivers(65, shape, src, seed=3, rmin=1.0, rmax=3.5)
        s = sh.Shot(np.array([src], np.int32), fo.ricker(NT, dt, 60.0), rec)
        s.d_obs = e.forward(c_true, (s.src_idx, s.wavelet), s.rec_idx, save=False)
        for kind, flags in (("log", (True, False, True, True)), ("l2", (True, True, False, False))):
            M, taps, fw, tw, f = sp.inputs(dtype, NT, 65, 8, flags, dt)
            _check(_compare(e, dtype, s, c0, kind, f, M, taps, fw, tw), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_off_grid_receivers(engines, dtype):
    e = engines(dtype)
    c_true, c0 = sp.models()
    rng = np.random.default_rng(11)
    ang, rad = 2.0 * np.pi * rng.random(9), 2.5 + 5.0 * rng.random(9)
    rec = np.array(sp.SRC) + 0.3 + np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
    s = sh.Shot.at_coordinates([np.array(sp.SRC) + 0.4], fo.ricker(NT, e.dt, 60.0).astype(dtype), rec, SHAPE)
    sh.model_data(e, c_true.astype(dtype), [s])
    assert s._on_device(e) and s.d_obs.shape == (NT, 9)
    for kind, flags in (("log", (True, True, True, True)), ("phase", (False, False, False, False))):
        M, taps, fw, tw, f = sp.inputs(dtype, NT, 9, 3, flags, e.dt)
        r = _compare(e, dtype, s, c0.astype(dtype), kind, f, M, taps, fw, tw)
        assert r.phi.shape == (3, 9)  # ntr is the number of points
        _check(r, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_call_is_reproducible_bit_for_bit_and_leaves_the_synthetics_alone(engines, dtype):
    e = engines(dtype)
    shot, d_syn = _shot(e, dtype, 2 * SEG + 5, 65)
    _, c0 = sp.models()
    M, taps, fw, tw, f = sp.inputs(dtype, 2 * SEG + 5, 65, 9, (True, True, True, True), e.dt)
    f2 = f[:3].copy()
    out = []
    for _ in range(2):
        d = e.forward(c0, (shot.src_idx, shot.wavelet), shot.rec_idx, save=True)
        assert np.array_equal(d, d_syn)  # what forward returned is the caller's, and the same again
        e.reset_gradient()
        first = e.misfit_spectral(shot.d_obs, f, "log", 1e-3, M, taps, fw, tw, per_pair=True)
        e.misfit_spectral(shot.d_obs, f2, "l2", 0.0)  # other frequencies in between: the table is rebuilt, twice
        again = e.misfit_spectral(shot.d_obs, f, "log", 1e-3, M, taps, fw, tw, per_pair=True)  # the synthetics are still there
        assert all(np.array_equal(x, y) for x, y in zip(first, again))
        e.adjoint(None)
        out.append(first + (e.gradient(),))
    assert out[0][0] > 0.0 and np.any(out[0][4] != 0.0)
    assert all(np.array_equal(x, y) for x, y in zip(out[0], out[1]))
    e.forward(c0, (shot.src_idx, shot.wavelet), shot.rec_idx, save=True)
    assert e.misfit_spectral(shot.d_obs, f, "log", 1e-3, M, taps, fw, tw) == out[0][0]  # per_pair=False returns J alone


@pytest.mark.parametrize("dtype", DTYPES)
def test_state_and_argument_errors(engines, dtype):
    e = engines(dtype)
    lib, ctx = e._lib, e._c
    shot, _ = _shot(e, dtype, NT, 5)
    d_obs, src, rec = shot.d_obs, (shot.src_idx, shot.wavelet), shot.rec_idx
    _, c0 = sp.models()
    J = C.c_double(-1.0)
    taps = np.ones(5000)
    nyq = 0.5 / e.dt
    vp = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(C.c_void_p)  # noqa: E731
    keep = {k: np.ascontiguousarray(v, np.float64) for k, v in dict(
        ok=[30.0, 40.0], neg=[30.0, -1.0], nan=[np.nan, 40.0], inf=[30.0, np.inf], same=[30.0, 30.0], high=[30.0, nyq * 1.001],
        dc=[0.0, 40.0], nyq=[30.0, nyq], many=np.linspace(1.0, 65.0, 65), w_neg=[1.0, -0.5], w_nan=[np.nan, 1.0],
        tw_neg=[1.0, 1.0, -0.5, 1.0, 1.0], tw_inf=[1.0, 1.0, 1.0, 1.0, np.inf]).items()}
    ptr = {k: v.ctypes.data_as(C.c_void_p) for k, v in keep.items()}
    tp, dp, jp = vp(taps), d_obs.ctypes.data_as(C.c_void_p), C.byref(J)

    def call(d=dp, t=None, R=0, F=2, f="ok", kind=0, eps=0.0, fw=None, tw=None, j=jp, c=ctx):
        return lib.fwi_misfit_spectral(c, d, None, t, R, F, ptr[f] if f else None, kind, eps, ptr[fw] if fw else None,
                                       ptr[tw] if tw else None, j, None, None, None)

    assert call(c=None) == EINVAL
    with Engine(SHAPE, H, sp.dt_of(), NT, order=ORDER, npml=NPML, dtype=dtype) as fresh:
        fresh.set_model(c0)
        assert call(c=fresh._c) == ESTATE  # no forward yet
        assert b"fwi_misfit_spectral" in lib.fwi_last_error(fresh._c)
    e.forward(c0, src, rec, save=True)
    for kw, word in ((dict(j=None), b"null"), (dict(d=None), b"null"), (dict(f=None), b"null frequencies"),
                     (dict(F=0), b"nfreq"), (dict(F=65, f="many"), b"nfreq"), (dict(f="neg"), b"negative"),
                     (dict(f="nan"), b"not finite"), (dict(f="inf"), b"not finite"), (dict(f="same"), b"equal"),
                     (dict(f="high"), b"Nyquist"), (dict(f="dc", kind=1), b"real"), (dict(f="nyq", kind=3), b"real"),
                     (dict(kind=4), b"kind"), (dict(kind=-1), b"kind"), (dict(eps=-1.0), b"eps"),
                     (dict(eps=float("nan")), b"eps"), (dict(eps=float("inf")), b"eps"), (dict(fw="w_neg"), b"freq_weights"),
                     (dict(fw="w_nan"), b"freq_weights"), (dict(tw="tw_neg"), b"trace_weights"),
                     (dict(tw="tw_inf"), b"trace_weights"), (dict(t=tp, R=4097), b"R="), (dict(t=tp, R=-1), b"R="),
                     (dict(t=None, R=3), b"taps")):
        assert call(**kw) == EINVAL, kw
        msg = lib.fwi_last_error(ctx)
        assert b"fwi_misfit_spectral" in msg and word in msg, (kw, msg)
    assert call(t=tp, R=4096) == 0 and np.isfinite(J.value)  # R > nt: harmless
    assert call(f="dc", kind=0) == 0 and call(f="nyq", kind=2, eps=1e-3) == 0  # real spectra where no phase is read
    assert call(F=64, f="many", kind=0) == 0
    e.adjoint(None)
    assert call() == ESTATE  # the synthetics are gone
    assert b"fwi_misfit_spectral" in lib.fwi_last_error(ctx)
    with pytest.raises(FwiError) as ei:
        e.misfit_spectral(d_obs, [30.0])
    assert ei.value.code == ESTATE
    e.forward(c0, src, rec, save=True)
    e.born(np.ones(SHAPE, dtype), download=False)
    assert call() == ESTATE  # ... after a Born sweep as well
    e.forward(c0, src, rec, save=True)
    for bad in (dict(weights=np.ones((NT, 4))), dict(taps=np.ones((2, 2))), dict(taps=np.ones(0)),
                dict(trace_weights=np.ones(4)), dict(freq_weights=np.ones(3)), dict(kind="amp")):
        with pytest.raises(ValueError):
            e.misfit_spectral(d_obs, [30.0, 40.0], **bad)
    for bad in ([], np.ones((2, 2))):
        with pytest.raises(ValueError):
            e.misfit_spectral(d_obs, bad)
    with pytest.raises(ValueError):
        e.misfit_spectral(d_obs[:, :4], [30.0])
    for bad in (dict(eps=-1.0), dict(freq_weights=[1.0, -1.0]), dict(trace_weights=keep["tw_neg"]), dict(kind="phase")):
        with pytest.raises(FwiError) as ei:
            e.misfit_spectral(d_obs, [0.0, 40.0] if "kind" in bad else [30.0, 40.0], **bad)
        assert ei.value.code == EINVAL
    J1, phi, a, counts = e.misfit_spectral(d_obs, [30.0, 40.0], "log", per_pair=True)
    assert J1 > 0.0 and phi.shape == a.shape == counts.shape == (2, 5) and counts.dtype == np.uint8 and counts.all()
    assert np.all(np.abs(phi) <= np.pi) and e.misfit_spectral(d_obs, [30.0, 40.0], "log") == J1
    assert "fwi_misfit_spectral" in _lib.SIGNATURES and lib.fwi_abi_version() == 14


@pytest.mark.parametrize("dtype", DTYPES)
def test_shot_loop_device_branch_is_the_per_shot_calls_summed(engines, dtype):
    """one shot on the nodes, one off the grid, weights rounded to the engine's dtype: the loop takes the device path
    (once per shot) and returns the bits of the same calls made by hand"""
    e = engines(dtype)
    rng = np.random.default_rng(21)
    c_true, c0 = sp.models()
    c0 = c0.astype(dtype)
    dt = e.dt
    wav = fo.ricker(NT, dt, 60.0).astype(dtype)
    ang, rad = 2.0 * np.pi * rng.random(9), 2.5 + 5.0 * rng.random(9)
    shots = [sh.Shot(np.array([sp.SRC], np.int32), wav, sp.receivers(11)),
             sh.Shot.at_coordinates([np.array(sp.SRC) + 0.4], wav,
                                    np.array(sp.SRC) + 0.3 + np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1), SHAPE)]
    sh.model_data(e, c_true.astype(dtype), shots)
    for s in shots:
        s.weights = (df.laplace_damping(NT, dt, 5.0) * sp.weights(NT, s.d_obs.shape[1])).astype(dtype)
    shots[1].trace_weights = sp.trace_weights(9)
    f = fourier.fourier_bins(NT, dt, 1, 20.0, 70.0)
    obj = df.SpectralMisfit(dt, f, "log", None, df.bandpass_taps(dt, 8.0, 150.0, sp.TAPS_R), dtype=dtype,
                            freq_weights=df.whitening_weights(shots[0].d_obs, dt, f))
    calls = []
    raw = e.misfit_spectral
    e.misfit_spectral = lambda *a, **k: (calls.append(1), raw(*a, **k))[1]
    try:
        Jd, gd = sh.misfit_and_gradient(e, c0, shots, objective=obj)
    finally:
        del e.misfit_spectral
    assert len(calls) == 2  # the device path ran, once per shot
    e.set_model(c0)
    e.reset_gradient()
    Js = 0.0
    for s in shots:
        s.forward(e, save=True)
        Js += e.misfit_spectral(s.d_obs, f, "log", obj.eps_of(s.d_obs, s.weights), s.weights, obj.taps, obj.freq_weights,
                                s.trace_weights)
        e.adjoint(None)
    assert Jd > 0.0 and Jd == Js and np.any(gd != 0.0) and np.array_equal(gd, e.gradient())


def test_the_call_composes_with_the_fourier_store_on_the_same_bins(gpu):
    """A composition check only: misfit_spectral and adjoint(None) on an engine whose forward term is kept at the same
    bins run and return a finite, non-zero gradient.  No accuracy claim is made for the band-limited gradient."""
    dtype, dt = "float32", sp.dt_of()
    f = fourier.fourier_bins(NT, dt, 1, 20.0, 70.0)
    c_true, c0 = sp.models()
    with Engine(SHAPE, H, dt, NT, order=ORDER, npml=NPML, dtype=dtype, fourier=f) as e:
        assert np.array_equal(e.fourier_freqs, f)
        s = sh.Shot(np.array([sp.SRC], np.int32), fo.ricker(NT, dt, 60.0), sp.receivers(65))
        s.d_obs = e.forward(c_true, (s.src_idx, s.wavelet), s.rec_idx, save=False)
        e.set_model(c0)
        s.forward(e, save=True)
        e.reset_gradient()
        J = e.misfit_spectral(s.d_obs, f, "phase", sp.floor_of(s.d_obs, dt, f, None))
        e.adjoint(None)
        g = e.gradient()
    assert J > 0.0 and np.all(np.isfinite(g)) and np.any(g != 0.0)
