"""Born and extended Born modelling on the Fourier store without a GPU: the transpose statements of include/fwi.h
(fwi_fourier_born, fwi_fourier_born_extended) on the NumPy twin and the oracle alone, the argument checks of the binding,
and the choice the shot layer makes between ``born`` and ``fourier_born``.

The Born side is ``_born_imaging.born_imaging`` on the oracle's propagator with its store replaced by what the twin
synthesises (tests/_fborn.py); the imaging side is the oracle's adjoint field through ``fourier.spectral_image``,
``fourier.offset_image`` and ``fourier.lag_image``.  fp64 on both sides: held to 1e-12 relative, and every dot product is
asserted to be far from zero first."""
import ctypes as C

import numpy as np
import pytest

import _fborn as FB
import _fimage as FI
from full_waveform_inversion_amd import _lib, fourier, shots
from full_waveform_inversion_amd.engine import Engine

TOL = 1e-12
HOST_CASES = [c[0] for c in FB.CASES]


def _dots(d, r, lhs_parts, rhs_parts):
    """<J E, r> against sum <E, J^T r>, after the check that neither side is an accident of cancellation"""
    lhs = float(np.sum(d * r))
    rhs = float(sum(np.sum(e * g) for e, g in zip(lhs_parts, rhs_parts)))
    assert abs(lhs) >= 1e-6 * np.linalg.norm(d) * np.linalg.norm(r), (lhs, np.linalg.norm(d), np.linalg.norm(r))
    return abs(lhs - rhs) / abs(lhs)


@pytest.mark.parametrize("wrt", ["velocity", "slowness2"])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", HOST_CASES)
def test_born_source_transposes_the_band_limited_imaging_sum(name, weighted, wrt):
    R, freqs, Q = FB.setup(name)
    M = FB.adjoint_spectrum(name)
    a = FB.weights(name) if weighted else None
    dm = FB.perturbation(R.p.shape)
    d = FB.born_ref(name, dm, a, wrt)
    g = FI.gradient_of_image(R, fourier.spectral_image(Q, M, R.nt, R.stride, R.dt, freqs, a), wrt)
    assert _dots(d, R.res, [dm], [g]) <= TOL


@pytest.mark.parametrize("name", HOST_CASES)
def test_unit_weights_transpose_the_oracles_own_adjoint_on_the_projected_store(name):
    """a = 1: the imaging side is the oracle's adjoint + gradient with its store replaced by the projection"""
    R, freqs, _ = FB.setup(name)
    dm = FB.perturbation(R.p.shape)
    g = R.gradient_with(fourier.project(R.q, R.nt, R.stride, R.dt, freqs))
    assert _dots(FB.born_ref(name, dm), R.res, [dm], [g]) <= TOL


@pytest.mark.parametrize("name", HOST_CASES)
def test_extended_offset_source_transposes_the_offset_images(name):
    R, freqs, Q = FB.setup(name)
    M = FB.adjoint_spectrum(name)
    a = FB.weights(name)
    for axis, n in enumerate(R.p.shape):
        lags = FB.offsets_cpu(n)
        E = FB.gather_of(R.p.shape, len(lags), seed=10 + axis)
        d = FB.extended_ref(name, "offset", lags, E, axis, a)
        imgs = [FI.gradient_of_image(R, fourier.offset_image(Q, M, R.nt, R.stride, R.dt, freqs, axis, h, a), "slowness2")
                for h in lags]
        assert np.count_nonzero(imgs[-1]) == 0  # the lag past (n - 1) / 2 ...
        without = FB.extended_ref(name, "offset", lags[:-1], E[:-1], axis, a)
        assert np.array_equal(d, without)       # ... contributes exactly nothing
        assert _dots(d, R.res, E, imgs) <= TOL, axis
        for l, h in enumerate(lags[:-1]):       # and lag by lag
            one = FB.extended_ref(name, "offset", [h], E[l:l + 1], axis, a)
            assert _dots(one, R.res, [E[l]], [imgs[l]]) <= TOL, (axis, h)


@pytest.mark.parametrize("name", HOST_CASES)
def test_extended_timelag_source_transposes_the_lag_images(name):
    R, freqs, Q = FB.setup(name)
    M = FB.adjoint_spectrum(name)
    a = FB.weights(name)
    taus = FB.taus_cpu(R.stride, R.dt)
    E = FB.gather_of(R.p.shape, len(taus), seed=20)
    d = FB.extended_ref(name, "timelag", taus, E, None, a)
    imgs = [FI.gradient_of_image(R, fourier.lag_image(Q, M, R.nt, R.stride, R.dt, freqs, tau, a), "slowness2")
            for tau in taus]
    assert _dots(d, R.res, E, imgs) <= TOL
    for l, tau in enumerate(taus):
        one = FB.extended_ref(name, "timelag", [tau], E[l:l + 1], None, a)
        assert _dots(one, R.res, [E[l]], [imgs[l]]) <= TOL, tau


@pytest.mark.parametrize("kind,lag", [("offset", 0), ("timelag", 0.0)])
def test_zero_lag_extended_source_is_the_born_source_of_slowness2(kind, lag):
    name = HOST_CASES[0]
    R, freqs, Q = FB.setup(name)
    dm = FB.perturbation(R.p.shape)
    P = fourier.extended_source(Q, dm[None], kind, [lag], R.nt, R.stride, R.dt, freqs, 0)
    assert FB.rel(P, dm[None] * Q) <= 1e-15
    assert FB.rel(FB.extended_ref(name, kind, [lag], dm[None], 0), FB.born_ref(name, dm, None, "slowness2")) <= TOL


def test_born_source_is_the_synthesis_and_rounds_where_the_device_rounds():
    rng = np.random.default_rng(0)
    nt, S, dt = 37, 3, 1e-3
    freqs = fourier.fourier_bins(nt, dt, S, 0.0, np.inf)[1:4]
    Q = rng.standard_normal((3, 5, 6)) + 1j * rng.standard_normal((3, 5, 6))
    assert np.array_equal(fourier.born_source(Q, nt, S, dt, freqs), fourier.synthesise(Q, nt, S, dt, freqs))
    a = np.array([0.5, 2.0, 1.25])
    parts = sum(a[k] * fourier.born_source(Q * np.eye(3)[k][:, None, None], nt, S, dt, freqs) for k in range(3))
    assert FB.rel(fourier.born_source(Q, nt, S, dt, freqs, a), parts) <= 1e-14
    s32 = fourier.born_source(Q, nt, S, dt, freqs, a, np.float32)
    assert s32.dtype == np.float32 and 2.0 ** -27 < FB.rel(s32, fourier.born_source(Q, nt, S, dt, freqs, a)) < 1e-6
    E = rng.standard_normal((2, 5, 6))
    P32 = fourier.extended_source(Q, E, "offset", [1, -2], nt, S, dt, freqs, 1, np.float32)
    P64 = fourier.extended_source(Q, E, "offset", [1, -2], nt, S, dt, freqs, 1)
    assert P32.dtype == np.complex64 and 2.0 ** -27 < FB.rel(P32, P64) < 1e-6
    with pytest.raises(ValueError):
        fourier.extended_source(Q, E, "depth", [1, -2], nt, S, dt, freqs, 1)
    with pytest.raises(ValueError):
        fourier.extended_source(Q, E[:1], "offset", [1, -2], nt, S, dt, freqs, 1)
    with pytest.raises(ValueError):
        fourier.extended_source(Q, E, "offset", [1, -2], nt, S, dt, freqs, 2)


# -- the binding --------------------------------------------------------------------------------------------------

def test_signatures_follow_the_header():
    sig = _lib.SIGNATURES
    P, I, = C.c_void_p, C.c_int32
    assert sig["fwi_fourier_born"] == (C.c_int, [P, I, P, P, I, P])
    assert sig["fwi_fourier_born_vec"] == (C.c_int, [P, I, I, P, I, P])
    assert sig["fwi_fourier_born_extended"] == (C.c_int, [P, I, I, I, P, P, P, P, I, P])
    assert sig["fwi_fourier_born_extended_vec"] == (C.c_int, [P, I, I, I, P, P, P, P, I, P])
    assert _lib.ABI_VERSION == 14 and _lib.EXT_KINDS["offset"] == 0 and _lib.EXT_KINDS["timelag"] == 1


class _Calls:
    """Stands in for the loaded library: records every call and returns FWI_OK"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


def _stub_engine(shape=(4, 5, 6), F=3):
    e = Engine.__new__(Engine)
    e.shape, e.ndim, e.dtype = shape, len(shape), np.dtype(np.float32)
    e._lib, e._ctx = _Calls(), C.c_void_p(1)
    e._fourier = np.arange(1.0, F + 1.0)
    e._nt, e._nrec, e._nsrc = 7, 2, 1
    return e


def test_engine_checks_its_arguments_before_the_library_is_called():
    e = _stub_engine()
    E = np.zeros((2,) + e.shape)
    bad = [
        lambda: e.fourier_born(np.zeros((4, 5, 5))),
        lambda: e.fourier_born(np.zeros(e.shape), freq_weights=np.ones(2)),
        lambda: e.fourier_born(np.zeros(e.shape), wrt="density"),
        lambda: e.fourier_born(np.zeros(e.shape), mode="fast"),
        lambda: e.fourier_born_extended("depth", [0, 1], E, axis=0),
        lambda: e.fourier_born_extended("offset", [0, 1], E),                 # no axis
        lambda: e.fourier_born_extended("offset", [0, 1], E, axis="w"),
        lambda: e.fourier_born_extended("offset", [0, 1.5], E, axis=0),       # no whole number of cells
        lambda: e.fourier_born_extended("offset", [0, 1, 2], E, axis=0),      # one image per lag
        lambda: e.fourier_born_extended("offset", [], E[:0], axis=0),
        lambda: e.fourier_born_extended("timelag", [0.0, 1e-3], E, freq_weights=np.ones(4)),
        lambda: e.fourier_born_extended_vec("offset", [0, 1], [0], axis=0),   # one slot per lag
    ]
    for call in bad:
        with pytest.raises((ValueError, KeyError)):
            call()
    assert e._lib.calls == []
    d = e.fourier_born_extended("offset", [0, -3], E, axis="x", mode="scatter")
    assert d.shape == (7, 2) and d.dtype == np.float32
    name, args = e._lib.calls[-1]
    assert name == "fwi_fourier_born_extended" and args[1:4] == (0, 2, 2) and args[5] is None and args[8] == 1
    assert e.fourier_born_extended_vec("timelag", [0.0, 2e-3], [3, 4], download=False) is None
    name, args = e._lib.calls[-1]
    assert name == "fwi_fourier_born_extended_vec" and args[1:4] == (1, 0, 2) and args[4] is None and args[9] is None
    assert e.fourier_born_vec(2, freq_weights=[1, 2, 3], wrt="slowness2", download=False) is None
    name, args = e._lib.calls[-1]
    assert name == "fwi_fourier_born_vec" and args[1:3] == (1, 2) and args[3] is not None and args[4] == 0


# -- the shot layer -----------------------------------------------------------------------------------------------

class _Recorder:
    """An engine that records the calls of one Gauss-Newton product"""
    born_leaves_residual = True
    born_operators = ("exact", "imaging")

    def __init__(self, fourier_freqs):
        self.fourier_freqs, self.shape, self.log = fourier_freqs, (3, 4), []

    def set_model(self, m):
        self.log.append("set_model")

    def reset_gradient(self):
        self.log.append("reset")

    def forward(self, model, src, rec, save=True):
        self.log.append("forward")
        return np.zeros((5, 1))

    def born(self, dm, wrt, download=True, operator="exact"):
        self.log.append(("born", operator))

    def fourier_born(self, dm, freq_weights=None, wrt="velocity", mode="auto", download=True):
        self.log.append(("fourier_born", None if freq_weights is None else tuple(freq_weights), wrt))

    def adjoint(self, r):
        self.log.append("adjoint")

    def adjoint_spectral(self, residual=None, freq_weights=None, image=True):
        self.log.append(("adjoint_spectral", None if freq_weights is None else tuple(freq_weights), image))

    def gradient(self, wrt="velocity"):
        return np.zeros(self.shape)

    def fourier_born_extended(self, kind, lags, images, axis=None, freq_weights=None, mode="auto", download=True):
        self.log.append(("fourier_born_extended", kind, tuple(lags), axis, download))

    def fourier_offset_images(self, axis, offsets, freq_weights=None):
        self.log.append(("fourier_offset_images", axis, tuple(offsets)))
        return np.ones((len(offsets),) + self.shape)


def _shot():
    return shots.Shot(np.array([[1, 1]]), np.zeros(5), np.array([[2, 2]]))


def test_gauss_newton_hvp_takes_the_born_operator_of_the_engines_store():
    v = np.zeros((3, 4))
    plain = _Recorder(None)
    shots.gauss_newton_hvp(plain, None, [_shot()], v)
    assert plain.log == ["reset", "forward", ("born", "imaging"), "adjoint"]
    for kw in ({"freq_weights": [1.0, 2.0]}, {"spectral_imaging": True}):
        with pytest.raises(ValueError):
            shots.gauss_newton_hvp(_Recorder(None), None, [_shot()], v, **kw)
    four = _Recorder(np.array([3.0, 4.0]))
    shots.gauss_newton_hvp(four, None, [_shot()], v, wrt="slowness2")
    assert four.log == ["reset", "forward", ("fourier_born", None, "slowness2"), "adjoint"]
    four = _Recorder(np.array([3.0, 4.0]))
    shots.gauss_newton_hvp(four, None, [_shot()], v, freq_weights=[1.0, 2.0], spectral_imaging=True)
    assert four.log == ["reset", "forward", ("fourier_born", (1.0, 2.0), "velocity"),
                        ("adjoint_spectral", (1.0, 2.0), True)]
    with pytest.raises(ValueError):  # adjoint(image) transposes unit weights only
        shots.gauss_newton_hvp(_Recorder(np.array([3.0, 4.0])), None, [_shot()], v, freq_weights=[1.0, 2.0])


def test_extended_hvp_is_born_then_the_gather_of_the_spectral_adjoint():
    four = _Recorder(np.array([3.0, 4.0]))
    E = np.zeros((2, 3, 4))
    H = shots.extended_hvp(four, None, [_shot(), _shot()], "offset", [0, 1], E, axis="x")
    per_shot = ["forward", ("fourier_born_extended", "offset", (0, 1), "x", False), ("adjoint_spectral", None, False),
                ("fourier_offset_images", "x", (0, 1))]
    assert four.log == per_shot * 2
    assert H.shape == (2, 3, 4) and np.all(H == 2.0)
    with pytest.raises(ValueError):
        shots.extended_hvp(_Recorder(None), None, [_shot()], "offset", [0, 1], E, axis="x")
    with pytest.raises(ValueError):
        shots.extended_born(four, None, [_shot()], "offset", [0, 1], E)  # no axis
