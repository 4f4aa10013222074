"""Extended images on the Fourier store without a GPU: the two identities they rest on, on the NumPy twin and the oracle
(full_waveform_inversion_amd/fourier.py, tests/_feximage.py), the binding, and the flags of tools/run_config.py.

1. Offset identity, for ANY set of frequencies: ``sum_j mu^{jS+1}(x + h e) q~^{jS}(x - h e) = sum_k w_k Re(Q_k(x - h e)
   conj M_k(x + h e))``.  fp64 on both sides: held to 1e-12.
2. Time-lag identity, on bins and whole samples only: with ``tau = m S dt`` the lag image is the imaging sum with the
   sampled ``q~`` shifted circularly by ``m`` samples.  Off the bins it FAILS except at zero lag, which is the documented
   limit of ``fwi_fourier_lag_image`` and is asserted here.
3. The definition against the oracle's fields: with all bins the offset image of the oracle's ``Q``, ``M`` is the sum over
   the oracle's own stored term and adjoint field at the shifted cells."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _feximage as FX
import _fimage as FI
import _fourier as F
from full_waveform_inversion_amd import _lib, fourier

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12


def _random(shape, nt, S, seed):
    rng = np.random.default_rng(seed)
    N = fourier.n_samples(nt, S)
    return rng.standard_normal((N,) + shape), rng.standard_normal((N,) + shape), N


def _sets(nt, S, dt):
    bins = fourier.fourier_bins(nt, dt, S, 0.0, np.inf)
    return {"all": bins, "few": bins[[1, 2, bins.size - 1]], "off_bin": np.array([0.13, 0.21, 0.29]) / (S * dt)}


@pytest.mark.parametrize("fname", ["all", "few", "off_bin"])
@pytest.mark.parametrize("shape,nt,S", [((7, 9), 37, 4), ((5, 6, 7), 37, 1), ((6, 4, 5), 40, 3)], ids=str)
def test_offset_image_is_the_imaging_sum_of_the_shifted_fields(shape, nt, S, fname):
    dt = 1e-3
    q, mu, N = _random(shape, nt, S, 1)
    freqs = _sets(nt, S, dt)[fname]
    Q, M = fourier.analyse(q, nt, S, dt, freqs), fourier.adjoint_spectrum(mu, nt, S, dt, freqs)
    qt = fourier.synthesise(Q, nt, S, dt, freqs)
    a = 0.25 + np.arange(freqs.size) % 3
    for axis, n in enumerate(shape):
        for h in (0, 1, -1, 2, -3, (n - 1) // 2, -((n - 1) // 2)):
            img = fourier.offset_image(Q, M, nt, S, dt, freqs, axis, h)
            if 2 * abs(h) >= n:  # (the smallest axes: no cell is left)
                assert np.count_nonzero(img) == 0 and np.count_nonzero(FX.offset_sum(mu, qt, axis, h)) == 0
                continue
            assert np.linalg.norm(img) > 0
            assert F.rel(img, FX.offset_sum(mu, qt, axis, h)) <= TOL, (axis, h)
            # the weights are linear: the sum of the weighted one-frequency images
            parts = [fourier.offset_image(Q, M, nt, S, dt, freqs, axis, h, a[k] * np.eye(freqs.size)[k])
                     for k in range(freqs.size)]
            assert F.rel(fourier.offset_image(Q, M, nt, S, dt, freqs, axis, h, a), np.sum(parts, axis=0)) <= TOL
        # zero where either shifted cell leaves the grid; nothing left past (n - 1) / 2, whatever the size of h
        h = (n - 1) // 2
        edge = fourier.offset_image(Q, M, nt, S, dt, freqs, axis, h)
        assert np.count_nonzero(np.moveaxis(edge, axis, 0)[:h]) == 0
        assert np.count_nonzero(np.moveaxis(edge, axis, 0)[n - h:]) == 0
        for h in ((n - 1) // 2 + 1, -((n - 1) // 2 + 1), n, -n, 2 ** 31 - 1, -2 ** 31):
            assert np.count_nonzero(fourier.offset_image(Q, M, nt, S, dt, freqs, axis, h)) == 0, (axis, h)
    with pytest.raises(ValueError):
        fourier.offset_image(Q, M, nt, S, dt, freqs, len(shape), 1)


@pytest.mark.parametrize("shape,nt,S", [((7, 9), 37, 4), ((5, 6, 7), 37, 1), ((6, 4, 5), 40, 3)], ids=str)
def test_lag_image_is_a_circular_shift_on_bins_and_only_there(shape, nt, S):
    dt = 1e-3
    q, mu, N = _random(shape, nt, S, 2)
    sets = _sets(nt, S, dt)
    shifts = (0, 1, -1, 3, -4, N // 2 + 1, -(N // 2 + 2), N, 2 * N + 1)  # negative ones, and above N / 2
    for fname in ("all", "few"):
        freqs = sets[fname]
        Q, M = fourier.analyse(q, nt, S, dt, freqs), fourier.adjoint_spectrum(mu, nt, S, dt, freqs)
        qt = fourier.synthesise(Q, nt, S, dt, freqs)
        for m in shifts:
            img = fourier.lag_image(Q, M, nt, S, dt, freqs, m * S * dt)
            assert F.rel(img, FX.lag_sum(mu, qt, m)) <= TOL, (fname, m)
    # all bins: q~ is the sampled term itself
    freqs = sets["all"]
    Q, M = fourier.analyse(q, nt, S, dt, freqs), fourier.adjoint_spectrum(mu, nt, S, dt, freqs)
    assert F.rel(fourier.lag_image(Q, M, nt, S, dt, freqs, 2 * S * dt), FX.lag_sum(mu, q, 2)) <= TOL
    # off the bins: the identity at zero lag only, a definition elsewhere
    freqs = sets["off_bin"]
    Q, M = fourier.analyse(q, nt, S, dt, freqs), fourier.adjoint_spectrum(mu, nt, S, dt, freqs)
    qt = fourier.synthesise(Q, nt, S, dt, freqs)
    assert F.rel(fourier.lag_image(Q, M, nt, S, dt, freqs, 0.0), FX.lag_sum(mu, qt, 0)) <= TOL
    for m in (1, -1, 3):
        assert F.rel(fourier.lag_image(Q, M, nt, S, dt, freqs, m * S * dt), FX.lag_sum(mu, qt, m)) > 0.01, m
    for bad in (np.inf, -np.inf, np.nan):
        with pytest.raises(ValueError):
            fourier.lag_image(Q, M, nt, S, dt, freqs, bad)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_zero_lag_is_the_spectral_image_bit_for_bit(dtype):
    shape, nt, S, dt = (5, 6, 7), 37, 4, 1e-3
    q, mu, _ = _random(shape, nt, S, 3)
    for fname, freqs in _sets(nt, S, dt).items():
        Q, M = fourier.analyse(q, nt, S, dt, freqs, dtype), fourier.adjoint_spectrum(mu, nt, S, dt, freqs, dtype)
        for a in (None, 0.5 + np.arange(freqs.size) % 2):
            img = fourier.spectral_image(Q, M, nt, S, dt, freqs, a, dtype)
            assert img.dtype == np.dtype(dtype) and np.linalg.norm(img) > 0
            for axis in range(3):
                assert np.array_equal(fourier.offset_image(Q, M, nt, S, dt, freqs, axis, 0, a, dtype), img), (fname, axis)
            assert np.array_equal(fourier.lag_image(Q, M, nt, S, dt, freqs, 0.0, a, dtype), img), fname
    # the dtype restatement: coefficients held in fp32, one rounding of the fp64 sum
    Q, M = fourier.analyse(q, nt, S, dt, freqs), fourier.adjoint_spectrum(mu, nt, S, dt, freqs)
    for img64, img32 in ((fourier.offset_image(Q, M, nt, S, dt, freqs, 2, -1),
                          fourier.offset_image(Q, M, nt, S, dt, freqs, 2, -1, dtype=np.float32)),
                         (fourier.lag_image(Q, M, nt, S, dt, freqs, 1.7 * dt),
                          fourier.lag_image(Q, M, nt, S, dt, freqs, 1.7 * dt, dtype=np.float32))):
        assert img32.dtype == np.float32 and 0 < F.rel(img32, img64) < 1e-6


def test_offset_image_of_the_oracles_spectra_is_the_sum_over_its_own_fields():
    """The definition against the oracle's fields, not just the transforms: (21, 23) order 4 npml 3 nt 33 S 4, all bins"""
    name = "2d_33_4_4"
    _, _, shape, order, npml, nt, S, _, _, opts, _, _, _ = FI.case(name)
    R, freqs, Q, M = FX.oracle_spectra(name)
    mu = FI.mu_samples(shape, order, npml, nt, S, "float64", FI.opts_key(opts))
    q = np.asarray(R.q)[::S]
    for axis, n in enumerate(shape):
        lags = (0, 1, -1, 3, -4, -5, (n - 1) // 2)
        E = np.stack([fourier.offset_image(Q, M, nt, S, R.dt, freqs, axis, h) for h in lags])
        ref = np.stack([FX.offset_sum(mu, q, axis, h) for h in lags])
        # Every lag, its error over the largest lag norm of the gather (the normalisation of tests/test_gpu_feximage.py).
        # The last lag pairs the two border columns, which the fields have barely reached (|E_h| is 1e-6 and 2e-12 of
        # |E_0|): its terms cancel to 1e-9 of their size, so its error is round-off of the terms, not of the sum ...
        assert np.all(FX.lag_errors(E, ref) <= FI.TOL64), FX.lag_errors(E, ref)
        # ... and every lag with something to compare, over its own norm
        for l, h in enumerate(lags[:-1]):
            assert np.linalg.norm(ref[l]) > 1e-2 * np.linalg.norm(ref[0])
            assert F.rel(E[l], ref[l]) <= FI.TOL64, (axis, h)
    # ... and the time-lag image of the same spectra against the circularly delayed stored term
    for m in (0, 1, -1, 5):
        err = F.rel(fourier.lag_image(Q, M, nt, S, R.dt, freqs, m * S * R.dt), FX.lag_sum(mu, q, m))
        assert err <= FI.TOL64, (m, err)


def test_focusing_of_a_hand_made_gather():
    lags = np.array([-2.0, -1.0, 0.0, 1.0, 2.0])
    E = np.zeros((5, 3, 4))
    E[2] = 7.0
    assert fourier.focusing(E, lags) == 0.0  # all energy at zero lag
    E[:] = 0.0
    E[0, 1, 1], E[4, 2, 3] = 3.0, -3.0
    assert fourier.focusing(E, lags) == 4.0  # all of it at |lag| = 2
    E[:] = 0.0
    E[2, 0, 0], E[3, 0, 0], E[3, 1, 1] = 2.0, 1.0, 1.0  # energies 4 at lag 0, 2 at lag 1
    assert fourier.focusing(E, lags) == pytest.approx(2.0 / 6.0, rel=1e-15)
    assert fourier.focusing(E.astype(np.float32), 0.5 * lags) == pytest.approx(0.25 * 2.0 / 6.0, rel=1e-15)
    assert np.isnan(fourier.focusing(np.zeros((5, 2)), lags))
    with pytest.raises(ValueError):
        fourier.focusing(E, lags[:4])


NEW = ("fwi_fourier_offset_image", "fwi_fourier_offset_image_vec", "fwi_fourier_lag_image", "fwi_fourier_lag_image_vec")


def test_binding_and_header_declare_the_four_calls_under_the_same_abi():
    header = open(os.path.join(ROOT, "include", "fwi.h")).read()
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        assert re.search(r"^int %s\(fwi_ctx \*ctx" % name, header, re.M), name
    assert "#define FWI_ABI_VERSION 14" in header and _lib.ABI_VERSION == 14
    # the limit of the time-lag image is stated where a caller reads it
    assert "NO SUCH SUM" in header
    lib = _lib.load()
    assert lib.fwi_abi_version() == 14
    for name in NEW:  # null context: refused without touching a device
        args = [0 if t is _lib._I32 else 0.0 if t is _lib._D else None for t in _lib.SIGNATURES[name][1][1:]]
        assert getattr(lib, name)(None, *args) == 1


def test_run_config_knows_the_extended_image_flags_and_refuses_bad_combinations():
    """tools/run_config.py --extended-image / --extended-out: checked before any engine exists"""
    tool = os.path.join(ROOT, "tools", "run_config.py")
    out = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--extended-image" in out.stdout and "--extended-out" in out.stdout
    store = ["--fourier-store", "2,12"]
    for bad, word in ((["--extended-image", "offset:x:4", "--extended-out", "g.npz"], "--fourier-store"),
                      (["--extended-image", "offset:x:4"] + store, "--extended-out"),
                      (["--extended-out", "g.npz"] + store, "--extended-image"),
                      (["--extended-image", "offset:w:4", "--extended-out", "g.npz"] + store, "offset:AXIS:L"),
                      (["--extended-image", "time:0:4", "--extended-out", "g.npz"] + store, "time:DTAU:L"),
                      (["--extended-image", "depth:1:4", "--extended-out", "g.npz"] + store, "offset:AXIS:L")):
        out = subprocess.run([sys.executable, tool] + bad, capture_output=True, text=True)
        assert out.returncode == 2 and word in out.stderr, (bad, out.stderr[-400:])
