"""Tests-only helper of the extended images on the Fourier store (include/fwi.h fwi_fourier_offset_image,
fwi_fourier_lag_image): the references of tests/test_gpu_feximage.py and tests/test_feximage_host.py, built from what
tests/_fourier.py and tests/_fimage.py take out of the NumPy oracle (``_fourier.reference``, ``_fimage.mu_samples``,
``_fimage.adjoint_spectrum_ref``, ``_fimage.twin32``).  Nothing under ``oracle/`` changes.  The oracle's coefficients are
computed once per process (``functools.lru_cache``); callers must not write into what they get."""
import functools

import numpy as np

import _fimage as FI
import _fourier as F
from full_waveform_inversion_amd import fourier


def shifted(a, axis, h):
    """``a(x + h e_axis)`` where that cell lies in the grid, 0 elsewhere; ``a`` is ``(N, *shape)`` and ``axis`` counts
    the model axes.  Written with index arrays, independently of the slices of ``fourier.offset_image``."""
    a = np.asarray(a)
    n = a.shape[1 + axis]
    idx = np.arange(n) + int(h)
    ok = (idx >= 0) & (idx < n)
    dst, src = [slice(None)] * a.ndim, [slice(None)] * a.ndim
    dst[1 + axis], src[1 + axis] = np.nonzero(ok)[0], idx[ok]
    out = np.zeros_like(a)
    out[tuple(dst)] = a[tuple(src)]
    return out


def offset_sum(mu, q, axis, h):
    """``sum_j mu^{jS+1}(x + h e) q^{jS}(x - h e)`` from the samples themselves, ``(N, *shape)`` each"""
    return np.sum(shifted(mu, axis, h) * shifted(q, axis, -h), axis=0)


def lag_sum(mu, q, m):
    """``sum_j mu^{jS+1} q^{((j - m) mod N) S}``: the sampled forward term delayed circularly by ``m`` samples"""
    return np.sum(np.asarray(mu) * np.roll(np.asarray(q), int(m), axis=0), axis=0)


@functools.lru_cache(maxsize=None)
def oracle_spectra(name):
    """(R, freqs, Q, M) of the fp64 oracle for the configuration ``name`` of ``_fimage.CASES``"""
    _, fname, shape, order, npml, nt, S, _, _, opts, off_grid, _, _ = FI.case(name)
    key = FI.opts_key(opts)
    R = F.reference(shape, order, npml, nt, S, "float64", key, off_grid)
    freqs = FI.subset_freqs(fname, nt, R.dt, S)
    Q = fourier.analyse(np.asarray(R.q)[::S], nt, S, R.dt, freqs)
    M = FI.adjoint_spectrum_ref(shape, order, npml, nt, S, freqs, key, off_grid)
    return R, freqs, Q, M


@functools.lru_cache(maxsize=None)
def twin_spectra32(name):
    """(Q, M) of the fp32 oracle through the fp32 / batched twin of the two analyses (``_fimage.twin32``)"""
    _, fname, shape, order, npml, nt, S, B, _, opts, off_grid, _, _ = FI.case(name)
    key = FI.opts_key(opts)
    freqs = oracle_spectra(name)[1]
    return FI.twin32(shape, order, npml, nt, S, freqs, B, key, off_grid)


def offsets_of(n):
    """The offsets every axis of ``n`` cells is asked for: both signs, a multiple of the fp32 thread's 4 cells and of
    the fp64 thread's 2, odd ones, -4 and -5 (which step past the padded row where nx = 13), the last offsets that leave
    one or two cells, and one that leaves none"""
    return [0, 1, -1, 3, 4, -4, -5, (n - 1) // 2, n]


def taus_of(S, dt):
    """Zero, one sample either way (a circular shift on bins), and two lags that are no whole number of samples"""
    return [0.0, S * dt, -S * dt, 2.5 * S * dt, -7.3 * dt]


def gather(Q, M, R, nt, freqs, kind, lags, axis=None, a=None, dtype=np.float64):
    """The twin's gather in the units of ``Engine.fourier_gradient(wrt="slowness2")``, ``(len(lags), *shape)`` fp64"""
    S = R.stride
    if kind == "offset":
        imgs = [fourier.offset_image(Q, M, nt, S, R.dt, freqs, axis, h, a, dtype) for h in lags]
    else:
        imgs = [fourier.lag_image(Q, M, nt, S, R.dt, freqs, tau, a, dtype) for tau in lags]
    return np.stack([FI.gradient_of_image(R, img, "slowness2") for img in imgs])


def lag_errors(E, ref):
    """Per lag, ``|E_l - ref_l|`` over the largest ``|ref_l|`` of the gather (L2 norms over the image)"""
    E, ref = np.asarray(E, np.float64), np.asarray(ref, np.float64)
    norms = np.sqrt(np.sum(ref.reshape(ref.shape[0], -1) ** 2, axis=1))
    diff = np.sqrt(np.sum((E - ref).reshape(ref.shape[0], -1) ** 2, axis=1))
    return diff / norms.max()
