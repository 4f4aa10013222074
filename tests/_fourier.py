"""Tests-only helper of the Fourier-compressed forward-term store: the small problems the GPU tests run, and their
references from the NumPy oracle.  The reference of a Fourier-store gradient is the oracle's own gradient with its
``q_store`` replaced by ``fourier.project(q_store, ...)``; nothing under ``oracle/`` changes.  Every reference is
computed once per process and shared (``functools.lru_cache``); callers must not write into what they get."""
import functools

import numpy as np

from full_waveform_inversion_amd import fourier
from full_waveform_inversion_amd.points import Spread
from oracle import fwi_oracle as fo

ORACLE_KEYS = ("abc", "pml_alpha_max")


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.complex128) - np.asarray(b, np.complex128)) / np.linalg.norm(b))


@functools.lru_cache(maxsize=None)
def problem(shape, order, nt, off_grid=False, seed=0):
    """(c, h, dt, src, rec, wavelet, residual): one source, six receivers, a residual of unit-variance noise (every
    frequency of the time axis takes part in the imaging).  ``off_grid``: the source at fractional coordinates, src is
    then a :class:`Spread`."""
    rng = np.random.default_rng(seed)
    c = 2000.0 + 600.0 * rng.random(shape)
    h = 10.0
    dt = 0.6 * fo.cfl_dt(c.max(), h, len(shape), order)
    if off_grid:
        src = Spread(np.array([[s / 2.0 - 0.3 - 0.1 * a for a, s in enumerate(shape)]]), shape)
    else:
        src = np.array([[s // 2 for s in shape]])
    rec = np.stack([rng.integers(0, s, 6) for s in shape], 1)
    wav = fo.ricker(nt, dt, 1.0 / (10.0 * dt), t0=12.0 * dt)[:, None]  # a period of 10 steps, its peak at step 12
    res = rng.standard_normal((nt, 6))
    return c, h, dt, src, rec, wav, res


class Reference:
    """The oracle's run of one problem in ``dtype``, and the gradients it gives for whatever replaces its store."""

    def __init__(self, shape, order, npml, nt, stride, dtype, opts, off_grid):
        c, h, dt, src, rec, wav, res = problem(shape, order, nt, off_grid)
        self.nt, self.stride, self.dt = nt, stride, dt
        self.p = fo.Propagator(c, h, dt, order, npml, dtype=np.dtype(dtype), image_stride=stride,
                               **{k: v for k, v in opts if k in ORACLE_KEYS})
        if off_grid:
            self.p.forward(src.idx, src.scatter(wav), rec)
        else:
            self.p.forward(src, wav, rec)
        self.q = self.p.q_store
        self.res = res
        self.native = self.gradient_with(self.q)

    def gradient_with(self, q_store):
        self.p.q_store = q_store
        self.p.adjoint(self.res)
        self.p.q_store = self.q
        return self.p.gradient()

    def fourier(self, freqs, dtype=np.float64, batch=None):
        """(gradient, Q) with the forward term replaced by its projection, transforms in ``dtype`` / ``batch``"""
        g = self.gradient_with(fourier.project(self.q, self.nt, self.stride, self.dt, freqs, dtype, batch))
        Q = fourier.analyse(np.asarray(self.q)[::self.stride], self.nt, self.stride, self.dt, freqs, dtype, batch)
        return g, Q


@functools.lru_cache(maxsize=None)
def reference(shape, order, npml, nt, stride, dtype="float64", opts=(), off_grid=False):
    return Reference(shape, order, npml, nt, stride, dtype, opts, off_grid)


def all_bins(nt, dt, stride):
    return fourier.fourier_bins(nt, dt, stride, 0.0, np.inf)


@functools.lru_cache(maxsize=None)
def identity_bound32(shape, order, npml, nt, stride, batch, opts=(), off_grid=False):
    """What an fp32 engine with all bins may differ by from its own native store, relative L2 of the gradient: the twin's
    own error -- its fp32 transforms (accumulators and slots in fp32, sums per batch in fp64, as on the device) against
    its fp64 ones, on the same fp64 history and the same adjoint field -- and the caller allows 4 times that."""
    R = reference(shape, order, npml, nt, stride, "float64", opts, off_grid)
    f = all_bins(nt, R.dt, stride)
    g64, _ = R.fourier(f)
    g32, _ = R.fourier(f, np.float32, batch)
    return rel(g32, g64)
