"""Tests-only helper of spectral imaging on the Fourier store (include/fwi.h fwi_adjoint_spectral): the references of
tests/test_gpu_fimage.py and tests/test_fimage_host.py, all from the NumPy oracle through what tests/_fourier.py builds.
Nothing under ``oracle/`` changes: the adjoint field is read out of the oracle's imaging sum by giving it a store that is
constant in space.  ``gradient_with(store)`` with ``store[jS] = cos theta_kj`` leaves ``p._img = S sum_j mu^{jS+1} cos
theta_kj = S Re M_k``, with ``sin`` it leaves ``-S Im M_k``, and a store that is one at the single step ``jS`` leaves
``S mu^{jS+1}`` itself.  Every reference is computed once per process (``functools.lru_cache``); callers must not write
into what they get."""
import functools

import numpy as np

import _fourier as F
from full_waveform_inversion_amd import fourier

MARGIN = 4.0
TOL64 = 1e-12


def opts_key(opts):
    return tuple(sorted(opts.items()))


def subset_freqs(name, nt, dt, S):
    """The frequency sets of tests/test_gpu_fourier.py (``_subset_freqs``), and ``all``"""
    bins = F.all_bins(nt, dt, S)
    nyq = 1.0 / (2 * S * dt)
    if name == "all":
        return bins
    if name == "one_bin":  # the bin next to the wavelet's peak frequency 1 / (10 dt)
        return bins[[int(np.argmin(np.abs(bins - 1.0 / (10.0 * dt))))]]
    if name == "mid_third":
        n = bins.size
        return bins[n // 6: n // 6 + max(1, n // 3)]
    if name == "off_bin_3":
        return np.array([0.13, 0.21, 0.29]) * 2 * nyq
    if name == "off_bin_64":  # F = FWI_FOURIER_FMAX, none of them a bin of the 40 samples
        return (np.arange(64) + 0.37) / 64.5 * nyq
    raise KeyError(name)


def _img_with(R, per_step):
    """The oracle's imaging sum for a store that is ``per_step[n]`` at every cell of step n"""
    store = np.asarray(per_step, np.float64).reshape((R.nt,) + (1,) * R.p.ndim)
    R.gradient_with(store)
    return np.array(R.p._img, np.float64)


@functools.lru_cache(maxsize=None)
def mu_samples(shape, order, npml, nt, stride, dtype="float64", opts=(), off_grid=False):
    """``mu^{jS+1}``, ``(N, *shape)``, of the oracle run in ``dtype`` (exact in fp64: the oracle's sum has one term)"""
    R = F.reference(shape, order, npml, nt, stride, dtype, opts, off_grid)
    N = fourier.n_samples(nt, stride)
    out = np.zeros((N,) + tuple(shape))
    for j in range(N):
        hot = np.zeros(nt)
        hot[j * stride] = 1.0
        out[j] = _img_with(R, hot) / stride
    return out


def adjoint_spectrum_ref(shape, order, npml, nt, stride, freqs, opts=(), off_grid=False):
    """``M_k`` of the fp64 oracle, from its own imaging sums against cos / sin stores"""
    R = F.reference(shape, order, npml, nt, stride, "float64", opts, off_grid)
    th = fourier.phases(nt, stride, R.dt, freqs)
    M = np.zeros((th.shape[0],) + tuple(shape), np.complex128)
    for k in range(th.shape[0]):
        c, s = np.zeros(nt), np.zeros(nt)
        c[::stride], s[::stride] = np.cos(th[k]), np.sin(th[k])
        M[k] = (_img_with(R, c) - 1j * _img_with(R, s)) / stride
    return M


def gradient_of_image(R, image, wrt="velocity"):
    """The oracle's gradient if its imaging sum were ``S image`` (``image`` in the units of ``sum_j mu^{jS+1} q^{jS}``)"""
    g_m = -R.stride * np.asarray(image, np.float64) / R.dt ** 2
    return g_m * (-2.0 / R.p.c ** 3) if wrt == "velocity" else g_m


def twin32(shape, order, npml, nt, stride, freqs, batch, opts=(), off_grid=False):
    """(Q, M) of the fp32 oracle run through the fp32 / batched twin of the two analyses"""
    R32 = F.reference(shape, order, npml, nt, stride, "float32", opts, off_grid)
    Q = fourier.analyse(np.asarray(R32.q)[::stride], nt, stride, R32.dt, freqs, np.float32, batch)
    mu = mu_samples(shape, order, npml, nt, stride, "float32", opts, off_grid)
    M = fourier.adjoint_spectrum(mu, nt, stride, R32.dt, freqs, np.float32, batch)
    return Q, M


def in_band(own):
    """An fp32 round-off, neither nothing nor everything"""
    assert 2.0 ** -27 < own < 1e-5, own
    return own


def illumination_of(R, sum_sq, wrt="velocity"):
    """``(S / dt^4) sum_sq``, times ``(2 / c^3)^2`` w.r.t. velocity: the units of ``Engine.illumination``"""
    H = R.stride * np.asarray(sum_sq, np.float64) / R.dt ** 4
    return H * (2.0 / R.p.c ** 3) ** 2 if wrt == "velocity" else H


BOTH, F32 = ("float64", "float32"), ("float32",)

# id, frequency set, shape, order, npml, nt, S, B, dtypes, engine options, off-grid source, fused-capable 2-D context,
# creation-time environment: the configurations of tests/test_gpu_fourier.py (ID_CASES with all bins, SUB_CASES with
# their sets).  nx = 23, 13 and 14 leave pad columns; N % B != 0 in 2d_33_4_4 (9 samples, batch 4) and others.
CASES = [
    ("2d_33_4_4", "all", (21, 23), 4, 3, 33, 4, 4, BOTH, {"kernel": "point"}, False, False, {}),
    ("2d_N_below_B", "all", (21, 23), 4, 3, 20, 4, 8, BOTH, {"kernel": "point"}, False, False, {}),
    ("2d_fused_capable", "all", (20, 24), 8, 3, 32, 1, 8, F32, {}, False, True, {}),
    ("2d_tile", "all", (21, 23), 4, 3, 31, 1, 4, F32, {"kernel": "stream"}, False, True, {}),
    ("3d_stream_sponge", "all", (12, 10, 14), 8, 3, 33, 4, 4, BOTH, {}, False, False, {}),
    ("3d_stream_ty8", "all", (12, 10, 14), 8, 3, 33, 4, 4, BOTH, {}, False, False, {"FWI_STREAM_TY": "8"}),
    ("3d_cpml", "all", (9, 10, 13), 4, 3, 31, 1, 4, BOTH, {"abc": "cpml", "pml_alpha_max": 30.0}, False, False, {}),
    ("3d_increment", "all", (12, 10, 14), 8, 3, 32, 1, 8, BOTH, {"update_form": "increment"}, False, False, {}),
    ("3d_graph", "all", (9, 10, 13), 8, 0, 40, 4, 1, BOTH, {"launch_mode": "graph"}, False, False, {}),
    ("3d_off_grid", "all", (12, 10, 14), 8, 3, 31, 1, 4, BOTH, {}, True, False, {}),
    ("one_bin", "one_bin", (21, 23), 4, 3, 33, 1, 4, BOTH, {"kernel": "point"}, False, False, {}),
    ("mid_third", "mid_third", (12, 10, 14), 8, 3, 40, 1, 8, BOTH, {}, False, False, {}),
    ("off_bin_3", "off_bin_3", (9, 10, 13), 4, 3, 33, 4, 4, BOTH, {"abc": "cpml", "pml_alpha_max": 30.0}, False, False, {}),
    ("off_bin_64", "off_bin_64", (20, 24), 8, 0, 40, 1, 4, BOTH, {"kernel": "point"}, False, False, {}),
]


def case(name):
    return next(c for c in CASES if c[0] == name)
