"""Band-limited, weighted least-squares data misfit: filter taps, the fp64 NumPy twin, data weights, staged bands.

For one shot, with ``x = d_syn - d_obs`` shaped ``(nt, ntr)`` (time along axis 0, one column per trace), ``B`` a symmetric
FIR filter along time on the zero-extended trace, taps ``b_0 .. b_R`` with ``b_-k = b_k``,

    (B x)[n, j] = sum_{k=-R..R} b_|k| x[n + k, j]      (terms with n + k outside [0, nt) omitted: B^T = B)

and ``M >= 0`` per-sample weights of the data's shape:

    e = M . (B x)        J = 1/2 sum e^2        dJ/dd_syn = r = B (M . e)

The engine forms ``e``, ``J`` and ``r`` on the device (``Engine.misfit_weighted``, ``fwi_misfit_weighted``,
``csrc/fwi_data.hip``) and applies the Gauss-Newton weight ``W = B M^2 B`` to a Born residual there
(``Engine.residual_weight``); :class:`WeightedL2` is the twin of both in NumPy and the ``objective=`` that
``shots.misfit_and_gradient`` recognises.  Band-limiting the residual is how frequency continuation from low to high
bands avoids cycle skipping (:func:`frequency_continuation`); the weights carry trace kills, direct-arrival mutes and
offset / time windows (:func:`offset_time_mute`).  No reference counterpart.
"""
from __future__ import annotations

import math

import numpy as np

R_MAX = 4096  # the largest half-width the device path accepts (fwi_misfit_weighted)


def _lowpass_raw(dt, f, R):
    k = np.arange(int(R) + 1, dtype=np.float64)
    fc = 2.0 * float(f) * float(dt)
    return fc * np.sinc(fc * k) * 0.5 * (1.0 + np.cos(np.pi * k / (int(R) + 1)))


def _two_sided_sum(b):
    return math.fsum([float(b[0])] + [2.0 * float(v) for v in b[1:]])


def _check_band(dt, f, R):
    if not (float(dt) > 0.0 and np.isfinite(dt)):
        raise ValueError("dt must be > 0")
    if int(R) != R or not 0 <= int(R) <= R_MAX:
        raise ValueError("R must be an integer in [0, %d]" % R_MAX)
    if not (0.0 < float(f) < 0.5 / float(dt)):
        raise ValueError("corner frequency %g outside (0, Nyquist = %g)" % (f, 0.5 / float(dt)))


def lowpass_taps(dt, f_hi, R):
    """One-sided taps ``b_0 .. b_R`` of a Hann-windowed sinc low-pass with corner ``f_hi`` (Hz) at the sampling interval
    ``dt``: ``2 f dt sinc(2 f dt k) (1 + cos(pi k / (R + 1))) / 2``, scaled so that the two-sided sum (the gain at zero
    frequency) is exactly 1.  The transition band is about ``2 / ((R + 1) dt)`` wide."""
    _check_band(dt, f_hi, R)
    b = _lowpass_raw(dt, f_hi, R)
    return b / _two_sided_sum(b)


def bandpass_taps(dt, f_lo, f_hi, R):
    """``lowpass_taps(f_hi) - lowpass_taps(f_lo)``: the band ``f_lo .. f_hi``, gain 0 at zero frequency."""
    _check_band(dt, f_hi, R)
    _check_band(dt, f_lo, R)
    if not float(f_lo) < float(f_hi):
        raise ValueError("f_lo = %g must be below f_hi = %g" % (f_lo, f_hi))
    return lowpass_taps(dt, f_hi, R) - lowpass_taps(dt, f_lo, R)


def _checked_taps(taps):
    if taps is None:
        return None
    b = np.ascontiguousarray(np.asarray(taps, np.float64))
    if b.ndim != 1 or b.size < 1 or not np.all(np.isfinite(b)):
        raise ValueError("taps must be a finite 1-D array b_0 .. b_R")
    return b


def fir_matrix(taps, nt):
    """``B`` as the dense symmetric ``nt x nt`` Toeplitz matrix of the zero-extended filter."""
    col = np.zeros(nt)
    m = min(len(taps), nt)
    col[:m] = taps[:m]
    i = np.arange(nt)
    return col[np.abs(i[:, None] - i[None, :])]


_DENSE_MIN_R, _DENSE_MAX_NT = 16, 4096  # longer filters on traces this short: one matrix product instead of 2 R passes


def fir_time(x, taps):
    """``B x`` along axis 0 in fp64 (``taps=None``: a copy of x)."""
    x = np.asarray(x, np.float64)
    if taps is None:
        return x.copy()
    nt = x.shape[0]
    if min(len(taps), nt) - 1 > _DENSE_MIN_R and nt <= _DENSE_MAX_NT and x.ndim == 2:
        return fir_matrix(taps, nt) @ x
    out = taps[0] * x
    for k in range(1, min(len(taps) - 1, nt - 1) + 1):
        out[:nt - k] += taps[k] * x[k:]
        out[k:] += taps[k] * x[:nt - k]
    return out


class WeightedL2:
    """``objective(d_syn, d_obs, weights=None) -> (J, r)`` of the definition above, in fp64 NumPy.  ``taps``: the one-sided
    ``b_0 .. b_R`` (:func:`lowpass_taps`, :func:`bandpass_taps`) or None for ``B = I``.  ``shots.misfit_and_gradient``
    hands it each shot's ``Shot.weights`` and, on an engine that has ``misfit_weighted``, replaces it by the device path."""

    def __init__(self, taps=None):
        self.taps = _checked_taps(taps)

    def filter(self, x):
        return fir_time(x, self.taps)

    @staticmethod
    def _weights(weights, shape):
        if weights is None:
            return None
        M = np.asarray(weights, np.float64)
        if M.shape != tuple(shape):
            raise ValueError("weights have shape %r, the data %r" % (M.shape, tuple(shape)))
        if np.any(M < 0.0):
            raise ValueError("weights must be >= 0")
        return M

    def __call__(self, d_syn, d_obs, weights=None):
        x = np.asarray(d_syn, np.float64) - np.asarray(d_obs, np.float64)
        M = self._weights(weights, x.shape)
        e = self.filter(x)
        if M is not None:
            e *= M
        return 0.5 * float(np.sum(e * e)), self.filter(e if M is None else M * e)

    def normal(self, x, weights=None):
        """``W x = B M^2 B x``: the Gauss-Newton weight of this misfit (``Engine.residual_weight``'s twin)."""
        x = np.asarray(x, np.float64)
        M = self._weights(weights, x.shape)
        e = self.filter(x)
        return self.filter(e if M is None else M * M * e)


def offset_time_mute(shot, h, dt, v_fast, t_pad=0.0, taper=0):
    """Weights ``(nt, ntr)`` that mute everything up to the direct arrival: with ``t_cut = |x_r - x_s| / v_fast + t_pad``
    per trace (the offset from the shot's first source, grid spacing ``h``), 0 for ``t < t_cut``, then a raised cosine
    over ``taper`` samples, 1 from ``t_cut + taper dt`` on.  Off-grid shots use their points' coordinates."""
    if not (float(v_fast) > 0.0 and float(dt) > 0.0 and float(h) > 0.0) or int(taper) < 0:
        raise ValueError("h, dt and v_fast must be > 0 and taper >= 0")

    def coords(spread_pts, idx):
        return np.asarray(idx if spread_pts is None else spread_pts, np.float64)

    src = coords(getattr(shot.src_spread, "coords", None), shot.src_idx)
    rec = coords(getattr(shot.rec_spread, "coords", None), shot.rec_idx)
    src, rec = np.atleast_2d(src), np.atleast_2d(rec)
    nt = np.asarray(shot.wavelet if shot.point_wavelet is None else shot.point_wavelet).shape[0]
    off = float(h) * np.sqrt(np.sum((rec - src[0]) ** 2, axis=1))
    s = np.arange(nt, dtype=np.float64)[:, None] - (off / float(v_fast) + float(t_pad))[None, :] / float(dt)
    if int(taper) == 0:
        return (s >= 0.0).astype(np.float64)
    w = 0.5 * (1.0 - np.cos(np.pi * np.clip(s / int(taper), 0.0, 1.0)))
    return np.where(s >= int(taper), 1.0, w)


def frequency_continuation(run_band, x0, bands, taps_of=None):
    """Staged inversion from the first band to the last: ``x, log = run_band(x, taps)`` per band, each started from the
    band before's ``x``.  ``bands`` holds the taps of each stage (None: the full band), or whatever ``taps_of(band)``
    turns into them.  ``run_band`` must start a fresh optimiser: curvature pairs of another band's objective are invalid.
    Returns the last ``x`` and the list of per-band logs."""
    x, logs = x0, []
    for band in bands:
        x, log = run_band(x, taps_of(band) if taps_of is not None else band)
        logs.append(log)
    return x, logs
