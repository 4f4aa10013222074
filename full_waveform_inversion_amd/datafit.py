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

Matching-filter (source-independent) misfit, :class:`MatchedL2` (``Engine.misfit_matched``, ``fwi_misfit_matched``,
``csrc/fwi_match.hip``): the source signature is never known exactly, and a wrong wavelet leaks into the model update.
Per shot a short two-sided filter ``f = (f_-L .. f_L)``, ``K = 2 L + 1``, along time on the zero-extended trace takes
it up and is eliminated by variable projection.  With ``s = d_syn``, ``d = d_obs``, ``B`` and ``M`` as above:

    s' = B s,   d' = B d
    (C_f x)[n, j]   = sum_{k=-L..L} f_k x[n - k, j]      terms with n - k outside [0, nt) omitted
    (C_f^T y)[m, j] = sum_{k=-L..L} f_k y[m + k, j]      terms with m + k outside [0, nt) omitted
    e = M . (C_f s' - d')
    Phi(f; s) = 1/2 sum e^2 + mu/2 |f|^2                 mu >= 0 absolute, given by the caller
    G[k, l] = sum_{n, j} M^2[n, j] s'[n - k, j] s'[n - l, j],    b[k] = sum_{n, j} M^2[n, j] s'[n - k, j] d'[n, j]
    f* = (G + mu I)^-1 b,     J(s) = Phi(f*; s),     r = dJ/ds = B C_{f*}^T (M . e)       (dPhi/df = 0 at f*)

``G`` is not Toeplitz (the weights, the truncation at both ends of the trace).  ``mu`` is independent of ``s`` on purpose:
one that depended on ``s`` would add a term to the gradient (:func:`prewhitening` is a data-only choice).
``L = 0, f = (1), mu = 0`` with a given filter is :class:`WeightedL2`'s ``e`` and ``r``.

Envelope misfit, :class:`EnvelopeL2` (``Engine.misfit_envelope``, ``fwi_misfit_envelope``, ``csrc/fwi_envelope.hip``):
when the starting model puts an arrival more than half a period off, every least-squares misfit above pulls the wrong
way (cycle skipping), and band-limiting only helps where the data have energy at low frequencies.  The envelope of a
trace carries its low-frequency content even when its spectrum does not (Bozdag et al. 2011; Wu et al. 2014).  The
Hilbert transformer ``H`` is an FIR filter with an antisymmetric impulse response, one-sided taps ``h_1 .. h_Q``
(:func:`hilbert_taps`), on the zero-extended trace, so that ``H^T = -H`` exactly; the power ``p`` is 1 or 2.  With
``s = d_syn``, ``d = d_obs``, ``B`` and ``M`` as above:

    s' = B s,   d' = B d
    (H x)[n, j] = sum_{k=1..Q} h_k (x[n - k, j] - x[n + k, j])      terms outside [0, nt) omitted
    E(x) = sqrt(x^2 + (H x)^2 + eps^2)                               eps absolute, independent of s
    e = M . (E(s')^p - E(d')^p)        J = 1/2 sum e^2
    c = p . M . e . E(s')^(p-2)        g1 = c . s'      g2 = c . (H s')
    r = dJ/ds = B (g1 - H g2)

``eps > 0`` is required for ``p = 1`` (``E`` is not differentiable at 0), ``eps >= 0`` allowed for ``p = 2``.  Like
``mu`` it must not follow ``s``: :func:`envelope_floor` is a data-only choice.  An envelope has no linear Gauss-Newton
weight: :class:`EnvelopeL2` is not a :class:`WeightedL2`.

Trace-normalised correlation misfit, :class:`NormalizedCorrelation` (``Engine.misfit_correlation``,
``fwi_misfit_correlation``, ``csrc/fwi_corr.hip``): every misfit above is a difference of amplitudes, and a constant-
density acoustic engine cannot model elastic amplitude-versus-offset, attenuation, receiver coupling or source strength.
The zero-lag normalised ("global") correlation of Choi & Alkhalifah 2012 reads phase only and ignores the gain of every
trace; it is the reference's ``CC`` measure (``objectives.correlation``) with weights, a band and a floor.  With
``s = d_syn``, ``d = d_obs``, ``B`` and ``M`` as above, ``w_j >= 0`` optional weights per trace (default 1) and
``eps >= 0`` an absolute floor:

    s' = B s,  d' = B d            (rounded to the context dtype once, only when taps are given)
    sh = M . s',  dh = M . d'
    a_j = sum_n sh[n,j]^2    b_j = sum_n dh[n,j]^2    c_j = sum_n sh[n,j] dh[n,j]
    ns_j = sqrt(a_j + eps^2)  nd_j = sqrt(b_j + eps^2)   rho_j = c_j / (ns_j nd_j)
    trace j counts iff  b_j > 0 and a_j + eps^2 > 0;  otherwise J_j = 0, rho_j = 0 and its adjoint source is 0
    J = sum_j w_j (1 - rho_j)
    alpha_j = -w_j / (ns_j nd_j)     beta_j = c_j / ns_j^2
    g = M . alpha_j (dh - beta_j sh)           (rounded to the dtype once)
    r = dJ/ds = B g

A scale per trace inside ``M`` cancels, so ``w`` is the only way to down-weight a trace.  Like ``mu`` and the envelope's
floor, ``eps`` must not follow ``s``: :func:`correlation_floor` is a data-only choice.  With ``eps = 0``, no weights, no
taps and mean-free traces, ``J / ntr`` and ``r / ntr`` are ``objectives.correlation(per_trace=True)``.  There is no
Gauss-Newton weight of the form ``B M^2 B``: :class:`NormalizedCorrelation` is not a :class:`WeightedL2`.

Cross-correlation traveltime misfit, :class:`TraveltimeL2` (``Engine.misfit_traveltime``, ``fwi_misfit_traveltime``,
``csrc/fwi_ttime.hip``): every misfit above compares the data at zero lag; none measures how late an arrival is, which
is what a poor starting model gets wrong first (Luo & Schuster 1991; the traveltime adjoint source of Tromp et al. 2005).
It grows with the square of the time shift however many periods the shift spans, ignores each trace's gain and returns a
physical number per trace, the delay in seconds.  With ``s = d_syn``, ``d = d_obs``, ``B``, ``M`` and ``w_j`` as above,
``K = max_lag >= 1`` in samples, ``Ke = min(K, nt - 1)`` and ``dt`` the sampling interval:

    s' = B s,  d' = B d            (rounded to the context dtype once, only when taps are given)
    sh = M . s',  dh = M . d'
    c_j(k) = sum_n sh[n + k, j] dh[n, j],   k = -Ke .. Ke       (terms with n + k outside [0, nt) omitted)
    k*_j = the smallest k with c_j(k) = max_k c_j(k)
    c-, c0, c+ = c_j(k* - 1), c_j(k*), c_j(k* + 1);   N = c- - c+,   Q = c- - 2 c0 + c+
    trace j counts iff  |k*| < Ke, c0 > 0 and Q < 0;  otherwise tau_j = 0, J_j = 0 and its adjoint source is 0
    delta_j = N / (2 Q) in [-1/2, 1/2],   tau_j = (k* + delta_j) dt,   J = 1/2 sum_j w_j tau_j^2        (s^2)
    D- = (Q - N) / (2 Q^2),  D0 = N / Q^2,  D+ = (-Q - N) / (2 Q^2)
    g[m, j] = M[m, j] w_j tau_j dt (D- dh[m - k* + 1, j] + D0 dh[m - k*, j] + D+ dh[m - k* - 1, j])
    r = dJ/ds = B g                (g rounded to the dtype once; rows outside [0, nt) contribute 0)

``tau > 0`` means the synthetics arrive late: for ``s(t) = d(t - tau)``, ``c`` peaks at ``+tau``.  A dead trace has
``c = 0`` everywhere, so ``k* = -Ke`` and it does not count; neither does a trace shifted beyond the window.  The picked
lag is locally constant and ``c`` is linear in ``sh``, so ``r`` is the exact gradient of this discrete ``J``.  ``J`` is
not differentiable where a trace starts or stops counting; ``tau`` is continuous where ``k*`` moves between neighbouring
lags (both parabolas then give ``delta = -+1/2`` at the same point).  No linear Gauss-Newton weight either.

Trace-by-trace optimal-transport misfit, :class:`TransportW2` (``Engine.misfit_transport``, ``fwi_misfit_transport``,
``csrc/fwi_ot.hip``): the envelope widens the basin by throwing the phase away, the traveltime misfit by reducing a trace
to one picked number.  The quadratic Wasserstein distance between the traces as densities along time (Engquist & Froese
2014; Yang, Engquist, Sun & Hamfeldt 2018) uses the whole trace, needs no pick and no window, and grows with the square
of a time shift however many periods the shift spans.  With ``s = d_syn``, ``d = d_obs``, ``B``, ``M``, ``w_j`` and
``dt`` as above and ``P`` a map onto positive numbers (below), per trace ``j``:

    s' = B s,  d' = B d            (rounded to the context dtype once, only when taps are given)
    sh = M . s',  dh = M . d'
    p_n = P(sh[n, j]),  q_n = P(dh[n, j])
    S_s = sum_n p_n,  S_d = sum_n q_n;   f_n = p_n / S_s,  g_n = q_n / S_d
    F_n = sum_{i<=n} f_i,  G_n = sum_{i<=n} g_i                      n = 0 .. nt - 1
    for n = 1 .. nt - 1, with the level y = F_{n-1}:
        m+(n) = min(#{m : G_m <= y}, nt - 1),   m-(n) = min(#{m : G_m < y}, nt - 1)
        a_n = 2 n - 1 - m+(n) - m-(n)                                an integer
      and the same with f and g exchanged: n+(m), n-(m), b_m = 2 m - 1 - n+(m) - n-(m)
    phi_0 = psi_0 = 0,  phi_n = sum_{i=1..n} a_i,  psi_m = sum_{i=1..m} b_i     integers, exact
    W_j = dt^2 (sum_n phi_n f_n + sum_m psi_m g_m)                   (s^2)
    J = 1/2 sum_j w_j W_j
    phibar_j = sum_n phi_n f_n
    g[n, j] = M[n, j] (w_j / 2) dt^2 (phi_n - phibar_j) / S_s  P'(sh[n, j])      (rounded to the dtype once)
    r = dJ/ds = B g

``W_j`` is the exact squared 2-Wasserstein distance between the atomic measures ``sum f_n delta(t_n)`` and
``sum g_n delta(t_n)``, ``(phi, psi) dt^2`` an optimal pair of Kantorovich potentials, and ``r`` the gradient of this
discrete ``J`` wherever no level ``F_n`` equals a level ``G_m``.  ``J`` is piecewise smooth: the gradient jumps where a
level of ``F`` crosses a level of ``G``; at a tie the two-sided count ``m+ + m-`` selects the midpoint subgradient, so
that ``d_obs == d_syn`` gives ``phi = psi = 0``, ``J = 0`` and ``r = 0`` exactly.  ``P`` is ``x + c`` (``linear``,
``c = param > 0``) or ``log(1 + exp(b x)) / b`` (``softplus``, ``b = param > 0``); like ``eps`` above, ``param`` is
absolute and must not follow ``s``.  A trace counts iff every ``p_n`` and ``q_n`` is finite and ``>= 0`` and both sums
are finite and ``> 0``; otherwise ``W_j = 0``, its term of ``J`` is 0 and its adjoint source is 0 (under ``linear`` a
trace that goes below ``-c`` drops out).  No linear Gauss-Newton weight either.

Adaptive (per-trace matching-filter) misfit, :class:`AdaptiveMatching` (``Engine.misfit_adaptive``,
``fwi_misfit_adaptive``, ``csrc/fwi_awi.hip``): adaptive waveform inversion (Warner & Guasch 2016).  The matching filter
above estimates one filter per shot, which absorbs the source signature and nothing else; this one designs one Wiener
filter per trace that turns the observed trace into the synthetic one, and penalises the filter's energy away from zero
lag, normalised by its energy.  It needs no pick and no window, keeps amplitude and phase, grows with the square of a time
shift up to the filter's half-length, and a gain per trace cancels exactly.  With ``s = d_syn``, ``d = d_obs``, ``B``,
``M``, the per-trace weights ``tw_j`` and ``dt`` as above, ``L >= 1``, ``K = 2 L + 1`` coefficients ``w_k``,
``k = -L .. L``, stored at ``w[k + L]``, and ``lam > 0`` a relative ridge, per trace ``j``, every trace zero-extended
outside ``[0, nt)``:

    s' = B s,  d' = B d            (rounded to the context dtype once, only when taps are given)
    sh = M . s',  dh = M . d'
    a_j(m) = sum_n dh[n, j] dh[n + m, j]            m = 0 .. 2 L   (0 once m > nt - 1)
    c_j(k) = sum_n sh[n + k, j] dh[n, j]            k = -L .. L    (= sum_n dh[n - k, j] sh[n, j])
    G_j[k, l] = a_j(|k - l|) + lam a_j(0) [k == l]  exactly Toeplitz: the fit runs over the whole convolution output
    w_j = G_j^-1 c_j                                the filter with  w * dh ~= sh,  linear in s
    N_j = sum_k w_k^2
    W_j = sum_k (k dt)^2 w_k^2 / N_j                (s^2)
    J   = 1/2 sum_j tw_j W_j
    y_k = tw_j w_k ((k dt)^2 - W_j) / N_j
    z_j = G_j^-1 y_j
    g[n, j] = M[n, j] sum_k z_k dh[n - k, j]        (rounded to the dtype once)
    r = dJ/ds = B g

``G_j`` depends on the data only, so the ridge relative to ``a_j(0)`` adds no term to the gradient and ``r`` is the exact
gradient of this discrete ``J``.  A trace counts iff ``a_j(0)`` is finite and ``> 0``, every Cholesky pivot of ``G_j`` is
finite and ``> 0`` and ``N_j`` is finite and ``> 0`` (a dead synthetic trace gives ``w = 0``); otherwise ``W_j = 0``, its
term of ``J``, its filter and its adjoint source are 0.  ``W_j <= (L dt)^2``; ``L`` may exceed ``nt - 1``.
``d_obs == d_syn`` does NOT give ``J = 0``: it gives the second moment of ``G^-1 a``, a band-limited delta, and a
non-zero ``r``; ``sqrt(W)`` is then the width the ridge and the bandwidth leave (4.1 samples for a 25 Hz Ricker at
2 ms, ``L = 64``, ``lam = 1e-2``), the floor below which a shift cannot be read.  ``J`` is not differentiable where a
trace starts or stops counting.  The condition number of ``G_j`` is at most ``1 + K / lam``.  No linear Gauss-Newton
weight either.

Frequency-domain (spectral) misfit, :class:`SpectralMisfit` (``Engine.misfit_spectral``, ``fwi_misfit_spectral``,
``csrc/fwi_spec.hip``): every misfit above compares traces in the time domain.  This one compares the discrete Fourier
coefficients of the weighted, filtered gathers at up to 64 frequencies of the caller's choice -- their difference, their
phases, their logarithmic amplitudes or both (the logarithmic misfit of Shin & Min 2006) -- with a weight per frequency
and per trace: the data side of frequency-domain FWI from time-domain modelling, whose model side is the Fourier store
(:mod:`fourier`).  The definition stands in the class's docstring, in the words of ``include/fwi.h``;
:func:`spectral_floor`, :func:`whitening_weights` and :func:`laplace_damping` are its data-only helpers.  No linear
Gauss-Newton weight is offered either.
"""
from __future__ import annotations

import math

import numpy as np

R_MAX = 4096  # the largest half-width the device path accepts (fwi_misfit_weighted)
L_MAX = 64    # the largest half-length of a matching filter the device path accepts (fwi_misfit_matched)
K_MAX = 1024  # the largest window of lags, in samples, the device path accepts (fwi_misfit_traveltime)


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

    # What the shot loop asks of an objective (shots._sweep_shots): the engine method of its device path, that call for
    # shot number i (returns J; the adjoint source stays on the device), and the host call (returns J and the residual)
    engine_method = "misfit_weighted"

    def device(self, engine, shot, i):
        return engine.misfit_weighted(shot.d_obs, shot.weights, self.taps)

    def host(self, d_syn, shot, i):
        return self(d_syn, shot.d_obs, shot.weights)

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


class _Prefiltered:
    """What the misfits that filter both gathers first share: ``taps`` and ``dtype``, the rounding a device context of
    that dtype does, ``s' = B s`` and ``d' = B d`` with the checked weights."""

    def _band(self, taps, dtype):
        self.taps = _checked_taps(taps)
        self.dtype = None if dtype is None else np.dtype(dtype)

    def _round(self, x):
        return x if self.dtype is None else x.astype(self.dtype).astype(np.float64)

    def filter(self, x):
        """``B x`` (rounded to ``dtype`` once)"""
        return self._round(fir_time(x, self.taps))

    def _prepared(self, d_syn, d_obs, weights):
        s, d = np.asarray(d_syn, np.float64), np.asarray(d_obs, np.float64)
        if s.ndim != 2 or s.shape != d.shape:
            raise ValueError("d_syn %r and d_obs %r must be (nt, ntr) alike" % (s.shape, d.shape))
        return self.filter(s), self.filter(d), WeightedL2._weights(weights, s.shape)


class _PerTrace(_Prefiltered):
    """... and the sums over traces on top: the weighted gathers ``sh = M . s'`` and ``dh = M . d'``, the weights per trace
    (the shot loop hands them ``Shot.trace_weights``) and the way from ``g`` to the residual ``B g``."""

    def filter(self, x):
        """``B x`` (rounded to ``dtype`` once; without taps a copy of x)"""
        return fir_time(x, None) if self.taps is None else self._round(fir_time(x, self.taps))

    def _weighted(self, d_syn, d_obs, weights):
        """``(sh, dh, M)``"""
        sh, dh, M = self._prepared(d_syn, d_obs, weights)
        return (sh, dh, M) if M is None else (M * sh, M * dh, M)

    @staticmethod
    def _trace_weights(trace_weights, ntr):
        """``w``: the checked weights per trace, or ones"""
        w = np.ones(ntr) if trace_weights is None else np.asarray(trace_weights, np.float64)
        if w.shape != (ntr,):
            raise ValueError("trace_weights have shape %r, the data %d traces" % (w.shape, ntr))
        if not np.all(np.isfinite(w)) or np.any(w < 0.0):
            raise ValueError("trace_weights must be finite and >= 0")
        return w

    def _residual(self, g, weights):
        """``B`` (``M . g`` rounded to ``dtype`` once)"""
        g = self._round(g if weights is None else np.asarray(weights, np.float64) * g)
        return g if self.taps is None else fir_time(g, self.taps)

    def host(self, d_syn, shot, i):
        return self(d_syn, shot.d_obs, shot.weights, shot.trace_weights)


def _conv_time(x, f, transpose=False):
    """``C_f x`` (``C_f^T x`` with ``transpose``) along axis 0, ``f = (f_-L .. f_L)``, added over ascending k in fp64."""
    x = np.asarray(x, np.float64)
    f = np.asarray(f, np.float64)
    L, nt = (len(f) - 1) // 2, x.shape[0]
    out = np.zeros_like(x)
    for k in range(-L, L + 1):
        sh = -k if transpose else k  # out[n] += f_k x[n - sh]
        if abs(sh) >= nt:
            continue
        if sh >= 0:
            out[sh:] += f[k + L] * x[:nt - sh]
        else:
            out[:nt + sh] += f[k + L] * x[-sh:]
    return out


class MatchedL2(_Prefiltered):
    """The matching-filter misfit of the module's definition in fp64 NumPy, and the ``objective=`` that
    ``shots.misfit_and_gradient`` recognises (an engine that has ``misfit_matched`` replaces it by the device path).

    ``L``: the half-length of the filter, ``K = 2 L + 1`` coefficients ``f[k + L] = f_k``.  ``mu``: the absolute damping
    ``>= 0`` of the normal equations -- one number for every shot, or a sequence indexed like the list of shots (the shot
    loop passes ``shot=`` and reads ``mu[shot]``): data-only numbers such as :func:`prewhitening` of each shot's
    ``d_obs``, computed once and held through an inversion.  ``taps``: the one-sided ``b_0 .. b_R`` of ``B``, or None.
    ``dtype``: round ``B s`` and ``B d`` to it once, as a device context of that dtype does (None: keep fp64).

    ``filters`` maps a shot's index to the last ``f*`` the shot loop estimated for it (device or host branch alike).
    Not a :class:`WeightedL2`: the Gauss-Newton operator of the reduced objective is not ``B M^2 B``."""

    def __init__(self, L, mu, taps=None, dtype=None):
        if int(L) != L or not 0 <= int(L) <= L_MAX:
            raise ValueError("L must be an integer in [0, %d]" % L_MAX)
        self.L, self.K = int(L), 2 * int(L) + 1
        mu_all = np.atleast_1d(np.asarray(mu, np.float64))
        if mu_all.ndim != 1 or not np.all(np.isfinite(mu_all)) or np.any(mu_all < 0.0):
            raise ValueError("mu must be finite and >= 0 (a number, or one per shot)")
        self.mu = float(mu) if np.ndim(mu) == 0 else mu_all
        self._band(taps, dtype)
        self.filters = {}

    def mu_of(self, shot=None):
        """the damping of shot ``shot`` (the scalar ``mu`` for every shot, or ``mu[shot]``)"""
        if np.ndim(self.mu) == 0:
            return self.mu
        if shot is None:
            raise ValueError("mu is given per shot: the call needs shot=")
        return float(self.mu[shot])

    engine_method = "misfit_matched"

    def device(self, engine, shot, i):
        J, self.filters[i] = engine.misfit_matched(shot.d_obs, self.L, self.mu_of(i), shot.weights, self.taps)
        return J

    def host(self, d_syn, shot, i):
        return self(d_syn, shot.d_obs, shot.weights, shot=i)

    def normal(self, d_syn, d_obs, weights=None):
        """``(G, b)`` of the definition: ``G`` is ``K x K``, symmetric, without ``mu``."""
        s1, d1, M = self._prepared(d_syn, d_obs, weights)
        nt, ntr = s1.shape
        L, K = self.L, self.K
        G, b = np.zeros((K, K)), np.zeros(K)
        step = max(1, (1 << 22) // (K * nt))  # traces per block: the K shifted copies stay below 32 MB
        for j0 in range(0, ntr, step):
            sl = slice(j0, min(j0 + step, ntr))
            Z = np.zeros((K, nt, sl.stop - sl.start))
            for k in range(-L, L + 1):  # Z[k + L][n] = s'[n - k]
                if k >= nt or -k >= nt:
                    continue
                if k >= 0:
                    Z[k + L, k:] = s1[:nt - k, sl]
                else:
                    Z[k + L, :nt + k] = s1[-k:, sl]
            Zw = Z if M is None else Z * (M[:, sl] * M[:, sl])
            Z2, Zw2 = Z.reshape(K, -1), Zw.reshape(K, -1)
            G += Zw2 @ Z2.T
            b += Zw2 @ d1[:, sl].reshape(-1)
        return 0.5 * (G + G.T), b

    def solve(self, G, b, mu=None):
        """``f* = (G + mu I)^-1 b``; ``mu``: this objective's scalar unless given.  Raises
        ``ValueError`` when ``G + mu I`` is not positive definite (raise ``mu``)."""
        mu = self.mu_of() if mu is None else float(mu)
        A = np.asarray(G, np.float64) + mu * np.eye(len(b))
        try:
            np.linalg.cholesky(A)  # (the test of definiteness the device path makes)
        except np.linalg.LinAlgError:
            raise ValueError("the normal matrix G + mu I (mu = %g) is not positive definite: raise mu" % mu) from None
        return np.linalg.solve(A, np.asarray(b, np.float64))

    def apply(self, d_syn, d_obs, f, weights=None, mu=None):
        """``(J, r)`` at the given filter: ``J = Phi(f; d_syn)``, ``r = B C_f^T (M . e)``, which is ``dJ/dd_syn`` of the
        reduced objective when ``f`` is the minimiser :meth:`solve` returns."""
        mu = self.mu_of() if mu is None else float(mu)
        f = np.asarray(f, np.float64)
        if f.shape != (self.K,):
            raise ValueError("f must hold the 2 L + 1 = %d coefficients f_-L .. f_L" % self.K)
        s1, d1, M = self._prepared(d_syn, d_obs, weights)
        e = _conv_time(s1, f) - d1
        if M is not None:
            e *= M
        J = 0.5 * float(np.sum(e * e)) + 0.5 * mu * float(np.sum(f * f))
        return J, fir_time(_conv_time(e if M is None else M * e, f, transpose=True), self.taps)

    def __call__(self, d_syn, d_obs, weights=None, shot=None):
        """Estimate ``f*``, then :meth:`apply` it.  ``shot``: the index whose ``mu`` is read and under which ``f*`` is kept
        in ``filters`` (the shot loop passes it)."""
        mu = self.mu_of(shot)
        f = self.solve(*self.normal(d_syn, d_obs, weights), mu=mu)
        if shot is not None:
            self.filters[shot] = f
        return self.apply(d_syn, d_obs, f, weights, mu=mu)


def hilbert_taps(Q):
    """One-sided taps ``h_1 .. h_Q`` of a Hann-windowed FIR Hilbert transformer: ``2 / (pi k)`` for odd ``k``, 0 for even
    ``k``, times ``(1 + cos(pi k / (Q + 1))) / 2``.  Its response ``2 sum h_k sin(w k)`` is within 2e-3 of 1 from
    ``w = 4 pi / (Q + 1)`` to ``pi - 4 pi / (Q + 1)`` (:func:`hilbert_halfwidth`)."""
    if int(Q) != Q or not 1 <= int(Q) <= R_MAX:
        raise ValueError("Q must be an integer in [1, %d]" % R_MAX)
    k = np.arange(1, int(Q) + 1, dtype=np.float64)
    h = np.where(np.arange(1, int(Q) + 1) % 2 == 1, 2.0 / (np.pi * k), 0.0)
    return h * 0.5 * (1.0 + np.cos(np.pi * k / (int(Q) + 1)))


def hilbert_halfwidth(dt, f_lo):
    """``Q = ceil(2 / (f_lo dt)) - 1``: the half-width at which :func:`hilbert_taps` is good from ``f_lo`` (Hz) to
    Nyquist minus ``f_lo`` at the sampling interval ``dt``.  Raises above ``R_MAX``."""
    if not (float(dt) > 0.0 and np.isfinite(dt)):
        raise ValueError("dt must be > 0")
    if not (0.0 < float(f_lo) < 0.5 / float(dt)):
        raise ValueError("f_lo = %g outside (0, Nyquist = %g)" % (f_lo, 0.5 / float(dt)))
    Q = max(int(math.ceil(round(2.0 / (float(f_lo) * float(dt)), 9))) - 1, 1)  # (2 / (5 * 1e-3) is not 400 in fp64)
    if Q > R_MAX:
        raise ValueError("f_lo = %g at dt = %g needs Q = %d taps, above %d: raise f_lo" % (f_lo, dt, Q, R_MAX))
    return Q


def _checked_hilbert(h):
    h = np.ascontiguousarray(np.asarray(h, np.float64))
    if h.ndim != 1 or not 1 <= h.size <= R_MAX or not np.all(np.isfinite(h)):
        raise ValueError("hilbert must be a finite 1-D array h_1 .. h_Q, Q in [1, %d]" % R_MAX)
    return h


def hilbert_matrix(h, nt):
    """``H`` as the dense antisymmetric ``nt x nt`` Toeplitz matrix of the zero-extended filter: ``H[n, n - k] = h_k``,
    ``H[n, n + k] = -h_k``."""
    col = np.zeros(nt)
    m = min(len(h), nt - 1)
    col[1:m + 1] = h[:m]
    i = np.arange(nt)
    d = i[:, None] - i[None, :]
    return np.sign(d) * col[np.abs(d)]


def hilbert_time(x, h):
    """``H x`` along axis 0 in fp64."""
    x = np.asarray(x, np.float64)
    h = np.asarray(h, np.float64)
    nt = x.shape[0]
    if min(len(h), nt - 1) > _DENSE_MIN_R and nt <= _DENSE_MAX_NT and x.ndim == 2:
        return hilbert_matrix(h, nt) @ x
    out = np.zeros_like(x)
    for k in range(1, min(len(h), nt - 1) + 1):
        if h[k - 1] != 0.0:
            out[k:] += h[k - 1] * x[:nt - k]
            out[:nt - k] -= h[k - 1] * x[k:]
    return out


def envelope_floor(d_obs, percent=1.0):
    """``percent / 100 * max |d_obs|``: a floor ``eps`` for :class:`EnvelopeL2` that depends on the data only -- like
    :func:`prewhitening`, compute it once per shot and hold it through an inversion."""
    if not (float(percent) >= 0.0 and np.isfinite(percent)):
        raise ValueError("percent must be finite and >= 0")
    d = np.asarray(d_obs, np.float64)
    return float(percent) / 100.0 * (float(np.max(np.abs(d))) if d.size else 0.0)


class EnvelopeL2(_Prefiltered):
    """The envelope misfit of the module's definition in fp64 NumPy, ``objective(d_syn, d_obs, weights=None) -> (J, r)``,
    and the ``objective=`` that ``shots.misfit_and_gradient`` recognises (an engine that has ``misfit_envelope`` replaces
    it by the device path).

    ``hilbert``: the one-sided taps ``h_1 .. h_Q`` (:func:`hilbert_taps`).  ``power``: 1 or 2.  ``eps``: the absolute
    floor under the envelope, ``> 0`` for ``power=1``; None: :func:`envelope_floor` of each call's ``d_obs`` at
    ``floor_percent``, a data-only number.  ``taps``: the one-sided ``b_0 .. b_R`` of ``B``, or None.  ``dtype``: round
    ``B s``, ``B d``, ``g1``, ``g2`` and ``g1 - H g2`` to it once each, as a device context of that dtype does (None:
    keep fp64).

    Not a :class:`WeightedL2`: an envelope has no linear Gauss-Newton weight, and ``gauss_newton_hvp`` refuses it."""

    def __init__(self, hilbert, power=1, eps=None, taps=None, dtype=None, floor_percent=1.0):
        self.hilbert = _checked_hilbert(hilbert)
        if power not in (1, 2):
            raise ValueError("power must be 1 or 2")
        self.power = int(power)
        if eps is not None and not (float(eps) >= 0.0 and np.isfinite(eps) and (float(eps) > 0.0 or self.power == 2)):
            raise ValueError("eps must be finite and >= 0, and > 0 for power 1")
        self.eps = None if eps is None else float(eps)
        self.floor_percent = float(floor_percent)
        self._band(taps, dtype)

    def eps_of(self, d_obs):
        """the floor of a shot: ``eps``, or :func:`envelope_floor` of its observed data"""
        return self.eps if self.eps is not None else envelope_floor(d_obs, self.floor_percent)

    engine_method = "misfit_envelope"

    def device(self, engine, shot, i):
        return engine.misfit_envelope(shot.d_obs, self.hilbert, self.power, self.eps_of(shot.d_obs), shot.weights, self.taps)

    host = WeightedL2.host

    def envelope2(self, x1, eps):
        """``(E(x')^2, H x')`` of an already filtered gather"""
        hx = hilbert_time(x1, self.hilbert)
        return x1 * x1 + (hx * hx + eps * eps), hx

    def __call__(self, d_syn, d_obs, weights=None):
        s1, d1, M = self._prepared(d_syn, d_obs, weights)
        eps = self.eps_of(np.asarray(d_obs, np.float64))
        if self.power == 1 and not eps > 0.0:
            raise ValueError("power 1 needs eps > 0")
        es2, hs = self.envelope2(s1, eps)
        ed2, _ = self.envelope2(d1, eps)
        if self.power == 1:
            es = np.sqrt(es2)
            e = es - np.sqrt(ed2)
        else:
            e = es2 - ed2
        if M is not None:
            e = M * e
        c = e if M is None else M * e
        c = c / es if self.power == 1 else 2.0 * c
        g1, g2 = self._round(c * s1), self._round(c * hs)
        q = self._round(g1 - hilbert_time(g2, self.hilbert))
        return 0.5 * float(np.sum(e * e)), (q if self.taps is None else fir_time(q, self.taps))


def correlation_floor(d_obs, percent=1.0):
    """``percent / 100 * max_j ||d_obs[:, j]||_2``: a floor ``eps`` for :class:`NormalizedCorrelation` that depends on the
    data only -- like :func:`envelope_floor`, compute it once per shot and hold it through an inversion."""
    if not (float(percent) >= 0.0 and np.isfinite(percent)):
        raise ValueError("percent must be finite and >= 0")
    d = np.asarray(d_obs, np.float64)
    if d.ndim != 2:
        raise ValueError("d_obs must be (nt, ntr)")
    return float(percent) / 100.0 * (float(np.sqrt(np.max(np.sum(d * d, axis=0)))) if d.size else 0.0)


class NormalizedCorrelation(_PerTrace):
    """The trace-normalised correlation misfit of the module's definition in fp64 NumPy,
    ``objective(d_syn, d_obs, weights=None, trace_weights=None) -> (J, r)``, and the ``objective=`` that
    ``shots.misfit_and_gradient`` recognises (an engine that has ``misfit_correlation`` replaces it by the device path;
    the shot loop hands it ``Shot.weights`` and ``Shot.trace_weights``).

    ``eps``: the absolute floor ``>= 0`` under the trace norms; None: :func:`correlation_floor` of each call's ``d_obs``
    at ``floor_percent``, a data-only number.  ``taps``: the one-sided ``b_0 .. b_R`` of ``B``, or None.  ``dtype``: round
    ``B s``, ``B d`` (with taps) and ``g`` to it once each, as a device context of that dtype does (None: keep fp64).

    ``correlations`` holds the ``rho_j`` of the last call (0 where a trace does not count).  Not a :class:`WeightedL2`:
    there is no linear Gauss-Newton weight, and ``gauss_newton_hvp`` refuses it."""

    def __init__(self, eps=None, taps=None, dtype=None, floor_percent=1.0):
        if eps is not None and not (float(eps) >= 0.0 and np.isfinite(eps)):
            raise ValueError("eps must be finite and >= 0")
        if not (float(floor_percent) >= 0.0 and np.isfinite(floor_percent)):
            raise ValueError("floor_percent must be finite and >= 0")
        self.eps = None if eps is None else float(eps)
        self.floor_percent = float(floor_percent)
        self._band(taps, dtype)
        self.correlations = None

    def eps_of(self, d_obs):
        """the floor of a shot: ``eps``, or :func:`correlation_floor` of its observed data"""
        return self.eps if self.eps is not None else correlation_floor(d_obs, self.floor_percent)

    engine_method = "misfit_correlation"

    def device(self, engine, shot, i):
        return engine.misfit_correlation(shot.d_obs, self.eps_of(shot.d_obs), shot.weights, self.taps, shot.trace_weights)

    def sums(self, d_syn, d_obs, weights=None):
        """``(a, b, c, sh, dh)`` of the definition: the per-trace sums and the weighted, filtered gathers"""
        sh, dh, _ = self._weighted(d_syn, d_obs, weights)
        return np.sum(sh * sh, axis=0), np.sum(dh * dh, axis=0), np.sum(sh * dh, axis=0), sh, dh

    def __call__(self, d_syn, d_obs, weights=None, trace_weights=None):
        a, b, c, sh, dh = self.sums(d_syn, d_obs, weights)
        w = self._trace_weights(trace_weights, a.size)
        eps = self.eps_of(d_obs)
        a2, b2 = a + eps * eps, b + eps * eps
        counts = (b > 0.0) & (a2 > 0.0)
        nn = np.where(counts, np.sqrt(a2) * np.sqrt(b2), 1.0)
        rho = np.where(counts, c / nn, 0.0)
        alpha = np.where(counts, -w / nn, 0.0)
        beta = np.where(counts, c / np.where(counts, a2, 1.0), 0.0)
        self.correlations = rho
        return float(np.sum(np.where(counts, w * (1.0 - rho), 0.0))), self._residual(alpha * (dh - beta * sh), weights)


class TraveltimeL2(_PerTrace):
    """The cross-correlation traveltime misfit of the module's definition in fp64 NumPy,
    ``objective(d_syn, d_obs, weights=None, trace_weights=None) -> (J, r)``, and the ``objective=`` that
    ``shots.misfit_and_gradient`` recognises (an engine that has ``misfit_traveltime`` replaces it by the device path;
    the shot loop hands it ``Shot.weights`` and ``Shot.trace_weights``).

    ``dt``: the sampling interval in seconds.  ``max_lag``: the half-width ``K`` of the window of lags in samples,
    ``1 .. K_MAX``.  ``taps``: the one-sided ``b_0 .. b_R`` of ``B``, or None.  ``dtype``: round ``B s``, ``B d`` (with taps)
    and ``g`` to it once each, as a device context of that dtype does (None: keep fp64).

    ``delays`` holds the ``tau_j`` of the last call in seconds (0 where a trace does not count), ``lags`` the picked
    ``k*_j`` (counting or not) and ``counts`` which traces count.  ``J`` is not differentiable where a trace starts or
    stops counting; ``tau`` is continuous where ``k*`` moves between neighbouring lags.  Not a :class:`WeightedL2`: there
    is no linear Gauss-Newton weight, and ``gauss_newton_hvp`` refuses it."""

    def __init__(self, dt, max_lag, taps=None, dtype=None):
        if not (float(dt) > 0.0 and np.isfinite(dt)):
            raise ValueError("dt must be > 0")
        if int(max_lag) != max_lag or not 1 <= int(max_lag) <= K_MAX:
            raise ValueError("max_lag must be an integer number of samples in [1, %d]" % K_MAX)
        self.dt = float(dt)
        self.max_lag = int(max_lag)
        self._band(taps, dtype)
        self.delays = self.lags = self.counts = None

    engine_method = "misfit_traveltime"

    def device(self, engine, shot, i):
        return engine.misfit_traveltime(shot.d_obs, self.max_lag, shot.weights, self.taps, shot.trace_weights)

    def correlations(self, d_syn, d_obs, weights=None, majorants=True):
        """``(c, A, sh, dh)``: ``c[k + Ke, j] = c_j(k)`` of the definition for ``k = -Ke .. Ke``, its majorant
        ``A[k + Ke, j] = sum_n |sh[n + k, j]| |dh[n, j]|`` (None without ``majorants``) and the weighted, filtered
        gathers"""
        sh, dh, _ = self._weighted(d_syn, d_obs, weights)
        nt, ntr = sh.shape
        Ke = max(min(self.max_lag, nt - 1), 0)
        c, A = np.zeros((2 * Ke + 1, ntr)), (np.zeros((2 * Ke + 1, ntr)) if majorants else None)
        ash, adh = (np.abs(sh), np.abs(dh)) if majorants else (None, None)
        for k in range(-Ke, Ke + 1):
            a, b = (slice(k, nt), slice(0, nt - k)) if k >= 0 else (slice(0, nt + k), slice(-k, nt))
            c[k + Ke] = np.sum(sh[a] * dh[b], axis=0)
            if majorants:
                A[k + Ke] = np.sum(ash[a] * adh[b], axis=0)
        return c, A, sh, dh

    def pick(self, c, trace_weights=None):
        """``(lags, counts, tau, coef, w)`` from ``c``: ``coef[i + 1, j] = w_j tau_j dt D_i`` for ``i = -1, 0, 1``, with
        ``(c-, c0, c+)`` stacked behind them in ``coef[3:6]``, and the trace weights as used"""
        nlag, ntr = c.shape
        Ke = (nlag - 1) // 2
        w = self._trace_weights(trace_weights, ntr)
        if ntr == 0:
            return np.zeros(0, np.int32), np.zeros(0, bool), np.zeros(0), np.zeros((6, 0)), w
        q = np.argmax(c, axis=0)  # the first maximum
        j = np.arange(ntr)
        inside = (q > 0) & (q < nlag - 1)
        qs = np.where(inside, q, 1 if nlag >= 3 else 0)
        cm = np.where(inside, c[np.maximum(qs - 1, 0), j], 0.0)
        c0 = c[q, j]
        cp = np.where(inside, c[np.minimum(qs + 1, nlag - 1), j], 0.0)
        N, Q = cm - cp, cm - 2.0 * c0 + cp
        counts = inside & (c0 > 0.0) & (Q < 0.0)
        Qs = np.where(counts, Q, 1.0)
        tau = np.where(counts, ((q - Ke).astype(np.float64) + N / (2.0 * Qs)) * self.dt, 0.0)
        a, q2 = w * tau * self.dt, Qs * Qs
        coef = np.zeros((6, ntr))
        coef[0] = np.where(counts, a * ((Q - N) / (2.0 * q2)), 0.0)
        coef[1] = np.where(counts, a * (N / q2), 0.0)
        coef[2] = np.where(counts, a * ((-Q - N) / (2.0 * q2)), 0.0)
        coef[3], coef[4], coef[5] = cm, c0, cp
        return (q - Ke).astype(np.int32), counts, tau, coef, w

    def __call__(self, d_syn, d_obs, weights=None, trace_weights=None):
        c, _, _, dh = self.correlations(d_syn, d_obs, weights, majorants=False)
        nt, ntr = dh.shape
        lags, counts, tau, coef, w = self.pick(c, trace_weights)
        self.lags, self.counts, self.delays = lags, counts, tau
        # dh at the rows m - k* + 1, m - k*, m - k* - 1; rows outside [0, nt) contribute 0
        g = np.zeros((nt, ntr))
        if nt and ntr:
            m = np.arange(nt)[:, None]
            for i, off in enumerate((1, 0, -1)):
                rows = m - lags[None, :].astype(np.int64) + off
                ok = (rows >= 0) & (rows < nt)
                g += coef[i] * np.where(ok, np.take_along_axis(dh, np.clip(rows, 0, nt - 1), axis=0), 0.0)
        return float(np.sum(np.where(counts, 0.5 * w * (tau * tau), 0.0))), self._residual(g, weights)


OT_TRANSFORMS = {"linear": 0, "softplus": 1}  # FWI_OT_LINEAR, FWI_OT_SOFTPLUS


class TransportW2(_PerTrace):
    """The trace-by-trace optimal-transport (W2) misfit of the module's definition in fp64 NumPy,
    ``objective(d_syn, d_obs, weights=None, trace_weights=None) -> (J, r)``, and the ``objective=`` that
    ``shots.misfit_and_gradient`` recognises (an engine that has ``misfit_transport`` replaces it by the device path; the
    shot loop hands it ``Shot.weights`` and ``Shot.trace_weights``).

    ``dt``: the sampling interval in seconds.  ``transform``: ``"softplus"`` or ``"linear"``.  ``param``: the absolute
    ``b`` or ``c`` of the transform, ``> 0``; None: :meth:`param_of` of each call's ``d_obs``, a data-only number,
    ``b = sharpness / max|d_obs|`` or ``c = factor * max|d_obs|``.  The defaults ``sharpness = 4`` and ``factor = 10``
    keep ``W`` strictly increasing with the shift of a Ricker wavelet through 60 samples (a sharpness
    of 2 or a factor of 3 and less do not; the linear transform is nearly flat beyond 30 samples even so, and a factor
    below 1 lets the observed data themselves violate positivity).  ``taps``: the one-sided ``b_0 .. b_R`` of ``B``, or
    None.  ``dtype``: round ``B s``, ``B d`` (with taps) and ``g`` to it once each, as a device context of that dtype
    does (None: keep fp64).

    ``distances`` holds the ``W_j`` of the last call in s^2 (0 where a trace does not count) and ``counts`` which traces
    count.  ``J`` is piecewise smooth: its gradient jumps where a level of ``F`` crosses a level of ``G``.  Not a
    :class:`WeightedL2`: there is no linear Gauss-Newton weight, and ``gauss_newton_hvp`` refuses it."""

    def __init__(self, dt, transform="softplus", param=None, taps=None, dtype=None, sharpness=4.0, factor=10.0):
        if not (float(dt) > 0.0 and np.isfinite(dt)):
            raise ValueError("dt must be > 0")
        if transform not in OT_TRANSFORMS:
            raise ValueError("transform must be one of %s" % sorted(OT_TRANSFORMS))
        for name, v in (("param", param), ("sharpness", sharpness), ("factor", factor)):
            if v is not None and not (float(v) > 0.0 and np.isfinite(v)):
                raise ValueError("%s must be finite and > 0" % name)
        self.dt = float(dt)
        self.transform = transform
        self.param = None if param is None else float(param)
        self.sharpness, self.factor = float(sharpness), float(factor)
        self._band(taps, dtype)
        self.distances = self.counts = None

    def param_of(self, d_obs):
        """the parameter of a shot: ``param``, or ``sharpness / max|d_obs|`` (softplus), ``factor * max|d_obs|`` (linear)"""
        if self.param is not None:
            return self.param
        d = np.asarray(d_obs, np.float64)
        peak = float(np.max(np.abs(d))) if d.size else 0.0
        if not (peak > 0.0 and np.isfinite(peak)):
            raise ValueError("d_obs is all zero or not finite: give param")
        return self.sharpness / peak if self.transform == "softplus" else self.factor * peak

    engine_method = "misfit_transport"

    def device(self, engine, shot, i):
        return engine.misfit_transport(shot.d_obs, self.transform, self.param_of(shot.d_obs), shot.weights, self.taps,
                                       shot.trace_weights)

    def positive(self, x, param):
        """``(P(x), P'(x))`` of the transform"""
        if self.transform == "linear":
            return x + param, np.ones_like(x)
        z = param * x
        with np.errstate(over="ignore", invalid="ignore"):
            e = np.exp(-np.abs(z))
            return (np.maximum(z, 0.0) + np.log1p(e)) / param, np.where(x >= 0.0, 1.0 / (1.0 + e), e / (1.0 + e))

    def cdfs(self, d_syn, d_obs, weights=None, param=None):
        """``(F, G, f, g, S_s, S_d, counts, dP, M)``: the normalised CDFs and densities ``(nt, ntr)``, the masses, which
        traces count, ``P'(sh)`` and the weights as used.  A trace that does not count is given uniform densities, so
        that everything downstream of it stays finite; its results are zeroed by the caller."""
        sh, dh, M = self._weighted(d_syn, d_obs, weights)
        param = self.param_of(d_obs) if param is None else float(param)
        p, dP = self.positive(sh, param)
        q, _ = self.positive(dh, param)
        with np.errstate(over="ignore", invalid="ignore"):
            Ss, Sd = np.sum(p, axis=0), np.sum(q, axis=0)
            counts = (np.all(np.isfinite(p) & (p >= 0.0), axis=0) & np.all(np.isfinite(q) & (q >= 0.0), axis=0)
                      & np.isfinite(Ss) & np.isfinite(Sd) & (Ss > 0.0) & (Sd > 0.0))
        p, q, dP = np.where(counts, p, 1.0), np.where(counts, q, 1.0), np.where(counts, dP, 0.0)
        Ss, Sd = np.sum(p, axis=0), np.sum(q, axis=0)
        return np.cumsum(p, axis=0) / Ss, np.cumsum(q, axis=0) / Sd, p / Ss, q / Sd, Ss, Sd, counts, dP, M

    @staticmethod
    def indices(F, G):
        """``(m+, m-, n+, n-)``, each ``(nt - 1, ntr)`` int64: row ``n - 1`` holds the counts of the definition for the
        level ``F_{n-1}`` among ``G`` (``m+``: ``<=``, ``m-``: ``<``), and for ``G_{m-1}`` among ``F`` (``n+``, ``n-``),
        clipped at ``nt - 1``"""
        nt, ntr = F.shape
        L = max(nt - 1, 0)
        out = [np.zeros((L, ntr), np.int64) for _ in range(4)]
        for j in range(ntr):
            for k, (X, Y) in enumerate(((F[:, j], G[:, j]), (G[:, j], F[:, j]))):
                # the clip at nt - 1 leaves the last level out of the counts
                out[2 * k][:, j] = np.searchsorted(Y[:L], X[:L], side="right")
                out[2 * k + 1][:, j] = np.searchsorted(Y[:L], X[:L], side="left")
        return tuple(out)

    @classmethod
    def potentials(cls, F, G):
        """``(phi, psi)``: the integer Kantorovich potentials ``(nt, ntr)`` int64 in units of ``dt^2``"""
        nt, ntr = F.shape
        mp, mm, np_, nm = cls.indices(F, G)
        base = (2 * np.arange(1, nt, dtype=np.int64) - 1)[:, None]
        phi, psi = np.zeros((nt, ntr), np.int64), np.zeros((nt, ntr), np.int64)
        if nt > 1:
            phi[1:], psi[1:] = np.cumsum(base - mp - mm, axis=0), np.cumsum(base - np_ - nm, axis=0)
        return phi, psi

    def primal(self, F, G):
        """``W_j`` in s^2 by the primal formula, independent of the potentials: ``dt^2`` times the integral over the
        level ``u`` in (0, 1) of the squared distance between the two quantile functions, a sum over the merged
        breakpoints of ``F`` and ``G``"""
        nt, ntr = F.shape
        L = max(nt - 1, 0)
        W = np.zeros(ntr)
        for j in range(ntr):
            u = np.unique(np.clip(np.concatenate(([0.0], F[:L, j], G[:L, j], [1.0])), 0.0, 1.0))
            mid = 0.5 * (u[1:] + u[:-1])
            n, m = np.searchsorted(F[:L, j], mid, side="left"), np.searchsorted(G[:L, j], mid, side="left")
            W[j] = self.dt * self.dt * float(np.sum(np.diff(u) * (n - m).astype(np.float64) ** 2))
        return W

    def __call__(self, d_syn, d_obs, weights=None, trace_weights=None):
        F, G, f, g, Ss, _, counts, dP, M = self.cdfs(d_syn, d_obs, weights)
        w = self._trace_weights(trace_weights, F.shape[1])
        phi, psi = self.potentials(F, G)
        dt2 = self.dt * self.dt
        phibar = np.sum(phi * f, axis=0)
        W = np.where(counts, dt2 * (phibar + np.sum(psi * g, axis=0)), 0.0)
        self.distances, self.counts = W, counts
        src = np.where(counts, 0.5 * w * dt2 / Ss, 0.0) * (phi - phibar) * dP
        return float(np.sum(0.5 * w * W)), self._residual(src, M)


class AdaptiveMatching(_PerTrace):
    """The adaptive (per-trace matching-filter) misfit of the module's definition in fp64 NumPy,
    ``objective(d_syn, d_obs, weights=None, trace_weights=None) -> (J, r)``, and the ``objective=`` that
    ``shots.misfit_and_gradient`` recognises (an engine that has ``misfit_adaptive`` replaces it by the device path; the
    shot loop hands it ``Shot.weights`` and ``Shot.trace_weights``).

    ``dt``: the sampling interval in seconds.  ``L``: the half-length of the filters in samples, ``1 .. L_MAX``.
    ``lam``: the ridge ``> 0``, relative to each trace's ``a_j(0)``.  ``taps``: the one-sided ``b_0 .. b_R`` of ``B``, or
    None.  ``dtype``: round ``B s``, ``B d`` (with taps) and ``g`` to it once each, as a device context of that dtype
    does (None: keep fp64).

    ``moments`` holds the ``W_j`` of the last call in s^2, ``filters`` its ``w_j`` as ``(ntr, 2 L + 1)`` (both 0 where a
    trace does not count) and ``counts`` which traces count.  ``d_obs == d_syn`` does not give ``J = 0`` (the module's
    docstring).  The systems are solved by this class's own dense Cholesky factorisation, batched over the traces.  Not a
    :class:`WeightedL2`: there is no linear Gauss-Newton weight, and ``gauss_newton_hvp`` refuses it."""

    L_MAX = 64  # the largest half-length the device path accepts (fwi_misfit_adaptive)

    def __init__(self, dt, L, lam=1e-2, taps=None, dtype=None):
        if not (float(dt) > 0.0 and np.isfinite(dt)):
            raise ValueError("dt must be > 0")
        if int(L) != L or not 1 <= int(L) <= self.L_MAX:
            raise ValueError("L must be an integer number of samples in [1, %d]" % self.L_MAX)
        if not (float(lam) > 0.0 and np.isfinite(lam)):
            raise ValueError("lam must be finite and > 0")
        self.dt = float(dt)
        self.L = int(L)
        self.lam = float(lam)
        self._band(taps, dtype)
        self.moments = self.filters = self.counts = None

    engine_method = "misfit_adaptive"

    def device(self, engine, shot, i):
        return engine.misfit_adaptive(shot.d_obs, self.L, self.lam, shot.weights, self.taps, shot.trace_weights)

    def correlations(self, d_syn, d_obs, weights=None, majorants=True):
        """``(a, c, (Aa, Ac), sh, dh)``: ``a[m, j] = a_j(m)`` for ``m = 0 .. 2 L``, ``c[k + L, j] = c_j(k)`` for
        ``k = -L .. L``, their majorants, the same sums of absolute products (None without ``majorants``), and the
        weighted, filtered gathers"""
        sh, dh, _ = self._weighted(d_syn, d_obs, weights)
        nt, ntr = sh.shape
        L = self.L
        a, c = np.zeros((2 * L + 1, ntr)), np.zeros((2 * L + 1, ntr))
        Aa, Ac = (np.zeros_like(a), np.zeros_like(c)) if majorants else (None, None)
        ash, adh = (np.abs(sh), np.abs(dh)) if majorants else (None, None)
        for m in range(min(2 * L, nt - 1) + 1):
            a[m] = np.sum(dh[:nt - m] * dh[m:], axis=0)
            if majorants:
                Aa[m] = np.sum(adh[:nt - m] * adh[m:], axis=0)
        for k in range(-min(L, nt - 1), min(L, nt - 1) + 1):
            p, q = (slice(k, nt), slice(0, nt - k)) if k >= 0 else (slice(0, nt + k), slice(-k, nt))
            c[k + L] = np.sum(sh[p] * dh[q], axis=0)
            if majorants:
                Ac[k + L] = np.sum(ash[p] * adh[q], axis=0)
        return a, c, ((Aa, Ac) if majorants else None), sh, dh

    def normal(self, a):
        """``(G, alive)``: the ``(ntr, K, K)`` Toeplitz matrices ``a_j(|k - l|) + lam a_j(0) [k == l]`` and which traces
        have a finite ``a_j(0) > 0`` (the others are given the identity, so that everything downstream stays finite)"""
        K = 2 * self.L + 1
        a0 = a[0]
        alive = np.isfinite(a0) & (a0 > 0.0)
        k = np.arange(K)
        G = np.transpose(a[np.abs(k[:, None] - k[None, :])], (2, 0, 1)).copy()
        G[:, k, k] = a0[:, None] + self.lam * a0[:, None]
        G[~alive] = np.eye(K)
        return G, alive

    @staticmethod
    def cholesky(G):
        """``(F, ok)``: the lower Cholesky factors ``(ntr, K, K)`` of the batch, column by column, and which matrices had
        every pivot finite and ``> 0`` (a failed pivot is replaced by 1)"""
        n, K, _ = G.shape
        F, ok = np.zeros_like(G), np.ones(n, bool)
        for j in range(K):
            with np.errstate(invalid="ignore", over="ignore"):
                s = G[:, j:, j] - np.einsum("nik,nk->ni", F[:, j:, :j], F[:, j, :j])
                good = np.isfinite(s[:, 0]) & (s[:, 0] > 0.0)
            ok &= good
            p = np.sqrt(np.where(good, s[:, 0], 1.0))
            F[:, j, j] = p
            F[:, j + 1:, j] = s[:, 1:] / p[:, None]
        return F, ok

    @staticmethod
    def solve(F, b):
        """``(F F^T)^-1 b`` for the batch: ``b`` is ``(ntr, K)``"""
        K = F.shape[1]
        x = np.array(b, np.float64)
        for k in range(K):
            x[:, k] /= F[:, k, k]
            x[:, k + 1:] -= F[:, k + 1:, k] * x[:, k:k + 1]
        for k in range(K - 1, -1, -1):
            x[:, k] /= F[:, k, k]
            x[:, :k] -= F[:, k, :k] * x[:, k:k + 1]
        return x

    def __call__(self, d_syn, d_obs, weights=None, trace_weights=None):
        a, c, _, _, dh = self.correlations(d_syn, d_obs, weights, majorants=False)
        nt, ntr = dh.shape
        L, K = self.L, 2 * self.L + 1
        tw = self._trace_weights(trace_weights, ntr)
        G, alive = self.normal(a)
        F, ok = self.cholesky(G)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            w = self.solve(F, c.T)
            t2 = (np.arange(-L, L + 1, dtype=np.float64) * self.dt) ** 2
            N, S = np.sum(w * w, axis=1), np.sum(t2 * (w * w), axis=1)
            counts = alive & ok & np.isfinite(N) & (N > 0.0) & np.isfinite(S)
        Ns = np.where(counts, N, 1.0)
        w = np.where(counts[:, None], w, 0.0)
        W = np.where(counts, S / Ns, 0.0)
        y = np.where(counts[:, None], tw[:, None] * w * (t2[None, :] - W[:, None]) / Ns[:, None], 0.0)
        z = np.where(counts[:, None], self.solve(np.where(counts[:, None, None], F, np.eye(K)), y), 0.0)
        self.moments, self.filters, self.counts = W, w, counts
        g = np.zeros((nt, ntr))
        for k in range(-min(L, nt - 1), min(L, nt - 1) + 1):  # g[n] += z_k dh[n - k]
            if k >= 0:
                g[k:] += z[:, k + L] * dh[:nt - k]
            else:
                g[:nt + k] += z[:, k + L] * dh[-k:]
        g = np.where(counts[None, :], g, 0.0)
        return float(np.sum(0.5 * tw * W)), self._residual(g, weights)


ROBUST_KINDS = ("huber", "hybrid", "cauchy")  # FWI_ROBUST_HUBER, FWI_ROBUST_HYBRID, FWI_ROBUST_CAUCHY
# the threshold in units of the scale at which each norm keeps 95 % of least squares' efficiency on Gaussian residuals
# (Huber 1964; Holland & Welsch 1977); the hybrid norm's is the conventional 1
ROBUST_C = {"huber": 1.345, "hybrid": 1.0, "cauchy": 2.385}
MAD_TO_SIGMA = 1.4826  # 1 / Phi^-1(3/4): the median of |x| of a Gaussian sample, times this, estimates its sigma


def median_abs(e, weights=None, per_trace=True):
    """``(med, count)``: the lower median of ``|e|`` over the samples that count -- all of them, or with ``weights`` those
    whose weight is ``> 0`` -- and their number, per trace of the ``(nt, ntr)`` gather (two ``(ntr,)`` arrays) or with
    ``per_trace=False`` of the whole gather (two numbers).  The lower median is the order statistic ``(count - 1) // 2``,
    0-based, of ``np.sort``, which puts ``+inf`` and NaN last; ``count == 0`` gives 0.  The twin of
    ``Engine.residual_median``, which is handed ``d_obs`` and forms ``e = M . B (d_syn - d_obs)`` itself."""
    a = np.abs(np.asarray(e))
    if a.ndim != 2:
        raise ValueError("e must be (nt, ntr)")
    if not np.issubdtype(a.dtype, np.floating):
        a = a.astype(np.float64)
    keep = np.ones(a.shape, bool) if weights is None else np.asarray(weights) > 0
    if keep.shape != a.shape:
        raise ValueError("weights have shape %r, the data %r" % (keep.shape, a.shape))
    if not per_trace:
        a, keep = a.reshape(-1, 1), keep.reshape(-1, 1)
    count = np.sum(keep, axis=0).astype(np.int64)
    # the samples that do not count go behind everything, a NaN that counts included (which NaN is then all the same)
    s = np.sort(np.where(keep, a, np.nan), axis=0) if a.size else np.zeros((1, a.shape[1]))
    med = np.where(count > 0, s[np.maximum(count - 1, 0) // 2, np.arange(a.shape[1])], 0.0).astype(np.float64)
    return (med, count) if per_trace else (float(med[0]), int(count[0]))


def mad_scale(e, weights=None, per_trace=True):
    """``1.4826 *`` the lower median of ``|e|`` (:func:`median_abs`): the scale ``sigma`` of the residuals that a few
    outliers do not move, per trace or of the whole gather."""
    return MAD_TO_SIGMA * median_abs(e, weights, per_trace)[0]


class RobustMisfit(_PerTrace):
    """The robust (M-estimator) misfits in fp64 NumPy, ``objective(d_syn, d_obs, weights=None, trace_weights=None) ->
    (J, r)``, and the ``objective=`` that ``shots.misfit_and_gradient`` and ``shots.gauss_newton_hvp`` recognise (an
    engine that has ``misfit_robust`` replaces it by the device path; the shot loop hands it ``Shot.weights`` and
    ``Shot.trace_weights``).  With ``a_j = c sigma_j`` the threshold of trace j::

        e = M . B (s - d)                    (rounded to ``dtype`` once)
        v = (e / a_j)^2
        huber :  rho = e^2 / 2 if |e| <= a_j, a_j |e| - a_j^2 / 2 otherwise        psi = min(1, a_j / |e|)
        hybrid:  rho = e^2 / (1 + sqrt(1 + v))  = a^2 (sqrt(1 + v) - 1)            psi = 1 / sqrt(1 + v)
        cauchy:  rho = (a_j^2 / 2) log1p(v)                                        psi = 1 / (1 + v)
        J = sum_j tw_j sum_n rho[n, j]     g = tw_j psi e     r = dJ/ds = B (M . g)

    ``d_obs == d_syn`` gives ``J = 0`` and ``r = 0`` exactly.  ``|d(psi e)/de| <= 1``; huber is C^1 and the other two are
    smooth (no non-differentiable set); cauchy is NOT convex (``d(psi e)/de = -1/8`` at ``v = 3``).  huber with an
    infinite threshold is :class:`WeightedL2`, bit for bit.

    ``kind``: one of ``ROBUST_KINDS``.  ``c``: the threshold in units of the scale (None: ``ROBUST_C[kind]``).  ``scale``:
    the ``sigma`` of the residuals, which MUST NOT depend on the synthetics of the call it is used in (a threshold that
    did would add a term to the gradient): a float; a sequence indexed like ``shots`` of floats or ``(ntr,)`` arrays
    (``shots.residual_scales`` measures one at a given model: hold it through a stage); or None, a data-only default,
    ``1.4826 *`` the lower median of ``|M . B d_obs|`` per trace, which is CRUDE: it is the scale of the data, not of the
    residuals, and far too large near convergence.  A trace whose scale is 0 (dead, or more than half its samples zero)
    takes the largest threshold of its gather.  ``taps``, ``dtype`` as in the siblings.

    ``J_trace``, ``nout`` and ``psi`` hold the terms of J per trace, the number of samples beyond the threshold per trace
    and ``psi(e)`` of the last call; :meth:`normal` is the IRLS Gauss-Newton weight ``B (tw M^2 psi . B x)``
    (``Engine.residual_weight_robust``'s twin), positive semi-definite for every kind."""

    def __init__(self, kind="huber", c=None, scale=None, taps=None, dtype=None):
        if kind not in ROBUST_KINDS:
            raise ValueError("kind must be one of %s" % (ROBUST_KINDS,))
        c = ROBUST_C[kind] if c is None else float(c)
        if not (c > 0.0) or (np.isinf(c) and kind != "huber"):
            raise ValueError("c must be > 0, and finite unless kind is 'huber'")
        if self._one_number(scale) and not float(scale) > 0.0:
            raise ValueError("scale must be > 0")
        self.kind, self.c, self.scale = kind, c, scale
        self._band(taps, dtype)
        self.J_trace = self.nout = self.psi = None

    @staticmethod
    def _one_number(scale):
        """one scale for every shot (not None, not a sequence indexed like the shots, whose entries may differ in shape)"""
        return isinstance(scale, (int, float, np.integer, np.floating)) or (isinstance(scale, np.ndarray) and scale.ndim == 0)

    def residuals(self, d_syn, d_obs, weights=None):
        """``(e, M)``: ``e = M . B (d_syn - d_obs)`` rounded to ``dtype`` once, and the checked weights"""
        s, d = np.asarray(d_syn, np.float64), np.asarray(d_obs, np.float64)
        if s.ndim != 2 or s.shape != d.shape:
            raise ValueError("d_syn %r and d_obs %r must be (nt, ntr) alike" % (s.shape, d.shape))
        M = WeightedL2._weights(weights, s.shape)
        e = fir_time(s - d, self.taps)
        return self._round(e if M is None else M * e), M

    def scale_of(self, i, d_obs=None, weights=None):
        """the scale of shot ``i``: ``scale``, its entry ``i``, or the data-only default of the class's docstring"""
        if self.scale is None:
            if d_obs is None:
                raise ValueError("the default scale is formed from the observed data")
            d = np.asarray(d_obs, np.float64)
            return mad_scale(self.residuals(np.zeros_like(d), d, weights)[0], weights)
        if self._one_number(self.scale):
            return float(self.scale)
        if i is None:
            raise ValueError("a scale per shot needs the shot's index")
        return self.scale[i]

    def thresh_of(self, i, d_obs, weights=None):
        """the ``(ntr,)`` thresholds ``a_j = c sigma_j`` of shot ``i``"""
        ntr = np.shape(d_obs)[1]
        with np.errstate(invalid="ignore"):
            a = self.c * np.broadcast_to(np.asarray(self.scale_of(i, d_obs, weights), np.float64), (ntr,)).copy()
        if np.any(np.isnan(a)) or np.any(a < 0.0) or (np.any(np.isinf(a)) and self.kind != "huber"):
            raise ValueError("the scales must be >= 0, and finite unless kind is 'huber'")
        if np.any(a == 0.0):
            a[a == 0.0] = np.max(a) if np.any(a > 0.0) else 1.0
        return a

    engine_method = "misfit_robust"

    def device(self, engine, shot, i, keep_irls=False):
        return engine.misfit_robust(shot.d_obs, self.kind, self.thresh_of(i, shot.d_obs, shot.weights), shot.weights,
                                    self.taps, shot.trace_weights, keep_irls=keep_irls)

    def host(self, d_syn, shot, i):
        return self(d_syn, shot.d_obs, shot.weights, shot.trace_weights, shot=i)

    def irls(self, d_syn, shot, i):
        """``psi(e)`` of shot ``i`` at these synthetics, for :meth:`normal` (nothing is kept on the objective)"""
        e, _ = self.residuals(d_syn, shot.d_obs, shot.weights)
        return self.psi_rho(e, self.thresh_of(i, shot.d_obs, shot.weights))[0]

    def psi_rho(self, e, a):
        """``(psi, rho)`` of the kind, elementwise; ``a``: the ``(ntr,)`` thresholds"""
        ae = np.abs(e)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            if self.kind == "huber":
                inside = ae <= a
                psi = np.where(inside, 1.0, a / np.where(inside, 1.0, ae))
                return psi, np.where(inside, 0.5 * e * e, a * ae - 0.5 * a * a)
            v = (e / a) ** 2
            if self.kind == "hybrid":
                s = np.sqrt(1.0 + v)
                return 1.0 / s, e * e / (1.0 + s)
            return 1.0 / (1.0 + v), 0.5 * a * a * np.log1p(v)

    def __call__(self, d_syn, d_obs, weights=None, trace_weights=None, shot=None, thresh=None):
        e, M = self.residuals(d_syn, d_obs, weights)
        ntr = e.shape[1]
        tw = self._trace_weights(trace_weights, ntr)
        a = self.thresh_of(shot, d_obs, weights) if thresh is None else np.broadcast_to(
            np.asarray(thresh, np.float64), (ntr,))
        if not np.all(a > 0.0) or (np.any(np.isinf(a)) and self.kind != "huber"):
            raise ValueError("thresholds must be > 0, and finite unless kind is 'huber'")
        psi, rho = self.psi_rho(e, a)
        g = self._round(tw * (psi * e))
        self.psi, self.J_trace, self.nout = psi, tw * np.sum(rho, axis=0), np.sum(np.abs(e) > a, axis=0).astype(np.int32)
        return float(np.sum(tw * rho)), fir_time(g if M is None else M * g, self.taps)

    def normal(self, x, weights=None, trace_weights=None, W=None):
        """``B (tw M^2 W . B x)`` with ``W = psi(e)`` (None: that of the last call): the IRLS (majoriser) Gauss-Newton
        weight, symmetric positive semi-definite since ``psi >= 0``"""
        x = np.asarray(x, np.float64)
        W = self.psi if W is None else np.asarray(W, np.float64)
        if W is None or W.shape != x.shape:
            raise ValueError("no psi(e) of the shape of x: call the objective on this shot first")
        M = WeightedL2._weights(weights, x.shape)
        full = self._round(self._trace_weights(trace_weights, x.shape[1]) * (W if M is None else M * M * W))
        return fir_time(self._round(full * fir_time(x, self.taps)), self.taps)


SPECTRAL_KINDS = ("l2", "phase", "logamp", "log")


def _spectral_tables(nt, dt, freqs, kind):
    """``(f, cos theta, sin theta)``, the tables ``(F, nt)``; the frequencies checked as ``fwi_misfit_spectral`` does"""
    from . import fourier
    from ._lib import FOURIER_FMAX
    f = np.atleast_1d(np.asarray(freqs, np.float64))
    if f.ndim != 1 or not 1 <= f.size <= FOURIER_FMAX:
        raise ValueError("freqs must hold 1 .. %d frequencies in Hz" % FOURIER_FMAX)
    th = fourier.phases(nt, 1, dt, f)  # (finite, >= 0, distinct, at most the Nyquist frequency: checked there)
    if kind in ("phase", "log") and np.any((f == 0.0) | (np.abs(2.0 * f * float(dt) - 1.0) <= fourier.NYQUIST_RTOL)):
        raise ValueError("kinds 'phase' and 'log' take no frequency of 0 or at the Nyquist frequency: the spectrum is "
                         "real there")
    return f, np.cos(th), np.sin(th)


def spectrum(x, dt, freqs):
    """``X_kj = sum_n x[n, j] (cos theta_kn - i sin theta_kn)``, ``theta_kn = 2 pi frac(f_k n dt)``: the ``(F, ntr)``
    complex Fourier coefficients of the ``(nt, ntr)`` gather at the frequencies ``freqs`` (Hz), in fp64."""
    x = np.asarray(x, np.float64)
    if x.ndim != 2:
        raise ValueError("the gather must be (nt, ntr)")
    _, c, s = _spectral_tables(x.shape[0], dt, freqs, "l2")
    return c @ x - 1j * (s @ x)


def spectral_floor(d_obs, dt, freqs, percent=1.0, weights=None):
    """``percent / 100 * max_kj |O_kj|`` of the (weighted) observed data: a floor ``eps`` for :class:`SpectralMisfit`
    that depends on the data only -- like :func:`correlation_floor`, compute it once per shot and hold it."""
    if not (float(percent) >= 0.0 and np.isfinite(percent)):
        raise ValueError("percent must be finite and >= 0")
    d = np.asarray(d_obs, np.float64)
    if d.ndim != 2:
        raise ValueError("d_obs must be (nt, ntr)")
    M = WeightedL2._weights(weights, d.shape)
    return float(percent) / 100.0 * (float(np.max(np.abs(spectrum(d if M is None else M * d, dt, freqs)))) if d.size else 0.0)


def laplace_damping(nt, dt, sigma):
    """The ``(nt, 1)`` weights ``exp(-sigma n dt)`` of a Laplace-Fourier misfit (``sigma >= 0`` in 1/s), to be multiplied
    into ``Shot.weights``."""
    if not (float(sigma) >= 0.0 and np.isfinite(sigma) and float(dt) > 0.0 and np.isfinite(dt) and int(nt) >= 1):
        raise ValueError("nt >= 1, dt > 0 and a finite sigma >= 0")
    return np.exp(-float(sigma) * float(dt) * np.arange(int(nt), dtype=np.float64))[:, None]


def whitening_weights(d_obs, dt, freqs, percent=1.0):
    """``fw_k = 1 / (mean_j |O_kj|^2 + floor)``, ``floor = (percent / 100)^2 max_k mean_j |O_kj|^2``: frequency weights
    that whiten the spectrum of the observed data, so that its weak frequencies are not drowned out (data-only)."""
    if not (float(percent) >= 0.0 and np.isfinite(percent)):
        raise ValueError("percent must be finite and >= 0")
    p = np.mean(np.abs(spectrum(d_obs, dt, freqs)) ** 2, axis=1)
    denom = p + (float(percent) / 100.0) ** 2 * float(np.max(p))
    if not np.all(denom > 0.0):
        raise ValueError("the observed data have no energy at a frequency and percent = 0: no weight to give")
    return 1.0 / denom


class SpectralMisfit(_PerTrace):
    """The frequency-domain (spectral) misfit in fp64 NumPy, ``objective(d_syn, d_obs, weights=None, trace_weights=None)
    -> (J, r)``, and the ``objective=`` that ``shots.misfit_and_gradient`` recognises (an engine that has
    ``misfit_spectral`` replaces it by the device path; the shot loop hands it ``Shot.weights`` and
    ``Shot.trace_weights``).  The definition (``include/fwi.h`` ``fwi_misfit_spectral``, ``csrc/fwi_spec.hip``):

        sh = M . B d_syn,  dh = M . B d_obs    (M, B as in NormalizedCorrelation; B s, B d rounded to the dtype once)
        theta_kn = 2 pi frac(f_k n dt)         formed in fp64 from the fractional part, as fourier.phases does
        S_kj = sum_n sh[n,j] (cos theta_kn - i sin theta_kn)        O_kj likewise from dh
        w_kj = fw_k * tw_j                     fw: F weights per frequency (none: 1), tw: ntr weights per trace (none: 1),
                                               all finite and >= 0
        kind L2      J = 1/2 sum_kj w_kj |S_kj - O_kj|^2                        G_kj = w_kj (S_kj - O_kj)
        kind LOGAMP  a_kj = 1/2 ln((|S_kj|^2 + eps^2) / (|O_kj|^2 + eps^2))
                     J = 1/2 sum w a^2                                           G_kj = w_kj a_kj S_kj / (|S_kj|^2 + eps^2)
        kind PHASE   phi_kj = atan2(Im(S_kj conj O_kj), Re(S_kj conj O_kj)) in (-pi, pi]
                     J = 1/2 sum w phi^2                                         G_kj = w_kj phi_kj (i S_kj) / |S_kj|^2
        kind LOG     the sum of LOGAMP and PHASE (the logarithmic misfit), over the pairs that count under PHASE
        g[n,j] = M[n,j] sum_k (Re G_kj cos theta_kn - Im G_kj sin theta_kn)     (rounded to the dtype once)
        r = dJ/ds = B g

    Under PHASE and LOG a pair ``(k, j)`` counts iff ``|S_kj|^2 > eps^2`` and ``|O_kj|^2 > eps^2``; otherwise its term of
    ``J`` and its ``G`` are 0.  Under L2 and LOGAMP every pair counts.  ``eps >= 0`` is in the units of ``|S|`` and must
    not follow ``s``.  ``Im(S conj O) = S_i O_r - S_r O_i`` is formed from two rounded products, so that equal gathers
    give ``J = 0`` and ``r = 0`` exactly for every kind.  PHASE is exactly invariant under a gain on the synthetics.
    ``J`` is not differentiable where ``phi = +-pi`` (a cycle skip at that frequency) nor where a pair starts or stops
    counting, and ``phi`` wraps: a shift beyond half a period of ``f_k`` reads as a smaller one of the other sign.

    ``dt``: the sampling interval in seconds.  ``freqs``: the ``1 .. 64`` frequencies in Hz (``fourier.fourier_bins(nt,
    dt, 1, fmin, fmax)`` lists the bins of a band).  ``kind``: one of ``"l2"``, ``"phase"``, ``"logamp"``, ``"log"``.
    ``eps``: the floor; None: :func:`spectral_floor` of each call's ``d_obs`` and weights at ``floor_percent``.  ``taps``:
    the one-sided ``b_0 .. b_R`` of ``B``, or None.  ``dtype``: round ``B s``, ``B d`` (with taps) and ``g`` to it once
    each, as a device context of that dtype does (None: keep fp64).  ``freq_weights``: the ``fw_k``, or None
    (:func:`whitening_weights`).

    ``spectra`` holds ``(S, O)`` of the last call, ``phases`` its ``phi_kj`` (wherever the pair passes the counting rule
    of PHASE, whatever the kind; 0 elsewhere), ``logamps`` its ``a_kj`` (wherever the kind uses it or the pair passes that
    rule; 0 elsewhere) and ``counts`` which pairs count under ``kind``, each ``(F, ntr)``.  Not a :class:`WeightedL2`:
    ``gauss_newton_hvp`` refuses it (a Gauss-Newton weight for kind L2 is out of scope)."""

    def __init__(self, dt, freqs, kind="l2", eps=None, taps=None, dtype=None, freq_weights=None, floor_percent=1.0):
        if not (float(dt) > 0.0 and np.isfinite(dt)):
            raise ValueError("dt must be > 0")
        if kind not in SPECTRAL_KINDS:
            raise ValueError("kind must be one of %r" % (SPECTRAL_KINDS,))
        if eps is not None and not (float(eps) >= 0.0 and np.isfinite(eps)):
            raise ValueError("eps must be finite and >= 0")
        if not (float(floor_percent) >= 0.0 and np.isfinite(floor_percent)):
            raise ValueError("floor_percent must be finite and >= 0")
        self.dt, self.kind = float(dt), kind
        self.freqs = _spectral_tables(1, self.dt, freqs, kind)[0].copy()  # (checked)
        self.freq_weights = None
        if freq_weights is not None:
            fw = np.asarray(freq_weights, np.float64)
            if fw.shape != self.freqs.shape or not np.all(np.isfinite(fw)) or np.any(fw < 0.0):
                raise ValueError("freq_weights must be %d finite weights >= 0" % self.freqs.size)
            self.freq_weights = fw
        self.eps = None if eps is None else float(eps)
        self.floor_percent = float(floor_percent)
        self._band(taps, dtype)
        self.spectra = self.phases = self.logamps = self.counts = None

    def eps_of(self, d_obs, weights=None):
        """the floor of a shot: ``eps``, or :func:`spectral_floor` of its observed data and weights"""
        if self.eps is not None:
            return self.eps
        return spectral_floor(d_obs, self.dt, self.freqs, self.floor_percent, weights)

    engine_method = "misfit_spectral"

    def device(self, engine, shot, i):
        return engine.misfit_spectral(shot.d_obs, self.freqs, self.kind, self.eps_of(shot.d_obs, shot.weights),
                                      shot.weights, self.taps, self.freq_weights, shot.trace_weights)

    def __call__(self, d_syn, d_obs, weights=None, trace_weights=None):
        sh, dh, _ = self._weighted(d_syn, d_obs, weights)
        nt, ntr = sh.shape
        _, c, s = _spectral_tables(nt, self.dt, self.freqs, self.kind)
        fw = np.ones(self.freqs.size) if self.freq_weights is None else self.freq_weights
        w = fw[:, None] * self._trace_weights(trace_weights, ntr)[None, :]
        e2 = self.eps_of(d_obs, weights) ** 2
        Sr, Si, Or, Oi = c @ sh, -(s @ sh), c @ dh, -(s @ dh)
        s2, o2 = Sr * Sr + Si * Si, Or * Or + Oi * Oi
        both = (s2 > e2) & (o2 > e2)  # the counting rule of PHASE and LOG
        amp = np.ones_like(both) if self.kind == "logamp" else both if self.kind == "log" else np.zeros_like(both)
        ph = both if self.kind in ("phase", "log") else np.zeros_like(both)
        with np.errstate(divide="ignore", invalid="ignore"):
            a = np.where(amp | both, 0.5 * np.log((s2 + e2) / (o2 + e2)), 0.0)
            # (two rounded products and their difference: equal spectra give exactly 0)
            phi = np.where(both, np.arctan2(Si * Or - Sr * Oi, Sr * Or + Si * Oi), 0.0)
            ca = np.where(amp, w * a / (s2 + e2), 0.0)
            cp = np.where(ph, w * phi / s2, 0.0)
        Gr, Gi = ca * Sr - cp * Si, ca * Si + cp * Sr
        terms = np.where(amp, 0.5 * w * a * a, 0.0) + np.where(ph, 0.5 * w * phi * phi, 0.0)
        if self.kind == "l2":
            Dr, Di = Sr - Or, Si - Oi
            Gr, Gi, terms = w * Dr, w * Di, 0.5 * w * (Dr * Dr + Di * Di)
        self.spectra = (Sr + 1j * Si, Or + 1j * Oi)
        self.phases, self.logamps = phi, a
        self.counts = np.ones_like(both) if self.kind in ("l2", "logamp") else both
        return float(np.sum(terms)), self._residual(c.T @ Gr - s.T @ Gi, weights)


def matched_wavelet(wavelet, f):
    """``C_f`` applied to a wavelet ``(nt,)`` or ``(nt, nsrc)``: the source signature a shot's matching filter
    ``f = (f_-L .. f_L)`` implies, ``w'[n] = sum_k f_k w[n - k]``."""
    f = np.asarray(f, np.float64)
    if f.ndim != 1 or f.size % 2 != 1:
        raise ValueError("f must hold 2 L + 1 coefficients f_-L .. f_L")
    return _conv_time(wavelet, f)


def prewhitening(d_obs, weights=None, percent=0.1):
    """``percent / 100 * sum (M d_obs)^2``: a damping ``mu`` for :class:`MatchedL2` that depends on the data only --
    compute it once per shot and hold it through an inversion (a ``mu`` that followed ``d_syn`` would break the
    gradient)."""
    d = np.asarray(d_obs, np.float64)
    M = WeightedL2._weights(weights, d.shape)
    if not (float(percent) >= 0.0 and np.isfinite(percent)):
        raise ValueError("percent must be finite and >= 0")
    md = d if M is None else M * d
    return float(percent) / 100.0 * float(np.sum(md * md))


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
    return first_arrival_mute(off / float(v_fast), nt, dt, t_pad, taper)


def first_arrival_mute(times, nt, dt, t_pad=0.0, taper=0):
    """:func:`offset_time_mute` with a first-arrival time per trace in place of ``offset / v_fast`` -- picks
    (:func:`first_breaks`) or eikonal times (``Engine.eikonal_times``): weights ``(nt, ntr)`` that are 0 for
    ``t < times + t_pad``, then a raised cosine over ``taper`` samples, 1 after it.  A NaN time mutes its whole trace."""
    times = np.asarray(times, np.float64).reshape(-1)
    if not float(dt) > 0.0 or int(taper) < 0 or int(nt) < 1:
        raise ValueError("dt must be > 0, nt >= 1 and taper >= 0")
    s = np.arange(int(nt), dtype=np.float64)[:, None] - (times + float(t_pad))[None, :] / float(dt)
    if int(taper) == 0:
        return (s >= 0.0).astype(np.float64)
    w = 0.5 * (1.0 - np.cos(np.pi * np.clip(s / int(taper), 0.0, 1.0)))
    return np.where(np.isnan(s), 0.0, np.where(s >= int(taper), 1.0, w))


def first_breaks(d, dt, fraction=0.1):
    """First-break picks of the traces ``d`` ``(nt, ntr)``: per trace the time at which ``|d|`` first reaches ``fraction``
    (in (0, 1]) of the trace's maximum of ``|d|``, interpolated linearly between the last sample below the threshold and
    the first one at or above it.  NaN for a dead trace (all zeros, or anything not finite)."""
    d = np.abs(np.asarray(d, np.float64))
    if d.ndim == 1:
        d = d[:, None]
    if d.ndim != 2 or not 0.0 < float(fraction) <= 1.0 or not float(dt) > 0.0:
        raise ValueError("d must be (nt, ntr), 0 < fraction <= 1 and dt > 0")
    peak = d.max(axis=0)
    live = np.isfinite(peak) & (peak > 0.0)
    thr = np.where(live, float(fraction) * peak, np.inf)
    k = np.argmax(d >= thr[None, :], axis=0)  # the first sample at or above the threshold (0 for dead traces)
    cols = np.arange(d.shape[1])
    hi, lo = d[k, cols], d[np.maximum(k - 1, 0), cols]
    with np.errstate(invalid="ignore", divide="ignore"):
        frac = np.where((k > 0) & (hi > lo), (thr - lo) / (hi - lo), 1.0)  # position between sample k - 1 and k
    return np.where(live, (k - 1 + frac) * float(dt), np.nan)


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
