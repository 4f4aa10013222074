"""The Fourier-compressed forward-term store in NumPy: the definition of ``fwi_set_fourier_store`` (include/fwi.h) and
the fp64 twin of its two device transforms (csrc/fwi_fourier.hip).

With ``S`` the image stride and ``N = ceil(nt / S)``, sample ``j`` of the forward term is time step ``n = j S``.  For the
frequencies ``f_k >= 0`` (Hz) and the phases ``theta_kj = 2 pi f_k j S dt``::

    analysis    Q_k(x)     = sum_j q^{jS}(x) (cos theta_kj - i sin theta_kj)
    synthesis   q~^{jS}(x) = sum_k w_k (Re Q_k(x) cos theta_kj - Im Q_k(x) sin theta_kj)
    weights     w_k = 1 / N where f_k = 0 or f_k = 1 / (2 S dt), the Nyquist frequency of the sampled axis; else 2 / N

On the bin frequencies ``k / (N S dt)``, ``k = 0 .. floor(N / 2)``, synthesis after analysis is the orthogonal projection
of the sampled history onto those bins, and the identity with all of them.  With fewer bins the gradient is that of the
forward term band-passed to the bins kept: an approximation of the full gradient, as good as the bins cover the band of
the source.  :func:`fourier_bins` lists the bins inside a band.  For a Ricker wavelet of peak frequency ``f0``, whose
amplitude spectrum is ``f^2 exp(-f^2 / f0^2)``, the band ``[0, 2.5 f0]`` leaves out 1.4e-4 of the wavelet's energy and
3.0e-3 of that of its second derivative in time, which is what the forward term is away from the source; ``[0, 3 f0]``
leaves out 9.5e-7 and 4.0e-5.  Frequencies off the bins are allowed (phase-sensitive
detection); the result is then no projection.
"""
from __future__ import annotations

import numpy as np

NYQUIST_RTOL = 1e-9  # FOURIER_NYQUIST_RTOL of the engine: how close to 1 / (2 S dt) counts as the Nyquist frequency


def n_samples(nt, stride):
    """``N = ceil(nt / S)``: the samples ``j = 0 .. N - 1`` are the time steps ``j S < nt``."""
    nt, stride = int(nt), max(1, int(stride))
    if nt < 1:
        raise ValueError("nt must be >= 1")
    return (nt + stride - 1) // stride


def fourier_bins(nt, dt, stride, fmin, fmax):
    """The bin frequencies ``k / (N S dt)``, ``k = 0 .. floor(N / 2)``, with ``fmin <= f <= fmax`` (Hz; both ends count,
    to 1e-12 of the sampling rate), ascending.  Empty when the band holds no bin; ``fmax`` above the Nyquist frequency ends
    at the highest bin."""
    S = max(1, int(stride))
    N = n_samples(nt, S)
    f = np.arange(N // 2 + 1) / (N * S * float(dt))
    tol = 1e-12 / (S * float(dt))
    return f[(f >= float(fmin) - tol) & (f <= float(fmax) + tol)]


def _freqs(nt, stride, dt, freqs):
    S = max(1, int(stride))
    f = np.atleast_1d(np.asarray(freqs, np.float64))
    if f.ndim != 1 or f.size < 1:
        raise ValueError("freqs must be a non-empty 1-D array of frequencies in Hz")
    nyq = 1.0 / (2.0 * S * float(dt))
    if not np.all(np.isfinite(f)) or np.any(f < 0) or np.any(f > nyq * (1.0 + NYQUIST_RTOL)):
        raise ValueError("frequencies must be finite, >= 0 and at most the Nyquist frequency %g Hz" % nyq)
    if np.unique(f).size != f.size:
        raise ValueError("frequencies must differ")
    return f, S, n_samples(nt, S)


def phases(nt, stride, dt, freqs):
    """``theta_kj`` as ``(F, N)``, from the fractional part of ``f_k j S dt`` (the engine's table does the same)."""
    f, S, N = _freqs(nt, stride, dt, freqs)
    x = (f * (S * float(dt)))[:, None] * np.arange(N)[None, :]
    return 2.0 * np.pi * (x - np.floor(x))


def weights(nt, stride, dt, freqs):
    """``w_k``: ``1 / N`` at ``f_k = 0`` and at the Nyquist frequency ``1 / (2 S dt)``, else ``2 / N``."""
    f, S, N = _freqs(nt, stride, dt, freqs)
    edge = (f == 0.0) | (np.abs(2.0 * f * S * float(dt) - 1.0) <= NYQUIST_RTOL)
    return np.where(edge, 1.0, 2.0) / N


def analyse(samples, nt, stride, dt, freqs, dtype=np.float64, batch=None, reverse=False):
    """``Q_k`` as a complex ``(F, ...)`` array from the samples ``q^{jS}``, ``(N, ...)``.

    ``dtype`` and ``batch`` restate the device's arithmetic: the samples and the accumulators are held in ``dtype``, the
    sums over a batch of ``batch`` samples (None: all at once) are taken in fp64 and added to the accumulators once per
    batch.  ``reverse``: the same batches, the last one first (the order of a reverse sweep)."""
    th = phases(nt, stride, dt, freqs)
    F, N = th.shape
    dtype = np.dtype(dtype)
    q = np.asarray(samples)
    if q.shape[0] != N:
        raise ValueError("expected the N = %d samples of the time axis, got %d" % (N, q.shape[0]))
    q = q.astype(dtype).astype(np.float64)
    B = N if batch is None else max(1, int(batch))
    re = np.zeros((F,) + q.shape[1:], dtype)
    im = np.zeros((F,) + q.shape[1:], dtype)
    for j0 in (range(0, N, B)[::-1] if reverse else range(0, N, B)):
        sl = slice(j0, min(N, j0 + B))
        re = (re.astype(np.float64) + np.tensordot(np.cos(th[:, sl]), q[sl], axes=1)).astype(dtype)
        im = (im.astype(np.float64) - np.tensordot(np.sin(th[:, sl]), q[sl], axes=1)).astype(dtype)
    return re + 1j * im


def synthesise(Q, nt, stride, dt, freqs, dtype=np.float64):
    """The band-limited samples ``q~^{jS}`` as ``(N, ...)`` in ``dtype`` from ``Q_k``, ``(F, ...)`` complex; the sums run in
    fp64."""
    th = phases(nt, stride, dt, freqs)
    w = weights(nt, stride, dt, freqs)
    Q = np.asarray(Q)
    if Q.shape[0] != th.shape[0]:
        raise ValueError("expected one coefficient array per frequency")
    re, im = Q.real.astype(np.float64), Q.imag.astype(np.float64)
    out = np.tensordot((w[:, None] * np.cos(th)).T, re, axes=1) - np.tensordot((w[:, None] * np.sin(th)).T, im, axes=1)
    return out.astype(np.dtype(dtype))


def project(q_history, nt, stride, dt, freqs, dtype=np.float64, batch=None):
    """What the imaging condition reads with the Fourier store in the place of the history ``q^n``, ``(nt, ...)``: the rows
    ``n = j S`` hold ``synthesise(analyse(.))`` of those rows, the rows in between (which the imaging never reads) zeros."""
    q = np.asarray(q_history)
    S = max(1, int(stride))
    if q.shape[0] != int(nt):
        raise ValueError("expected the nt = %d steps of the history, got %d" % (int(nt), q.shape[0]))
    Q = analyse(q[::S], nt, S, dt, freqs, dtype, batch)
    out = np.zeros(q.shape, np.dtype(dtype))
    out[::S] = synthesise(Q, nt, S, dt, freqs, dtype)
    return out


# -- spectral imaging (fwi_adjoint_spectral, fwi_fourier_image, fwi_fourier_illumination; csrc/fwi_fimage.hip) ----------
#
# With ``M_k`` the analysis of the adjoint field at the imaging samples, ``mu^{jS+1}`` (what the imaging condition pairs
# with ``q^{jS}``), the band-limited imaging sum is a sum over frequencies, for ANY set of them::
#
#     sum_j mu^{jS+1} q~^{jS} = sum_k w_k Re(Q_k conj M_k) = sum_k w_k (Re Q_k Re M_k + Im Q_k Im M_k)
#
# (insert the synthesis and exchange the sums).  On bin frequencies Parseval also gives ``sum_j (q~^{jS})^2 = sum_k w_k
# |Q_k|^2``, the illumination of the band-limited term; off the bins that identity does NOT hold and
# :func:`spectral_illumination` is a definition.

def adjoint_spectrum(mu_samples, nt, stride, dt, freqs, dtype=np.float64, batch=None):
    """``M_k`` as a complex ``(F, ...)`` array from the samples ``mu^{jS+1}``, ``(N, ...)``: :func:`analyse`, its batches
    in the order of the reverse sweep."""
    return analyse(mu_samples, nt, stride, dt, freqs, dtype, batch, reverse=True)


def _weighted(Q, nt, stride, dt, freqs, freq_weights):
    a = weights(nt, stride, dt, freqs)
    Q = np.asarray(Q)
    if Q.shape[0] != a.size:
        raise ValueError("expected one coefficient array per frequency")
    if freq_weights is not None:
        fw = np.asarray(freq_weights, np.float64)
        if fw.shape != a.shape:
            raise ValueError("freq_weights must hold one weight per frequency, shape (%d,)" % a.size)
        a = fw * a
    return a, Q


def spectral_image(Q, M, nt, stride, dt, freqs, freq_weights=None, dtype=np.float64):
    """``sum_k a_k w_k Re(Q_k conj M_k)`` in the units of the imaging sum ``sum_j mu^{jS+1} q^{jS}`` (times
    ``-S / dt^2`` it is the gradient w.r.t. ``1 / c^2``); ``a = freq_weights`` (None: 1).  ``dtype`` restates the
    device's arithmetic: the coefficients are held in ``dtype``, the sum runs in fp64 with k ascending and is rounded to
    ``dtype`` once."""
    a, Q = _weighted(Q, nt, stride, dt, freqs, freq_weights)
    M = np.asarray(M)
    dtype = np.dtype(dtype)
    part = lambda z: z.astype(dtype).astype(np.float64)  # noqa: E731
    s = np.zeros(Q.shape[1:], np.float64)
    for k in range(a.size):
        s = s + a[k] * (part(Q[k].real) * part(M[k].real) + part(Q[k].imag) * part(M[k].imag))
    return s.astype(dtype)


def spectral_illumination(Q, nt, stride, dt, freqs, freq_weights=None, dtype=np.float64):
    """``sum_k a_k w_k |Q_k|^2`` in the units of ``sum_j (q^{jS})^2`` (times ``S / dt^4`` it is
    ``Engine.fourier_illumination(wrt="slowness2")``).  On bin frequencies, with unit ``a``, this equals
    ``sum_j (q~^{jS})^2``; off the bins it does not.  ``dtype`` as in :func:`spectral_image`."""
    a, Q = _weighted(Q, nt, stride, dt, freqs, freq_weights)
    dtype = np.dtype(dtype)
    part = lambda z: z.astype(dtype).astype(np.float64)  # noqa: E731
    s = np.zeros(Q.shape[1:], np.float64)
    for k in range(a.size):
        s = s + a[k] * (part(Q[k].real) ** 2 + part(Q[k].imag) ** 2)
    return s.astype(dtype)


# -- extended images (fwi_fourier_offset_image, fwi_fourier_lag_image; csrc/fwi_feximage.hip) ---------------------------
#
# The same exchange of sums with the two fields read at different cells, ``x - h e`` and ``x + h e``, gives the
# subsurface-offset image, again for ANY set of frequencies::
#
#     sum_j mu^{jS+1}(x + h e) q~^{jS}(x - h e) = sum_k w_k Re(Q_k(x - h e) conj M_k(x + h e))
#
# A delay of the forward term by ``tau`` multiplies ``Q_k`` by ``exp(-i 2 pi f_k tau)``.  On bin frequencies and with
# ``tau = m S dt`` that is the circular shift of the sampled ``q~`` by ``m`` samples, and :func:`lag_image` is the imaging
# sum of the shifted term; off the bins, or at any other ``tau``, it is a definition and no such sum (only ``tau = 0`` is
# the imaging sum for every frequency set).

def offset_image(Q, M, nt, stride, dt, freqs, axis, h, freq_weights=None, dtype=np.float64):
    """``sum_k a_k w_k Re(Q_k(x - h e) conj M_k(x + h e))`` for the integer ``h`` (cells along the model axis ``axis``,
    0 = the first axis after the frequencies), zero wherever ``x - h e`` or ``x + h e`` lies outside the grid; in the units
    of the imaging sum, as :func:`spectral_image`, which it equals bit for bit at ``h = 0``.  ``dtype`` as there."""
    a, Q = _weighted(Q, nt, stride, dt, freqs, freq_weights)
    M = np.asarray(M)
    dtype = np.dtype(dtype)
    axis, h = int(axis), int(h)
    if not 0 <= axis < Q.ndim - 1:
        raise ValueError("axis %d outside [0, %d)" % (axis, Q.ndim - 1))
    n = Q.shape[1 + axis]
    out = np.zeros(Q.shape[1:], dtype)
    if 2 * abs(h) >= n:
        return out
    # the cells x with abs(h) <= x_a < n - abs(h); Q is read at x - h, M at x + h
    cut = lambda lo: (slice(None),) * axis + (slice(lo, lo + n - 2 * abs(h)),)  # noqa: E731
    part = lambda z: z.astype(dtype).astype(np.float64)  # noqa: E731
    s = np.zeros(out[cut(abs(h))].shape, np.float64)
    for k in range(a.size):
        q, m = Q[k][cut(abs(h) - h)], M[k][cut(abs(h) + h)]
        s = s + a[k] * (part(q.real) * part(m.real) + part(q.imag) * part(m.imag))
    out[cut(abs(h))] = s.astype(dtype)
    return out


def lag_image(Q, M, nt, stride, dt, freqs, tau, freq_weights=None, dtype=np.float64):
    """``sum_k a_k w_k Re(Q_k conj(M_k) exp(-i 2 pi f_k tau))`` for a finite ``tau`` in seconds, in the units of the imaging
    sum, as :func:`spectral_image`, which it equals bit for bit at ``tau = 0``.  With ``P_k = Q_k conj M_k`` the terms are
    ``a_k w_k (Re P_k cos phi_k + Im P_k sin phi_k)``, ``phi_k = 2 pi f_k tau`` from the fractional part of ``f_k tau`` (as
    :func:`phases`).  On bin frequencies with ``tau = m S dt`` this is ``sum_j mu^{jS+1} q~^{((j - m) mod N) S}``; off the
    bins, or at any other ``tau``, it is this formula and no such sum.  ``dtype`` as in :func:`spectral_image`."""
    a, Q = _weighted(Q, nt, stride, dt, freqs, freq_weights)
    M = np.asarray(M)
    dtype = np.dtype(dtype)
    tau = float(tau)
    if not np.isfinite(tau):
        raise ValueError("tau must be finite")
    f, _, _ = _freqs(nt, stride, dt, freqs)
    x = f * tau
    phi = 2.0 * np.pi * (x - np.floor(x))
    c, d = a * np.cos(phi), a * np.sin(phi)
    part = lambda z: z.astype(dtype).astype(np.float64)  # noqa: E731
    s = np.zeros(Q.shape[1:], np.float64)
    for k in range(a.size):
        qr, qi, mr, mi = part(Q[k].real), part(Q[k].imag), part(M[k].real), part(M[k].imag)
        s = s + c[k] * (qr * mr + qi * mi) + d[k] * (qi * mr - qr * mi)
    return s.astype(dtype)


# -- tomographic / migration split (fwi_fourier_split_image; csrc/fwi_fsplit.hip) ---------------------------------------
#
# With ``H`` a Hilbert transformer along one grid axis, ``U^+- = (U +- i H U) / 2`` are the parts of a coefficient ``U``
# with positive and negative wavenumber along that axis.  The pairs of equal and of opposite direction are then::
#
#     Re(Q+ conj M+) + Re(Q- conj M-) = (Re(Q conj M) + Re(HQ conj HM)) / 2      low wavenumber: tomographic
#     Re(Q+ conj M-) + Re(Q- conj M+) = (Re(Q conj M) - Re(HQ conj HM)) / 2      high wavenumber: migration
#
# (expand the products; the cross terms ``Im(HQ conj M) - Im(Q conj HM)`` cancel in the first sum and never enter the
# second), so the one new quantity is ``X = sum_k a_k w_k Re(HQ_k conj HM_k)``.  ``H`` is the FIR of
# ``datafit.hilbert_taps``: antisymmetric, zero-extended at the faces of the grid.

SPLIT_RMAX = 64  # FWI_SPLIT_RMAX
_SPLIT = {"same": (0.5, 0.5), "opposite": (0.5, -0.5), "hilbert": (0.0, 1.0)}


def hilbert_axis(u, taps, axis):
    """``(H u)(i) = sum_r t_r (u(i - r) - u(i + r))`` along ``axis`` of the real fp64 array ``u`` for the one-sided taps
    ``t_1 .. t_R``: cells outside the array contribute nothing, taps that are exactly zero are skipped (as
    ``datafit.hilbert_time`` skips them), the sum runs with ``r`` ascending."""
    u = np.asarray(u, np.float64)
    t = np.asarray(taps, np.float64)
    if t.ndim != 1:
        raise ValueError("taps must be the 1-D one-sided taps t_1 .. t_R")
    axis = int(axis)
    if not 0 <= axis < u.ndim:
        raise ValueError("axis %d outside [0, %d)" % (axis, u.ndim))
    n = u.shape[axis]
    cut = lambda lo, hi: (slice(None),) * axis + (slice(lo, hi),)  # noqa: E731
    # every cell adds t_r (u(i - r) - u(i + r)) in one step, an absent neighbour as 0: the device's order
    out = np.zeros_like(u)
    for r in range(1, min(t.size, n - 1) + 1):
        if t[r - 1] != 0.0:
            d = np.zeros_like(u)
            d[cut(r, n)] += u[cut(0, n - r)]
            d[cut(0, n - r)] -= u[cut(r, n)]
            out += t[r - 1] * d
    return out


def split_image(Q, M, nt, stride, dt, freqs, axis, taps, part, freq_weights=None, dtype=np.float64):
    """One part of the split of :func:`spectral_image` along the model axis ``axis`` (0 = the first axis after the
    frequencies), in its units::

        sum_k a_k w_k [alpha Re(Q_k conj M_k) + beta Re(H Q_k conj H M_k)]

    with ``H`` of :func:`hilbert_axis` on ``Re`` and ``Im`` separately and ``(alpha, beta) = (1/2, 1/2)`` for
    ``part="same"`` (tomographic), ``(1/2, -1/2)`` for ``"opposite"`` (migration), ``(0, 1)`` for ``"hilbert"``.
    ``same + opposite`` is :func:`spectral_image` to round-off.  At most ``SPLIT_RMAX`` taps.  ``dtype`` restates the
    device's arithmetic: the coefficients are held in ``dtype``; the filter sums (``r`` ascending, zero taps skipped), the
    products ``p = Re HQ Re HM + Im HQ Im HM`` and ``t = Re Q Re M + Im Q Im M`` and the sum over k (ascending, each term
    ``a_k (alpha t + beta p)``) run in fp64, and the result is rounded to ``dtype`` once."""
    a, Q = _weighted(Q, nt, stride, dt, freqs, freq_weights)
    M = np.asarray(M)
    dtype = np.dtype(dtype)
    if part not in _SPLIT:
        raise ValueError("part must be one of 'same', 'opposite', 'hilbert'")
    alpha, beta = _SPLIT[part]
    t = np.asarray(taps, np.float64)
    if t.ndim != 1 or not 1 <= t.size <= SPLIT_RMAX or not np.all(np.isfinite(t)):
        raise ValueError("taps must be a finite 1-D array t_1 .. t_R, R in [1, %d]" % SPLIT_RMAX)
    axis = int(axis)
    if not 0 <= axis < Q.ndim - 1:
        raise ValueError("axis %d outside [0, %d)" % (axis, Q.ndim - 1))
    part_ = lambda z: z.astype(dtype).astype(np.float64)  # noqa: E731
    s = np.zeros(Q.shape[1:], np.float64)
    for k in range(a.size):
        qr, qi, mr, mi = part_(Q[k].real), part_(Q[k].imag), part_(M[k].real), part_(M[k].imag)
        p = hilbert_axis(qr, t, axis) * hilbert_axis(mr, t, axis) + hilbert_axis(qi, t, axis) * hilbert_axis(mi, t, axis)
        s = s + a[k] * (alpha * (qr * mr + qi * mi) + beta * p)
    return s.astype(dtype)


def split_halfwidth(cycles_per_cell):
    """``R = ceil(2 / kappa) - 1``: the half-width at which ``datafit.hilbert_taps(R)`` is good (within 2e-3 of a Hilbert
    transformer) from ``kappa`` cycles per cell to Nyquist minus ``kappa`` along the axis; below ``kappa`` the split
    leaves energy in both parts.  Raises above ``SPLIT_RMAX``."""
    kappa = float(cycles_per_cell)
    if not 0.0 < kappa < 0.5:
        raise ValueError("cycles_per_cell = %g outside (0, Nyquist = 0.5)" % kappa)
    R = max(int(np.ceil(round(2.0 / kappa, 9))) - 1, 1)
    if R > SPLIT_RMAX:
        raise ValueError("%g cycles per cell needs R = %d taps, above %d: raise it" % (kappa, R, SPLIT_RMAX))
    return R


# -- Born and extended Born modelling (fwi_fourier_born, fwi_fourier_born_extended; csrc/fwi_fbornx.hip) ---------------
#
# The transposes of the imaging paths above take their scattering source from the coefficients.  The transpose of the
# band-limited imaging sum with the weights ``a`` reads ``q~_a``, the synthesis with ``a_k w_k`` in the place of ``w_k``.
# The transpose of an extended image moves the shift onto the source: with ``y = x + h e`` the pairing
# ``mu(x + h e) E(x) q~(x - h e)`` is ``mu(y) E(y - h e) q~(y - 2 h e)``, so the spectrum of the extended source is
# ``P_k(y) = E(y - h e) Q_k(y - 2 h e)``; a delay of the forward term by ``tau`` gives ``P_k = E Q_k exp(-i 2 pi f_k tau)``.

def born_source(Q, nt, stride, dt, freqs, freq_weights=None, dtype=np.float64):
    """The sampled scattering term ``q~_a^{jS} = sum_k a_k w_k (Re Q_k cos theta_kj - Im Q_k sin theta_kj)`` of
    ``Engine.fourier_born`` as ``(N, ...)`` in ``dtype``; ``a = freq_weights`` (None: 1, then this is :func:`synthesise`).
    ``dtype`` restates the device's arithmetic: the coefficients are held in ``dtype``, the sums run in fp64 and every
    sample is rounded to ``dtype`` once."""
    a, Q = _weighted(Q, nt, stride, dt, freqs, freq_weights)
    th = phases(nt, stride, dt, freqs)
    dtype = np.dtype(dtype)
    re, im = Q.real.astype(dtype).astype(np.float64), Q.imag.astype(dtype).astype(np.float64)
    out = np.tensordot((a[:, None] * np.cos(th)).T, re, axes=1) - np.tensordot((a[:, None] * np.sin(th)).T, im, axes=1)
    return out.astype(dtype)


def extended_source(Q, images, kind, lags, nt, stride, dt, freqs, axis=None, dtype=np.float64):
    """The extended scattering spectrum ``P_k`` of ``Engine.fourier_born_extended`` as a complex ``(F, ...)`` array from the
    gather ``images``, ``(len(lags), ...)``.  ``kind="offset"``: ``P_k(y) = sum_l E_l(y - h_l e) Q_k(y - 2 h_l e)`` over the
    integer lags whose two shifted cells lie in the grid (``axis``: the model axis, 0 = the first after the frequencies);
    ``kind="timelag"``: ``P_k = sum_l E_l Q_k exp(-i 2 pi f_k tau_l)``, the phase from the fractional part of ``f_k tau``.
    ``born_source(P, ...)`` of the result, times ``-c^2 S``, is the scattering source of the sweep.  ``dtype`` restates the
    device's arithmetic: images, ``Q`` and ``P`` are held in ``dtype``, each lag's product is formed in fp64 and added to
    ``P`` with one rounding."""
    f, _, _ = _freqs(nt, stride, dt, freqs)
    Q = np.asarray(Q)
    E = np.asarray(images)
    lags = np.atleast_1d(lags)
    if Q.shape[0] != f.size:
        raise ValueError("expected one coefficient array per frequency")
    if E.shape != (lags.size,) + Q.shape[1:]:
        raise ValueError("expected one image per lag, shape %s" % ((lags.size,) + Q.shape[1:],))
    if kind not in ("offset", "timelag"):
        raise ValueError("kind must be 'offset' or 'timelag'")
    dtype = np.dtype(dtype)
    part = lambda z: np.asarray(z).astype(dtype).astype(np.float64)  # noqa: E731
    qr, qi = part(Q.real), part(Q.imag)
    pr, pi = np.zeros(Q.shape, dtype), np.zeros(Q.shape, dtype)
    for l, lag in enumerate(lags):
        e = part(E[l])
        if kind == "timelag":
            if not np.isfinite(lag):
                raise ValueError("tau must be finite")
            x = f * float(lag)
            phi = (2.0 * np.pi * (x - np.floor(x))).reshape((-1,) + (1,) * e.ndim)
            pr = (pr.astype(np.float64) + e * (qr * np.cos(phi) + qi * np.sin(phi))).astype(dtype)
            pi = (pi.astype(np.float64) + e * (qi * np.cos(phi) - qr * np.sin(phi))).astype(dtype)
            continue
        ax, h = int(axis), int(lag)
        if not 0 <= ax < e.ndim:
            raise ValueError("axis %d outside [0, %d)" % (ax, e.ndim))
        n = e.shape[ax]
        if 2 * abs(h) >= n:
            continue
        # the cells y with y, y - h and y - 2 h in [0, n): max(0, 2 h) <= y_a < n + min(0, 2 h)
        m = n - 2 * abs(h)
        cut = lambda lo, lead: (slice(None),) * (ax + lead) + (slice(lo, lo + m),)  # noqa: E731
        y0 = max(0, 2 * h)
        es = e[cut(y0 - h, 0)]
        dst, src = cut(y0, 1), cut(y0 - 2 * h, 1)
        pr[dst] = (pr[dst].astype(np.float64) + es * qr[src]).astype(dtype)
        pi[dst] = (pi[dst].astype(np.float64) + es * qi[src]).astype(dtype)
    return pr + 1j * pi


def focusing(E, lags):
    """``sum_l lag_l^2 |E_l|^2 / sum_l |E_l|^2`` of a gather ``E``, ``(len(lags), ...)``, with ``|.|^2`` summed over the
    whole image: the energy-weighted mean squared lag, 0 for a gather focused at zero lag, in the units of ``lags``
    squared.  nan for a gather that is zero everywhere."""
    lags = np.asarray(lags, np.float64)
    E = np.asarray(E)
    if lags.ndim != 1 or E.shape[:1] != lags.shape:
        raise ValueError("expected one image per lag")
    e = np.sum(np.abs(E.astype(np.float64)).reshape(lags.size, -1) ** 2, axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.sum(lags ** 2 * e) / np.sum(e))


# -- angle-domain gathers (fwi_vec_shift_sum; csrc/fwi_slant.hip) ------------------------------------------------------
#
# A slant stack of a subsurface-offset gather over depth and half-offset (Sava and Fomel 2003).  Depth is the first model
# axis, the half-offsets ``h_l`` are whole cells along a horizontal axis and share the grid spacing with depth, so the
# tangents ``p_j = tan(gamma_j)`` are dimensionless::
#
#     S_s a (z, .) = (1 - f) a(z + n, .) + f a(z + n + 1, .),   n = floor(s), f = s - n
#     A_j  = sum_l t_l S_{p_j h_l} E_l            angle gather; t: an optional taper over the lags
#     E'_l = t_l sum_j S_{-p_j h_l} A_j           its exact transpose
#
# A tap outside ``0 .. nz - 1`` contributes zero and the other still counts, the second tap is not counted when its
# coefficient is zero, ``|s| >= nz + 1`` gives zeros: with this masking ``S_s^T = S_{-s}`` exactly.  The transform is
# kinematic: a plain slant stack with no rho filter and no claim on amplitudes.  An event that is flat across ``j`` says
# that the model is right; the sign of ``gamma`` is a convention of this definition.  The horizontal axis of the offsets
# does not enter, it only selects which gather was formed.

SHIFT_SUM_MAX = 64  # FWI_SHIFT_SUM_MAX: the sources of one device call (the twin takes any number)


def tangents(degrees):
    """``tan(gamma)`` of the angles ``gamma`` in degrees, ``|gamma| < 90``, as a 1-D fp64 array."""
    g = np.atleast_1d(np.asarray(degrees, np.float64))
    if g.ndim != 1 or not np.all(np.abs(g) < 90.0):
        raise ValueError("angles must be a 1-D array of degrees inside (-90, 90)")
    return np.tan(np.deg2rad(g))


def _shift_coeffs(s, w):
    """``(n, c0, c1)`` of the shift ``s`` and the weight ``w`` as the engine's host path forms them in fp64"""
    s, w = float(s), float(w)
    if not np.isfinite(s) or not np.isfinite(w):
        raise ValueError("shifts and weights must be finite")
    n = int(np.floor(s))
    f = s - n
    return n, w * (1.0 - f), w * f


def shift_sum(srcs, shifts, weights=None, beta=0.0, dst=None):
    """``beta dst + sum_i w_i S_{s_i} src_i`` in fp64: the twin of ``Engine.vec_shift_sum``.  ``srcs``: ``(nsrc, *shape)``
    with depth the first model axis; ``shifts``: ``nsrc`` finite numbers of cells; ``weights``: ``nsrc`` (None: ones).
    With ``beta == 0`` ``dst`` is not read.  The sum runs per cell with the sources ascending, the first tap of a source
    before its second, as on the device (which fuses each multiply-add and rounds to its dtype once at the end)."""
    srcs = np.asarray(srcs, np.float64)
    shifts = np.atleast_1d(np.asarray(shifts, np.float64))
    if srcs.ndim < 2 or shifts.shape != srcs.shape[:1]:
        raise ValueError("expected one shift per source, srcs as (nsrc, *shape)")
    w = np.ones(shifts.size) if weights is None else np.atleast_1d(np.asarray(weights, np.float64))
    if w.shape != shifts.shape:
        raise ValueError("weights must hold one weight per source")
    beta = float(beta)
    if not np.isfinite(beta):
        raise ValueError("beta must be finite")
    nz = srcs.shape[1]
    z = np.arange(nz)
    acc = np.zeros(srcs.shape[1:], np.float64)
    for i in range(shifts.size):
        n, c0, c1 = _shift_coeffs(shifts[i], w[i])
        if abs(float(shifts[i])) >= nz + 1:
            continue
        for off, c in ((n, c0), (n + 1, c1)):
            if off == n + 1 and c == 0.0:
                continue
            ok = (z + off >= 0) & (z + off < nz)
            acc[z[ok]] = acc[z[ok]] + c * srcs[i][z[ok] + off]
    if beta == 0.0:
        return acc
    if dst is None:
        raise ValueError("beta != 0 needs dst")
    dst = np.asarray(dst, np.float64)
    if dst.shape != acc.shape:
        raise ValueError("dst must have the shape of one source")
    return beta * dst + acc


def _gather_args(G, offsets, n, taper):
    G = np.asarray(G, np.float64)
    h = np.atleast_1d(np.asarray(offsets, np.float64))
    if h.ndim != 1 or not np.all(h == np.round(h)):
        raise ValueError("offsets must be a 1-D array of whole cells")
    if G.ndim < 2 or G.shape[0] != n:
        raise ValueError("expected %d images, got shape %s" % (n, G.shape))
    t = np.ones(h.size) if taper is None else np.atleast_1d(np.asarray(taper, np.float64))
    if t.shape != h.shape or not np.all(np.isfinite(t)):
        raise ValueError("taper must hold one finite weight per offset")
    return G, h, t


def angle_gather(E, offsets, tangents, taper=None):
    """``A_j = sum_l t_l S_{p_j h_l} E_l`` as ``(len(tangents), *shape)`` fp64 from the offset gather ``E``,
    ``(len(offsets), *shape)``, of the integer half-offsets ``offsets`` (``Engine.fourier_offset_images``)."""
    p = np.atleast_1d(np.asarray(tangents, np.float64))
    E, h, t = _gather_args(E, offsets, np.size(offsets), taper)
    return np.stack([shift_sum(E, pj * h, t) for pj in p])


def angle_gather_adjoint(A, offsets, tangents, taper=None):
    """``E'_l = t_l sum_j S_{-p_j h_l} A_j`` as ``(len(offsets), *shape)`` fp64: the exact transpose of
    :func:`angle_gather`, ``<A, T E> = <T^T A, E>`` to round-off."""
    p = np.atleast_1d(np.asarray(tangents, np.float64))
    A, h, t = _gather_args(A, offsets, p.size, taper)
    return np.stack([shift_sum(A, -(p * h[l]), np.full(p.size, t[l])) for l in range(h.size)])
