"""Host-side engine: one context per GPU behind the C-ABI (include/fwi.h).

No reference counterpart; entry-point names and argument
meaning follow BASELINE.json's north_star: forward(model, src, rec),
adjoint(residual), gradient().  NumPy is used only to own host buffers.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib

_COEF_ABS_SUM = {2: 4.0, 4: 16.0 / 3.0, 8: 2048.0 / 315.0}


def cfl_dt(c_max, h, ndim, order):
    """Stability limit of the leapfrog scheme, 2 h / (c_max sqrt(D sum|a_k|))."""
    return 2.0 * h / (c_max * math.sqrt(ndim * _COEF_ABS_SUM[order]))


def default_sigma_max(c_max, h, npml, refl=1e-3):
    """Peak damping rate of the quadratic sponge for a target reflection coefficient."""
    return 0.0 if npml <= 0 else 3.0 * c_max * math.log(1.0 / refl) / (2.0 * npml * h)


def ricker(nt, dt, f0, t0=None, dtype=np.float32):
    t0 = 1.5 / f0 if t0 is None else t0
    a = (np.pi * f0 * (np.arange(nt) * dt - t0)) ** 2
    return ((1.0 - 2.0 * a) * np.exp(-a)).astype(dtype)


class Engine:
    """Acoustic forward / adjoint / gradient on one MI355X.

    ``shape`` is (nz, nx) or (nz, ny, nx); ``model`` arrays are velocities in
    m/s of that shape.  Stateful like the C-ABI: ``adjoint`` uses the last
    ``forward``; ``gradient`` returns the sum over all adjoint calls since
    ``reset_gradient``.  ``ckpt_interval = K > 0`` replaces the store of every step's imaging term
    (``nt_max`` model-sized arrays) by wavefield snapshots every K steps plus recomputation.
    ``image_stride = S > 1`` stores and correlates the imaging term every S-th step only (weight S): an
    approximation of the time integral that is accurate while ``S * dt`` still samples the wavelet's
    band, with a store S times smaller and less adjoint traffic.
    ``update_form="increment"`` carries the recursion as (u, v = u - u_prev): same mathematics, ~4x less fp32
    round-off growth, 25 % more traffic.  ``abc="cpml"`` replaces the sponge by a convolutional PML.
    ``store_dtype="bf16"`` halves the forward-term store of an fp32 engine.
    ``illumination=True`` accumulates the source-side illumination (the pseudo-Hessian diagonal) beside the gradient:
    :meth:`illumination`; off by default, when it costs nothing.
    ``fourier=freqs`` (Hz) keeps ``len(freqs)`` Fourier coefficients of the forward term per cell instead of its history
    (:meth:`set_fourier_store`): ``2 F + fourier_batch + 1`` model-sized arrays, and a gradient of the forward term
    band-passed to those frequencies (:mod:`full_waveform_inversion_amd.fourier`).
    """

    def __init__(self, shape, h, dt, nt_max, order=8, npml=0, sigma_max=None, dtype="float32",
                 device=0, kernel="auto", zchunk=0, ckpt_interval=0, image_stride=1, update_form="standard",
                 abc="sponge", pml_alpha_max=0.0, store_dtype="native", launch_mode="auto",
                 illumination=False, fourier=None, fourier_batch=8):
        shape = tuple(int(s) for s in shape)
        if len(shape) not in (2, 3):
            raise ValueError("shape must be (nz, nx) or (nz, ny, nx)")
        self.shape, self.ndim = shape, len(shape)
        self.h, self.dt, self.order, self.npml = float(h), float(dt), int(order), int(npml)
        self.nt_max = int(nt_max)
        self.dtype = np.dtype(dtype)
        if self.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError("dtype must be float32 or float64")
        self.sigma_max = sigma_max
        self.device = int(device)
        self._kernel = {"auto": _lib.KERNEL_AUTO, "point": _lib.KERNEL_POINT,
                        "stream": _lib.KERNEL_STREAM}[kernel]
        self._zchunk = int(zchunk)
        self._ckpt = int(ckpt_interval)
        self._istride = int(image_stride)
        self._update_form = _lib.UPDATE_FORMS[update_form]
        self.update_form = update_form
        self._abc = _lib.ABCS[abc]
        self._store_dtype = _lib.STORE_DTYPES[store_dtype]
        # "graph": each sweep's time loop as one hipGraph; "auto": where that was measured to pay (fwi_config.launch_mode)
        self._launch_mode = _lib.LAUNCH_MODES[launch_mode]
        self.pml_alpha_max = float(pml_alpha_max)
        self._illum = bool(illumination)
        self._fourier = None if fourier is None else np.ascontiguousarray(np.atleast_1d(fourier), dtype=np.float64)
        # samples per transform launch.  8: the fastest at every F measured, profiles/fourier_probe.json
        self._fourier_batch = int(fourier_batch)
        self._lib = _lib.load()
        self._ctx = None
        self._nsrc = self._nrec = self._nt = 0
        if self.npml == 0 or self.sigma_max is not None:
            self._create(0.0)  # damping does not depend on the model: create the context now

    # -- context ---------------------------------------------------------------
    def _create(self, c_max):
        if self.sigma_max is None:
            self.sigma_max = default_sigma_max(c_max, self.h, self.npml)
        nz, nx = self.shape[0], self.shape[-1]
        ny = self.shape[1] if self.ndim == 3 else 1
        cfg = _lib.Config(C.sizeof(_lib.Config), self.ndim, nz, ny, nx, self.order, self.nt_max,
                          self.npml, self.device,
                          _lib.F32 if self.dtype == np.float32 else _lib.F64, self._kernel,
                          self._zchunk, self._ckpt, self._istride, self._update_form, self._abc,
                          self._store_dtype, self._launch_mode, self.h, self.dt, float(self.sigma_max),
                          self.pml_alpha_max)
        ctx = C.c_void_p()
        _lib.check(None, self._lib.fwi_create(C.byref(cfg), C.byref(ctx)))
        self._ctx = ctx
        if self._illum:
            self._chk(self._lib.fwi_set_illumination(ctx, 1))
        if self._fourier is not None:
            self._set_fourier()

    def close(self):
        if self._ctx is not None:
            self._lib.fwi_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _chk(self, code):
        _lib.check(self._ctx, code)

    @property
    def _c(self):
        """The context handle, or a clear error when it does not exist yet (with ``npml > 0`` and no
        ``sigma_max`` the context is created by the first ``set_model``, which knows ``c_max``)."""
        if self._ctx is None:
            raise _lib.FwiError(3, "no context yet: call set_model() first (npml > 0 without sigma_max defers "
                                   "fwi_create until the model's maximum velocity is known)")
        return self._ctx

    def _host(self, a, shape=None):
        a = np.ascontiguousarray(a, dtype=self.dtype)
        if shape is not None and a.shape != tuple(shape):
            raise ValueError("expected shape %s, got %s" % (tuple(shape), a.shape))
        return a

    def _idx(self, idx):
        idx = np.ascontiguousarray(np.asarray(idx, dtype=np.int32).reshape(-1, self.ndim))
        return idx

    @property
    def kernel_name(self):
        return self._lib.fwi_kernel_name(self._ctx).decode() if self._ctx is not None else ""

    # -- the three entry points ------------------------------------------------
    def set_model(self, model):
        model = self._host(model, self.shape)
        if self._ctx is None:
            self._create(float(model.max()))
        self._chk(self._lib.fwi_set_model(self._ctx, model.ctypes.data_as(C.c_void_p)))

    def forward(self, model, src, rec, save=True):
        """Seismograms ``(nt, nrec)``.  ``src = (src_idx (nsrc, ndim), wavelet (nt[, nsrc]))``."""
        if model is not None:
            self.set_model(model)
        if self._ctx is None:
            raise _lib.FwiError(3, "forward: no model set")
        src_idx, wavelet = src
        src_idx = self._idx(src_idx)
        rec_idx = self._idx(rec)
        wavelet = np.asarray(wavelet)
        if wavelet.ndim == 1:
            wavelet = wavelet[:, None]
        wavelet = self._host(wavelet)
        nt = wavelet.shape[0]
        if wavelet.shape[1] != len(src_idx):
            raise ValueError("wavelet must be (nt, nsrc)")
        seis = np.zeros((nt, len(rec_idx)), self.dtype)
        self._chk(self._lib.fwi_forward(
            self._ctx, nt, len(src_idx), src_idx.ctypes.data_as(C.c_void_p),
            wavelet.ctypes.data_as(C.c_void_p), len(rec_idx), rec_idx.ctypes.data_as(C.c_void_p),
            int(bool(save)), seis.ctypes.data_as(C.c_void_p)))
        self._nt, self._nsrc, self._nrec = nt, len(src_idx), len(rec_idx)
        return seis

    def forward_at(self, model, src, rec, save=True):
        """``forward`` with sources / receivers at fractional grid coordinates (cells; multilinear interpolation):
        ``src = (src_xyz (nsrc, ndim) | points.Spread, wavelet (nt[, nsrc]))``, ``rec = rec_xyz | Spread``.
        The per-point series are spread onto / gathered from the grid nodes ON THE DEVICE (``fwi_forward_spread``);
        the following ``adjoint`` / ``misfit_l2`` then work per point as well."""
        from .points import Spread
        if model is not None:
            self.set_model(model)
        if self._ctx is None:
            raise _lib.FwiError(3, "forward_at: no model set")
        S, wavelet = src
        S = S if isinstance(S, Spread) else Spread(S, self.shape)
        R = rec if isinstance(rec, Spread) else Spread(rec, self.shape)
        wavelet = np.asarray(wavelet)
        if wavelet.ndim == 1:
            wavelet = wavelet[:, None]
        wavelet = self._host(wavelet)
        nt = wavelet.shape[0]
        if wavelet.shape[1] != S.n:
            raise ValueError("wavelet must be (nt, nsrc points)")
        sw, rw = self._host(S.weights), self._host(R.weights)
        seis = np.zeros((nt, R.n), self.dtype)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        self._chk(self._lib.fwi_forward_spread(
            self._ctx, nt, S.n, len(S.idx), vp(S.idx), vp(S.pt_start), vp(sw), vp(wavelet), R.n, len(R.idx),
            vp(R.idx), vp(R.pt_start), vp(rw), int(bool(save)), vp(seis)))
        self._nt, self._nsrc, self._nrec = nt, S.n, R.n
        return seis

    def adjoint(self, residual, image=True):
        """Back-propagate ``residual (nt, nrec)``; returns ``F^T residual`` as ``(nt, nsrc)``.
        ``residual=None``: the residual :meth:`misfit_l2` formed on the device."""
        if self._ctx is None:
            raise _lib.FwiError(3, "adjoint: no forward run to adjoin")
        rp = None
        if residual is not None:
            residual = self._host(residual, (self._nt, self._nrec))
            rp = residual.ctypes.data_as(C.c_void_p)
        out = np.zeros((self._nt, self._nsrc), self.dtype)
        self._chk(self._lib.fwi_adjoint(self._ctx, rp, int(bool(image)), out.ctypes.data_as(C.c_void_p)))
        return out

    def misfit_l2(self, d_obs):
        """``J = 1/2 ||d_syn - d_obs||^2`` for the last forward's seismograms, residual formed and reduced on
        the device and kept there for ``adjoint(None)``."""
        d_obs = self._host(d_obs, (self._nt, self._nrec))
        J = C.c_double(0.0)
        self._chk(self._lib.fwi_misfit_l2(self._c, d_obs.ctypes.data_as(C.c_void_p), C.byref(J)))
        return J.value

    def _data_args(self, weights, taps):
        """(weights pointer, taps pointer, R) of ``fwi_misfit_weighted`` / ``fwi_residual_weight``, and the arrays they
        point into"""
        wp = tp = None
        R = 0
        if weights is not None:
            weights = self._host(weights, (self._nt, self._nrec))
            wp = weights.ctypes.data_as(C.c_void_p)
        if taps is not None:
            taps = np.ascontiguousarray(taps, dtype=np.float64)
            if taps.ndim != 1 or taps.size < 1:
                raise ValueError("taps must be the 1-D array b_0 .. b_R")
            tp, R = taps.ctypes.data_as(C.c_void_p), taps.size - 1
        return wp, tp, R, (weights, taps)

    def _trace_weights(self, trace_weights):
        """(pointer, array) of the weights per trace, (None, None) without any"""
        if trace_weights is None:
            return None, None
        tw = np.ascontiguousarray(trace_weights, dtype=np.float64)
        if tw.shape != (self._nrec,):
            raise ValueError("trace_weights must hold one weight per trace, shape (%d,)" % self._nrec)
        return tw.ctypes.data_as(C.c_void_p), tw

    def _per_trace(self, wanted, *dtypes):
        """(arrays, pointers) of the optional outputs per trace: zeros of these dtypes, or no arrays and null pointers"""
        arrays = tuple(np.zeros(self._nrec, t) for t in dtypes) if wanted else ()
        return arrays, tuple(a.ctypes.data_as(C.c_void_p) for a in arrays) or (None,) * len(dtypes)

    def _misfit(self, fn, d_obs, weights, taps, mid=(), outs=()):
        """J of the data misfit ``fn(ctx, d_obs, weights, taps, R, *mid, &J, *outs)`` of the last forward's seismograms"""
        d_obs = self._host(d_obs, (self._nt, self._nrec))
        wp, tp, R, _keep = self._data_args(weights, taps)
        J = C.c_double(0.0)
        self._chk(fn(self._c, d_obs.ctypes.data_as(C.c_void_p), wp, tp, R, *mid, C.byref(J), *outs))
        return J.value

    def misfit_weighted(self, d_obs, weights=None, taps=None):
        """``J = 1/2 ||M . B (d_syn - d_obs)||^2`` for the last forward's seismograms: ``B`` the symmetric FIR filter along
        time with the one-sided ``taps`` ``b_0 .. b_R`` (None: the identity), ``M`` the ``weights >= 0`` of the data's
        shape (None: 1; a negative weight is NOT refused on the device and acts as its absolute value).  The adjoint
        source ``B (M^2 . B (d_syn - d_obs))`` is formed on the device and kept there for ``adjoint(None)``
        (``fwi_misfit_weighted``; the NumPy twin is :class:`datafit.WeightedL2`)."""
        return self._misfit(self._lib.fwi_misfit_weighted, d_obs, weights, taps)

    def misfit_matched(self, d_obs, L, mu, weights=None, taps=None, f=None, normal=False):
        """Matching-filter (source-independent) misfit of the last forward's seismograms: with ``s' = B d_syn``,
        ``d' = B d_obs``, ``e = M . (C_f s' - d')`` and ``C_f`` the convolution along time with the two-sided filter
        ``f = (f_-L .. f_L)``, ``J = 1/2 sum e^2 + mu/2 |f|^2``.  ``f=None``: the filter is the minimiser
        ``(G + mu I)^-1 b`` of J (normal equations on the device), so that J is the reduced objective and the adjoint
        source ``B C_f^T (M . e)``, formed on the device and kept for ``adjoint(None)``, its gradient; otherwise the
        given ``2 L + 1`` coefficients are used.  ``mu >= 0`` is absolute (``datafit.prewhitening``).  ``weights`` and
        ``taps`` as in :meth:`misfit_weighted`.  Returns ``(J, f)``, with ``normal=True`` ``(J, f, G, b)``, ``G`` the
        ``K x K`` normal matrix without ``mu`` (``fwi_misfit_matched``; the NumPy twin is :class:`datafit.MatchedL2`)."""
        if int(L) != L:
            raise ValueError("L must be an integer")
        L = int(L)
        K = 2 * max(L, 0) + 1
        fp = None
        if f is not None:
            f = np.ascontiguousarray(f, dtype=np.float64)
            if f.shape != (K,):
                raise ValueError("f must hold the 2 L + 1 = %d coefficients f_-L .. f_L" % K)
            fp = f.ctypes.data_as(C.c_void_p)
        f_out = np.zeros(K)
        nrm = np.zeros(K * K + K) if normal else None
        J = self._misfit(self._lib.fwi_misfit_matched, d_obs, weights, taps, (
            L, float(mu), fp, f_out.ctypes.data_as(C.c_void_p), nrm.ctypes.data_as(C.c_void_p) if normal else None))
        if normal:
            return J, f_out, nrm[:K * K].reshape(K, K).copy(), nrm[K * K:].copy()
        return J, f_out

    def misfit_envelope(self, d_obs, hilbert, power=1, eps=None, weights=None, taps=None):
        """Envelope misfit of the last forward's seismograms: with ``s' = B d_syn``, ``d' = B d_obs``, ``H`` the
        antisymmetric Hilbert FIR filter along time with the one-sided taps ``hilbert = h_1 .. h_Q``
        (``datafit.hilbert_taps``) and ``E(x) = sqrt(x^2 + (H x)^2 + eps^2)``, ``J = 1/2 ||M . (E(s')^p - E(d')^p)||^2``,
        ``p = power`` in {1, 2}.  ``eps >= 0`` is absolute and must not depend on the synthetics (``> 0`` for ``p = 1``);
        None: ``datafit.envelope_floor(d_obs)``, 1 % of the largest observed amplitude.  ``weights`` and ``taps`` as in
        :meth:`misfit_weighted`.  The adjoint source ``dJ/dd_syn`` is formed on the device and kept there for
        ``adjoint(None)``.  Returns J (``fwi_misfit_envelope``; the NumPy twin is :class:`datafit.EnvelopeL2`)."""
        if eps is None:
            from .datafit import envelope_floor
            eps = envelope_floor(d_obs)
        h = np.ascontiguousarray(hilbert, dtype=np.float64)
        if h.ndim != 1 or h.size < 1:
            raise ValueError("hilbert must be the 1-D array h_1 .. h_Q")
        if int(power) != power:
            raise ValueError("power must be 1 or 2")
        return self._misfit(self._lib.fwi_misfit_envelope, d_obs, weights, taps,
                            (h.ctypes.data_as(C.c_void_p), h.size, int(power), float(eps)))

    def misfit_correlation(self, d_obs, eps=None, weights=None, taps=None, trace_weights=None, per_trace=False):
        """Trace-normalised zero-lag correlation misfit of the last forward's seismograms, which reads phase only and
        ignores the gain of every trace: with ``sh = M . B d_syn``, ``dh = M . B d_obs``,
        ``rho_j = <sh_j, dh_j> / (sqrt(|sh_j|^2 + eps^2) sqrt(|dh_j|^2 + eps^2))`` per trace and
        ``J = sum_j w_j (1 - rho_j)``.  ``eps >= 0`` is an absolute floor that must not depend on the synthetics; None:
        ``datafit.correlation_floor(d_obs)``, 1 % of the largest trace norm of the observed data.  ``weights`` and
        ``taps`` as in :meth:`misfit_weighted`; ``trace_weights``: the ``ntr`` weights ``w_j >= 0`` (None: 1), the only
        way to down-weight a trace.  A trace whose weighted data are zero does not count.  The adjoint source
        ``dJ/dd_syn`` is formed on the device and kept there for ``adjoint(None)``.  Returns J, with ``per_trace=True``
        ``(J, rho)`` (``fwi_misfit_correlation``; the NumPy twin is :class:`datafit.NormalizedCorrelation`)."""
        if eps is None:
            from .datafit import correlation_floor
            eps = correlation_floor(d_obs)
        twp, _keep = self._trace_weights(trace_weights)
        out, outp = self._per_trace(per_trace, np.float64)
        J = self._misfit(self._lib.fwi_misfit_correlation, d_obs, weights, taps, (twp, float(eps)), outp)
        return (J,) + out if per_trace else J

    def misfit_traveltime(self, d_obs, max_lag, weights=None, taps=None, trace_weights=None, per_trace=False):
        """Cross-correlation traveltime misfit of the last forward's seismograms, which measures how late every trace is:
        with ``sh = M . B d_syn``, ``dh = M . B d_obs`` and ``c_j(k) = sum_n sh[n + k, j] dh[n, j]`` over the lags
        ``|k| <= min(max_lag, nt - 1)``, ``tau_j`` is ``dt`` times the lag of the first maximum of ``c_j``, refined by the
        parabola through it and its two neighbours, and ``J = 1/2 sum_j w_j tau_j^2`` (s^2).  ``tau_j > 0``: the
        synthetics arrive late.  ``max_lag`` is in samples, ``1 .. 1024``.  A trace counts only if its maximum is positive,
        lies strictly inside the window and is a proper peak; otherwise its delay, its term of J and its adjoint source
        are 0 (a dead trace; a shift beyond the window).  ``weights`` and ``taps`` as in :meth:`misfit_weighted`,
        ``trace_weights`` as in :meth:`misfit_correlation`.  The adjoint source ``dJ/dd_syn`` is formed on the device and
        kept there for ``adjoint(None)``.  Returns J, with ``per_trace=True`` ``(J, tau, lag)``: the ``ntr`` delays in
        seconds and the picked lags ``k*`` of every trace, counting or not (``fwi_misfit_traveltime``; the NumPy twin is
        :class:`datafit.TraveltimeL2`)."""
        if int(max_lag) != max_lag:
            raise ValueError("max_lag must be an integer number of samples")
        twp, _keep = self._trace_weights(trace_weights)
        out, outp = self._per_trace(per_trace, np.float64, np.int32)
        J = self._misfit(self._lib.fwi_misfit_traveltime, d_obs, weights, taps, (twp, int(max_lag)), outp)
        return (J,) + out if per_trace else J

    def misfit_transport(self, d_obs, transform="softplus", param=None, weights=None, taps=None, trace_weights=None,
                         per_trace=False):
        """Trace-by-trace optimal-transport (W2) misfit of the last forward's seismograms, which compares whole traces as
        densities along time and grows with the square of a time shift however many periods it spans: with
        ``sh = M . B d_syn``, ``dh = M . B d_obs``, ``f = P(sh) / sum P(sh)`` and ``g = P(dh) / sum P(dh)`` per trace,
        ``W_j`` is the squared 2-Wasserstein distance between ``f`` and ``g`` as measures on the time samples (s^2) and
        ``J = 1/2 sum_j w_j W_j``.  ``transform``: ``"softplus"``, ``P(x) = log(1 + exp(b x)) / b`` with ``b = param``,
        or ``"linear"``, ``P(x) = x + c`` with ``c = param``; ``param > 0`` is absolute and must not depend on the
        synthetics; None: :meth:`datafit.TransportW2.param_of` of ``d_obs``.  A trace counts only if all its densities
        are finite and ``>= 0`` with positive sums (under ``linear``: nothing below ``-c``); otherwise its distance, its
        term of J and its adjoint source are 0.  ``weights`` and ``taps`` as in :meth:`misfit_weighted`,
        ``trace_weights`` as in :meth:`misfit_correlation`.  The adjoint source ``dJ/dd_syn`` is formed on the device and
        kept there for ``adjoint(None)``.  Returns J, with ``per_trace=True`` ``(J, w2, counts)``: the ``ntr`` distances
        ``W_j`` and 1 / 0 per trace (``fwi_misfit_transport``; the NumPy twin is :class:`datafit.TransportW2`)."""
        if transform not in _lib.OT_TRANSFORMS:
            raise ValueError("transform must be one of %s" % sorted(_lib.OT_TRANSFORMS))
        if param is None:
            from .datafit import TransportW2
            param = TransportW2(self.dt, transform).param_of(d_obs)
        twp, _keep = self._trace_weights(trace_weights)
        out, outp = self._per_trace(per_trace, np.float64, np.int32)
        J = self._misfit(self._lib.fwi_misfit_transport, d_obs, weights, taps,
                         (twp, _lib.OT_TRANSFORMS[transform], float(param)), outp)
        return (J,) + out if per_trace else J

    def misfit_adaptive(self, d_obs, L, lam=1e-2, weights=None, taps=None, trace_weights=None, per_trace=False):
        """Adaptive (per-trace matching-filter) misfit of the last forward's seismograms (adaptive waveform inversion,
        Warner & Guasch 2016), which keeps amplitude and phase, needs no pick and no window and grows with the square of
        a time shift up to the filter's half-length: with ``sh = M . B d_syn``, ``dh = M . B d_obs``, ``w_j`` the Wiener
        filter of ``2 L + 1`` coefficients with ``w_j * dh_j ~= sh_j`` (normal equations ``(A_j + lam a_j(0) I) w_j =
        c_j`` from the lag correlations, solved per trace on the device), ``W_j = sum_k (k dt)^2 w_k^2 / sum_k w_k^2``
        (s^2) and ``J = 1/2 sum_j tw_j W_j``.  ``L`` is in samples, ``1 .. 64``; ``lam > 0`` is a ridge relative to the
        trace's energy.  A gain per trace cancels.  ``d_obs == d_syn`` does NOT give ``J = 0``: ``sqrt(W)`` is then the
        width of the band-limited delta the ridge leaves, the floor below which a shift cannot be read.  A trace counts
        only if its data are alive, its system is positive definite and its filter has energy; otherwise its ``W``, its
        term of J and its adjoint source are 0.  ``weights`` and ``taps`` as in :meth:`misfit_weighted`,
        ``trace_weights`` as in :meth:`misfit_correlation`.  The adjoint source ``dJ/dd_syn`` is formed on the device and
        kept there for ``adjoint(None)``.  Returns J, with ``per_trace=True`` ``(J, W, counts, filters)``: the ``ntr``
        moments ``W_j``, 1 / 0 per trace and the filters ``(ntr, 2 L + 1)`` (``fwi_misfit_adaptive``; the NumPy twin is
        :class:`datafit.AdaptiveMatching`)."""
        if int(L) != L:
            raise ValueError("L must be an integer number of samples")
        L = int(L)
        twp, _keep = self._trace_weights(trace_weights)
        out, outp = self._per_trace(per_trace, np.float64, np.int32)
        if per_trace:
            filters = np.zeros((self._nrec, 2 * max(L, 0) + 1))
            out, outp = out + (filters,), outp + (filters.ctypes.data_as(C.c_void_p),)
        else:
            outp = outp + (None,)
        J = self._misfit(self._lib.fwi_misfit_adaptive, d_obs, weights, taps, (twp, L, float(lam)), outp)
        return (J,) + out if per_trace else J

    def misfit_adaptive_ms(self):
        """``(correlations, solve, source)``: the device times in ms of the three phases of the last
        :meth:`misfit_adaptive` call, from HIP events on the context's stream (``fwi_misfit_adaptive_ms``)."""
        ms = np.zeros(3)
        self._chk(self._lib.fwi_misfit_adaptive_ms(self._c, ms.ctypes.data_as(C.c_void_p)))
        return tuple(float(v) for v in ms)

    def misfit_robust(self, d_obs, kind, thresh, weights=None, taps=None, trace_weights=None, keep_irls=False,
                      per_trace=False):
        """Robust (M-estimator) misfit of the last forward's seismograms, which a few spiky traces or a noise burst do
        not dominate: with ``e = M . B (d_syn - d_obs)`` as in :meth:`misfit_weighted` and ``a_j > 0`` a threshold per
        trace in the units of the data, ``J = sum_j tw_j sum_n rho(e[n,j]; a_j)`` with ``kind`` ``"huber"``
        (``e^2 / 2`` up to ``|e| = a``, ``a |e| - a^2 / 2`` beyond), ``"hybrid"`` (``a^2 (sqrt(1 + (e/a)^2) - 1)``) or
        ``"cauchy"`` (``a^2 / 2 log(1 + (e/a)^2)``, NOT convex).  ``thresh``: the ``ntr`` thresholds, or one number for
        all; it is ``c`` times a scale of the residuals (``datafit.mad_scale``, :meth:`residual_median`) and must not
        depend on the synthetics; ``inf`` is huber's alone and makes it :meth:`misfit_weighted`.  ``weights`` and
        ``taps`` as there, ``trace_weights`` as in :meth:`misfit_correlation`.  The adjoint source ``B (M . tw psi e)``
        is formed on the device and kept there for ``adjoint(None)``; ``keep_irls=True`` also keeps
        ``W = tw M^2 psi(e)`` for :meth:`residual_weight_robust`.  Returns J, with ``per_trace=True``
        ``(J, J_trace, nout)``: the ``ntr`` terms of J and the number of samples of every trace beyond its threshold
        (``fwi_misfit_robust``; the NumPy twin is :class:`datafit.RobustMisfit`)."""
        if kind not in _lib.ROBUST_KINDS:
            raise ValueError("kind must be one of %s" % sorted(_lib.ROBUST_KINDS))
        a = np.asarray(thresh, dtype=np.float64)
        a = np.ascontiguousarray(np.broadcast_to(a, (self._nrec,)) if a.ndim == 0 else a)
        if a.shape != (self._nrec,):
            raise ValueError("thresh must be one number or one per trace, shape (%d,)" % self._nrec)
        twp, _keep = self._trace_weights(trace_weights)
        out, outp = self._per_trace(per_trace, np.float64, np.int32)
        J = self._misfit(self._lib.fwi_misfit_robust, d_obs, weights, taps,
                         (_lib.ROBUST_KINDS[kind], a.ctypes.data_as(C.c_void_p), twp, int(bool(keep_irls))) + outp)
        return (J,) + out if per_trace else J

    def residual_weight_robust(self, taps=None):
        """The residual on the device (what ``born`` left for ``adjoint(None)``) := ``B (W . (B residual))`` with the
        ``W = tw M^2 psi(e)`` that ``misfit_robust(keep_irls=True)`` kept on this forward: the IRLS (majoriser)
        Gauss-Newton weight of :meth:`misfit_robust`, positive semi-definite for every kind
        (``fwi_residual_weight_robust``; ``FWI_ESTATE`` without a kept ``W``, which the next forward drops)."""
        _wp, tp, R, _keep = self._data_args(None, taps)
        self._chk(self._lib.fwi_residual_weight_robust(self._c, tp, R))

    def residual_median(self, d_obs, weights=None, taps=None, per_trace=True):
        """``(med, count)``: the lower median of ``|e|``, ``e = M . B (d_syn - d_obs)`` of the last forward's
        seismograms, and the number of samples it is taken over (all, or with ``weights`` those whose weight is
        ``> 0``), per trace (``ntr`` values) or with ``per_trace=False`` of the whole gather (two numbers).  An exact
        order statistic, number ``(count - 1) // 2`` in ascending order, found on the device by a radix select; 0 where
        nothing counts.  ``1.4826 * med`` is the scale of :func:`datafit.mad_scale`.  Leaves no residual on the device;
        a misfit call can follow on the same forward (``fwi_residual_median``; the NumPy twin is
        :func:`datafit.median_abs`)."""
        d_obs = self._host(d_obs, (self._nt, self._nrec))
        wp, tp, R, _keep = self._data_args(weights, taps)
        n = self._nrec if per_trace else 1
        med, count = np.zeros(n), np.zeros(n, np.int64)
        self._chk(self._lib.fwi_residual_median(self._c, d_obs.ctypes.data_as(C.c_void_p), wp, tp, R,
                                                0 if per_trace else 1, med.ctypes.data_as(C.c_void_p),
                                                count.ctypes.data_as(C.c_void_p)))
        return (med, count) if per_trace else (float(med[0]), int(count[0]))

    def misfit_spectral(self, d_obs, freqs, kind="l2", eps=0.0, weights=None, taps=None, freq_weights=None,
                        trace_weights=None, per_pair=False):
        """Frequency-domain (spectral) misfit of the last forward's seismograms: with ``sh = M . B d_syn``,
        ``dh = M . B d_obs`` and ``S_kj``, ``O_kj`` their discrete Fourier coefficients at the ``F <= 64`` frequencies
        ``freqs`` (Hz; ``fourier.fourier_bins(nt, dt, 1, fmin, fmax)`` lists the bins of a band, off-bin frequencies
        are allowed), ``J = 1/2 sum_kj fw_k tw_j m_kj^2`` with ``m = |S - O|`` (``kind="l2"``), the phase difference
        ``phi`` in (-pi, pi] (``"phase"``), the logarithmic amplitude ratio ``a = 1/2 ln((|S|^2 + eps^2) / (|O|^2 +
        eps^2))`` (``"logamp"``) or both (``"log"``, the logarithmic misfit).  ``eps >= 0`` is an absolute floor in the
        units of ``|S|`` that must not depend on the synthetics (``datafit.spectral_floor``); under ``"phase"`` and
        ``"log"`` a pair counts only if ``|S|^2 > eps^2`` and ``|O|^2 > eps^2``.  ``weights`` and ``taps`` as in
        :meth:`misfit_weighted` (``datafit.laplace_damping`` gives the weights of a Laplace-Fourier misfit);
        ``freq_weights``: the ``F`` weights ``fw_k >= 0`` (None: 1; ``datafit.whitening_weights``); ``trace_weights`` as
        in :meth:`misfit_correlation`.  ``phi`` wraps: a shift beyond half a period of ``f_k`` reads as a smaller one of
        the other sign, and J is not differentiable at ``phi = +-pi``.  The adjoint source ``dJ/dd_syn`` is formed on
        the device and kept there for ``adjoint(None)``.  Returns J, with ``per_pair=True`` ``(J, phi, a, counts)``, each
        ``(F, ntr)`` (``fwi_misfit_spectral``; the NumPy twin is :class:`datafit.SpectralMisfit`)."""
        if kind not in _lib.SPEC_KINDS:
            raise ValueError("kind must be one of %s" % sorted(_lib.SPEC_KINDS))
        f = np.ascontiguousarray(np.atleast_1d(np.asarray(freqs, np.float64)))
        if f.ndim != 1 or f.size < 1:
            raise ValueError("freqs must be a non-empty 1-D array of frequencies in Hz")
        fwp = fw = None
        if freq_weights is not None:
            fw = np.ascontiguousarray(freq_weights, dtype=np.float64)
            if fw.shape != f.shape:
                raise ValueError("freq_weights must hold one weight per frequency, shape (%d,)" % f.size)
            fwp = fw.ctypes.data_as(C.c_void_p)
        twp, _keep = self._trace_weights(trace_weights)
        out = outp = ()
        if per_pair:
            out = tuple(np.zeros((f.size, self._nrec), t) for t in (np.float64, np.float64, np.uint8))
            outp = tuple(a.ctypes.data_as(C.c_void_p) for a in out)
        J = self._misfit(self._lib.fwi_misfit_spectral, d_obs, weights, taps,
                         (f.size, f.ctypes.data_as(C.c_void_p), _lib.SPEC_KINDS[kind], float(eps), fwp, twp),
                         outp or (None, None, None))
        return (J,) + out if per_pair else J

    def residual_weight(self, weights=None, taps=None):
        """The residual on the device (what ``born`` or a misfit call left for ``adjoint(None)``) := ``B M^2 B`` residual,
        the Gauss-Newton weight of :meth:`misfit_weighted` (``fwi_residual_weight``)."""
        wp, tp, R, _keep = self._data_args(weights, taps)
        self._chk(self._lib.fwi_residual_weight(self._c, wp, tp, R))

    def gradient(self, wrt="velocity"):
        if self._ctx is None:
            raise _lib.FwiError(3, "gradient: no model set")
        g = np.zeros(self.shape, self.dtype)
        w = {"velocity": _lib.WRT_VELOCITY, "slowness2": _lib.WRT_SLOWNESS2}[wrt]
        self._chk(self._lib.fwi_gradient(self._ctx, w, g.ctypes.data_as(C.c_void_p)))
        return g

    def reset_gradient(self):
        if self._ctx is not None:
            self._chk(self._lib.fwi_gradient_reset(self._ctx))

    def gradient_add_from(self, other):
        """This engine's gradient accumulator += ``other``'s (same shape, same GPU)."""
        self._chk(self._lib.fwi_gradient_add(self._ctx, other._ctx))

    # -- source-side illumination (include/fwi.h fwi_set_illumination) ------------
    @property
    def illumination_enabled(self):
        return self._illum

    def set_illumination(self, on):
        """Switch the illumination accumulator on (allocated and zeroed) or off (freed); takes effect with the next
        adjoint sweep.  A context that does not exist yet gets it when it is created."""
        if self._ctx is not None:
            self._chk(self._lib.fwi_set_illumination(self._ctx, int(bool(on))))  # (refused with the Fourier store)
        self._illum = bool(on)

    def illumination(self, wrt="velocity"):
        """H summed over the adjoint sweeps since ``reset_gradient``: ``(S / dt^4) sum_n q^n(x)^2`` for
        ``wrt="slowness2"``, times ``(2 / c^3)^2`` for ``wrt="velocity"``.  Raises while illumination is off."""
        h = np.zeros(self.shape, self.dtype)
        w = {"velocity": _lib.WRT_VELOCITY, "slowness2": _lib.WRT_SLOWNESS2}[wrt]
        self._chk(self._lib.fwi_illumination(self._c, w, h.ctypes.data_as(C.c_void_p)))
        return h

    def illumination_vec(self, slot, wrt="velocity"):
        """Vector ``slot`` := :meth:`illumination` on the device."""
        w = {"velocity": _lib.WRT_VELOCITY, "slowness2": _lib.WRT_SLOWNESS2}[wrt]
        self._chk(self._lib.fwi_illumination_vec(self._c, w, slot))

    def allreduce_illumination(self):
        self._chk(self._lib.fwi_allreduce_illumination(self._c))

    # -- Fourier-compressed forward-term store (include/fwi.h fwi_set_fourier_store) ------------------
    def _set_fourier(self):
        f = self._fourier
        if f is None:
            self._chk(self._lib.fwi_set_fourier_store(self._ctx, 0, None, 0))
        else:
            self._chk(self._lib.fwi_set_fourier_store(self._ctx, f.size, f.ctypes.data_as(C.c_void_p), self._fourier_batch))

    @property
    def fourier_freqs(self):
        """The frequencies (Hz) of the Fourier store, None while the engine keeps its configured store."""
        return None if self._fourier is None else self._fourier.copy()

    def set_fourier_store(self, freqs, batch=None):
        """Keep the forward term as its Fourier coefficients at ``freqs`` (Hz; 1 .. 64 of them, each in
        ``[0, 1 / (2 image_stride dt)]``) from the next ``forward(save=True)`` on, ``batch`` (1 .. 8; None: as it is)
        samples per transform launch; ``freqs=None`` frees the coefficients and returns to the configured store.  What an
        earlier forward stored is discarded.  Refused with ``ckpt_interval > 0``, ``store_dtype="bf16"`` and while
        illumination is on.  A context that does not exist yet gets the store when it is created."""
        if freqs is not None:
            freqs = np.ascontiguousarray(np.atleast_1d(freqs), dtype=np.float64)
            if freqs.ndim != 1:
                raise ValueError("freqs must be a 1-D array of frequencies in Hz")
        old = self._fourier, self._fourier_batch
        self._fourier = freqs
        if batch is not None:
            self._fourier_batch = int(batch)
        if self._ctx is not None:
            try:
                self._set_fourier()
            except _lib.FwiError:
                self._fourier, self._fourier_batch = old  # a refused call leaves the context as it was
                raise

    def fourier_spectrum(self):
        """``Q_k`` of the last ``forward(save=True)`` as a complex ``(F, *shape)`` array: the monochromatic forward terms
        ``sum_j q^{jS} exp(-i 2 pi f_k j S dt)`` (``fwi_fourier_spectrum``)."""
        if self._fourier is None:
            raise _lib.FwiError(3, "fourier_spectrum: the Fourier store is off (set_fourier_store)")
        out = np.zeros((self._fourier.size,) + self.shape, np.complex64 if self.dtype == np.float32 else np.complex128)
        re, im = np.zeros(self.shape, self.dtype), np.zeros(self.shape, self.dtype)
        for k in range(self._fourier.size):
            self._chk(self._lib.fwi_fourier_spectrum(self._c, k, re.ctypes.data_as(C.c_void_p),
                                                     im.ctypes.data_as(C.c_void_p)))
            out[k] = re + 1j * im
        return out

    # -- spectral imaging on the Fourier store (include/fwi.h fwi_adjoint_spectral) -------------------------------
    def _freq_weights(self, freq_weights):
        """(pointer, array) of the ``F`` weights per frequency, (None, None) without any (or without a store: the call
        that follows refuses)"""
        if freq_weights is None or self._fourier is None:
            return None, None
        fw = np.ascontiguousarray(freq_weights, dtype=np.float64)
        if fw.shape != self._fourier.shape:
            raise ValueError("freq_weights must hold one weight per frequency, shape (%d,)" % self._fourier.size)
        return fw.ctypes.data_as(C.c_void_p), fw

    def adjoint_spectral(self, residual=None, freq_weights=None, image=True):
        """:meth:`adjoint` of a Fourier-store engine with the imaging done in the frequency domain: the sweep of
        ``adjoint(residual, image=False)`` (the same ``F^T residual``, bit for bit) with the Fourier coefficients ``M_k`` of
        the adjoint field accumulated behind it (``fwi_adjoint_spectral``), then, with ``image``, the gradient accumulator
        ``+= sum_k a_k w_k Re(Q_k conj M_k)`` with ``a = freq_weights`` (None: 1; ``fwi_fourier_image``).  With unit
        weights that is what ``adjoint(residual)`` adds on this engine, to round-off.  The per-frequency terms stay
        readable: :meth:`fourier_gradient`, :meth:`fourier_gradients`, :meth:`fourier_adjoint_spectrum`."""
        fwp, _keep = self._freq_weights(freq_weights)
        rp = None
        if residual is not None:
            residual = self._host(residual, (self._nt, self._nrec))
            rp = residual.ctypes.data_as(C.c_void_p)
        out = np.zeros((self._nt, self._nsrc), self.dtype)
        self._chk(self._lib.fwi_adjoint_spectral(self._c, rp, out.ctypes.data_as(C.c_void_p)))
        if image:
            self._chk(self._lib.fwi_fourier_image(self._c, fwp))
        return out

    def fourier_image(self, freq_weights=None):
        """Gradient accumulator ``+= sum_k a_k w_k Re(Q_k conj M_k)`` of the last :meth:`adjoint_spectral`
        (``fwi_fourier_image``): what ``adjoint_spectral(image=True)`` ends with, for a sweep run with ``image=False``."""
        fwp, _keep = self._freq_weights(freq_weights)
        self._chk(self._lib.fwi_fourier_image(self._c, fwp))

    def fourier_gradient(self, freq_weights=None, wrt="velocity"):
        """``sum_k a_k g_k`` of the last :meth:`adjoint_spectral`, model-shaped: the gradient :meth:`gradient` would return
        if the accumulator held that shot's spectral image alone (``fwi_fourier_gradient``).  The accumulator is not
        touched."""
        fwp, _keep = self._freq_weights(freq_weights)
        g = np.zeros(self.shape, self.dtype)
        w = {"velocity": _lib.WRT_VELOCITY, "slowness2": _lib.WRT_SLOWNESS2}[wrt]
        self._chk(self._lib.fwi_fourier_gradient(self._c, w, fwp, g.ctypes.data_as(C.c_void_p)))
        return g

    def fourier_gradient_vec(self, slot, freq_weights=None, wrt="velocity"):
        """Vector ``slot`` := :meth:`fourier_gradient` on the device."""
        fwp, _keep = self._freq_weights(freq_weights)
        w = {"velocity": _lib.WRT_VELOCITY, "slowness2": _lib.WRT_SLOWNESS2}[wrt]
        self._chk(self._lib.fwi_fourier_gradient_vec(self._c, w, fwp, slot))

    def fourier_gradients(self, wrt="velocity"):
        """Every per-frequency gradient ``g_k`` of the last :meth:`adjoint_spectral` as ``(F, *shape)``."""
        if self._fourier is None:
            raise _lib.FwiError(3, "fourier_gradients: the Fourier store is off (set_fourier_store)")
        eye = np.eye(self._fourier.size)
        return np.stack([self.fourier_gradient(eye[k], wrt) for k in range(self._fourier.size)])

    def fourier_adjoint_spectrum(self):
        """``M_k`` of the last :meth:`adjoint_spectral` as a complex ``(F, *shape)`` array: the monochromatic adjoint
        fields ``sum_j mu^{jS+1} exp(-i 2 pi f_k j S dt)`` (``fwi_fourier_adjoint_spectrum``)."""
        if self._fourier is None:
            raise _lib.FwiError(3, "fourier_adjoint_spectrum: the Fourier store is off (set_fourier_store)")
        out = np.zeros((self._fourier.size,) + self.shape, np.complex64 if self.dtype == np.float32 else np.complex128)
        re, im = np.zeros(self.shape, self.dtype), np.zeros(self.shape, self.dtype)
        for k in range(self._fourier.size):
            self._chk(self._lib.fwi_fourier_adjoint_spectrum(self._c, k, re.ctypes.data_as(C.c_void_p),
                                                             im.ctypes.data_as(C.c_void_p)))
            out[k] = re + 1j * im
        return out

    def fourier_illumination(self, freq_weights=None, wrt="velocity"):
        """``(S / dt^4) sum_k a_k w_k |Q_k|^2`` of the last ``forward(save=True)`` (times ``(2 / c^3)^2`` for
        ``wrt="velocity"``), in the units of :meth:`illumination` (``fwi_fourier_illumination``); ``a = freq_weights >= 0``
        (None: 1).  On bin frequencies this is the illumination of the band-limited forward term, with all bins that of
        the term itself; off the bins it is this formula.  One shot's; the caller sums over shots."""
        fwp, _keep = self._freq_weights(freq_weights)
        h = np.zeros(self.shape, self.dtype)
        w = {"velocity": _lib.WRT_VELOCITY, "slowness2": _lib.WRT_SLOWNESS2}[wrt]
        self._chk(self._lib.fwi_fourier_illumination(self._c, w, fwp, h.ctypes.data_as(C.c_void_p)))
        return h

    def fourier_illumination_vec(self, slot, freq_weights=None, wrt="velocity"):
        """Vector ``slot`` := :meth:`fourier_illumination` on the device."""
        fwp, _keep = self._freq_weights(freq_weights)
        w = {"velocity": _lib.WRT_VELOCITY, "slowness2": _lib.WRT_SLOWNESS2}[wrt]
        self._chk(self._lib.fwi_fourier_illumination_vec(self._c, w, fwp, slot))

    # -- extended images on the Fourier store (include/fwi.h fwi_fourier_offset_image, fwi_fourier_lag_image) -----
    def _axis(self, axis):
        """Grid axis ``0 .. ndim - 1`` from an index or ``"z"`` / ``"y"`` / ``"x"`` (``"y"``: 3-D only)"""
        if isinstance(axis, str):
            names = "zyx" if len(self.shape) == 3 else "zx"
            if len(axis) != 1 or axis not in names:
                raise ValueError("axis must be an index or one of %s" % ", ".join(repr(n) for n in names))
            return names.index(axis)
        return int(axis)

    def fourier_offset_image_vec(self, slot, axis, h, freq_weights=None):
        """Vector ``slot`` := the subsurface-offset image ``E_h`` of the last :meth:`adjoint_spectral` on the device
        (``fwi_fourier_offset_image_vec``; one lag of :meth:`fourier_offset_images`)."""
        fwp, _keep = self._freq_weights(freq_weights)
        self._chk(self._lib.fwi_fourier_offset_image_vec(self._c, self._axis(axis), int(h), fwp, slot))

    def fourier_offset_images(self, axis, offsets, freq_weights=None):
        """Subsurface-offset common-image gather of the last :meth:`adjoint_spectral` as ``(len(offsets), *shape)``: for
        every integer ``h`` of ``offsets`` (cells along ``axis``, an index in grid order or ``"z"`` / ``"y"`` / ``"x"``)

            ``E_h(x) = -(S / dt^2) sum_k a_k w_k Re(Q_k(x - h e) conj M_k(x + h e))``

        in the units of ``fourier_gradient(wrt="slowness2")``, zero wherever ``x - h e`` or ``x + h e`` leaves the grid
        (``fwi_fourier_offset_image``).  ``h = 0`` is that gradient, bit for bit.  For any set of frequencies this is the
        band-limited imaging sum ``sum_j mu^{jS+1}(x + h e) q~^{jS}(x - h e)``.  One streaming pass over the resident
        coefficients per lag, no further sweep; ``a = freq_weights`` (None: 1).  One shot's; the caller sums over shots
        (:func:`shots.extended_image`)."""
        fwp, _keep = self._freq_weights(freq_weights)
        ax = self._axis(axis)
        offsets = [int(h) for h in np.atleast_1d(offsets)]
        E = np.zeros((len(offsets),) + self.shape, self.dtype)
        for l, h in enumerate(offsets):
            self._chk(self._lib.fwi_fourier_offset_image(self._c, ax, h, fwp, E[l].ctypes.data_as(C.c_void_p)))
        return E

    def fourier_lag_image_vec(self, slot, tau, freq_weights=None):
        """Vector ``slot`` := the time-lag image ``E_tau`` of the last :meth:`adjoint_spectral` on the device
        (``fwi_fourier_lag_image_vec``; one lag of :meth:`fourier_lag_images`)."""
        fwp, _keep = self._freq_weights(freq_weights)
        self._chk(self._lib.fwi_fourier_lag_image_vec(self._c, float(tau), fwp, slot))

    def fourier_lag_images(self, taus, freq_weights=None):
        """Time-lag common-image gather of the last :meth:`adjoint_spectral` as ``(len(taus), *shape)``: for every finite
        ``tau`` of ``taus`` (seconds)

            ``E_tau(x) = -(S / dt^2) sum_k a_k w_k Re(Q_k(x) conj M_k(x) exp(-i 2 pi f_k tau))``

        in the units of ``fourier_gradient(wrt="slowness2")`` (``fwi_fourier_lag_image``); ``tau = 0`` is that gradient,
        bit for bit.  Where every frequency is a bin of the sampled axis and ``tau = m S dt`` this is the imaging sum with
        the sampled forward term delayed circularly by ``m`` samples; off the bins, or at any other ``tau``, it is this
        formula and no such sum.  One streaming pass per lag; ``a = freq_weights`` (None: 1)."""
        fwp, _keep = self._freq_weights(freq_weights)
        taus = [float(t) for t in np.atleast_1d(taus)]
        E = np.zeros((len(taus),) + self.shape, self.dtype)
        for l, tau in enumerate(taus):
            self._chk(self._lib.fwi_fourier_lag_image(self._c, tau, fwp, E[l].ctypes.data_as(C.c_void_p)))
        return E

    # -- tomographic / migration split of the Fourier-store gradient (include/fwi.h fwi_fourier_split_image) ---------
    _SPLIT_PARTS = {"same": _lib.SPLIT_SAME, "opposite": _lib.SPLIT_OPPOSITE, "hilbert": _lib.SPLIT_HILBERT}

    def _split_args(self, part, axis, taps, wrt):
        if part not in self._SPLIT_PARTS:
            raise ValueError("part must be one of 'same', 'opposite', 'hilbert'")
        t = np.ascontiguousarray(np.asarray(taps, np.float64))
        if t.ndim != 1:
            raise ValueError("taps must be the 1-D one-sided taps t_1 .. t_R")
        w = {"velocity": _lib.WRT_VELOCITY, "slowness2": _lib.WRT_SLOWNESS2}[wrt]
        return w, self._SPLIT_PARTS[part], self._axis(axis), t.size, t.ctypes.data_as(C.c_void_p), t

    def fourier_split_image_vec(self, slot, part, axis, taps, freq_weights=None, wrt="velocity"):
        """Vector ``slot`` := one part of the split of :meth:`fourier_gradient` on the device
        (``fwi_fourier_split_image_vec``); ``part``: ``"same"``, ``"opposite"`` or ``"hilbert"``, as
        :meth:`fourier_split_image`."""
        fwp, _keep = self._freq_weights(freq_weights)
        w, p, ax, n, tp, _t = self._split_args(part, axis, taps, wrt)
        self._chk(self._lib.fwi_fourier_split_image_vec(self._c, w, p, ax, n, tp, fwp, slot))

    def fourier_split_image(self, part, axis, taps, freq_weights=None, wrt="velocity"):
        """One part of the split of :meth:`fourier_gradient` along ``axis`` (an index in grid order or ``"z"`` / ``"y"`` /
        ``"x"``), model-shaped (``fwi_fourier_split_image``).  With ``H`` the antisymmetric FIR of the one-sided ``taps``
        ``t_1 .. t_R`` along that axis (``datafit.hilbert_taps(R)``: a Hilbert transformer; zero extension at the grid's
        faces, zero taps skipped, at most ``_lib.SPLIT_RMAX`` taps)

            ``part(x) = kappa sum_k a_k w_k [alpha Re(Q_k conj M_k) + beta Re(H Q_k conj H M_k)]``

        with ``(alpha, beta) = (1/2, 1/2)`` for ``"same"`` (the pairs of equal direction along the axis: low wavenumber,
        tomographic), ``(1/2, -1/2)`` for ``"opposite"`` (high wavenumber, migration) and ``(0, 1)`` for ``"hilbert"``;
        ``kappa`` and ``wrt`` as in :meth:`fourier_gradient`, which ``same + opposite`` equals to round-off.  Neither part
        is the gradient of the misfit: they are the two halves of it.  One streaming pass over the resident coefficients,
        no further sweep; nothing on the context is written.  One shot's; the caller sums over shots
        (:func:`shots.split_gradient`)."""
        fwp, _keep = self._freq_weights(freq_weights)
        w, p, ax, n, tp, _t = self._split_args(part, axis, taps, wrt)
        g = np.zeros(self.shape, self.dtype)
        self._chk(self._lib.fwi_fourier_split_image(self._c, w, p, ax, n, tp, fwp, g.ctypes.data_as(C.c_void_p)))
        return g

    def fourier_gradient_split(self, axis, taps, freq_weights=None, wrt="velocity"):
        """``(tomographic, migration)``: the ``"same"`` and ``"opposite"`` parts of :meth:`fourier_split_image`.  Their sum
        is :meth:`fourier_gradient` to round-off; neither is the gradient of the misfit, they are the two halves of it.
        Below about ``2 / (R + 1)`` cycles per cell along the axis the filter's transition band leaves energy in both,
        and zero extension distorts the ``R`` cells next to each face."""
        return (self.fourier_split_image("same", axis, taps, freq_weights, wrt),
                self.fourier_split_image("opposite", axis, taps, freq_weights, wrt))

    def fourier_hilbert_image(self, axis, taps, freq_weights=None, wrt="velocity"):
        """``X = kappa sum_k a_k w_k Re(H Q_k conj H M_k)``, the ``"hilbert"`` part of :meth:`fourier_split_image`:
        ``tomographic = (g + X) / 2`` and ``migration = (g - X) / 2`` with ``g`` of :meth:`fourier_gradient`."""
        return self.fourier_split_image("hilbert", axis, taps, freq_weights, wrt)

    def store_bytes(self):
        """Device bytes held for the forward store of whichever kind (``fwi_store_bytes``); 0 before the first
        ``forward(save=True)`` allocates it."""
        n = C.c_int64(0)
        self._chk(self._lib.fwi_store_bytes(self._c, C.byref(n)))
        return int(n.value)

    # -- Born modelling (include/fwi.h fwi_born, fwi_born_imaging) -----------------------------------
    born_leaves_residual = True  # ``born`` keeps J dm on the device as the residual of ``adjoint(None)``

    def _born(self, call, wrt, mode, download):
        w = {"velocity": _lib.WRT_VELOCITY, "slowness2": _lib.WRT_SLOWNESS2}[wrt]
        out = np.zeros((self._nt, self._nrec), self.dtype) if download else None
        self._chk(call(w, _lib.BORN_MODES[mode], out.ctypes.data_as(C.c_void_p) if download else None))
        return out

    born_operators = ("exact", "imaging")  # what ``born(..., operator=)`` accepts (shots.Shot.born asks)

    def _born_call(self, operator, vec):
        if operator not in self.born_operators:
            raise ValueError("operator must be 'exact' or 'imaging'")
        return getattr(self._lib, "fwi_born" + ("_imaging" if operator == "imaging" else "") + ("_vec" if vec else ""))

    def born(self, dm, wrt="velocity", mode="auto", download=True, operator="exact"):
        """Linearised (Born) data ``J dm`` as ``(nt, nrec)`` at the receivers of the last ``forward(save=True)``, whose
        store it reads: the derivative of ``forward`` along the model perturbation ``dm`` (a velocity perturbation, or
        one of ``1 / c^2`` with ``wrt="slowness2"``).  The data also stay on the device as the residual of the next
        ``adjoint(None)``, so ``forward(save=True)``, ``born``, ``adjoint(None)``, ``gradient`` is the Gauss-Newton
        product ``J^T J dm``; ``download=False`` skips the copy to the host and returns None.  ``mode``: "scatter"
        (every engine), "fused" (3-D fp32 O(8) stream-kernel engines without the CPML: the scattering source inside the
        step kernel, about 0.6 - 0.75 of the time) or "auto" (fused where it exists); :attr:`born_path` names the path
        taken.

        ``operator="exact"`` is the derivative of ``forward`` and needs a store that holds every step in the field's
        type: it is refused with ``image_stride > 1``, ``store_dtype="bf16"`` or ``ckpt_interval > 0``.
        ``operator="imaging"`` is the operator whose exact transpose THIS engine's ``adjoint(image)`` + ``gradient``
        are (``fwi_born_imaging``): the same thing, bit for bit, on a plain engine and with checkpointing; with
        ``image_stride = S`` the scattering source acts on every S-th step with weight S, with the bf16 store it is
        formed from the rounded store.  It runs on every engine and keeps ``J^T J`` symmetric on each."""
        dm = self._host(dm, self.shape)
        call = self._born_call(operator, False)
        return self._born(lambda w, m, o: call(self._c, w, dm.ctypes.data_as(C.c_void_p), m, o), wrt, mode, download)

    def born_vec(self, slot, wrt="velocity", mode="auto", download=True, operator="exact"):
        """:meth:`born` with ``dm`` read from the device vector ``slot``."""
        call = self._born_call(operator, True)
        return self._born(lambda w, m, o: call(self._c, w, int(slot), m, o), wrt, mode, download)

    # -- Born and extended Born modelling on the Fourier store (include/fwi.h fwi_fourier_born) -------
    def fourier_born(self, dm, freq_weights=None, wrt="velocity", mode="auto", download=True):
        """:meth:`born` ``(operator="imaging")`` of a Fourier-store engine, which refuses :meth:`born` itself: the Born
        data ``J_a dm`` as ``(nt, nrec)`` with the scattering source synthesised from the coefficients ``Q_k`` of the last
        ``forward(save=True)``, ``q~_a = sum_k a_k w_k Re(Q_k exp(i theta_kj))``, ``a = freq_weights`` (None: 1;
        ``fwi_fourier_born``).  With ``a = 1`` the exact transpose of ``adjoint(image=True)`` + ``gradient`` on this
        engine, with any ``a`` that of ``adjoint_spectral`` + ``fourier_gradient(a)``: ``J_a^T J_a`` is symmetric positive
        semi-definite.  ``Q_k``, ``M_k`` and the gradient accumulator are not touched; the data stay on the device as the
        residual of the next ``adjoint(None)`` or ``adjoint_spectral(None)``.  ``mode``, ``download``: as :meth:`born`."""
        fwp, _keep = self._freq_weights(freq_weights)
        dm = self._host(dm, self.shape)
        call = self._lib.fwi_fourier_born
        return self._born(lambda w, m, o: call(self._c, w, dm.ctypes.data_as(C.c_void_p), fwp, m, o), wrt, mode, download)

    def fourier_born_vec(self, slot, freq_weights=None, wrt="velocity", mode="auto", download=True):
        """:meth:`fourier_born` with ``dm`` read from the device vector ``slot``."""
        fwp, _keep = self._freq_weights(freq_weights)
        call = self._lib.fwi_fourier_born_vec
        return self._born(lambda w, m, o: call(self._c, w, int(slot), fwp, m, o), wrt, mode, download)

    def _ext_lags(self, kind, lags, axis):
        """(kind code, grid axis, n, offsets pointer, taus pointer, keep-alive) of an extended Born call"""
        if kind not in _lib.EXT_KINDS:
            raise ValueError("kind must be 'offset' or 'timelag'")
        lags = np.atleast_1d(lags)
        if lags.ndim != 1 or lags.size < 1:
            raise ValueError("lags must hold at least one lag")
        if kind == "offset":
            if axis is None:
                raise ValueError("axis is required for kind='offset'")
            if not np.all(np.equal(np.mod(lags, 1), 0)):
                raise ValueError("the lags of kind='offset' are whole numbers of cells")
            arr = np.ascontiguousarray(lags, dtype=np.int32)
            return _lib.EXT_KINDS[kind], self._axis(axis), arr.size, arr.ctypes.data_as(C.c_void_p), None, arr
        arr = np.ascontiguousarray(lags, dtype=np.float64)
        return _lib.EXT_KINDS[kind], 0, arr.size, None, arr.ctypes.data_as(C.c_void_p), arr

    def fourier_born_extended(self, kind, lags, images, axis=None, freq_weights=None, mode="auto", download=True):
        """Extended Born modelling (demigration) on a Fourier-store engine: the data ``J_ext E`` as ``(nt, nrec)`` of the
        gather ``images`` (``(len(lags), *shape)``, in the units of :meth:`fourier_offset_images` /
        :meth:`fourier_lag_images`), defined as the exact transpose of those calls (``fwi_fourier_born_extended``):
        ``<J_ext E, r> = sum_l <E_l, image_l(r)>`` for every residual ``r``.  ``kind="offset"``: ``lags`` are integers in
        cells along ``axis`` (an index in grid order or ``"z"`` / ``"y"`` / ``"x"``); ``kind="timelag"`` (or ``"time"``,
        as :func:`shots.extended_image` names it): ``lags`` are seconds.  The extended scattering spectrum ``P_k(y) = sum_l E_l(y - h_l e) Q_k(y - 2 h_l e)`` (time lag:
        ``E_l Q_k exp(-i 2 pi f_k tau_l)``) is written INTO THE ARRAYS THAT HOLD ``M_k``: :meth:`fourier_gradient`, the
        extended images and :meth:`fourier_adjoint_spectrum` are refused until the next :meth:`adjoint_spectral`.  The
        sweep then injects ``S (-c^2) sum_k a_k w_k Re(P_k exp(i theta_kj))``.  With the single lag 0 and
        ``images[0] = dm`` it equals ``fourier_born(dm, wrt="slowness2")`` to round-off.  The data stay on the device as
        the residual of the next ``adjoint_spectral(None)``."""
        k, ax, n, op, tp, _lags = self._ext_lags(kind, lags, axis)
        fwp, _keep = self._freq_weights(freq_weights)
        images = self._host(images, (n,) + self.shape)
        call = self._lib.fwi_fourier_born_extended
        out = np.zeros((self._nt, self._nrec), self.dtype) if download else None
        self._chk(call(self._c, k, ax, n, op, tp, images.ctypes.data_as(C.c_void_p), fwp, _lib.BORN_MODES[mode],
                       out.ctypes.data_as(C.c_void_p) if download else None))
        return out

    def fourier_born_extended_vec(self, kind, lags, slots, axis=None, freq_weights=None, mode="auto", download=True):
        """:meth:`fourier_born_extended` with the gather read from the device vectors ``slots``, one per lag."""
        k, ax, n, op, tp, _lags = self._ext_lags(kind, lags, axis)
        fwp, _keep = self._freq_weights(freq_weights)
        sl = np.ascontiguousarray(np.atleast_1d(slots), dtype=np.int32)
        if sl.shape != (n,):
            raise ValueError("slots must hold one vector slot per lag, shape (%d,)" % n)
        out = np.zeros((self._nt, self._nrec), self.dtype) if download else None
        self._chk(self._lib.fwi_fourier_born_extended_vec(self._c, k, ax, n, op, tp, sl.ctypes.data_as(C.c_void_p), fwp,
                                                          _lib.BORN_MODES[mode],
                                                          out.ctypes.data_as(C.c_void_p) if download else None))
        return out

    @property
    def born_path(self):
        """Name of the path the last Born sweep took ("scatter" or "fused"; "none" before the first)."""
        return self._lib.fwi_born_path(self._ctx).decode() if self._ctx is not None else "none"

    # -- reductions, exchange, measurement --------------------------------------
    def dot(self, a, b):
        a, b = self._host(a).ravel(), self._host(b).ravel()
        if a.size != b.size:
            raise ValueError("dot: size mismatch")
        out = C.c_double(0.0)
        self._chk(self._lib.fwi_dot(self._c, a.ctypes.data_as(C.c_void_p),
                                    b.ctypes.data_as(C.c_void_p), a.size, C.byref(out)))
        return out.value

    @staticmethod
    def comm_unique_id():
        buf = C.create_string_buffer(_lib.UNIQUE_ID_BYTES)
        _lib.check(None, _lib.load().fwi_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, rank, nranks, unique_id):
        if len(unique_id) != _lib.UNIQUE_ID_BYTES:
            raise ValueError("unique id must be %d bytes" % _lib.UNIQUE_ID_BYTES)
        self._chk(self._lib.fwi_comm_init(self._c, rank, nranks, C.c_char_p(unique_id)))

    def allreduce_gradient(self):
        self._chk(self._lib.fwi_allreduce_gradient(self._c))

    def allreduce_f64(self, vals, op="sum"):
        arr = (C.c_double * len(vals))(*vals)
        fn = {"sum": self._lib.fwi_allreduce_f64, "max": self._lib.fwi_allreduce_f64_max}[op]
        self._chk(fn(self._c, arr, len(vals)))
        return list(arr)

    def comm_info(self):
        """(nranks, rank) as RCCL reports them for this context's communicator."""
        n, r = C.c_int32(0), C.c_int32(-1)
        self._chk(self._lib.fwi_comm_info(self._c, C.byref(n), C.byref(r)))
        return int(n.value), int(r.value)

    def comm_abort(self):
        if self._ctx is not None:
            self._chk(self._lib.fwi_comm_abort(self._ctx))

    # -- device-resident model-shaped vectors (optimiser state) ------------------------
    def vec_create(self, count):
        self._chk(self._lib.fwi_vec_create(self._c, int(count)))

    def vec_upload(self, slot, a):
        a = self._host(a, self.shape)
        self._chk(self._lib.fwi_vec_upload(self._c, slot, a.ctypes.data_as(C.c_void_p)))

    def vec_download(self, slot):
        out = np.empty(self.shape, self.dtype)
        self._chk(self._lib.fwi_vec_download(self._c, slot, out.ctypes.data_as(C.c_void_p)))
        return out

    def vec_copy(self, dst, src):
        self._chk(self._lib.fwi_vec_copy(self._c, dst, src))

    def vec_axpby(self, y, a, x, b=1.0):
        """y = a * x + b * y on the device."""
        self._chk(self._lib.fwi_vec_axpby(self._c, y, float(a), x, float(b)))

    def vec_dot(self, x, y):
        out = C.c_double(0.0)
        self._chk(self._lib.fwi_vec_dot(self._c, x, y, C.byref(out)))
        return out.value

    def vec_absmax(self, x):
        out = C.c_double(0.0)
        self._chk(self._lib.fwi_vec_absmax(self._c, x, C.byref(out)))
        return out.value

    def vec_mul(self, y, x):
        """y = x * y, elementwise, on the device."""
        self._chk(self._lib.fwi_vec_mul(self._c, y, x))

    def vec_recip(self, y, a=1.0, b=0.0):
        """y = a / (y + b), elementwise, on the device."""
        self._chk(self._lib.fwi_vec_recip(self._c, y, float(a), float(b)))

    def vec_smooth(self, slot, sigma):
        """Vector ``slot`` := S slot, the separable Gaussian of width ``sigma`` cells (a scalar: the same on every axis;
        else one width per axis in the order of ``shape``) with mirrored edges: scipy's
        ``gaussian_filter(mode="reflect", truncate=3.0)`` on the device, in place."""
        sg = np.atleast_1d(np.asarray(sigma, np.float64))
        if sg.ndim != 1 or sg.size not in (1, len(self.shape)):
            raise _lib.FwiError(_lib.EINVAL, "vec_smooth: sigma must be a scalar or %d widths, got shape %r"
                                % (len(self.shape), tuple(np.shape(sigma))))
        sg = np.ascontiguousarray(np.broadcast_to(sg, (len(self.shape),)))
        self._chk(self._lib.fwi_vec_smooth(self._c, int(slot), sg.ctypes.data_as(C.POINTER(C.c_double))))

    def vec_regularizer(self, x, out=None, kind="tv", x0=None, v=None, alpha=1.0, beta=0.0, weight=1.0, eps=None):
        """First-order Tikhonov (``kind="tikhonov"``) or smoothed isotropic total variation (``"tv"``, with ``eps`` > 0)
        of d = slot ``x`` - slot ``x0`` (``x0=None``: d = x): returns R(d) and, with a slot ``out``, sets
        ``out := alpha L(d; v) + beta out`` on the device (``v=None``: v = d, L(d; d) is the gradient of R; for fixed d, L
        is the symmetric positive semi-definite operator sum_a w_a D_a' diag(k(d)) D_a; ``include/fwi.h``).  ``weight``: a
        scalar for every axis, else one weight per axis in the order of ``shape``.  The host twin is
        :mod:`full_waveform_inversion_amd.regularizers`."""
        w = np.atleast_1d(np.asarray(weight, np.float64))
        if w.ndim != 1 or w.size not in (1, len(self.shape)):
            raise _lib.FwiError(_lib.EINVAL, "vec_regularizer: weight must be a scalar or %d weights, got shape %r"
                                % (len(self.shape), tuple(np.shape(weight))))
        w = np.ascontiguousarray(np.broadcast_to(w, (len(self.shape),)))
        k = _lib.REG_KINDS.get(kind, kind) if isinstance(kind, str) else kind
        if isinstance(k, str):
            raise _lib.FwiError(_lib.EINVAL, "vec_regularizer: unknown kind %r (one of %s)" % (kind, sorted(_lib.REG_KINDS)))
        if eps is None:
            if k == _lib.REG_KINDS["tv"]:
                raise _lib.FwiError(_lib.EINVAL, "vec_regularizer: total variation needs eps > 0")
            eps = 0.0
        slot = lambda s: -1 if s is None else int(s)  # noqa: E731
        val = C.c_double(0.0)
        self._chk(self._lib.fwi_vec_regularizer(self._c, int(k), int(x), slot(x0), slot(v), slot(out), float(alpha),
                                                float(beta), w.ctypes.data_as(C.POINTER(C.c_double)), float(eps),
                                                C.byref(val)))
        return val.value

    def vec_shift_sum(self, dst, srcs, shifts, weights=None, beta=0.0):
        """Slot ``dst := beta dst + sum_i weights[i] S_{shifts[i]} srcs[i]`` on the device (``fwi_vec_shift_sum``): every
        source slot shifted along depth (the first axis of ``shape``) by a real number of cells, linearly interpolated
        between the two nearest planes, planes outside the grid counting as zero.  At most ``_lib.SHIFT_SUM_MAX`` sources,
        none of them ``dst``; ``weights=None``: ones.  The fp64 twin is :func:`fourier.shift_sum`."""
        src = np.ascontiguousarray(np.atleast_1d(srcs), dtype=np.int32)
        s = np.ascontiguousarray(np.atleast_1d(shifts), dtype=np.float64)
        if src.ndim != 1 or s.shape != src.shape:
            raise _lib.FwiError(_lib.EINVAL, "vec_shift_sum: shifts must hold one shift per source slot, got %r and %r"
                                % (src.shape, s.shape))
        wp = None
        if weights is not None:
            w = np.ascontiguousarray(np.atleast_1d(weights), dtype=np.float64)
            if w.shape != src.shape:
                raise _lib.FwiError(_lib.EINVAL, "vec_shift_sum: weights must hold one weight per source slot, got %r"
                                    % (w.shape,))
            wp = w.ctypes.data_as(C.POINTER(C.c_double))
        self._chk(self._lib.fwi_vec_shift_sum(self._c, int(dst), int(src.size), src.ctypes.data_as(C.POINTER(C.c_int32)),
                                              s.ctypes.data_as(C.POINTER(C.c_double)), wp, float(beta)))

    def angle_gather_vec(self, angle_slots, lag_slots, offsets, tangents, taper=None, transpose=False):
        """The slant stack between an offset gather in ``lag_slots`` (half-offsets ``offsets``, whole cells) and an
        angle gather in ``angle_slots`` (``tangents = tan(gamma)``), on the device (:func:`fourier.angle_gather`):

            ``A_j = sum_l t_l S_{p_j h_l} E_l``, or with ``transpose``  ``E_l = t_l sum_j S_{-p_j h_l} A_j``

        with ``t = taper`` (None: ones).  One :meth:`vec_shift_sum` per slot written; more than ``_lib.SHIFT_SUM_MAX``
        sources are cut into chunks of that many, added up with ``beta = 1`` from the second chunk on.  The slots read
        are unchanged; no slot may be on both sides."""
        a = [int(s) for s in np.atleast_1d(angle_slots)]
        e = [int(s) for s in np.atleast_1d(lag_slots)]
        h = np.atleast_1d(np.asarray(offsets, np.float64))
        p = np.atleast_1d(np.asarray(tangents, np.float64))
        t = np.ones(h.size) if taper is None else np.atleast_1d(np.asarray(taper, np.float64))
        if h.shape != (len(e),) or p.shape != (len(a),) or t.shape != h.shape:
            raise _lib.FwiError(_lib.EINVAL, "angle_gather_vec: one offset (and taper weight) per lag slot and one "
                                "tangent per angle slot, got %d offsets, %d weights, %d lag slots; %d tangents, %d angle "
                                "slots" % (h.size, t.size, len(e), p.size, len(a)))
        if np.any(h != np.round(h)):
            raise _lib.FwiError(_lib.EINVAL, "angle_gather_vec: offsets must be whole cells")
        if transpose:
            calls = [(e[l], a, -(p * h[l]), np.full(p.size, t[l])) for l in range(h.size)]
        else:
            calls = [(a[j], e, p[j] * h, t) for j in range(p.size)]
        M = _lib.SHIFT_SUM_MAX
        for dst, srcs, shifts, w in calls:
            for k in range(0, len(srcs), M):
                self.vec_shift_sum(dst, srcs[k:k + M], shifts[k:k + M], w[k:k + M], 0.0 if k == 0 else 1.0)

    def gather_moment(self, slots, lags, power=2):
        """``(sum_l |lag_l|^power <E_l, E_l>, sum_l <E_l, E_l>)`` of the gather in ``slots`` from :meth:`vec_dot`, nothing
        downloaded.  The ratio at ``power=2`` is :func:`fourier.focusing`; half the first number at ``power=2`` is the
        differential-semblance functional of the gather."""
        slots = [int(s) for s in np.atleast_1d(slots)]
        lags = np.atleast_1d(np.asarray(lags, np.float64))
        if lags.shape != (len(slots),):
            raise _lib.FwiError(_lib.EINVAL, "gather_moment: one lag per slot, got %d lags and %d slots"
                                % (lags.size, len(slots)))
        e = np.array([self.vec_dot(s, s) for s in slots])
        return float(np.sum(np.abs(lags) ** power * e)), float(np.sum(e))

    # -- values at nodes, first-arrival traveltimes (fwi_eikonal*; the twin and definition is eikonal.py) -----------
    def _nodes(self, idx):
        idx = self._idx(idx)
        return idx, idx.ctypes.data_as(C.c_void_p)

    def vec_scatter_points(self, slot, idx, values, beta=0.0):
        """Slot ``:= beta slot``, then ``slot[idx_k] += values[k]`` for the unique nodes ``idx`` ``(n, ndim)``, on the
        device: NumPy's ``a = beta * a; a[idx] += values`` in the engine's dtype, bit for bit."""
        idx, pidx = self._nodes(idx)
        v = np.ascontiguousarray(np.atleast_1d(values), dtype=np.float64)
        if v.shape != (len(idx),):
            raise _lib.FwiError(_lib.EINVAL, "vec_scatter_points: one value per node, got %r for %d nodes"
                                % (v.shape, len(idx)))
        self._chk(self._lib.fwi_vec_scatter_points(self._c, int(slot), len(idx), pidx, v.ctypes.data_as(C.c_void_p),
                                                   float(beta)))

    def vec_gather_points(self, slot, idx):
        """``slot[idx_k]`` as float64, gathered on the device (nothing model-sized crosses)."""
        idx, pidx = self._nodes(idx)
        out = np.empty(len(idx), np.float64)
        self._chk(self._lib.fwi_vec_gather_points(self._c, int(slot), len(idx), pidx, out.ctypes.data_as(C.c_void_p)))
        return out

    last_eikonal_launches = 0  # launches of the latest eikonal / eikonal_adjoint call (also when it hit the cap)

    def _init_args(self, init):
        idx, dist, ref = init
        idx = self._idx(idx)
        dist = np.ascontiguousarray(np.atleast_1d(dist), dtype=np.float64)
        ref = np.ascontiguousarray(np.reshape(ref, -1), dtype=np.int32)
        if dist.shape != (len(idx),) or ref.shape != (self.ndim,):
            raise _lib.FwiError(_lib.EINVAL, "init list: one distance per node and one reference node, got %d nodes, "
                                "distances %r, reference %r" % (len(idx), dist.shape, ref.shape))
        return (idx, dist, ref), (len(idx), idx.ctypes.data_as(C.c_void_p), dist.ctypes.data_as(C.c_void_p),
                                  ref.ctypes.data_as(C.c_void_p))

    def eikonal(self, src, t_slot, scratch_slot, radius=0.0, max_sweeps=None, wall_slot=None):
        """First-arrival times of the engine's model into slot ``t_slot`` (``scratch_slot``: the other half of the
        ping-pong pair, its contents are lost).  ``src``: the source's grid coordinates, whole or fractional, turned
        into an init list by ``eikonal.ball(src, shape, h, radius)`` -- every node within ``radius`` cells starts at
        its straight-ray time in the velocity of the nearest node -- or such a list ``(idx, dist, ref)`` itself.
        Returns the init list, which :meth:`eikonal_gradient` takes.  ``max_sweeps=None``: ``4 * sum(shape)``;
        a cap that is reached raises ``FwiError`` (FWI_ESTATE) and leaves an upper bound in the slot.  ``wall_slot``:
        a slot whose cells ``!= 0`` the front may not enter (``+inf``; ``fwi_eikonal_stage``); None: ``fwi_eikonal``."""
        from . import eikonal as ek
        init, args = self._init_args(ek._source(src, self.shape, self.h, radius))
        n = C.c_int32(0)
        cap = 0 if max_sweeps is None else int(max_sweeps)
        try:
            if wall_slot is None:
                self._chk(self._lib.fwi_eikonal(self._c, int(t_slot), int(scratch_slot), *args, cap, C.byref(n)))
            else:
                self._chk(self._lib.fwi_eikonal_stage(self._c, int(t_slot), int(scratch_slot), int(wall_slot), *args,
                                                      cap, C.byref(n)))
        finally:
            self.last_eikonal_launches = int(n.value)
        return init

    def eikonal_restart(self, t_slot, scratch_slot, wall_slot=None, max_sweeps=None):
        """Slot ``t_slot`` := the first-arrival times started from what the slot holds (``fwi_eikonal_stage`` without a
        list; ``eikonal.solve_from`` is the definition): finite times ``>= 0`` on the secondary sources, ``+inf``
        elsewhere -- the second stage of a reflection, a plane wave, an exploding reflector, many sources at once.
        ``wall_slot``, ``max_sweeps`` and the cap as in :meth:`eikonal`."""
        n = C.c_int32(0)
        try:
            self._chk(self._lib.fwi_eikonal_stage(self._c, int(t_slot), int(scratch_slot),
                                                  -1 if wall_slot is None else int(wall_slot), 0, None, None, None,
                                                  0 if max_sweeps is None else int(max_sweeps), C.byref(n)))
        finally:
            self.last_eikonal_launches = int(n.value)

    def eikonal_handover(self, t_slot, in_slot, out_slot, beta=0.0):
        """Slot ``out_slot := beta out_slot +`` ``in_slot`` on the source-determined nodes of the times in ``t_slot``
        (finite and ``T_i < G_i``), 0 elsewhere (``fwi_eikonal_handover``): what a restarted solve hands to the stage
        before it (its adjoint variable) or takes from it (the tangent)."""
        self._chk(self._lib.fwi_eikonal_handover(self._c, int(t_slot), int(in_slot), int(out_slot), float(beta)))

    def eikonal_times(self, t_slot, rec):
        """The times of slot ``t_slot`` at receivers: node indices ``(n, ndim)``, or a ``points.Spread`` whose nodes
        are gathered on the device and combined with its multilinear weights here.  float64."""
        if hasattr(rec, "pt_start"):
            v = self.vec_gather_points(t_slot, rec.idx) * rec.weights
            return np.add.reduceat(v, rec.pt_start[:-1]) if len(v) else np.zeros(0)
        return self.vec_gather_points(t_slot, rec)

    def eikonal_adjoint(self, t_slot, rhs_slot, lam_slot, scratch_slot, max_sweeps=None):
        """Slot ``lam_slot`` := the solution of ``lambda = rhs + A^T lambda`` at the fixed point in ``t_slot``
        (``fwi_eikonal_adjoint``); four different slots."""
        n = C.c_int32(0)
        try:
            self._chk(self._lib.fwi_eikonal_adjoint(self._c, int(t_slot), int(rhs_slot), int(lam_slot), int(scratch_slot),
                                                    0 if max_sweeps is None else int(max_sweeps), C.byref(n)))
        finally:
            self.last_eikonal_launches = int(n.value)

    def eikonal_gradient(self, t_slot, lam_slot, out_slot, init=None, beta=0.0, wrt="velocity"):
        """Slot ``out_slot := beta out_slot +`` the gradient of ``sum_i rhs_i T_i`` with respect to the model, from the
        times, the adjoint variable and the init list :meth:`eikonal` returned.  ``init=None``: no source term
        (``fwi_eikonal_gradient_field``), the gradient of a restarted solve."""
        w = {"velocity": _lib.WRT_VELOCITY, "slowness2": _lib.WRT_SLOWNESS2}[wrt]
        if init is None:
            self._chk(self._lib.fwi_eikonal_gradient_field(self._c, w, int(t_slot), int(lam_slot), int(out_slot),
                                                           float(beta)))
            return
        _, args = self._init_args(init)
        self._chk(self._lib.fwi_eikonal_gradient(self._c, w, int(t_slot), int(lam_slot), int(out_slot), float(beta), *args))

    def eikonal_tangent(self, t_slot, dm_slot, out_slot, scratch_slot, init=None, wrt="velocity", max_sweeps=None,
                        b0_slot=None):
        """Slot ``out_slot`` := ``dT``, the derivative of the times in ``t_slot`` along the model perturbation in
        ``dm_slot`` (``fwi_eikonal_tangent``; ``eikonal.tangent`` is the definition): the exact transpose of
        :meth:`eikonal_adjoint` followed by :meth:`eikonal_gradient`.  ``init``: the list :meth:`eikonal` returned;
        four different slots, ``scratch_slot``'s contents are lost.  ``init=None``: no source term, and ``b0_slot``: a
        slot added to the right-hand side, ``x = b(dm) + b0 + A x`` (either: ``fwi_eikonal_tangent_stage``) -- the
        tangent of a restarted solve, ``b0`` the :meth:`eikonal_handover` of the stage before."""
        if wrt not in ("velocity", "slowness2"):
            raise ValueError("wrt must be 'velocity' or 'slowness2', got %r" % (wrt,))
        w = {"velocity": _lib.WRT_VELOCITY, "slowness2": _lib.WRT_SLOWNESS2}[wrt]
        args = (0, None, None, None) if init is None else self._init_args(init)[1]
        n = C.c_int32(0)
        cap = 0 if max_sweeps is None else int(max_sweeps)
        try:
            if init is not None and b0_slot is None:
                self._chk(self._lib.fwi_eikonal_tangent(self._c, w, int(t_slot), int(dm_slot), int(out_slot),
                                                        int(scratch_slot), *args, cap, C.byref(n)))
            else:
                self._chk(self._lib.fwi_eikonal_tangent_stage(self._c, w, int(t_slot), int(dm_slot),
                                                              -1 if b0_slot is None else int(b0_slot), int(out_slot),
                                                              int(scratch_slot), *args, cap, C.byref(n)))
        finally:
            self.last_eikonal_launches = int(n.value)

    def vec_clip(self, x, lo, hi):
        self._chk(self._lib.fwi_vec_clip(self._c, x, float(lo), float(hi)))

    def set_model_vec(self, slot):
        self._chk(self._lib.fwi_set_model_vec(self._c, slot))

    def gradient_vec(self, slot, wrt="velocity"):
        w = {"velocity": _lib.WRT_VELOCITY, "slowness2": _lib.WRT_SLOWNESS2}[wrt]
        self._chk(self._lib.fwi_gradient_vec(self._c, w, slot))

    def last_loop_ms(self):
        ms = C.c_double(0.0)
        self._chk(self._lib.fwi_last_loop_ms(self._c, C.byref(ms)))
        return ms.value

    def last_host_ms(self):
        """(submit_ms, graph_build_ms): host wall time spent forming and submitting the last time loop's launches, and
        the hipGraph capture + instantiation share of it (0 with ``launch_mode="stream"``)."""
        a, b = C.c_double(0.0), C.c_double(0.0)
        self._chk(self._lib.fwi_last_host_ms(self._c, C.byref(a), C.byref(b)))
        return a.value, b.value

    def placement_info(self):
        """(us_before, us_after, shifts) of the placement search a 3-D CPML or increment-form context runs at creation
        (include/fwi.h fwi_placement_info; shifts = bytes of the movable arrays in search order, then zeros); all zeros
        when the context ran none."""
        a, b = C.c_double(0.0), C.c_double(0.0)
        sh = (C.c_int64 * 8)()
        self._chk(self._lib.fwi_placement_info(self._c, C.byref(a), C.byref(b), sh))
        return a.value, b.value, tuple(int(v) for v in sh)

    def set_launch_mode(self, mode):
        """"auto" / "stream" / "graph" from the next sweep on (an A/B on one context: same buffers, same cache state)."""
        self._chk(self._lib.fwi_set_launch_mode(self._c, _lib.LAUNCH_MODES[mode]))

    def synchronize(self):
        self._chk(self._lib.fwi_synchronize(self._c))

    def dirty_padding(self):
        """Cells of the padded device fields outside the grid's interior that are not exactly zero (must be 0)."""
        n = C.c_int64(-1)
        self._chk(self._lib.fwi_check_padding(self._c, C.byref(n)))
        return int(n.value)
