"""Shot loop, shot-parallel sharding and the gradient exchange.

Shots are independent forward+adjoint problems on one model; only the gradient
(and the scalar misfit) is summed over them.  One process per GPU owns shots
``rank, rank + world, ...`` and the per-rank partial gradients are summed by a
single RCCL all-reduce on the device accumulators.  The
reference's only parallel pattern is the same shape -- independent Monte Carlo
samples per process, gather at the end (full_waveform_inversion.py:822-848).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np


@dataclass
class Shot:
    src_idx: np.ndarray          # (nsrc, ndim)
    wavelet: np.ndarray          # (nt,) or (nt, nsrc)
    rec_idx: np.ndarray          # (nrec, ndim)
    d_obs: np.ndarray | None = None  # (nt, nrec)
    # off-grid points (points.Spread): src_idx / rec_idx / wavelet then hold the expanded node lists and
    # the data are gathered back to the points; see Shot.at_coordinates
    src_spread: object = None
    rec_spread: object = None
    point_wavelet: np.ndarray | None = None  # (nt[, nsrc points]): the wavelets before spreading
    weights: np.ndarray | None = None  # (nt, nrec) data weights >= 0 of a datafit.WeightedL2 / MatchedL2 / EnvelopeL2 objective (None: 1)
    # (nrec,) weights >= 0 per trace of a datafit.NormalizedCorrelation objective (None: 1).  A plain attribute to assign,
    # not a field of the constructor: `weights` stays the last one
    trace_weights = None

    @classmethod
    def at_coordinates(cls, src_xyz, wavelet, rec_xyz, shape, d_obs=None):
        """A shot whose sources / receivers sit at fractional grid coordinates (multilinear interpolation)."""
        from .points import Spread
        S, R = Spread(src_xyz, shape), Spread(rec_xyz, shape)
        return cls(S.idx, S.scatter(wavelet), R.idx, d_obs, S, R, np.asarray(wavelet))

    def _on_device(self, engine):
        """off-grid points and an engine that spreads / gathers them on the device (fwi_forward_spread)"""
        return self.src_spread is not None and self.rec_spread is not None and hasattr(engine, "forward_at")

    def forward(self, engine, save):
        """Seismograms at this shot's receivers, ``(nt, nrec)``."""
        if self._on_device(engine):
            return engine.forward_at(None, (self.src_spread, self.point_wavelet), self.rec_spread, save=save)
        d = engine.forward(None, (self.src_idx, self.wavelet), self.rec_idx, save=save)
        return self.rec_spread.gather(d) if self.rec_spread is not None else d

    def adjoint(self, engine, residual):
        """Back-propagate a residual given at this shot's receivers (imaging into the engine's accumulator)."""
        if self._on_device(engine):
            engine.adjoint(None if residual is None else np.ascontiguousarray(residual))
            return
        r = self.rec_spread.scatter(residual) if self.rec_spread is not None else residual
        engine.adjoint(np.ascontiguousarray(r))

    def born(self, engine, dm, wrt="velocity", download=True, operator="exact"):
        """Born data ``J dm`` at this shot's receivers, ``(nt, nrec)``, after ``forward(engine, save=True)``.
        ``operator`` as in :meth:`Engine.born`; an engine that names no ``born_operators`` has the one Born operator
        its ``born(dm, wrt)`` computes, and gets no keyword."""
        kw = {} if download else {"download": False}
        if operator != "exact" and operator in getattr(engine, "born_operators", ()):
            kw["operator"] = operator
        d = engine.born(dm, wrt, **kw)
        if d is None or self._on_device(engine) or self.rec_spread is None:
            return d
        return self.rec_spread.gather(d)

    def fourier_born(self, engine, dm, freq_weights=None, wrt="velocity", download=True):
        """:meth:`born` on an engine that keeps the Fourier store: ``Engine.fourier_born(dm, freq_weights, wrt)``"""
        d = engine.fourier_born(dm, freq_weights, wrt, download=download)
        if d is None or self._on_device(engine) or self.rec_spread is None:
            return d
        return self.rec_spread.gather(d)

    def _residual_stays(self, engine):
        """``engine.born`` leaves exactly this shot's ``J dm`` on the device as the residual of ``adjoint(None)``"""
        return getattr(engine, "born_leaves_residual", False) and (self.rec_spread is None or self._on_device(engine))


def inversion_engine(shape, h, dt, nt_max, **kw):
    """The :class:`Engine` an INVERSION should run on: ``update_form="increment"`` unless the caller says otherwise.

    In fp32 the standard update form meets north_star's 1e-5 on seismograms and on the gradient of a GIVEN residual,
    but end to end -- the engine forming its own residual d_syn - d_obs -- the forward error is amplified by |d| / |r|
    (configs[1] at full size: 6.3e-5; profiles/r03_parity.json).  The increment form carries the same recursion as
    (u, v = u - u_prev) and meets a flat 1e-5 end to end on every BASELINE config family
    (tests/test_gpu_parity.py::test_end_to_end_fp32_increment_form_flat_1e5) at +4 B/update in 3-D (157 vs 110 ms per
    256^3 shot-gradient) and +2.5 % in 2-D.  Forward-only modelling and the headline bench keep the standard form
    (``Engine``'s default).  fp64 engines need neither; options the increment form does not combine with (the bf16
    store, an explicit 2-D "stream" kernel) fall back to the standard form.  Every other keyword goes to ``Engine`` as it
    is: ``fourier=freqs, fourier_batch=B`` make it keep the forward term as Fourier coefficients
    (``Engine.set_fourier_store``).
    """
    from .engine import Engine
    if "update_form" not in kw:
        fp32 = np.dtype(kw.get("dtype", "float32")) == np.dtype(np.float32)
        combinable = kw.get("store_dtype", "native") == "native" and not (len(shape) == 2 and kw.get("kernel") == "stream")
        # 2-D with the convolutional PML: the 4-steps-per-launch kernel that carries the border (step2d_fused_cpml) has
        # no increment form, and the standard form measures 6.5e-6 end to end there at full size (configs[1] + CPML)
        cpml2d = len(shape) == 2 and kw.get("abc", "sponge") == "cpml" and kw.get("npml", 0) > 0
        kw["update_form"] = "increment" if (fp32 and combinable and not cpml2d) else "standard"
    return Engine(shape, h, dt, nt_max, **kw)


def partition_shots(nshots, rank, world):
    """Round-robin: rank r of `world` owns shots r, r + world, ..."""
    if not (0 <= rank < world):
        raise ValueError("rank %d outside world of %d" % (rank, world))
    return list(range(rank, nshots, world))


class NoExchange:
    """Single process: nothing to sum."""
    rank, world = 0, 1

    def reduce(self, engine, misfit, wrt):
        return engine.gradient(wrt), misfit

    def reduce_device(self, engine, misfit):
        return misfit

    def reduce_illumination(self, engine, wrt="velocity", slot=None):
        """The illumination H (host array), or into the device vector ``slot`` (returns None)."""
        if slot is not None:
            return engine.illumination_vec(slot, wrt)
        return engine.illumination(wrt)

    def reduce_array(self, a):
        """The sum over the ranks of a host array that has no device accumulator (the spectral illumination)."""
        return a


class RcclExchange:
    """Production exchange: RCCL all-reduce (over xGMI) of the device-side accumulators.

    ``rdzv`` (:class:`rendezvous.Rendezvous`, or anything with ``rank`` / ``world`` / ``broadcast`` /
    ``allreduce``) is the control plane: it moves the 128-byte ncclUniqueId from rank 0 to everyone and
    agrees on whether every rank's communicator came up.  A communicator that fails on ANY rank is fatal
    on ALL of them (the ranks that succeeded abort theirs): there is no host-side fallback for the sum.
    """

    def __init__(self, engine, rdzv):
        self.rank, self.world = rdzv.rank, rdzv.world
        self.rdzv = rdzv
        uid = rdzv.broadcast(type(engine).comm_unique_id() if self.rank == 0 else None)
        err = ""
        try:
            engine.comm_init(self.rank, self.world, uid)
            seen = engine.comm_info()
            if seen != (self.world, self.rank):
                err = "RCCL reports rank %d of %d, expected %d of %d" % (seen[1], seen[0], self.rank, self.world)
        except Exception as ex:  # FwiError: reported to every rank below, then raised
            err = str(ex)
        ok = rdzv.allreduce([0.0 if err else 1.0], "min")[0] == 1.0
        if not ok:
            try:
                engine.comm_abort()
            except Exception:
                pass
            raise RuntimeError("RCCL communicator did not come up on every rank"
                               + (" (this rank: %s)" % err if err else " (failed on another rank)"))
        self.rccl_ranks = seen[0]

    def reduce(self, engine, misfit, wrt):
        engine.allreduce_gradient()
        return engine.gradient(wrt), engine.allreduce_f64([misfit])[0]

    def reduce_device(self, engine, misfit):
        """Sum the device-side accumulators only; the gradient stays on the GPU."""
        engine.allreduce_gradient()
        return engine.allreduce_f64([misfit])[0]

    def reduce_illumination(self, engine, wrt="velocity", slot=None):
        """Sum the device-side illumination accumulators over the ranks, then read H as NoExchange does."""
        engine.allreduce_illumination()
        return NoExchange.reduce_illumination(self, engine, wrt, slot)

    def reduce_array(self, a):
        """As :meth:`NoExchange.reduce_array`, over the control plane: the Fourier store has no illumination accumulator
        on the device for RCCL to sum, and this runs once per preconditioner."""
        return self.rdzv.allreduce_array(a).reshape(np.shape(a))


class HostExchange:
    """Sum on host arrays over the control plane (:class:`rendezvous.Rendezvous`): the path the CPU-only
    multi-process tests exercise with the oracle-backed engine; same sharding and reduction semantics as
    :class:`RcclExchange`.  Not a fallback of it -- nothing in the product path constructs this."""

    def __init__(self, rdzv):
        self.rdzv = rdzv
        self.rank, self.world = rdzv.rank, rdzv.world

    def reduce(self, engine, misfit, wrt):
        g = self.rdzv.allreduce_array(engine.gradient(wrt))
        return g, self.rdzv.allreduce([misfit])[0]

    def reduce_illumination(self, engine, wrt="velocity", slot=None):
        H = self.rdzv.allreduce_array(engine.illumination(wrt))
        if slot is None:
            return H
        engine.vec_upload(slot, H)

    def reduce_array(self, a):
        return self.rdzv.allreduce_array(a).reshape(np.shape(a))


class EnginePool:
    """Several engines (contexts + streams) on ONE GPU working through a rank's shots concurrently.

    A 2-D shot is latency-bound and cannot fill an MI355X; independent shots overlap when each has its own
    context and is driven by its own host thread (ctypes releases the GIL during the C-ABI calls).  Measured
    on configs[2] (32 shots of 1024^2 x 2000 steps, forward + adjoint + imaging): 0.44 s one after the other,
    0.35 s with two contexts, 0.35 - 0.38 s with three to six, 1.06 s with eight -- more streams than the
    runtime has hardware queues for serialise and pay for it; hence ``MAX_USEFUL``.  With the convolutional PML
    (``abc="cpml"``) a 1024^2 launch ends on its four corner tiles, and the overlap is what fills the idle CUs: 1.01 s
    one after the other, 0.65 s with two contexts, **0.55 s with three**, 1.24 s with four (round 3).  3-D shots are
    bandwidth-bound: use a pool of one.  Engines after the first only add into the first one's gradient
    accumulator (and illumination accumulator), which also owns the RCCL communicator.
    """

    MAX_USEFUL = 6

    def __init__(self, make_engine, size):
        size = max(1, int(size))
        if size > self.MAX_USEFUL:
            import warnings
            warnings.warn("EnginePool of %d contexts on one GPU: beyond %d the streams share hardware queues and the "
                          "shots slow down (configs[2]: 0.35 s with 2 - 6 contexts, 1.06 s with 8)"
                          % (size, self.MAX_USEFUL), RuntimeWarning, stacklevel=2)
        self.engines = [make_engine() for _ in range(size)]

    @property
    def primary(self):
        return self.engines[0]

    def close(self):
        for e in self.engines:
            e.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def map_shots(self, indices, fn):
        """Run ``fn(engine, shot_index)`` for every index, engines working in parallel; returns the
        results in index order."""
        import threading
        indices = list(indices)
        out = [None] * len(indices)
        err = []

        def work(k):
            e = self.engines[k]
            try:
                for pos in range(k, len(indices), len(self.engines)):
                    out[pos] = fn(e, indices[pos])
            except BaseException as ex:  # re-raised in the caller's thread
                err.append(ex)

        threads = [threading.Thread(target=work, args=(k,)) for k in range(len(self.engines))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        if err:
            raise err[0]
        return out


def _engines(engine):
    return engine.engines if isinstance(engine, EnginePool) else [engine]


def model_data(engine, model, shots, exchange=None):
    """Synthesise observed data for the shots this rank owns (in place, returns the shots)."""
    ex = exchange or NoExchange()
    for e in _engines(engine):
        e.set_model(model)

    def one(e, i):
        s = shots[i]
        s.d_obs = s.forward(e, save=False)

    mine = partition_shots(len(shots), ex.rank, ex.world)
    if isinstance(engine, EnginePool):
        engine.map_shots(mine, one)
    else:
        for i in mine:
            one(engine, i)
    return shots


def residual_scales(engine, model, shots, objective, per_trace=True, exchange=None):
    """The scale ``sigma`` of every shot's residuals at ``model`` (None: the model the engines hold) for a
    ``datafit.RobustMisfit(scale=...)``: ``1.4826 *`` the lower median of ``|e|``, ``e = M_s . B (d_syn - d_obs)`` with
    the shot's ``weights`` and the objective's ``taps``, per trace (an ``(ntr,)`` array per shot) or with
    ``per_trace=False`` of the whole gather (a float per shot).  One forward per shot, nothing is imaged; where the
    engine has ``residual_median`` and the shot's data stay on the device the median is an exact order statistic found
    there, else ``datafit.mad_scale`` of the downloaded synthetics.  Returns the list indexed like ``shots``, complete on
    every rank.  The scales are NUMBERS of this model: held fixed while the model moves (a ``--bands`` stage, a line
    search) they add no term to the gradient."""
    from .datafit import MAD_TO_SIGMA, RobustMisfit, mad_scale
    ex = exchange or NoExchange()
    if model is not None:
        for e in _engines(engine):
            e.set_model(model)
    twin = objective if isinstance(objective, RobustMisfit) else RobustMisfit(taps=getattr(objective, "taps", None))

    def one(e, i):
        s = shots[i]
        if s.d_obs is None:
            raise ValueError("shot %d has no observed data on rank %d" % (i, ex.rank))
        d = s.forward(e, save=False)
        if hasattr(e, "residual_median") and (s.rec_spread is None or s._on_device(e)):
            return MAD_TO_SIGMA * np.asarray(e.residual_median(s.d_obs, s.weights, twin.taps, per_trace)[0], np.float64)
        return np.asarray(mad_scale(twin.residuals(d, s.d_obs, s.weights)[0], s.weights, per_trace), np.float64)

    mine = partition_shots(len(shots), ex.rank, ex.world)
    got = engine.map_shots(mine, one) if isinstance(engine, EnginePool) else [one(engine, i) for i in mine]
    # every rank's shots side by side in one array, zeros for the others' shots: the sum over the ranks completes it
    sizes = [np.shape(s.d_obs)[1] if per_trace else 1 for s in shots]
    ends = np.cumsum([0] + sizes)
    flat = np.zeros(ends[-1])
    for i, v in zip(mine, got):
        flat[ends[i]:ends[i + 1]] = v
    flat = ex.reduce_array(flat)
    return [flat[ends[i]:ends[i + 1]].copy() if per_trace else float(flat[ends[i]]) for i in range(len(shots))]


class _Illuminated:
    """Turns illumination on in every engine for one evaluation, and back off afterwards if it was off."""

    def __init__(self, engine, on):
        self.engs = _engines(engine) if on else []
        self.was = [e.illumination_enabled for e in self.engs]

    def __enter__(self):
        for e in self.engs:
            e.set_illumination(True)
        return self

    def __exit__(self, *exc):
        for e, was in zip(self.engs, self.was):
            if not was:
                e.set_illumination(False)


class _Spectral:
    """Spectral imaging of one evaluation (``spectral_imaging=True``): every shot's adjoint is
    ``Engine.adjoint_spectral(residual, freq_weights)``, and with ``illum`` the shots' ``Engine.fourier_illumination`` are
    summed on the host, per engine (a pool drives each engine from one thread) and then over engines and ranks."""

    def __init__(self, engine, freq_weights, wrt, illum):
        for e in _engines(engine):
            if getattr(e, "fourier_freqs", None) is None or not hasattr(e, "adjoint_spectral"):
                raise ValueError("spectral_imaging needs engines that keep the Fourier store (Engine(fourier=freqs))")
        self.freq_weights, self.wrt, self.illum = freq_weights, wrt, bool(illum)
        self.H = {}

    @staticmethod
    def _residual(e, shot, residual):
        """the host residual as ``adjoint_spectral`` takes it (None: the one the misfit left on the device)"""
        if residual is not None and shot.rec_spread is not None and not shot._on_device(e):
            residual = shot.rec_spread.scatter(residual)
        return None if residual is None else np.ascontiguousarray(residual)

    def adjoint(self, e, shot, residual):
        e.adjoint_spectral(self._residual(e, shot, residual), self.freq_weights)
        if self.illum:
            h = np.asarray(e.fourier_illumination(self.freq_weights, self.wrt), np.float64)
            self.H[id(e)] = self.H[id(e)] + h if id(e) in self.H else h

    def illumination(self, engine, ex):
        """H of this evaluation summed over shots, engines and ranks (zeros on a rank that owned no shot)"""
        engs = _engines(engine)
        H = sum((self.H[id(e)] for e in engs if id(e) in self.H), np.zeros(engs[0].shape))
        return ex.reduce_array(H)


def misfit_and_gradient(engine, model, shots, exchange=None, wrt="velocity", objective=None, device_l2=True,
                        illumination=False, spectral_imaging=False, freq_weights=None):
    """J = sum_shots objective(F_s(model), d_obs,s) and dJ/dmodel, summed over all ranks.

    ``objective(d_syn, d_obs) -> (J, dJ/dd_syn)``; default least squares 1/2 ||d_syn - d_obs||^2
    (see objectives.py for the reference's similarity measures as misfits).

    An objective of :mod:`datafit` -- ``WeightedL2``, ``MatchedL2``, ``EnvelopeL2``, ``NormalizedCorrelation``,
    ``TraveltimeL2``, ``TransportW2``, ``AdaptiveMatching``, ``RobustMisfit``, ``SpectralMisfit`` or a subclass of one --
    names its own two calls.
    ``objective.host(d_syn, shot, i)`` is the NumPy twin with what its class takes from the shot: ``Shot.weights``, for
    the sums over traces and the spectral misfit ``Shot.trace_weights`` as well, for the matching filter ``shot=i``.
    Under ``device_l2``, an engine that has the
    method ``objective.engine_method`` (``misfit_weighted`` ... ``misfit_spectral``) is called through
    ``objective.device(engine, shot, i)`` instead: misfit and adjoint source are formed on the device, per node, or per
    off-grid point where the engine spreads them.

    Either branch uses the same per-shot numbers, which depend on the data only: ``objective.mu_of(i)`` (one damping for
    every shot, or a sequence indexed like ``shots``), ``objective.eps_of(d_obs)``, ``objective.param_of(d_obs)``; either
    leaves shot ``i``'s matching filter in ``objective.filters[i]``.  ``objective.dt`` of a traveltime, transport or
    adaptive objective must be the engine's time step.

    ``device_l2`` (least squares only): form the residual and J on the device (``fwi_misfit_l2``) -- in the
    engine's dtype, i.e. with an fp32 engine ``d_obs`` is rounded to fp32 before the subtraction, which puts
    ~6e-8 |d| / |r| of relative noise on J and on the residual (visible to a line search only once |r| / |d|
    approaches 1e-6).  ``device_l2=False`` keeps the residual in fp64 on the host, ``d_obs`` exact.

    ``illumination=True``: returns ``(J, g, H)`` with H the source-side illumination of the same sweeps, in the same
    parametrisation as g, summed over all ranks (``Engine.illumination``): no extra propagation.

    ``spectral_imaging=True`` (engines that keep the Fourier store): every shot's adjoint is
    ``Engine.adjoint_spectral(residual, freq_weights)``, the gradient formed per frequency with the weights
    ``freq_weights`` (None: 1).  ``illumination=True`` is then allowed on such engines and sums
    ``Engine.fourier_illumination(freq_weights, wrt)`` over shots, engines and ranks (on the host: the Fourier store has
    no accumulator of it on the device).  Without ``spectral_imaging`` nothing changes, and a Fourier engine refuses
    ``illumination=True``.
    """
    from .objectives import l2
    objective = objective or l2
    ex = exchange or NoExchange()
    spectral = _Spectral(engine, freq_weights, wrt, illumination) if spectral_imaging else None
    with _Illuminated(engine, illumination and spectral is None):
        for e in _engines(engine):
            e.set_model(model)
            e.reset_gradient()
        misfit = _sweep_shots(engine, shots, ex, objective, device_l2, spectral)
        out = ex.reduce(_engines(engine)[0], misfit, wrt)[::-1]
        if illumination and spectral is not None:
            out = out + (spectral.illumination(engine, ex),)
        elif illumination:
            out = out + (ex.reduce_illumination(_engines(engine)[0], wrt),)
    return out


def _sweep_shots(engine, shots, ex, objective, device_l2=True, spectral=None):
    """forward + adjoint of this rank's shots; returns the misfit, gradients summed into the
    (primary) engine's accumulator.  ``spectral`` (:class:`_Spectral`): the adjoint is its spectral one."""
    from .objectives import l2
    # a datafit objective names its device call and its host call itself (datafit.WeightedL2.device, .host); plain least
    # squares is a function with a device path, any other callable has none
    own = hasattr(objective, "engine_method")
    method = objective.engine_method if own else "misfit_l2" if objective is l2 else None

    def one(e, i):
        s = shots[i]
        if s.d_obs is None:
            raise ValueError("shot %d has no observed data on rank %d" % (i, ex.rank))
        d = s.forward(e, save=True)
        if device_l2 and method and hasattr(e, method) and (s.rec_spread is None or s._on_device(e)):
            # misfit and adjoint source are formed on the device (per node, or per off-grid point)
            j = objective.device(e, s, i) if own else e.misfit_l2(s.d_obs)
            if spectral is not None:
                spectral.adjoint(e, s, None)
            else:
                e.adjoint(None)
            return j
        j, r = objective.host(d, s, i) if own else objective(d, s.d_obs)
        if spectral is not None:
            spectral.adjoint(e, s, r)
        else:
            s.adjoint(e, r)
        return j

    mine = partition_shots(len(shots), ex.rank, ex.world)
    if isinstance(engine, EnginePool):
        misfit = float(sum(engine.map_shots(mine, one)))
        for other in engine.engines[1:]:
            engine.primary.gradient_add_from(other)
        return misfit
    return float(sum(one(engine, i) for i in mine))


class _Extended(_Spectral):
    """The adjoint of :func:`extended_image`: ``Engine.adjoint_spectral(residual, image=False)``, then the shot's gather
    added to its engine's fp64 sum on the host (a pool drives each engine from one thread)."""

    def __init__(self, engine, freq_weights, kind, lags, axis):
        super().__init__(engine, freq_weights, "slowness2", False)
        if kind not in ("offset", "time"):
            raise ValueError("kind must be 'offset' or 'time'")
        if kind == "offset" and axis is None:
            raise ValueError("an offset gather needs its axis")
        self.kind, self.lags, self.axis = kind, np.atleast_1d(lags), axis
        self.E = {}

    def adjoint(self, e, shot, residual):
        e.adjoint_spectral(self._residual(e, shot, residual), image=False)
        if self.kind == "offset":
            E = e.fourier_offset_images(self.axis, self.lags, self.freq_weights)
        else:
            E = e.fourier_lag_images(self.lags, self.freq_weights)
        E = np.asarray(E, np.float64)
        self.E[id(e)] = self.E[id(e)] + E if id(e) in self.E else E

    def gather(self, engine, ex):
        """E of this evaluation summed over shots, engines and ranks (zeros on a rank that owned no shot)"""
        engs = _engines(engine)
        E = sum((self.E[id(e)] for e in engs if id(e) in self.E), np.zeros((self.lags.size,) + tuple(engs[0].shape)))
        return ex.reduce_array(E)


def extended_image(engine, model, shots, kind, lags, axis=None, exchange=None, objective=None, freq_weights=None):
    """``(J, E)``: the misfit of :func:`misfit_and_gradient` and the extended image of the shots at ``model``, summed over
    shots, pool engines and ranks, ``(len(lags), *shape)`` in fp64 and in the units of
    ``Engine.fourier_gradient(wrt="slowness2")``.  ``kind="offset"``: ``lags`` are integer subsurface offsets in cells along
    ``axis`` (``Engine.fourier_offset_images``); ``kind="time"``: ``lags`` are time lags in seconds
    (``Engine.fourier_lag_images``).  Every shot takes the per-shot path of ``spectral_imaging=True``: forward, residual
    by ``objective``, then ``Engine.adjoint_spectral(image=False)`` and one streaming pass per lag; the gathers are summed
    on the host as the Fourier illumination is.  The gradient accumulators are reset and stay zero.  Energy that focuses at
    zero lag says that ``model`` is kinematically right (``fourier.focusing``).  Engines without the Fourier store raise
    ``ValueError``."""
    from .objectives import l2
    ex = exchange or NoExchange()
    ext = _Extended(engine, freq_weights, kind, lags, axis)
    for e in _engines(engine):
        e.set_model(model)
        e.reset_gradient()
    misfit = _sweep_shots(engine, shots, ex, objective or l2, True, ext)
    J = float(np.asarray(ex.reduce_array(np.array([misfit]))).ravel()[0])
    return J, ext.gather(engine, ex)


class _AngleGather(_Spectral):
    """The adjoint of :func:`angle_gather`: ``Engine.adjoint_spectral(residual, image=False)``, then every lag of the
    shot's offset gather formed in a scratch slot and added to that lag's slot on the device (an engine's first shot
    writes the lag slots themselves); nothing is downloaded per shot.  A pool drives each engine from one thread."""

    def __init__(self, engine, freq_weights, axis, offsets, tangents, slot0, taper):
        super().__init__(engine, freq_weights, "slowness2", False)
        self.axis = axis
        self.offsets = [int(h) for h in np.atleast_1d(offsets)]
        self.tangents = np.atleast_1d(np.asarray(tangents, np.float64))
        self.taper = taper
        L, n = len(self.offsets), self.tangents.size
        self.lag_slots = list(range(int(slot0), int(slot0) + L))
        self.angle_slots = list(range(int(slot0) + L, int(slot0) + L + n))
        self.scratch = int(slot0) + L + n
        self.seen = set()

    def adjoint(self, e, shot, residual):
        e.adjoint_spectral(self._residual(e, shot, residual), image=False)
        first = id(e) not in self.seen
        for slot, h in zip(self.lag_slots, self.offsets):
            e.fourier_offset_image_vec(slot if first else self.scratch, self.axis, h, self.freq_weights)
            if not first:
                e.vec_axpby(slot, 1.0, self.scratch, 1.0)
        self.seen.add(id(e))

    def _download(self, engine, ex, slots):
        engs = _engines(engine)
        out = np.zeros((len(slots),) + tuple(engs[0].shape))
        for e in engs:
            if id(e) in self.seen:
                out += np.stack([np.asarray(e.vec_download(s), np.float64) for s in slots])
        return ex.reduce_array(out)

    def gathers(self, engine, ex, return_offsets):
        """(A, E or None) of this evaluation summed over shots, engines and ranks (zeros on a rank that owned no shot)"""
        for e in _engines(engine):
            if id(e) in self.seen:
                e.angle_gather_vec(self.angle_slots, self.lag_slots, self.offsets, self.tangents, self.taper)
        A = self._download(engine, ex, self.angle_slots)
        return A, self._download(engine, ex, self.lag_slots) if return_offsets else None


def angle_gather(engine, model, shots, axis, offsets, tangents, slot0=0, exchange=None, objective=None,
                 freq_weights=None, taper=None, return_offsets=False):
    """``(J, A)``: the misfit of :func:`misfit_and_gradient` and the angle-domain common-image gather of the shots at
    ``model``, ``(len(tangents), *shape)`` in fp64, summed over shots, pool engines and ranks:

        ``A_j = sum_l t_l S_{p_j h_l} E_l``  (``fourier.angle_gather``)

    the slant stack over depth and half-offset of the subsurface-offset gather ``E`` of :func:`extended_image` with
    ``kind="offset"`` along ``axis``; ``offsets``: integer half-offsets ``h_l`` in cells, ``tangents``: ``p_j = tan
    gamma_j`` (``fourier.tangents``), ``taper``: ``t_l`` (None: ones).  Every shot takes the per-shot path of
    :func:`extended_image`, but its gather stays on the device: each lag is formed by
    ``Engine.fourier_offset_image_vec`` and added to that lag's vector slot, and after the engine's last shot
    ``Engine.angle_gather_vec`` runs the transform there.  Only the angle images are downloaded (with
    ``return_offsets=True`` the summed offset gather too: ``(J, A, E)``).  The sum over shots is therefore formed on the
    device in the context's dtype; :func:`extended_image` keeps its fp64 sum on the host.  Uses the
    ``len(offsets) + len(tangents) + 1`` vector slots from ``slot0`` on (lags, angles, one scratch) of every engine,
    which the caller has created (``Engine.vec_create`` frees every slot, so it is not called here; a missing slot is
    the engine's own error).  The transform is kinematic: an event that is flat across the angles says that ``model`` is
    right.  The gradient accumulators are reset and stay zero.  Engines without the Fourier store raise
    ``ValueError``."""
    from .objectives import l2
    ex = exchange or NoExchange()
    ang = _AngleGather(engine, freq_weights, axis, offsets, tangents, slot0, taper)
    for e in _engines(engine):
        e.set_model(model)
        e.reset_gradient()
    misfit = _sweep_shots(engine, shots, ex, objective or l2, True, ang)
    J = float(np.asarray(ex.reduce_array(np.array([misfit]))).ravel()[0])
    A, E = ang.gathers(engine, ex, return_offsets)
    return (J, A, E) if return_offsets else (J, A)


class _Split(_Spectral):
    """The adjoint of :func:`split_gradient`: ``Engine.adjoint_spectral(residual, image=False)``, then the shot's two parts
    added to its engine's fp64 sums on the host (a pool drives each engine from one thread)."""

    def __init__(self, engine, freq_weights, wrt, axis, taps):
        super().__init__(engine, freq_weights, wrt, False)
        self.axis, self.taps = axis, np.ascontiguousarray(np.asarray(taps, np.float64))
        self.G = {}

    def adjoint(self, e, shot, residual):
        e.adjoint_spectral(self._residual(e, shot, residual), image=False)
        G = np.stack(e.fourier_gradient_split(self.axis, self.taps, self.freq_weights, self.wrt)).astype(np.float64)
        self.G[id(e)] = self.G[id(e)] + G if id(e) in self.G else G

    def parts(self, engine, ex):
        """Both parts of this evaluation summed over shots, engines and ranks (zeros on a rank that owned no shot)"""
        engs = _engines(engine)
        G = sum((self.G[id(e)] for e in engs if id(e) in self.G), np.zeros((2,) + tuple(engs[0].shape)))
        return ex.reduce_array(G)


def split_gradient(engine, model, shots, axis, taps, exchange=None, objective=None, freq_weights=None, wrt="velocity"):
    """``(J, g_same, g_opposite)``: the misfit of :func:`misfit_and_gradient` and the two parts of the split of its
    spectral gradient along ``axis`` (``Engine.fourier_gradient_split`` with the one-sided ``taps``, e.g.
    ``datafit.hilbert_taps(fourier.split_halfwidth(kappa))``), summed over shots, pool engines and ranks the way
    :func:`extended_image` sums its gathers, model-shaped in fp64.  ``g_same`` pairs forward and adjoint coefficients
    that travel the same way along the axis (low wavenumber: the transmission paths, the tomographic part),
    ``g_opposite`` those that travel in opposite directions (high wavenumber: the reflectors, the migration part).
    NEITHER PART IS THE GRADIENT OF THE MISFIT: they are the two halves of it, ``g_same + g_opposite`` is the gradient of
    ``misfit_and_gradient(spectral_imaging=True, freq_weights=freq_weights, wrt=wrt)`` to round-off, and no line search
    may treat one of them as a gradient of ``J``.  Every shot takes the per-shot path of ``spectral_imaging=True``:
    forward, residual by ``objective``, ``Engine.adjoint_spectral(image=False)`` and two streaming passes.  The gradient
    accumulators are reset and stay zero.  Engines without the Fourier store raise ``ValueError``."""
    from .objectives import l2
    ex = exchange or NoExchange()
    split = _Split(engine, freq_weights, wrt, axis, taps)
    for e in _engines(engine):
        e.set_model(model)
        e.reset_gradient()
    misfit = _sweep_shots(engine, shots, ex, objective or l2, True, split)
    J = float(np.asarray(ex.reduce_array(np.array([misfit]))).ravel()[0])
    G = split.parts(engine, ex)
    return J, G[0], G[1]


def _extended_born_one(e, s, kind, lags, images, axis, freq_weights, download):
    """``J_ext,s E`` of one shot after its ``forward(save=True)``, per point where the shot has off-grid receivers"""
    d = e.fourier_born_extended(kind, lags, images, axis, freq_weights, download=download)
    return d if d is None or s._on_device(e) or s.rec_spread is None else s.rec_spread.gather(d)


def extended_born(engine, model, shots, kind, lags, images, axis=None, exchange=None, freq_weights=None):
    """Extended Born modelling (demigration) of the gather ``images``, ``(len(lags), *shape)`` in the units of
    :func:`extended_image`: the per-shot data ``J_ext,s E`` as a list indexed like ``shots`` (None for the shots of other
    ranks), each ``(nt, nrec)``.  ``kind``, ``lags``, ``axis`` as in :func:`extended_image`; per shot ``forward(save=True)``
    and ``Engine.fourier_born_extended``.  ``model=None`` keeps the model the engines hold.  Engines without the Fourier
    store raise ``ValueError``."""
    ex = exchange or NoExchange()
    _Extended(engine, freq_weights, kind, lags, axis)  # (the argument checks)
    for e in _engines(engine):
        if model is not None:
            e.set_model(model)
    out = [None] * len(shots)

    def one(e, i):
        shots[i].forward(e, save=True)
        out[i] = _extended_born_one(e, shots[i], kind, lags, images, axis, freq_weights, True)

    mine = partition_shots(len(shots), ex.rank, ex.world)
    if isinstance(engine, EnginePool):
        engine.map_shots(mine, one)
    else:
        for i in mine:
            one(engine, i)
    return out


def extended_hvp(engine, model, shots, kind, lags, images, axis=None, exchange=None, freq_weights=None):
    """``sum_s J_ext,s^T J_ext,s E`` as ``(len(lags), *shape)`` in fp64, summed over shots, pool engines and ranks as
    :func:`extended_image` sums its gather: the normal operator of extended least-squares migration, symmetric positive
    semi-definite, which ``newton.cg`` inverts for a gather.  Per shot ``forward(save=True)``,
    ``Engine.fourier_born_extended`` (the data stay on the device), ``Engine.adjoint_spectral(None, image=False)`` and one
    streaming pass per lag: three sweeps per shot and product.  ``freq_weights`` weigh both operators.  ``model=None``
    keeps the model the engines hold.  The gradient accumulators are not touched."""
    ex = exchange or NoExchange()
    ext = _Extended(engine, freq_weights, kind, lags, axis)
    for e in _engines(engine):
        if model is not None:
            e.set_model(model)

    def one(e, i):
        s = shots[i]
        s.forward(e, save=True)
        stays = s._residual_stays(e)
        d = _extended_born_one(e, s, kind, lags, images, axis, freq_weights, not stays)
        ext.adjoint(e, s, None if stays else d)

    mine = partition_shots(len(shots), ex.rank, ex.world)
    if isinstance(engine, EnginePool):
        engine.map_shots(mine, one)
    else:
        for i in mine:
            one(engine, i)
    return ext.gather(engine, ex)


def misfit_and_gradient_device(engine, model_slot, grad_slot, shots, exchange=None, wrt="velocity",
                               objective=None, device_l2=True, illum_slot=None, spectral_imaging=False,
                               freq_weights=None):
    """Like :func:`misfit_and_gradient`, with the model read from and the gradient written to
    device-resident vectors (``Engine.vec_*``): no model-sized array crosses PCIe.  ``illum_slot``: the vector
    that receives the illumination H of the same sweeps (see :func:`misfit_and_gradient`).  ``spectral_imaging`` and
    ``freq_weights`` as there; the spectral illumination is summed on the host and uploaded into ``illum_slot``."""
    from .objectives import l2
    objective = objective or l2
    ex = exchange or NoExchange()
    engs = _engines(engine)
    spectral = _Spectral(engine, freq_weights, wrt, illum_slot is not None) if spectral_imaging else None
    with _Illuminated(engine, illum_slot is not None and spectral is None):
        engs[0].set_model_vec(model_slot)
        if len(engs) > 1:  # the optimiser's vectors live in the primary engine: hand the model over
            model = engs[0].vec_download(model_slot)
            for e in engs[1:]:
                e.set_model(model)
        for e in engs:
            e.reset_gradient()
        misfit = _sweep_shots(engine, shots, ex, objective, device_l2, spectral)
        misfit = ex.reduce_device(engs[0], misfit)
        engs[0].gradient_vec(grad_slot, wrt)
        if illum_slot is not None and spectral is not None:
            engs[0].vec_upload(illum_slot, spectral.illumination(engine, ex))
        elif illum_slot is not None:
            ex.reduce_illumination(engs[0], wrt, illum_slot)
    return misfit


def _hvp_sweep(engine, shots, ex, born_one, objective=None, spectral=None):
    """forward(save) + Born + adjoint(imaging) of this rank's shots; ``born_one(e, s, download)`` applies J_s.  With a
    ``datafit.WeightedL2`` objective its weight ``W_s = B M_s^2 B`` acts on the Born data between the two: on the device
    where the residual stays there and the engine has ``residual_weight``, else through the host twin.  With a
    ``datafit.RobustMisfit`` the weight is the IRLS one at the current model, ``B (tw M^2 psi(e_s)) B``: the objective is
    evaluated on the forward's synthetics first (``device(..., keep_irls=True)``, which keeps the weight on the device
    for ``residual_weight_robust``; else the host twin and its ``normal``), so the shots need observed data.
    ``spectral`` (:class:`_Spectral`): the adjoint is its spectral one."""
    from .datafit import RobustMisfit, WeightedL2
    robust = isinstance(objective, RobustMisfit)
    if objective is not None and not robust and not isinstance(objective, WeightedL2):
        raise ValueError("objective must be a datafit.WeightedL2 (or None: plain least squares)")

    def one_robust(e, s, i):
        if s.d_obs is None:
            raise ValueError("shot %d has no observed data on rank %d" % (i, ex.rank))
        d = s.forward(e, save=True)
        if s._residual_stays(e) and hasattr(e, "residual_weight_robust"):
            objective.device(e, s, i, keep_irls=True)
            born_one(e, s, False)
            e.residual_weight_robust(objective.taps)
            r = None
        else:
            psi = objective.irls(d, s, i)
            r = objective.normal(born_one(e, s, True), s.weights, s.trace_weights, psi)
        if spectral is not None:
            spectral.adjoint(e, s, r)
        elif r is None:
            e.adjoint(None)
        else:
            s.adjoint(e, r)

    def one(e, i):
        s = shots[i]
        if robust:
            return one_robust(e, s, i)
        s.forward(e, save=True)
        if s._residual_stays(e) and (objective is None or hasattr(e, "residual_weight")):
            born_one(e, s, False)
            if objective is not None:
                e.residual_weight(s.weights, objective.taps)
            if spectral is not None:
                spectral.adjoint(e, s, None)
            else:
                e.adjoint(None)
        else:
            d = born_one(e, s, True)
            r = d if objective is None else objective.normal(d, s.weights)
            if spectral is not None:
                spectral.adjoint(e, s, r)
            else:
                s.adjoint(e, r)

    mine = partition_shots(len(shots), ex.rank, ex.world)
    if isinstance(engine, EnginePool):
        engine.map_shots(mine, one)
        for other in engine.engines[1:]:
            engine.primary.gradient_add_from(other)
    else:
        for i in mine:
            one(engine, i)


def _fourier_hvp(engine, freq_weights, spectral_imaging, wrt):
    """(the engines keep the Fourier store, the :class:`_Spectral` of the product or None).  On Fourier engines the Born
    operator is ``fourier_born`` with the weights of the adjoint that follows it: ``adjoint`` (unit weights) or, with
    ``spectral_imaging``, ``adjoint_spectral(freq_weights)``."""
    four = all(getattr(e, "fourier_freqs", None) is not None for e in _engines(engine))
    if not four:
        if freq_weights is not None or spectral_imaging:
            raise ValueError("freq_weights and spectral_imaging need engines that keep the Fourier store "
                             "(Engine(fourier=freqs))")
        return False, None
    if freq_weights is not None and not spectral_imaging:
        raise ValueError("freq_weights needs spectral_imaging=True: adjoint(image) transposes the Born operator of unit "
                         "weights only")
    return True, _Spectral(engine, freq_weights, wrt, False) if spectral_imaging else None


def gauss_newton_hvp(engine, model, shots, v, exchange=None, wrt="velocity", objective=None, freq_weights=None,
                     spectral_imaging=False):
    """Gauss-Newton Hessian-vector product ``H v = sum_s J_s^T J_s v`` at ``model`` (with ``objective`` a
    ``datafit.WeightedL2``: ``sum_s J_s^T W_s J_s v``, ``W_s = B M_s^2 B``), summed over all ranks: ``v`` and
    the result are model-shaped and in the parametrisation ``wrt``.  Per shot ``forward(save=True)``, ``born``,
    ``adjoint`` -- THREE sweeps per shot and product, because the forward-term store holds one shot at a time.
    J is the engine's imaging Born operator (``Engine.born(operator="imaging")``), the exact transpose of its
    ``adjoint`` + ``gradient``: H is symmetric positive semi-definite on every engine -- ``image_stride``, the bf16
    store and checkpointing included -- and is today's product, bit for bit, on a plain one.
    OVERWRITES the gradient accumulator of the engine(s) (``reset_gradient`` first, like :func:`misfit_and_gradient`).
    ``model=None`` keeps the model the engines already hold.  The shots need no observed data.
    With ``objective`` a ``datafit.RobustMisfit`` the weight is its IRLS (majoriser) one at ``model``,
    ``W_s = B (tw M_s^2 psi(e_s)) B`` with ``e_s`` the shot's residual there: positive semi-definite for every kind, and
    the shots then DO need their observed data.

    Engines that keep the Fourier store (``fourier_freqs`` is not None): J is ``Engine.fourier_born``, the transpose of
    ``adjoint`` on that store; with ``spectral_imaging=True`` the product is ``J_a^T J_a`` through
    ``fourier_born(v, freq_weights)`` and ``adjoint_spectral(freq_weights)``, ``a = freq_weights`` (None: 1).  On every
    other engine the two arguments must keep their defaults and nothing changes."""
    ex = exchange or NoExchange()
    engs = _engines(engine)
    four, spectral = _fourier_hvp(engine, freq_weights, spectral_imaging, wrt)
    for e in engs:
        if model is not None:
            e.set_model(model)
        e.reset_gradient()
    if four:
        born_one = lambda e, s, download: s.fourier_born(e, v, freq_weights, wrt, download=download)  # noqa: E731
    else:
        born_one = lambda e, s, download: s.born(e, v, wrt, download=download, operator="imaging")  # noqa: E731
    _hvp_sweep(engine, shots, ex, born_one, objective, spectral)
    return ex.reduce(engs[0], 0.0, wrt)[0]


def gauss_newton_hvp_device(engine, model_slot, v_slot, out_slot, shots, exchange=None, wrt="velocity", objective=None,
                            freq_weights=None, spectral_imaging=False):
    """:func:`gauss_newton_hvp` on device vectors (``Engine.vec_*``): the model is read from ``model_slot`` (None: the
    model the engines hold), v from ``v_slot`` and ``H v`` is written to ``out_slot``; the Born data stay on the device
    as the adjoint's residual, so no model- or data-sized array crosses PCIe (the further engines of a pool receive the
    model and v from the primary one through the host).  OVERWRITES the gradient accumulator; three sweeps per shot.
    ``objective`` as in :func:`gauss_newton_hvp`: its weight is applied by ``Engine.residual_weight`` on the device.
    ``freq_weights``, ``spectral_imaging``: as there, on engines that keep the Fourier store (``fourier_born_vec``)."""
    ex = exchange or NoExchange()
    engs = _engines(engine)
    four, spectral = _fourier_hvp(engine, freq_weights, spectral_imaging, wrt)
    if model_slot is not None:
        engs[0].set_model_vec(model_slot)
    if len(engs) > 1:  # the vectors live in the primary engine: hand model and v over
        v = engs[0].vec_download(v_slot)
        if model_slot is not None:
            model = engs[0].vec_download(model_slot)
            for e in engs[1:]:
                e.set_model(model)
    for e in engs:
        e.reset_gradient()

    def born_one(e, s, download):
        if e is not engs[0]:
            if four:
                return s.fourier_born(e, v, freq_weights, wrt, download=download)
            return s.born(e, v, wrt, download=download, operator="imaging")
        if four:
            d = e.fourier_born_vec(v_slot, freq_weights, wrt, download=download)
        else:
            d = e.born_vec(v_slot, wrt, download=download, operator="imaging")
        return d if d is None or s._on_device(e) or s.rec_spread is None else s.rec_spread.gather(d)

    _hvp_sweep(engine, shots, ex, born_one, objective, spectral)
    ex.reduce_device(engs[0], 0.0)
    engs[0].gradient_vec(out_slot, wrt)


# Relative floor of the illumination preconditioner p = 1 / (H / max(H) + eps).  max(H) sits on the source cells, so
# eps is a fraction of the illumination right at a source: cells lit by less than eps of that get a gain of about
# 1 / eps, the best-lit ones a gain of about 1.  Chosen by measurement ("Illumination preconditioning").
ILLUMINATION_EPS = 1e-3


def illumination_preconditioner(H, eps=ILLUMINATION_EPS):
    """p = 1 / (H / max(H) + eps), elementwise (host arrays)."""
    H = np.asarray(H, np.float64)
    m = float(np.abs(H).max())
    if not m > 0.0 or not np.isfinite(m):
        raise ValueError("illumination is zero or not finite: nothing to precondition with")
    return 1.0 / (H / m + float(eps))


def illumination_preconditioner_vec(engine, slot, eps=ILLUMINATION_EPS):
    """Vector ``slot`` holding H := 1 / (H / max(H) + eps), on the device."""
    m = engine.vec_absmax(slot)
    if not m > 0.0 or not np.isfinite(m):
        raise ValueError("illumination is zero or not finite: nothing to precondition with")
    engine.vec_recip(slot, m, float(eps) * m)


def preconditioned_fg_device(engine, shots, precond_slot, eps=ILLUMINATION_EPS, exchange=None, wrt="velocity",
                             **kw):
    """``fg(x_slot, g_slot) -> f`` for :func:`lbfgs.lbfgs_device` with ``precond_slot``: the first evaluation that
    finds the slot empty (all zeros, as ``lbfgs_device`` creates it) also accumulates the illumination and turns it
    into the preconditioner there; every other evaluation is a plain one.  A resumed run finds the slot filled from
    its state and never rebuilds it."""
    built = [False]

    def fg(x_slot, g_slot):
        if not built[0] and engine_of(engine).vec_absmax(precond_slot) == 0.0:
            f = misfit_and_gradient_device(engine, x_slot, g_slot, shots, exchange, wrt, illum_slot=precond_slot, **kw)
            illumination_preconditioner_vec(engine_of(engine), precond_slot, eps)
            built[0] = True
            return f
        built[0] = True
        return misfit_and_gradient_device(engine, x_slot, g_slot, shots, exchange, wrt, **kw)

    return fg


def engine_of(engine):
    """The engine that holds the optimiser's vectors (the primary one of a pool)."""
    return _engines(engine)[0]


# -- Gaussian model-space smoothing as the initial inverse Hessian of the L-BFGS -----------------------

def _axis_widths(sigma, ndim):
    s = np.atleast_1d(np.asarray(sigma, np.float64))
    if s.ndim != 1 or s.size not in (1, ndim) or not np.all(np.isfinite(s)) or np.any(s < 0.0):
        raise ValueError("sigma must be a finite width >= 0, or one per axis (%d), got %r" % (ndim, sigma))
    return tuple(float(v) for v in np.broadcast_to(s, (ndim,)))


def gaussian_smooth(x, sigma):
    """The operator of ``Engine.vec_smooth`` in NumPy: per axis ``R = int(3 sigma + 0.5)``, normalised weights
    ``exp(-k^2 / 2 sigma^2)``, half-sample mirror at both ends (one reflection: ``R <= n``).  Equals
    ``scipy.ndimage.gaussian_filter(x, sigma, mode="reflect", truncate=3.0)``; used when scipy is not installed."""
    x = np.asarray(x)
    out = x
    for ax, sg in reversed(list(enumerate(_axis_widths(sigma, x.ndim)))):  # x first, z last
        R = int(3.0 * sg + 0.5)
        if R == 0:
            continue
        n = x.shape[ax]
        if R > n:
            raise ValueError("sigma=%g gives radius %d on an axis of %d cells (one reflection only)" % (sg, R, n))
        k = np.arange(-R, R + 1)
        w = np.exp(-0.5 * (k / sg) ** 2)
        w /= w.sum()
        a = np.moveaxis(out, ax, 0)
        pad = np.concatenate([a[:R][::-1], a, a[n - R:][::-1]], 0)
        acc = np.zeros(a.shape, np.result_type(x.dtype, np.float64))
        for j in range(2 * R + 1):
            acc += w[j] * pad[j:j + n]
        out = np.moveaxis(acc.astype(x.dtype, copy=False), 0, ax)
    return out


def _default_smooth():
    try:
        from scipy.ndimage import gaussian_filter
    except ImportError:
        return gaussian_smooth
    return lambda x, sigma: gaussian_filter(x, sigma, mode="reflect", truncate=3.0)


def _h0_tag(sigma, mask, with_precond):
    import zlib
    crc = None if mask is None else zlib.crc32(np.ascontiguousarray(mask, np.float64).tobytes())
    return "gauss(sigma=%r,mask=%r,precond=%d)" % (list(sigma), crc, int(bool(with_precond)))


def _checked_mask(mask):
    m = np.asarray(mask, np.float64)
    if not (np.all(m >= 0.0) and np.all(m <= 1.0)):
        raise ValueError("mask must lie in [0, 1]")
    return m


def smoothing_h0(sigma, mask=None, precond=None, smooth=None):
    """``h0`` for :func:`lbfgs.lbfgs`: ``B = M S' D S' M`` with ``S'`` the Gaussian of width ``sigma / sqrt(2)`` (so
    that with D = M = I the composite has width ``sigma``), ``D = diag(precond)`` (an array, or a callable returning
    it when B is first applied; None: I) and ``M = diag(mask)`` (model-shaped, in [0, 1]; None: I).  B = A A^T with
    A = M S' D^(1/2): symmetric positive semi-definite whatever the spectrum of S', so ``-B g`` descends; cells with
    ``mask == 0`` never move.  ``smooth(x, sigma_per_axis)``: the filter (default scipy's
    ``gaussian_filter(mode="reflect", truncate=3.0)`` when scipy imports, else :func:`gaussian_smooth`)."""
    smooth = smooth or _default_smooth()
    M = None if mask is None else _checked_mask(mask)
    cache = {}

    def h0(q):
        q = np.asarray(q)
        s1 = cache.get("s1")
        if s1 is None:
            s1 = cache["s1"] = tuple(v / np.sqrt(2.0) for v in _axis_widths(sigma, q.ndim))
            cache["M"] = None if M is None else M.astype(q.dtype)
            cache["D"] = None if precond is None else np.asarray(precond() if callable(precond) else precond, q.dtype)
        v = q if cache["M"] is None else q * cache["M"]
        v = smooth(v, s1)
        if cache["D"] is not None:
            v = v * cache["D"]
        v = smooth(v, s1)
        return np.asarray(v if cache["M"] is None else v * cache["M"])

    h0.tag = _h0_tag(np.atleast_1d(np.asarray(sigma, np.float64)).tolist(), M, precond is not None)
    return h0


def smoothing_h0_device(engine, sigma, mask=None, precond_slot=None):
    """:func:`smoothing_h0` on device vectors, for :func:`lbfgs.lbfgs_device`: ``h0(slot)`` applies
    ``B = M S' D S' M`` in place with ``Engine.vec_mul`` and ``Engine.vec_smooth`` -- nothing model-sized crosses PCIe.
    D is read from ``precond_slot`` when B is applied; the mask is uploaded once into the one slot ``lbfgs_device``
    creates for it (``h0.nslots`` / ``h0.setup``).  Same tag as the host twin: a state file moves between the two."""
    e = engine_of(engine)
    s1 = tuple(v / np.sqrt(2.0) for v in _axis_widths(sigma, len(e.shape)))
    M = None if mask is None else _checked_mask(mask)
    if M is not None and M.shape != tuple(e.shape):
        raise ValueError("mask has shape %r, the grid %r" % (M.shape, tuple(e.shape)))
    where = {}

    def h0(slot):
        if M is not None:
            e.vec_mul(slot, where["mask"])
        e.vec_smooth(slot, s1)
        if precond_slot is not None:
            e.vec_mul(slot, precond_slot)
        e.vec_smooth(slot, s1)
        if M is not None:
            e.vec_mul(slot, where["mask"])

    def setup(first_slot):
        if M is not None:
            where["mask"] = int(first_slot)
            e.vec_upload(where["mask"], M)

    h0.nslots = 0 if M is None else 1
    h0.setup = setup
    h0.tag = _h0_tag(np.atleast_1d(np.asarray(sigma, np.float64)).tolist(), M, precond_slot is not None)
    return h0


def source_mute(shape, shots, radius):
    """Mask ``1 - exp(-(d / radius)^2)``, d the distance in cells to the nearest source node of ``shots``: 0 on the
    sources, ~1 a few radii away.  Damps the source imprint of the gradient (host NumPy, built once)."""
    if not float(radius) > 0.0:
        raise ValueError("radius must be > 0")
    src = np.unique(np.concatenate([np.asarray(s.src_idx).reshape(-1, len(shape)) for s in shots], 0), axis=0)
    axes = [np.arange(n, dtype=np.float64) for n in shape]
    d2 = np.full(shape, np.inf)
    for node in src:
        t = np.zeros(shape)
        for ax, (a, c) in enumerate(zip(axes, node)):
            sh_ = [1] * len(shape)
            sh_[ax] = -1
            t = t + ((a - float(c)) ** 2).reshape(sh_)
        np.minimum(d2, t, out=d2)
    return 1.0 - np.exp(-d2 / float(radius) ** 2)


TRAVELTIME_SLOTS = 5  # vector slots traveltime_fg uses from slot0 on: times, scratch, right-hand side, lambda, gradient


def _traveltime_points(shot):
    """(source coordinates, receivers) of a shot for the eikonal calls: its first source, the point itself when it is
    off-grid, and the receiver points (a ``points.Spread``) or nodes"""
    src = shot.src_spread.coords[0] if shot.src_spread is not None else np.asarray(shot.src_idx).reshape(-1, np.shape(shot.src_idx)[-1])[0]
    return np.asarray(src, np.float64), (shot.rec_spread if shot.rec_spread is not None else np.asarray(shot.rec_idx))


def _times_of_all_shots(engine, shots, ex, one):
    """``one(engine, i)``, the receiver times of shot ``i``, for this rank's shots: the list over all shots, complete on
    every rank"""
    mine = partition_shots(len(shots), ex.rank, ex.world)
    got = engine.map_shots(mine, one) if isinstance(engine, EnginePool) else [one(engine, i) for i in mine]
    sizes = [s.rec_spread.n if s.rec_spread is not None else len(np.asarray(s.rec_idx).reshape(-1, np.shape(s.rec_idx)[-1]))
             for s in shots]
    ends = np.cumsum([0] + sizes)
    flat = np.zeros(ends[-1])
    for i, v in zip(mine, got):
        flat[ends[i]:ends[i + 1]] = v
    flat = np.asarray(ex.reduce_array(flat))
    return [flat[ends[i]:ends[i + 1]].copy() for i in range(len(shots))]


def traveltime_times(engine, model, shots, radius=0.0, slot0=0, exchange=None):
    """First-arrival times of every shot at its receivers in ``model`` (None: the model the engines hold): a list
    indexed like ``shots``, complete on every rank.  The picks of a synthetic test, or the times of a
    ``datafit.first_arrival_mute``."""
    ex = exchange or NoExchange()
    if model is not None:
        for e in _engines(engine):
            e.set_model(model)

    def one(e, i):
        src, rec = _traveltime_points(shots[i])
        e.eikonal(src, slot0, slot0 + 1, radius=radius)
        return e.eikonal_times(slot0, rec)

    return _times_of_all_shots(engine, shots, ex, one)


def traveltime_fg(engine, model, shots, picks, pick_weights=None, radius=0.0, slot0=0, exchange=None, wrt="velocity"):
    """First-arrival traveltime tomography: ``(J, g)`` with

        ``J = 1/2 sum_s sum_r w_sr (T_s(x_r) - t_sr)^2``

    and ``g = dJ/dmodel`` (``wrt`` as in :func:`misfit_and_gradient`; ``model`` is a velocity), summed over shots, the
    engines of a pool and the ranks -- what ``lbfgs`` takes as ``lambda m: traveltime_fg(engine, m, ...)``.
    ``picks[i]``: the picked times of shot ``i`` at its receivers (NaN: no pick, the receiver does not count);
    ``pick_weights[i]``: weights >= 0 likewise (None: 1).  Per shot one eikonal solve from the shot's FIRST source
    (``src_spread.coords`` when it is off-grid, with every node within ``radius`` cells initialised, ``eikonal.ball``),
    the residuals scattered at the receivers' nodes (``rec_spread``: with the multilinear weights), one adjoint solve,
    and the gradient added into a slot (``beta = 1``) that is downloaded once per engine.  Uses the
    ``TRAVELTIME_SLOTS`` vector slots from ``slot0`` on, which must exist (``vec_create``).  The engine may be anything
    with ``set_model``, ``eikonal``, ``eikonal_times``, ``vec_scatter_points``, ``eikonal_adjoint``,
    ``eikonal_gradient`` and ``vec_download``: ``eikonal.TwinEngine`` runs it on the CPU."""
    ex = exchange or NoExchange()
    T, SC, B, L, G = (slot0 + k for k in range(TRAVELTIME_SLOTS))
    engines = _engines(engine)
    for e in engines:
        e.set_model(model)
    first = {id(e): True for e in engines}

    def one(e, i):
        s = shots[i]
        src, rec = _traveltime_points(s)
        t = np.asarray(picks[i], np.float64).reshape(-1)
        w = np.ones(t.shape) if pick_weights is None or pick_weights[i] is None else \
            np.asarray(pick_weights[i], np.float64).reshape(-1)
        init = e.eikonal(src, T, SC, radius=radius)
        tau = e.eikonal_times(T, rec)
        if t.shape != tau.shape or w.shape != tau.shape:
            raise ValueError("shot %d: %d receivers, %d picks, %d weights" % (i, tau.size, t.size, w.size))
        ok = ~np.isnan(t)
        r = np.where(ok, w * (tau - np.where(ok, t, 0.0)), 0.0)  # dJ/dT(x_r)
        nodes, vals = _receiver_nodes(rec, r)  # off-grid receivers: onto their nodes
        e.vec_scatter_points(B, nodes, vals, beta=0.0)
        e.eikonal_adjoint(T, B, L, SC)
        e.eikonal_gradient(T, L, G, init, beta=0.0 if first[id(e)] else 1.0, wrt=wrt)
        first[id(e)] = False
        return 0.5 * float(np.sum(np.where(ok, w * (tau - np.where(ok, t, 0.0)) ** 2, 0.0)))

    mine = partition_shots(len(shots), ex.rank, ex.world)
    if isinstance(engine, EnginePool):
        J = float(sum(engine.map_shots(mine, one)))
    else:
        J = float(sum(one(engine, i) for i in mine))
    shape = np.shape(model)
    g = np.zeros(shape, np.float64)
    for e in engines:
        if not first[id(e)]:
            g += np.asarray(e.vec_download(G), np.float64)
    g = np.asarray(ex.reduce_array(g)).reshape(shape)
    J = float(np.asarray(ex.reduce_array(np.array([J]))).ravel()[0])
    return J, g


def _receiver_nodes(rec, r):
    """Receiver values ``r`` onto the grid's nodes: ``(nodes, values)``, a node shared by two receivers once (a
    ``points.Spread``: with its multilinear weights)"""
    if hasattr(rec, "pt_start"):
        nodes, inv = np.unique(np.asarray(rec.idx), axis=0, return_inverse=True)
        vals = np.zeros(len(nodes))
        np.add.at(vals, np.reshape(inv, -1), r[rec.owner] * rec.weights)
    else:
        nodes, inv = np.unique(np.asarray(rec).reshape(-1, np.shape(rec)[-1]), axis=0, return_inverse=True)
        vals = np.zeros(len(nodes))
        np.add.at(vals, np.reshape(inv, -1), r)
    return nodes, vals


class TraveltimeOperator:
    """The linearisation of the first-arrival times at one model: ``J_s = dT_s(x_r)/dmodel`` of every shot, its
    transpose and the Gauss-Newton Hessian ``sum_s J_s^T W_s J_s`` of :func:`traveltime_fg`'s functional, over shots,
    the engines of a pool and the ranks.  ``J_s v`` is one ``eikonal_tangent`` solve, ``J_s^T r`` one ``eikonal_adjoint``
    solve and an ``eikonal_gradient`` pass; the two are exact transposes of each other.

    ``model``: a velocity (None: the model the engines hold).  ``pick_weights[i]``: the weights ``W_s`` (None: 1);
    ``picks[i]``: only its NaNs count, a receiver without a pick gets weight zero as in :func:`traveltime_fg`.  With
    ``keep_times`` each local shot's ``T`` is solved once, here, into a slot of its own and a product costs two solves;
    without, ``T`` is solved again in every product (three solves) and one slot holds it.  Uses
    ``slots_needed(n_local)`` vector slots from ``slot0`` on, on every engine.  The engine may be anything with the
    engine's calls: ``eikonal.TwinEngine`` runs it on the CPU.  ``solves`` counts this rank's eikonal / tangent /
    adjoint solves, those of the constructor (``keep_times``) included."""

    WORK_SLOTS = 6  # scratch, v, dT, right-hand side, lambda, gradient; the times follow

    def __init__(self, engine, model, shots, radius=0.0, slot0=0, exchange=None, wrt="velocity", pick_weights=None,
                 picks=None, keep_times=True):
        if wrt not in ("velocity", "slowness2"):
            raise ValueError("wrt must be 'velocity' or 'slowness2', got %r" % (wrt,))
        self.engine, self.shots, self.radius, self.wrt = engine, shots, float(radius), wrt
        self.ex = exchange or NoExchange()
        self.keep_times = bool(keep_times)
        self.engines = _engines(engine)
        self.SC, self.V, self.X, self.B, self.L, self.G = (int(slot0) + k for k in range(6))
        self.T0 = int(slot0) + self.WORK_SLOTS
        self.mine = partition_shots(len(shots), self.ex.rank, self.ex.world)
        self.solves = {"eikonal": 0, "tangent": 0, "adjoint": 0}
        self.model = None if model is None else np.array(model, np.float64)
        if model is not None:
            for e in self.engines:
                e.set_model(model)
        self.shape = tuple(self.engines[0].shape)
        self.points = [_traveltime_points(s) for s in shots]
        self.sizes = [rec.n if hasattr(rec, "pt_start") else len(np.asarray(rec).reshape(-1, np.shape(rec)[-1]))
                      for _, rec in self.points]
        self.weights = []
        for i, n in enumerate(self.sizes):
            w = np.ones(n) if pick_weights is None or pick_weights[i] is None else \
                np.asarray(pick_weights[i], np.float64).reshape(-1)
            if picks is not None and picks[i] is not None:
                t = np.asarray(picks[i], np.float64).reshape(-1)
                if t.shape != w.shape:
                    raise ValueError("shot %d: %d weights, %d picks" % (i, w.size, t.size))
                w = np.where(np.isnan(t), 0.0, w)
            if w.shape != (n,):
                raise ValueError("shot %d: %d receivers, %d weights" % (i, n, w.size))
            self.weights.append(w)
        self.inits = {}
        self._prepare()
        if self.keep_times:
            self._map(lambda e, pos, i: self._solve(e, pos, i))
            self.solves["eikonal"] += self.STAGES * len(self.mine)

    STAGES = 1       # eikonal solves per shot, and slots that hold a shot's times

    def _prepare(self):
        """what the engines need before the first solve (nothing here)"""

    def slots_needed(self, n_local):
        """vector slots used from ``slot0`` on by a rank with ``n_local`` shots (on each of its engines)"""
        per_engine = -(-int(n_local) // len(self.engines))
        return self.WORK_SLOTS + self.STAGES * (max(1, per_engine) if self.keep_times else 1)

    # position pos of this rank's shots runs on engine pos % n, as EnginePool.map_shots deals them out
    def _t_slot(self, pos):
        return self.T0 + self.STAGES * (pos // len(self.engines) if self.keep_times else 0) + self.STAGES - 1

    def _map(self, fn):
        pos_of = {i: pos for pos, i in enumerate(self.mine)}
        if isinstance(self.engine, EnginePool):
            return self.engine.map_shots(self.mine, lambda e, i: fn(e, pos_of[i], i))
        return [fn(self.engine, pos_of[i], i) for i in self.mine]

    def _solve(self, e, pos, i):
        self.inits[i] = e.eikonal(self.points[i][0], self._t_slot(pos), self.SC, radius=self.radius)

    def _times_slot(self, e, pos, i):
        if not self.keep_times:
            self._solve(e, pos, i)
        return self._t_slot(pos)

    def _complete(self, got):
        """this rank's per-shot receiver arrays -> the list over all shots, complete on every rank"""
        ends = np.cumsum([0] + self.sizes)
        flat = np.zeros(ends[-1])
        for i, v in zip(self.mine, got):
            flat[ends[i]:ends[i + 1]] = v
        flat = np.asarray(self.ex.reduce_array(flat))
        return [flat[ends[i]:ends[i + 1]].copy() for i in range(len(self.shots))]

    def _count(self, tangent=0, adjoint=0):
        n = self.STAGES * len(self.mine)
        self.solves["tangent"] += tangent * n
        self.solves["adjoint"] += adjoint * n
        self.solves["eikonal"] += 0 if self.keep_times else n

    def _upload(self, v):
        v = np.asarray(v, np.float64).reshape(self.shape)
        for e in self.engines:
            e.vec_upload(self.V, v.astype(getattr(e, "dtype", np.float64)))

    def _jvp_one(self, e, pos, i):
        """dT_s at the receivers of shot i, from the perturbation in slot V"""
        T = self._times_slot(e, pos, i)
        e.eikonal_tangent(T, self.V, self.X, self.SC, self.inits[i], wrt=self.wrt)
        rec = self.points[i][1]
        if hasattr(rec, "pt_start"):
            x = e.vec_gather_points(self.X, rec.idx) * rec.weights
            return np.add.reduceat(x, rec.pt_start[:-1]) if len(x) else np.zeros(0)
        return e.vec_gather_points(self.X, rec)

    def _vjp_one(self, e, pos, i, r, first, solve=True):
        """G (+)= J_s^T r"""
        T = self._times_slot(e, pos, i) if solve else self._t_slot(pos)
        nodes, vals = _receiver_nodes(self.points[i][1], np.asarray(r, np.float64).reshape(-1))
        e.vec_scatter_points(self.B, nodes, vals, beta=0.0)
        e.eikonal_adjoint(T, self.B, self.L, self.SC)
        e.eikonal_gradient(T, self.L, self.G, self.inits[i], beta=0.0 if first[id(e)] else 1.0, wrt=self.wrt)
        first[id(e)] = False

    def _gather_gradient(self, first):
        g = np.zeros(self.shape, np.float64)
        for e in self.engines:
            if not first[id(e)]:
                g += np.asarray(e.vec_download(self.G), np.float64)
        return np.asarray(self.ex.reduce_array(g)).reshape(self.shape)

    def times(self):
        """The times of every shot at its receivers, as :func:`traveltime_times`"""
        if not self.keep_times:
            self.solves["eikonal"] += self.STAGES * len(self.mine)
        return self._complete(self._map(lambda e, pos, i: e.eikonal_times(self._times_slot(e, pos, i), self.points[i][1])))

    def jvp(self, v):
        """``[J_s v]``: the change of every shot's times at its receivers for the model change ``v``, complete on
        every rank"""
        self._upload(v)
        self._count(tangent=1)
        return self._complete(self._map(self._jvp_one))

    def vjp(self, r_list):
        """``sum_s J_s^T r_s``, model-shaped fp64, summed over engines and ranks; ``r_list[i]``: one value per receiver"""
        first = {id(e): True for e in self.engines}
        for i in self.mine:
            if np.size(r_list[i]) != self.sizes[i]:
                raise ValueError("shot %d: %d receivers, %d values" % (i, self.sizes[i], np.size(r_list[i])))
        self._count(adjoint=1)
        self._map(lambda e, pos, i: self._vjp_one(e, pos, i, r_list[i], first))
        return self._gather_gradient(first)

    def hvp(self, v):
        """``sum_s J_s^T W_s J_s v``, model-shaped fp64, summed over engines and ranks"""
        first = {id(e): True for e in self.engines}
        self._upload(v)
        self._count(tangent=1, adjoint=1)

        def one(e, pos, i):
            self._vjp_one(e, pos, i, self.weights[i] * self._jvp_one(e, pos, i), first, solve=False)

        self._map(one)
        return self._gather_gradient(first)


# Reflection traveltimes off a fixed interface: two first-arrival solves in a row (eikonal.py defines
# every piece).  Stage 1 runs from the source inside the wall; stage 2 restarts from the interface nodes with the times
# they just got.  Out of scope: the reflector's depth as an unknown, head waves, multiples, transmitted conversions.
REFLECTION_SLOTS = 10  # reflection_fg from slot0 on: wall, start, T1, T2, scratch, right-hand side, lambda2, handover,
#                        lambda1, gradient


class Reflector:
    """A fixed interface: ``gamma`` marks its nodes and ``wall`` the cells beyond it that no front may enter, both
    boolean arrays of the grid's shape, as ``eikonal.interface(shape, depth)`` returns them."""

    def __init__(self, gamma, wall):
        self.gamma, self.wall = np.asarray(gamma) != 0, np.asarray(wall) != 0
        if self.gamma.shape != self.wall.shape:
            raise ValueError("gamma %r and wall %r must have the grid's shape" % (self.gamma.shape, self.wall.shape))
        if not self.gamma.any() or (self.gamma & self.wall).any():
            raise ValueError("the interface needs at least one node, and none of its nodes may be walled")
        self.gamma_nodes = np.ascontiguousarray(np.argwhere(self.gamma), dtype=np.int32)  # ascending flat order

    @classmethod
    def at_depth(cls, shape, depth):
        from . import eikonal as ek
        return cls(*ek.interface(shape, depth))

    def upload(self, e, wall_slot, start_slot):
        """the wall (1 in its cells) and the start's template (0 on the interface, +inf elsewhere) into two slots"""
        dtype = getattr(e, "dtype", np.float64)
        e.vec_upload(wall_slot, self.wall.astype(dtype))
        e.vec_upload(start_slot, np.where(self.gamma, 0.0, np.inf).astype(dtype))

    def solve(self, e, src, radius, W, S0, T1, T2, SC):
        """both stages on engine ``e``: T1, then T2 started on the device from T1's times on the interface (only the
        interface's values cross).  Returns the init list of stage 1."""
        init = e.eikonal(src, T1, SC, radius=radius, wall_slot=W)
        v = e.vec_gather_points(T1, self.gamma_nodes)
        if not np.all(np.isfinite(v)):
            raise ValueError("stage 1 does not reach %d of the interface's %d nodes" % (np.count_nonzero(~np.isfinite(v)), v.size))
        e.vec_copy(T2, S0)
        e.vec_scatter_points(T2, self.gamma_nodes, v, beta=1.0)  # 0 + T1 on the interface, +inf stays +inf
        e.eikonal_restart(T2, SC, wall_slot=W)
        return init


def _reflection_vjp(e, T1, T2, B, L2, H, L1, G, SC, init, beta, wrt):
    """G := beta G + the gradient of <B, T2> through both stages"""
    e.eikonal_adjoint(T2, B, L2, SC)
    e.eikonal_handover(T2, L2, H)
    e.eikonal_adjoint(T1, H, L1, SC)
    e.eikonal_gradient(T2, L2, G, None, beta=beta, wrt=wrt)
    e.eikonal_gradient(T1, L1, G, init, beta=1.0, wrt=wrt)


def reflection_times(engine, model, shots, reflector, radius=0.0, slot0=0, exchange=None):
    """Reflection times off ``reflector`` of every shot at its receivers in ``model`` (None: the model the engines
    hold), as :func:`traveltime_times`.  Uses the first five of the ``REFLECTION_SLOTS``."""
    ex = exchange or NoExchange()
    W, S0, T1, T2, SC = (slot0 + k for k in range(5))
    for e in _engines(engine):
        if model is not None:
            e.set_model(model)
        reflector.upload(e, W, S0)

    def one(e, i):
        src, rec = _traveltime_points(shots[i])
        reflector.solve(e, src, radius, W, S0, T1, T2, SC)
        return e.eikonal_times(T2, rec)

    return _times_of_all_shots(engine, shots, ex, one)


def reflection_fg(engine, model, shots, picks, reflector, pick_weights=None, radius=0.0, slot0=0, exchange=None,
                  wrt="velocity"):
    """Reflection traveltime tomography off a fixed ``reflector``: ``(J, g)`` of :func:`traveltime_fg`'s functional with
    the reflection times in place of the first arrivals, for ``lbfgs``.  Per shot two eikonal solves, two adjoint
    solves with one handover between them and two gradient passes; the wall and the start's template are uploaded once
    per engine, the stage-2 start is built on the device, and only receiver and interface values cross per shot.
    Uses the ``REFLECTION_SLOTS`` vector slots from ``slot0`` on.  Runs on ``eikonal.TwinEngine`` too."""
    ex = exchange or NoExchange()
    W, S0, T1, T2, SC, B, L2, H, L1, G = (slot0 + k for k in range(REFLECTION_SLOTS))
    engines = _engines(engine)
    for e in engines:
        e.set_model(model)
        reflector.upload(e, W, S0)
    first = {id(e): True for e in engines}

    def one(e, i):
        src, rec = _traveltime_points(shots[i])
        t = np.asarray(picks[i], np.float64).reshape(-1)
        w = np.ones(t.shape) if pick_weights is None or pick_weights[i] is None else \
            np.asarray(pick_weights[i], np.float64).reshape(-1)
        init = reflector.solve(e, src, radius, W, S0, T1, T2, SC)
        tau = e.eikonal_times(T2, rec)
        if t.shape != tau.shape or w.shape != tau.shape:
            raise ValueError("shot %d: %d receivers, %d picks, %d weights" % (i, tau.size, t.size, w.size))
        ok = ~np.isnan(t)
        r = np.where(ok, w * (tau - np.where(ok, t, 0.0)), 0.0)  # dJ/dT2(x_r)
        nodes, vals = _receiver_nodes(rec, r)
        e.vec_scatter_points(B, nodes, vals, beta=0.0)
        _reflection_vjp(e, T1, T2, B, L2, H, L1, G, SC, init, 0.0 if first[id(e)] else 1.0, wrt)
        first[id(e)] = False
        return 0.5 * float(np.sum(np.where(ok, w * (tau - np.where(ok, t, 0.0)) ** 2, 0.0)))

    mine = partition_shots(len(shots), ex.rank, ex.world)
    if isinstance(engine, EnginePool):
        J = float(sum(engine.map_shots(mine, one)))
    else:
        J = float(sum(one(engine, i) for i in mine))
    shape = np.shape(model)
    g = np.zeros(shape, np.float64)
    for e in engines:
        if not first[id(e)]:
            g += np.asarray(e.vec_download(G), np.float64)
    g = np.asarray(ex.reduce_array(g)).reshape(shape)
    J = float(np.asarray(ex.reduce_array(np.array([J]))).ravel()[0])
    return J, g


class ReflectionOperator(TraveltimeOperator):
    """:class:`TraveltimeOperator` for the reflection times off a fixed ``reflector``: ``times``, ``jvp``, ``vjp``,
    ``hvp`` and ``solves`` mean the same, every solve being two (one per stage, with a handover between them), so that
    ``newton.traveltime_newton_step(op, g, ...)`` runs on it.  With ``keep_times`` every local shot keeps both stages'
    times: ``slots_needed(n_local)`` is ``WORK_SLOTS + 2 * shots per engine``."""

    WORK_SLOTS = 11  # the parent's six; wall, start, handover, stage 1's dT, stage 1's lambda; the times follow
    STAGES = 2

    def __init__(self, engine, model, shots, reflector, **kw):
        self.reflector = reflector
        super().__init__(engine, model, shots, **kw)

    def _prepare(self):
        self.W, self.S0, self.H, self.X1, self.L1 = (self.SC + 6 + k for k in range(5))
        for e in self.engines:
            self.reflector.upload(e, self.W, self.S0)

    def _solve(self, e, pos, i):
        T2 = self._t_slot(pos)
        self.inits[i] = self.reflector.solve(e, self.points[i][0], self.radius, self.W, self.S0, T2 - 1, T2, self.SC)

    def _jvp_one(self, e, pos, i):
        T2 = self._times_slot(e, pos, i)
        e.eikonal_tangent(T2 - 1, self.V, self.X1, self.SC, self.inits[i], wrt=self.wrt)
        e.eikonal_handover(T2, self.X1, self.H)
        e.eikonal_tangent(T2, self.V, self.X, self.SC, None, wrt=self.wrt, b0_slot=self.H)
        rec = self.points[i][1]
        if hasattr(rec, "pt_start"):
            x = e.vec_gather_points(self.X, rec.idx) * rec.weights
            return np.add.reduceat(x, rec.pt_start[:-1]) if len(x) else np.zeros(0)
        return e.vec_gather_points(self.X, rec)

    def _vjp_one(self, e, pos, i, r, first, solve=True):
        T2 = self._times_slot(e, pos, i) if solve else self._t_slot(pos)
        nodes, vals = _receiver_nodes(self.points[i][1], np.asarray(r, np.float64).reshape(-1))
        e.vec_scatter_points(self.B, nodes, vals, beta=0.0)
        _reflection_vjp(e, T2 - 1, T2, self.B, self.L, self.H, self.L1, self.G, self.SC, self.inits[i],
                        0.0 if first[id(e)] else 1.0, self.wrt)
        first[id(e)] = False
