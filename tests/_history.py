"""History independence of one engine context: the catalogue of steps, the configurations, the sequences.

One context serves a production shot loop for thousands of shots of different lengths, point sets and objectives, and
keeps some forty device buffers that only grow, a dozen flags and three cached tables between them.  The question asked
here: DOES A CALL RETURN THE SAME BITS WHATEVER THE CONTEXT DID BEFORE?  The oracle is the library itself on a fresh
context, bit for bit -- every sum in it is taken in a fixed order, so there is no tolerance anywhere in these tests.

A STEP is a function ``run(engine, problem, model_id) -> {name: ndarray | float}``: it begins with ``reset_gradient()``
and its own ``forward`` / ``forward_at`` and ends by downloading everything it produced.  Steps come in FAMILIES; the
variants of a family differ in their sizes (``nt``, sources, receivers), consecutive variants alternating between a
larger and a smaller one so that buffers grow and are then used below their capacity.  A step leaves the context as it
found it -- illumination off, the configured launch mode and Fourier settings -- except for the model, which the
``model`` family changes: the model in force is part of a step's key.

``sequence(config, seed)`` walks an Euler circuit of the complete directed graph (loops included) over the families a
configuration allows: every ordered pair of families is adjacent exactly once.  tests/test_history_host.py asserts that
for every configuration, and runs every step against ``StubEngine``, a recorder that knows the refusals include/fwi.h
lists; tests/test_gpu_history.py runs the sequences and the directed cases on the device.
"""
from __future__ import annotations

import random
import zlib

import numpy as np

from full_waveform_inversion_amd import _lib
from full_waveform_inversion_amd._lib import FwiError
from full_waveform_inversion_amd.datafit import hilbert_taps
from full_waveform_inversion_amd.engine import cfl_dt, default_sigma_max, ricker
from full_waveform_inversion_amd.points import Spread

SEED = 20261020
NT_MAX, NPML, ORDER, H, C_MAX = 40, 4, 8, 10.0, 2600.0
SIGMA_MAX = default_sigma_max(C_MAX, H, NPML)
FIR_RMAX = 4096  # include/fwi.h, fwi_misfit_weighted: "R > 4096"
# 3-D: nx % 4 = 2, so the compact row stride differs from nx and the staging / repack path runs; 19 rows are two y tiles
# and a remainder.  2-D: more than one 64-point fused tile on each axis.
GRID3, GRID2 = (22, 19, 30), (70, 90)
# the box the points are drawn from, per axis [lo, hi): around the middle in 3-D (rows of two y tiles); across the tile
# seam at 64 on both axes in 2-D, two rows into the absorbing border
BOX = {3: ((5, 17), (3, 16), (8, 23)), 2: ((52, 68), (56, 74))}

CONFIGS = {
    "3d_f32_sponge": dict(shape=GRID3),
    "3d_f32_cpml_increment": dict(shape=GRID3, abc="cpml", update_form="increment"),
    "3d_f32_ckpt7": dict(shape=GRID3, ckpt_interval=7),
    "3d_f32_stride3": dict(shape=GRID3, image_stride=3),
    "3d_f32_bf16": dict(shape=GRID3, store_dtype="bf16"),
    "3d_f64": dict(shape=GRID3, dtype="float64"),
    "3d_f32_fourier": dict(shape=GRID3, fourier="A", fourier_batch=3),
    "3d_f32_graph": dict(shape=GRID3, launch_mode="graph"),
    "2d_f32_fused": dict(shape=GRID2),
    "2d_f32_fused_cpml": dict(shape=GRID2, abc="cpml"),
    "2d_f64_point": dict(shape=GRID2, dtype="float64", kernel="point"),
}

MISFITS = ("weighted", "matched", "envelope", "correlation", "traveltime", "transport", "spectral")
FOURIER_FAMILIES = ("four_spectral", "four_freqs", "four_count")
FAMILIES = (("fwd_save", "fwd_nosave", "adj_image", "adj_noimage", "l2") + tuple("misfit_" + m for m in MISFITS) +
            ("forward_at", "born_exact", "born_imaging", "illum", "vec", "launch", "model", "refused") + FOURIER_FAMILIES)

# What a configuration leaves out, and the sentence of include/fwi.h that says so (tests/test_history_host.py holds the
# table against the options of CONFIGS and looks the sentences up in the header).
_NO_EXACT_BORN = "fwi_born / fwi_born_vec return FWI_EINVAL"  # image_stride > 1, store_dtype = bf16, ckpt_interval > 0
_NO_BORN = "fwi_born* on it are FWI_ESTATE"                    # the Fourier store
_NO_ILLUM = "fails the same way on a context with this store"  # fwi_set_illumination(on) with the Fourier store
_NO_FOURIER = "for a context with ckpt_interval > 0 or store_dtype = bf16"  # fwi_set_fourier_store refuses these two
_OFF = "nfreq = 0 frees the arrays and returns the context to its configured store"  # not refused: the configuration
#                                                 simply runs on its configured store, and the families need the other
LEFT_OUT = {
    "3d_f32_sponge": dict.fromkeys(FOURIER_FAMILIES, _OFF),
    "3d_f32_cpml_increment": dict.fromkeys(FOURIER_FAMILIES, _OFF),
    "3d_f32_ckpt7": {"born_exact": _NO_EXACT_BORN, **dict.fromkeys(FOURIER_FAMILIES, _NO_FOURIER)},
    "3d_f32_stride3": {"born_exact": _NO_EXACT_BORN, **dict.fromkeys(FOURIER_FAMILIES, _OFF)},
    "3d_f32_bf16": {"born_exact": _NO_EXACT_BORN, **dict.fromkeys(FOURIER_FAMILIES, _NO_FOURIER)},
    "3d_f64": dict.fromkeys(FOURIER_FAMILIES, _OFF),
    "3d_f32_fourier": {"born_exact": _NO_BORN, "born_imaging": _NO_BORN, "illum": _NO_ILLUM},
    "3d_f32_graph": dict.fromkeys(FOURIER_FAMILIES, _OFF),
    "2d_f32_fused": dict.fromkeys(FOURIER_FAMILIES, _OFF),
    "2d_f32_fused_cpml": dict.fromkeys(FOURIER_FAMILIES, _OFF),
    "2d_f64_point": dict.fromkeys(FOURIER_FAMILIES, _OFF),
}


def families_of(config):
    return tuple(f for f in FAMILIES if f not in LEFT_OUT[config])


# ---------------------------------------------------------------------------------------------------------------------
# the problem a configuration poses: grid, time step, the two models, points, wavelets, data
# ---------------------------------------------------------------------------------------------------------------------
class Problem:
    def __init__(self, config):
        self.config, self.opts = config, dict(CONFIGS[config])
        self.shape = self.opts.pop("shape")
        self.ndim = len(self.shape)
        self.dtype = np.dtype(self.opts.get("dtype", "float32"))
        self.dt = 0.6 * cfl_dt(C_MAX, H, self.ndim, ORDER)
        self.graph = self.opts.get("launch_mode") == "graph"
        # Hz, all below the Nyquist frequency 1 / (2 dt) of the time axis and off the bins of every nt used
        self.freqs = {"A": np.array([0.04, 0.09, 0.15, 0.22]) / self.dt, "B": np.array([0.05, 0.10, 0.17, 0.30]) / self.dt,
                      "C": np.array([0.03, 0.07, 0.12, 0.19, 0.26, 0.33]) / self.dt}
        if "fourier" in self.opts:
            self.opts["fourier"] = self.freqs[self.opts["fourier"]]
        self.models = tuple((lo + (C_MAX - lo) * self.rng("model", k).random(self.shape)).astype(self.dtype)
                            for k, lo in enumerate((2000.0, 2100.0)))
        # [box, the two cells around its middle]: a star stencil of half-width 4 carries a signal over (a, b, c) cells in
        # ceil(a / 4) + ceil(b / 4) + ceil(c / 4) steps, so the points of a 5-step shot have to be neighbours for it to
        # record anything but exact zeros
        mid = tuple(((lo + hi) // 2 - 2, (lo + hi) // 2 + 3) for lo, hi in BOX[self.ndim])
        self._box = [np.array(b, np.float64) for b in (BOX[self.ndim], mid)]
        self._nodes = [np.stack([a.ravel() for a in np.meshgrid(*[np.arange(lo, hi) for lo, hi in b], indexing="ij")], 1)
                       for b in (BOX[self.ndim], mid)]

    def rng(self, *tag):
        return np.random.default_rng(zlib.crc32(repr((self.config,) + tag).encode()))

    def engine(self, **more):
        from full_waveform_inversion_amd.engine import Engine
        return Engine(self.shape, H, self.dt, NT_MAX, order=ORDER, npml=NPML, sigma_max=SIGMA_MAX, **{**self.opts, **more})

    def nodes(self, n, rng, near=False):
        """n distinct nodes of the box (``near``: of its middle), (n, ndim) int32"""
        nodes = self._nodes[bool(near)]
        return np.ascontiguousarray(nodes[rng.choice(len(nodes), n, replace=False)], dtype=np.int32)

    def points(self, n, rng, near=False):
        """n >= 1 points at fractional coordinates inside the box (``near``: inside its middle)"""
        lo, hi = self._box[bool(near)][:, 0], self._box[bool(near)][:, 1] - 1.0
        return Spread(lo + (hi - lo) * rng.random((n, self.ndim)), self.shape)

    def wavelet(self, nt, nsrc):
        """(nt, nsrc): a Ricker wavelet of 8 steps' period that peaks at step 4 -- the shortest shot (nt = 5) still holds
        its peak -- with another gain per source"""
        w = ricker(nt, self.dt, 1.0 / (8.0 * self.dt), t0=4.0 * self.dt, dtype=np.float64)
        return np.ascontiguousarray(w[:, None] * (1.0 + 0.5 * np.arange(nsrc))[None, :]).astype(self.dtype)

    def perturbation(self, rng):
        return (20.0 * rng.standard_normal(self.shape)).astype(self.dtype)


def observed(P, d, rng):
    """(d_obs, amax): the synthetics one sample late at 0.9 of their gain plus 5 % noise -- every misfit then has work to
    do, the traveltime one included -- and the amplitude the absolute floors are taken from (1 where ``d`` is empty or
    zero: a shot without sources, whose data are then the noise alone)"""
    amax = float(np.abs(d).max()) if d.size and np.abs(d).max() > 0 else 1.0
    d_obs = (0.9 * np.roll(d, 1, axis=0) + 0.05 * amax * rng.standard_normal(d.shape)).astype(P.dtype)
    return d_obs, amax


def taps_of(kind):
    """One-sided taps b_0 .. b_R: "long" with R = 44 > nt_max - 1 (clipped at every nt), "short" with R = 2"""
    if kind is None:
        return None
    R = {"long": 44, "short": 2}[kind]
    b = np.exp(-0.5 * (np.arange(R + 1) / (0.25 * R + 0.5)) ** 2)
    return b / (b[0] + 2.0 * b[1:].sum())


# ---------------------------------------------------------------------------------------------------------------------
# the steps
# ---------------------------------------------------------------------------------------------------------------------
class Step:
    """``run(e, P, model_id)`` of one variant of one family; ``refused``: (code, sentence of include/fwi.h) of the call
    the step expects to be refused, None for a step that computes something.  ``size``: nt * max(sources, receivers, 1),
    what the alternation between larger and smaller is measured by."""

    def __init__(self, family, variant, fn, size, refused=None, changes_model=False):
        self.family, self.variant, self.fn, self.size, self.refused = family, variant, fn, size, refused
        self.changes_model = changes_model

    def key(self, model_id):
        return (model_id, self.family, self.variant)

    def run(self, e, P, model_id):
        return self.fn(e, P, model_id, (self.family, self.variant))

    def __repr__(self):
        return "%s[%d]" % (self.family, self.variant)


def expect_refusal(code, call):
    try:
        call()
    except FwiError as err:
        assert err.code == code, "refused with %d instead of %d: %s" % (err.code, code, err)
        return
    raise AssertionError("the call was not refused (expected code %d)" % code)


def gradients(e, out):
    out["gradient_velocity"] = e.gradient()
    out["gradient_slowness2"] = e.gradient("slowness2")
    return out


def shoot(e, P, tag, nt, nsrc, nrec, save=True, off_grid=False):
    """The forward of a step: (seismograms, rng for what follows).  Sources and receivers are distinct nodes of the box,
    or points at fractional coordinates."""
    rng = P.rng(tag, "shot")
    wav = P.wavelet(nt, nsrc)
    near = nt < 16  # a short shot: neighbours (Problem.__init__)
    if off_grid:
        d = e.forward_at(None, (P.points(nsrc, rng, near), wav), P.points(nrec, rng, near), save=save)
    else:
        d = e.forward(None, (P.nodes(nsrc, rng, near), wav), P.nodes(nrec, rng, near), save=save)
    return d, rng


def host_residual(P, d, rng):
    return rng.standard_normal(d.shape).astype(P.dtype)


def _forward_only(save):
    def make(nt, nsrc, nrec):
        def fn(e, P, model_id, tag):
            e.reset_gradient()
            d, _ = shoot(e, P, tag, nt, nsrc, nrec, save=save)
            return {"seismograms": d}
        return fn
    return make


def _adjoint(image):
    def make(nt, nsrc, nrec):
        def fn(e, P, model_id, tag):
            e.reset_gradient()
            d, rng = shoot(e, P, tag, nt, nsrc, nrec, save=image)
            out = {"seismograms": d, "adjoint_series": e.adjoint(host_residual(P, d, rng), image=image)}
            return gradients(e, out)
        return fn
    return make


def _l2(nt, nsrc, nrec):
    def fn(e, P, model_id, tag):
        e.reset_gradient()
        d, rng = shoot(e, P, tag, nt, nsrc, nrec)
        d_obs, _ = observed(P, d, rng)
        out = {"seismograms": d, "J": e.misfit_l2(d_obs), "adjoint_series": e.adjoint(None)}
        return gradients(e, out)
    return fn


def call_misfit(e, P, name, d_obs, amax, weights, taps, tw, big, alt=False):
    """One data misfit with every optional output; ``big``: the larger of its two parameter sets (L, Q, max_lag);
    ``alt``: the other set of frequencies of the spectral misfit, which changes apart from nt (its table is cached
    against both)"""
    if name == "weighted":
        return {"J": e.misfit_weighted(d_obs, weights, taps)}
    if name == "matched":
        mu = 1e-3 * float((d_obs.astype(np.float64) ** 2).sum()) + 1e-12
        J, f = e.misfit_matched(d_obs, 6 if big else 2, mu, weights, taps)
        return {"J": J, "filter": f}
    if name == "envelope":
        return {"J": e.misfit_envelope(d_obs, hilbert_taps(9 if big else 3), power=1 if big else 2, eps=0.01 * amax,
                                       weights=weights, taps=taps)}
    if name == "correlation":
        J, rho = e.misfit_correlation(d_obs, 0.01 * amax, weights, taps, tw, per_trace=True)
        return {"J": J, "rho": rho}
    if name == "traveltime":
        J, tau, lag = e.misfit_traveltime(d_obs, 50 if big else 3, weights, taps, tw, per_trace=True)
        return {"J": J, "tau": tau, "lag": lag}
    if name == "transport":
        J, w2, counts = e.misfit_transport(d_obs, "softplus" if big else "linear", 3.0 / amax if big else 50.0 * amax,
                                           weights, taps, tw, per_trace=True)
        return {"J": J, "w2": w2, "counts": counts}
    if name == "spectral":
        f = P.freqs["A"] if alt else P.freqs["B"]  # as many as A: a table kept for the count alone is the wrong one
        fw = np.linspace(1.0, 2.0, f.size) if big else None
        J, phi, a, counts = e.misfit_spectral(d_obs, f, "log" if big else "l2", 0.01 * amax, weights, taps, fw, tw,
                                              per_pair=True)
        return {"J": J, "phase": phi, "logamp": a, "counts": counts}
    raise KeyError(name)


TAKES_TRACE_WEIGHTS = ("correlation", "traveltime", "transport", "spectral")


def misfit_args(P, d, rng, taps, weights, tw):
    """(weights (nt, ntr) | None, taps | None, trace weights (ntr,) | None) of one variant"""
    W = (0.5 + rng.random(d.shape)).astype(P.dtype) if weights else None
    TW = 0.25 + rng.random(d.shape[1]) if tw else None
    return W, taps_of(taps), TW


def _misfit(name):
    def make(nt, nsrc, nrec, taps=None, weights=False, tw=False, off_grid=False, big=False, alt=False):
        def fn(e, P, model_id, tag):
            e.reset_gradient()
            d, rng = shoot(e, P, tag, nt, nsrc, nrec, off_grid=off_grid)
            d_obs, amax = observed(P, d, rng)
            W, b, TW = misfit_args(P, d, rng, taps, weights, tw and name in TAKES_TRACE_WEIGHTS)
            out = {"seismograms": d}
            out.update(call_misfit(e, P, name, d_obs, amax, W, b, TW, big, alt))
            out["adjoint_series"] = e.adjoint(None)
            return gradients(e, out)
        return fn
    return make


def _forward_at(nt, nsrc, nrec, device_residual):
    def fn(e, P, model_id, tag):
        e.reset_gradient()
        d, rng = shoot(e, P, tag, nt, nsrc, nrec, off_grid=True)
        out = {"seismograms": d}
        if device_residual:
            out["J"] = e.misfit_l2(observed(P, d, rng)[0])
            out["adjoint_series"] = e.adjoint(None)
        else:
            out["adjoint_series"] = e.adjoint(host_residual(P, d, rng))
        return gradients(e, out)
    return fn


def _born(operator):
    def make(nt, nsrc, nrec):
        def fn(e, P, model_id, tag):
            e.reset_gradient()
            d, rng = shoot(e, P, tag, nt, nsrc, nrec)
            out = {"seismograms": d, "born_data": e.born(P.perturbation(rng), operator=operator),
                   "adjoint_series": e.adjoint(None)}
            return gradients(e, out)
        return fn
    return make


def _illum(nt, nsrc, nrec):
    def fn(e, P, model_id, tag):
        e.reset_gradient()
        e.set_illumination(True)
        d, rng = shoot(e, P, tag, nt, nsrc, nrec)
        out = {"seismograms": d, "adjoint_series": e.adjoint(host_residual(P, d, rng)),
               "illumination_velocity": e.illumination(), "illumination_slowness2": e.illumination("slowness2")}
        gradients(e, out)
        e.set_illumination(False)
        return out
    return fn


def _vec(nt, nsrc, nrec):
    def fn(e, P, model_id, tag):
        e.reset_gradient()
        d, rng = shoot(e, P, tag, nt, nsrc, nrec)
        out = {"seismograms": d, "adjoint_series": e.adjoint(host_residual(P, d, rng))}
        e.vec_create(4)
        e.vec_upload(0, P.perturbation(rng))
        e.vec_upload(1, P.perturbation(rng))
        e.vec_smooth(0, 1.5)
        out["tv"] = e.vec_regularizer(0, out=2, kind="tv", x0=1, eps=3.0, weight=[1.0, 0.5, 2.0][:P.ndim])
        out["tikhonov"] = e.vec_regularizer(1, kind="tikhonov")
        out["dot"] = e.vec_dot(0, 1)
        e.vec_axpby(1, -0.5, 0, 2.0)
        e.gradient_vec(3)
        for k in range(4):
            out["vec%d" % k] = e.vec_download(k)
        return out
    return fn


def _launch(nt, nsrc, nrec):
    def fn(e, P, model_id, tag):
        e.reset_gradient()
        e.set_launch_mode("stream" if P.graph else "graph")
        d, rng = shoot(e, P, tag, nt, nsrc, nrec)
        out = {"seismograms": d, "adjoint_series": e.adjoint(host_residual(P, d, rng))}
        gradients(e, out)
        e.set_launch_mode("graph" if P.graph else "stream")
        return out
    return fn


def _model(nt, nsrc, nrec):
    def fn(e, P, model_id, tag):
        e.reset_gradient()
        e.set_model(P.models[1 - model_id])
        d, rng = shoot(e, P, tag + (1 - model_id,), nt, nsrc, nrec)
        out = {"seismograms": d, "adjoint_series": e.adjoint(host_residual(P, d, rng))}
        return gradients(e, out)
    return fn


def _four_spectral(nt, nsrc, nrec):
    def fn(e, P, model_id, tag):
        e.reset_gradient()
        d, rng = shoot(e, P, tag, nt, nsrc, nrec)
        a = np.linspace(0.5, 1.5, len(e.fourier_freqs))
        out = {"seismograms": d, "adjoint_series": e.adjoint_spectral(host_residual(P, d, rng), freq_weights=a),
               "fourier_gradient_velocity": e.fourier_gradient(a), "fourier_gradient_slowness2": e.fourier_gradient(None, "slowness2"),
               "fourier_illumination": e.fourier_illumination(a), "spectrum": e.fourier_spectrum(),
               "adjoint_spectrum": e.fourier_adjoint_spectrum()}
        return gradients(e, out)
    return fn


def _four_shot(e, P, tag, nt, nsrc, nrec, out, label):
    d, rng = shoot(e, P, tag + (label,), nt, nsrc, nrec)
    out[label + "_seismograms"] = d
    out[label + "_adjoint_series"] = e.adjoint(host_residual(P, d, rng))
    return out


def _four_freqs(nt, nsrc, nrec):
    def fn(e, P, model_id, tag):  # other frequencies of the same count (the arrays stay, the table changes), and back
        e.reset_gradient()
        e.set_fourier_store(P.freqs["B"])
        out = _four_shot(e, P, tag, nt, nsrc, nrec, {}, "B")
        out["spectrum"] = e.fourier_spectrum()
        gradients(e, out)
        e.set_fourier_store(P.freqs["A"])
        return out
    return fn


def _four_count(nt, nsrc, nrec):
    def fn(e, P, model_id, tag):  # another count and batch, then off (the configured store), then on again as configured
        e.reset_gradient()
        e.set_fourier_store(P.freqs["C"], batch=2)
        out = _four_shot(e, P, tag, nt, nsrc, nrec, {}, "C")
        out["spectrum"] = e.fourier_spectrum()
        e.set_fourier_store(None)
        _four_shot(e, P, tag, nt, nsrc, nrec, out, "off")
        e.set_fourier_store(P.freqs["A"], batch=3)
        _four_shot(e, P, tag, nt, nsrc, nrec, out, "A")
        return gradients(e, out)
    return fn


# The refused calls: arguments and call orders include/fwi.h lists as FWI_EINVAL (1) / FWI_ESTATE (3), each refused before
# any state is touched (a refused forward gives up the shot before it -- the step's own).  (code, the header's words)
def _refused(which):
    nt, nsrc, nrec = 8, 1, 3

    def fn(e, P, model_id, tag):
        e.reset_gradient()
        if which == "nt_above_nt_max":
            rng = P.rng(tag, "shot")
            expect_refusal(1, lambda: e.forward(None, (P.nodes(1, rng), P.wavelet(NT_MAX + 1, 1)), P.nodes(3, rng)))
            return {}
        d, rng = shoot(e, P, tag, nt, nsrc, nrec, save=which != "image_without_store")
        d_obs, amax = observed(P, d, rng)
        if which == "taps_above_rmax":
            expect_refusal(1, lambda: e.misfit_weighted(d_obs, None, np.ones(FIR_RMAX + 2)))
        elif which == "negative_eps":
            expect_refusal(1, lambda: e.misfit_correlation(d_obs, -0.01 * amax))
        elif which == "unknown_spectral_kind":
            f = np.ascontiguousarray(P.freqs["A"])
            expect_refusal(1, lambda: e._misfit(e._lib.fwi_misfit_spectral, d_obs, None, None,
                                                (f.size, f.ctypes.data, 7, 0.0, None, None), (None, None, None)))
        elif which == "misfit_after_adjoint":
            e.adjoint(host_residual(P, d, rng), image=False)
            expect_refusal(3, lambda: e.misfit_l2(d_obs))
        elif which == "image_without_store":
            expect_refusal(3, lambda: e.adjoint(host_residual(P, d, rng), image=True))
        else:
            raise KeyError(which)
        return {}
    return fn


REFUSALS = (
    ("nt_above_nt_max", 1, "largest number of time steps a shot will use"),
    ("taps_above_rmax", 1, "R > 4096"),
    ("negative_eps", 1, "eps < 0 or not finite"),
    ("unknown_spectral_kind", 1, "an unknown kind"),
    ("misfit_after_adjoint", 3, "FWI_ESTATE without a forward or once an fwi_adjoint / fwi_born has run since"),
    ("image_without_store", 3, "call order violated (e.g. adjoint before forward)"),
)

# (nt, sources, receivers) of the four variants of a family: large, tiny, middling, small -- up and down in turn, the
# wrap from the last to the first included.  Between them the families cover nt in {5, 31, 33, nt_max} (the gather tiles
# hold 32 times, the 2-D fused kernel advances 4 steps per launch), receivers in {0, 1, 7, 65} (a tile has 64 trace
# lanes) and sources in {0, 1, 3}.  A shot without sources computes zeros and one without receivers records nothing, so
# those two sit where something else is left to compare: J of the noise (l2), the source-side illumination (illum,
# four_spectral).
SWEEPS = ((40, 1, 65), (5, 1, 1), (33, 3, 7), (31, 1, 1))
SIZES = {
    "l2": ((40, 3, 65), (5, 0, 1), (33, 1, 7), (31, 1, 1)),
    "illum": ((40, 1, 7), (5, 1, 0), (33, 3, 65), (31, 1, 1)),
    "four_spectral": ((40, 1, 7), (5, 1, 0), (33, 3, 65), (31, 1, 1)),
    "born_exact": ((40, 1, 7), (5, 1, 1), (33, 3, 65), (31, 3, 1)),
    "born_imaging": ((40, 1, 7), (5, 1, 1), (33, 3, 65), (31, 3, 1)),
    "four_count": ((40, 1, 7), (5, 1, 1), (33, 3, 7), (31, 1, 1)),
}
# the misfits: long taps (R > nt - 1: clipped), short ones and none; weights and none; trace weights (where the misfit
# takes them) and none; one variant with off-grid points; the larger parameter set on the larger sizes.  ``alt``: the
# frequencies of the spectral misfit -- the same from nt = 5 to nt = 33 and from nt = 31 to nt = 40 (a table kept for the
# shorter shot has zero rows where the longer one needs twiddles), others in between
MISFIT_VARIANTS = (
    dict(nt=40, nsrc=1, nrec=65, taps="long", weights=True, tw=True, big=True),
    dict(nt=5, nsrc=1, nrec=1, alt=True),
    dict(nt=33, nsrc=3, nrec=7, taps="short", tw=True, big=True, alt=True),
    dict(nt=31, nsrc=1, nrec=2, weights=True, off_grid=True),
)
FORWARD_AT = ((40, 3, 7, True), (5, 1, 1, False), (33, 1, 65, True), (31, 1, 2, False))


def _size(nt, nsrc, nrec):
    return nt * max(nsrc, nrec, 1)


def catalogue():
    """{family: tuple of Step}; the same for every configuration (families_of says which of them it runs)"""
    cat = {}

    def sized(family, make):
        cat[family] = tuple(Step(family, v, make(*s), _size(*s)) for v, s in enumerate(SIZES.get(family, SWEEPS)))

    sized("fwd_save", _forward_only(True))
    sized("fwd_nosave", _forward_only(False))
    sized("adj_image", _adjoint(True))
    sized("adj_noimage", _adjoint(False))
    sized("l2", _l2)
    for m in MISFITS:
        cat["misfit_" + m] = tuple(Step("misfit_" + m, v, _misfit(m)(**kw), _size(kw["nt"], kw["nsrc"], kw["nrec"]))
                                   for v, kw in enumerate(MISFIT_VARIANTS))
    cat["forward_at"] = tuple(Step("forward_at", v, _forward_at(*s), _size(*s[:3])) for v, s in enumerate(FORWARD_AT))
    sized("born_exact", _born("exact"))
    sized("born_imaging", _born("imaging"))
    sized("illum", _illum)
    sized("vec", _vec)
    sized("launch", _launch)
    cat["model"] = tuple(Step("model", v, _model(*s), _size(*s), changes_model=True) for v, s in enumerate(SWEEPS))
    cat["refused"] = tuple(Step("refused", v, _refused(which), 0, refused=(code, words))
                           for v, (which, code, words) in enumerate(REFUSALS))
    sized("four_spectral", _four_spectral)
    sized("four_freqs", _four_freqs)
    sized("four_count", _four_count)
    assert set(cat) == set(FAMILIES)
    return cat


# ---------------------------------------------------------------------------------------------------------------------
# sequences
# ---------------------------------------------------------------------------------------------------------------------
def family_circuit(families, seed):
    """A seeded Euler circuit of the complete directed graph with loops over ``families``: len(families)^2 + 1 entries in
    which every ordered pair (a, b), a == b included, is adjacent exactly once (Hierholzer; every vertex has as many
    edges in as out, so the circuit exists)."""
    rnd = random.Random(seed)
    todo = {}
    for a in families:
        nxt = list(families)
        rnd.shuffle(nxt)
        todo[a] = nxt
    stack, walk = [families[rnd.randrange(len(families))]], []
    while stack:
        if todo[stack[-1]]:
            stack.append(todo[stack[-1]].pop())
        else:
            walk.append(stack.pop())
    return walk[::-1]


def sequence(config, seed=SEED):
    """[(Step, model_id in force when it starts)]: the circuit over the configuration's families, each visit of a family
    taking its next variant (so that its sizes go up and down in turn)"""
    cat = catalogue()
    visits, model_id, seq = {}, 0, []
    for fam in family_circuit(families_of(config), "%s/%d" % (config, seed)):
        k = visits.get(fam, 0)
        visits[fam] = k + 1
        step = cat[fam][k % len(cat[fam])]
        seq.append((step, model_id))
        if step.changes_model:
            model_id = 1 - model_id
    return seq


def first_difference(got, ref):
    """Name and description of the first output of ``got`` that is not ``ref``'s bit for bit (NaNs equal nothing: they
    are reported too), or None"""
    if sorted(got) != sorted(ref):
        return "outputs", "%s against %s" % (sorted(got), sorted(ref))
    for name in got:
        a, b = np.asarray(got[name]), np.asarray(ref[name])
        if a.shape != b.shape or a.dtype != b.dtype:
            return name, "shape / dtype %s %s against %s %s" % (a.shape, a.dtype, b.shape, b.dtype)
        if not np.array_equal(a, b):
            bad = np.flatnonzero(~(a.ravel() == b.ravel()))
            at = tuple(int(i) for i in np.unravel_index(bad[0], a.shape)) if a.shape else ()
            return name, "%d of %d entries differ, the first at %s: %r against %r" % (
                bad.size, a.size, at, a.ravel()[bad[0]].item(), b.ravel()[bad[0]].item())
    return None


def check_outputs(step, out):
    """Every output finite; a step that computes something returns something that is not zero."""
    if step.refused:
        assert out == {}, "%r: a refused step returns nothing" % step
        return
    assert out, "%r returned nothing" % step
    for name, v in out.items():
        assert np.all(np.isfinite(np.asarray(v, dtype=np.complex128))), "%r: %s is not finite" % (step, name)
    assert any(np.any(np.asarray(v) != 0) for v in out.values()), "%r returned only zeros: a mistake in the step" % step


# ---------------------------------------------------------------------------------------------------------------------
# the recording stub (tests/test_history_host.py): logs method names, returns zeros of the right shapes, and refuses
# what include/fwi.h says the library refuses among the things the catalogue does
# ---------------------------------------------------------------------------------------------------------------------
class _Names:
    def __getattr__(self, name):
        return name


class StubEngine:
    def __init__(self, P):
        self.P, self.shape, self.dtype, self.calls = P, P.shape, P.dtype, []
        self._lib = _Names()
        self._fourier = P.opts.get("fourier")
        self._nt = self._nsrc = self._nrec = 0
        self._forward = self._stored = self._synthetics = self._residual = False
        self.refusals = 0

    def _refuse(self, code, why):
        self.refusals += 1
        raise FwiError(code, why)

    def _series(self, n):
        return np.zeros((self._nt, n), self.dtype)

    def _field(self):
        return np.zeros(self.shape, self.dtype)

    # sweeps
    def _shot(self, name, nt, nsrc, nrec, save):
        self.calls.append(name)
        self._forward = self._stored = self._synthetics = self._residual = False  # a refused forward leaves no forward
        if nt > NT_MAX:
            self._refuse(1, "nt outside [1, nt_max]")
        self._nt, self._nsrc, self._nrec = nt, nsrc, nrec
        self._forward, self._stored, self._synthetics = True, bool(save), True
        return self._series(nrec)

    def forward(self, model, src, rec, save=True):
        assert model is None
        return self._shot("forward", np.asarray(src[1]).shape[0], len(src[0]), len(rec), save)

    def forward_at(self, model, src, rec, save=True):
        assert model is None
        return self._shot("forward_at", np.asarray(src[1]).shape[0], src[0].n, rec.n, save)

    def _adjoint(self, name, residual, image):
        self.calls.append(name)
        if not self._forward:
            self._refuse(3, "no forward run to adjoin")
        if image and not self._stored:
            self._refuse(3, "imaging needs forward(save)")
        if residual is None:
            assert self._residual or not self._nrec, "adjoint(None) without a residual on the device"
        else:
            assert np.shape(residual) == (self._nt, self._nrec)
        self._synthetics = self._residual = False
        return self._series(self._nsrc)

    def adjoint(self, residual, image=True):
        return self._adjoint("adjoint", residual, image)

    def adjoint_spectral(self, residual=None, freq_weights=None, image=True):
        assert self._fourier is not None and self._stored
        return self._adjoint("adjoint_spectral", residual, False)

    def born(self, dm, wrt="velocity", mode="auto", download=True, operator="exact"):
        self.calls.append("born")
        assert self._forward and self._stored and np.shape(dm) == self.shape
        self._synthetics, self._residual = False, True
        return self._series(self._nrec)

    # misfits
    def _misfit_checks(self, name, d_obs, taps=None, eps=0.0):
        self.calls.append(name)
        if not self._forward:
            self._refuse(3, "no forward run whose data to compare")
        assert np.shape(d_obs) == (self._nt, self._nrec)
        if taps is not None and len(taps) - 1 > FIR_RMAX:
            self._refuse(1, "R outside [0, 4096]")
        if eps < 0:
            self._refuse(1, "eps must be finite and >= 0")
        if not self._synthetics:
            self._refuse(3, "the synthetics of the last forward are gone")
        self._residual = True

    def misfit_l2(self, d_obs):
        self._misfit_checks("misfit_l2", d_obs)
        return 0.0

    def misfit_weighted(self, d_obs, weights=None, taps=None):
        self._misfit_checks("misfit_weighted", d_obs, taps)
        return 0.0

    def misfit_matched(self, d_obs, L, mu, weights=None, taps=None, f=None, normal=False):
        self._misfit_checks("misfit_matched", d_obs, taps)
        return 0.0, np.zeros(2 * L + 1)

    def misfit_envelope(self, d_obs, hilbert, power=1, eps=None, weights=None, taps=None):
        self._misfit_checks("misfit_envelope", d_obs, taps, eps)
        return 0.0

    def misfit_correlation(self, d_obs, eps=None, weights=None, taps=None, trace_weights=None, per_trace=False):
        self._misfit_checks("misfit_correlation", d_obs, taps, eps)
        return (0.0, np.zeros(self._nrec)) if per_trace else 0.0

    def misfit_traveltime(self, d_obs, max_lag, weights=None, taps=None, trace_weights=None, per_trace=False):
        self._misfit_checks("misfit_traveltime", d_obs, taps)
        return (0.0, np.zeros(self._nrec), np.zeros(self._nrec, np.int32)) if per_trace else 0.0

    def misfit_transport(self, d_obs, transform="softplus", param=None, weights=None, taps=None, trace_weights=None,
                         per_trace=False):
        self._misfit_checks("misfit_transport", d_obs, taps)
        assert param > 0
        return (0.0, np.zeros(self._nrec), np.zeros(self._nrec, np.int32)) if per_trace else 0.0

    def misfit_spectral(self, d_obs, freqs, kind="l2", eps=0.0, weights=None, taps=None, freq_weights=None,
                        trace_weights=None, per_pair=False):
        self._misfit_checks("misfit_spectral", d_obs, taps, eps)
        assert kind in _lib.SPEC_KINDS
        z = np.zeros((len(freqs), self._nrec))
        return (0.0, z, z.copy(), z.astype(np.uint8)) if per_pair else 0.0

    def _misfit(self, fn, d_obs, weights, taps, mid=(), outs=()):
        assert fn == "fwi_misfit_spectral"
        self._misfit_checks("misfit_spectral", d_obs, taps, mid[3])
        if mid[2] not in _lib.SPEC_KINDS.values():
            self._refuse(1, "kind is none of FWI_SPEC_*")
        return 0.0

    # everything else: logged, answered with zeros of the right shape
    def gradient(self, wrt="velocity"):
        self.calls.append("gradient")
        return self._field()

    def illumination(self, wrt="velocity"):
        self.calls.append("illumination")
        return self._field()

    def vec_download(self, slot):
        self.calls.append("vec_download")
        return self._field()

    @property
    def fourier_freqs(self):
        return self._fourier

    def set_fourier_store(self, freqs, batch=None):
        self.calls.append("set_fourier_store")
        self._fourier, self._stored = freqs, False

    def fourier_gradient(self, freq_weights=None, wrt="velocity"):
        self.calls.append("fourier_gradient")
        return self._field()

    def fourier_illumination(self, freq_weights=None, wrt="velocity"):
        self.calls.append("fourier_illumination")
        return self._field()

    def _spectrum(self, name):
        self.calls.append(name)
        return np.zeros((len(self._fourier),) + self.shape, np.complex64)

    def fourier_spectrum(self):
        return self._spectrum("fourier_spectrum")

    def fourier_adjoint_spectrum(self):
        return self._spectrum("fourier_adjoint_spectrum")

    def __getattr__(self, name):  # reset_gradient, set_model, set_illumination, set_launch_mode, the vector algebra
        if name.startswith("_"):
            raise AttributeError(name)

        def call(*a, **k):
            self.calls.append(name)
            return 0.0
        return call
