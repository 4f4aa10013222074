#!/usr/bin/env python3
"""Run one of BASELINE.json's inversion configs end to end (shots -> gradient -> L-BFGS).

Single GPU:   python tools/run_config.py --config cfg3 --scale 0.25
Several GPUs: python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 \
                  --master-port P tools/run_config.py --config cfg5 --scale 0.5 --iters 5
Shots are sharded rank::world, the gradient is summed by one RCCL all-reduce per evaluation.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from full_waveform_inversion_amd import Engine, datafit, newton as nw, regularizers as rg, shots as sh, workloads  # noqa: E402
from full_waveform_inversion_amd.lbfgs import lbfgs, lbfgs_device, lbfgs_device_slots  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3", choices=["cfg3", "cfg5"])
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--shots", type=int, default=0, help="0 = the config's own count (32 / 64)")
    ap.add_argument("--iters", type=int, default=0, help="L-BFGS iterations; 0 = one gradient only")
    ap.add_argument("--host-lbfgs", action="store_true", help="keep the optimiser vectors on the host")
    ap.add_argument("--pool", type=int, default=0,
                    help="engines sharing this GPU's shots concurrently; 0 = auto (2 in 2-D, 1 in 3-D)")
    ap.add_argument("--abc", default="sponge", choices=["sponge", "cpml"], help="absorbing border (fwi_config.abc)")
    ap.add_argument("--image-stride", type=int, default=1,
                    help="imaging condition every S-th step (fwi_config.image_stride)")
    ap.add_argument("--fourier-store", default=None, metavar="FMIN,FMAX",
                    help="keep the forward term as its Fourier coefficients on the bins of the sampled time axis inside "
                         "[FMIN, FMAX] Hz (fourier.fourier_bins; at most 64) instead of its history: the gradient of the "
                         "forward term band-passed to them (Engine.set_fourier_store)")
    ap.add_argument("--fourier-batch", type=int, default=8, metavar="B",
                    help="samples per transform launch of --fourier-store, 1 .. 8 (B + 1 ring slots)")
    ap.add_argument("--fourier-imaging", nargs="?", const="plain", default=None, choices=["plain", "whiten"],
                    metavar="whiten",
                    help="with --fourier-store: form the gradient in the frequency domain, per frequency "
                         "(Engine.adjoint_spectral) instead of re-synthesising the forward term; --precondition then takes "
                         "the spectral illumination (Engine.fourier_illumination).  `whiten`: weight the per-frequency "
                         "gradients by 1 / (mean power of the observed data at the frequency + 1e-4 of the largest), scaled "
                         "to mean 1 (datafit.whitening_weights; one rank).  Composes with --spectral and --precondition")
    ap.add_argument("--extended-image", default=None, metavar="offset:AXIS:L | time:DTAU:L",
                    help="with --fourier-store: the extended image of the final model (shots.extended_image), the 2 L + 1 "
                         "lags -L .. L of a subsurface-offset gather along AXIS (z, y or x; lags in cells) or of a time-lag "
                         "gather in steps of DTAU seconds; written to --extended-out with its lags and fourier.focusing")
    ap.add_argument("--extended-out", default=None, metavar="PATH", help="the .npz file of --extended-image (rank 0 writes)")
    ap.add_argument("--angle-gather", default=None, metavar="AXIS:L:NANG:MAXDEG",
                    help="with --fourier-store: the angle-domain common-image gather of the final model "
                         "(shots.angle_gather): the 2 L + 1 subsurface half-offsets -L .. L in cells along AXIS (y or x) "
                         "are summed over the shots on the device and slant-stacked there to NANG angles from -MAXDEG to "
                         "MAXDEG degrees; written to --angle-out with its tangents, its offsets and "
                         "Engine.gather_moment of the offset gather")
    ap.add_argument("--angle-out", default=None, metavar="PATH", help="the .npz file of --angle-gather (rank 0 writes)")
    ap.add_argument("--split-gradient", default=None, metavar="AXIS:R",
                    help="with --fourier-store: the tomographic (same direction) and migration (opposite direction) parts "
                         "of the final model's spectral gradient along AXIS (z, y or x), with datafit.hilbert_taps(R), "
                         "1 <= R <= 64 (shots.split_gradient); neither part is the gradient of the misfit, the "
                         "optimiser never sees them; needs --split-out")
    ap.add_argument("--split-out", default=None, metavar="PATH", help="the .npz file of --split-gradient (rank 0 writes)")
    ap.add_argument("--update-form", default="auto", choices=["auto", "increment", "standard"],
                    help="fp32 update form; auto = shots.inversion_engine's choice (increment: 1e-5 end to end)")
    ap.add_argument("--launch-mode", default="auto", choices=["auto", "stream", "graph"])
    ap.add_argument("--checkpoint", default="", help="optimiser state file, rewritten after every iteration (rank 0 only)")
    ap.add_argument("--resume", default="", help="continue from such a state file (every rank reads it)")
    ap.add_argument("--precondition", nargs="?", type=float, const=sh.ILLUMINATION_EPS, default=None, metavar="EPS",
                    help="L-BFGS with the source-illumination preconditioner p = 1 / (H / max H + EPS), built from the "
                         "first evaluation (default EPS %g); off when absent" % sh.ILLUMINATION_EPS)
    ap.add_argument("--smooth", type=float, default=None, metavar="SIGMA",
                    help="L-BFGS initial inverse Hessian B = M S' D S' M: Gaussian smoothing of width SIGMA cells "
                         "(shots.smoothing_h0_device), D the --precondition diagonal when given; off when absent")
    ap.add_argument("--mute-sources", type=float, default=None, metavar="RADIUS",
                    help="mask M = 1 - exp(-(d / RADIUS)^2) around the source nodes (shots.source_mute), applied inside "
                         "the --smooth operator (SIGMA 0 when --smooth is absent)")
    ap.add_argument("--regularize", default=None, choices=["tikhonov", "tv"],
                    help="add LAMBDA R(m - prior) to the misfit (regularizers.py): first-order Tikhonov or smoothed "
                         "isotropic total variation; off when absent")
    ap.add_argument("--reg-weight", type=float, default=None, metavar="LAMBDA", help="the weight of --regularize")
    ap.add_argument("--reg-eps", type=float, default=None, metavar="EPS",
                    help="smoothing of the total variation, in the model's units per cell (default: 1e-3 max m0)")
    ap.add_argument("--reg-prior", default=None, choices=["start"],
                    help="penalise m - m_start (the starting model, kept in one more vector slot) instead of m")
    ap.add_argument("--bands", default=None, metavar="F1,F2,...",
                    help="frequency continuation (datafit.frequency_continuation): --iters L-BFGS iterations per band on the "
                         "residual low-passed at F1, then F2, ... Hz (datafit.WeightedL2, formed on the device), each band "
                         "from the model of the one before and with a fresh L-BFGS history")
    ap.add_argument("--band-halfwidth", type=int, default=64, metavar="R", help="half-width of the --bands filters in samples")
    ap.add_argument("--mute-direct", type=float, default=None, metavar="V_FAST",
                    help="data weights that mute every trace up to offset / V_FAST + 2 / f0, with a taper of half a period "
                         "(datafit.offset_time_mute)")
    ap.add_argument("--match-source", type=int, default=None, metavar="L",
                    help="matching-filter (source-independent) misfit: per shot a two-sided filter of 2 L + 1 coefficients "
                         "between synthetics and data is estimated and eliminated (datafit.MatchedL2, on the device); "
                         "composes with --bands and --mute-direct")
    ap.add_argument("--match-mu-percent", type=float, default=0.1, metavar="P",
                    help="damping of the filter's normal equations per shot: P / 100 of the energy of the shot's (weighted) "
                         "observed data (datafit.prewhitening), computed once and held through the run")
    ap.add_argument("--envelope", type=int, nargs="?", const=1, default=None, metavar="P", choices=(1, 2),
                    help="envelope misfit against cycle skipping: 1/2 |M . (E(s)^P - E(d)^P)|^2 with E the envelope from an "
                         "FIR Hilbert transformer (datafit.EnvelopeL2, on the device), P = 1 (default) or 2; needs "
                         "--hilbert-fmin; composes with --bands and --mute-direct, not with --match-source")
    ap.add_argument("--hilbert-fmin", type=float, default=None, metavar="F",
                    help="lowest frequency (Hz) at which the Hilbert transformer of --envelope is accurate: sets its "
                         "half-width Q = datafit.hilbert_halfwidth(dt, F)")
    ap.add_argument("--envelope-floor-percent", type=float, default=1.0, metavar="X",
                    help="floor under the envelopes per shot: X / 100 of the largest amplitude of the shot's observed data "
                         "(datafit.envelope_floor), computed once and held through the run")
    ap.add_argument("--correlation", type=float, nargs="?", const=1.0, default=None, metavar="FLOOR_PERCENT",
                    help="trace-normalised correlation misfit, sum over traces of 1 - the zero-lag normalised correlation of "
                         "synthetics and data: phase only, blind to the gain of a trace (datafit.NormalizedCorrelation, on "
                         "the device); the floor under the trace norms per shot is FLOOR_PERCENT / 100 (default 1) of the "
                         "largest trace norm of the shot's observed data (datafit.correlation_floor); composes with --bands "
                         "and --mute-direct, not with --envelope or --match-source")
    ap.add_argument("--traveltime", type=int, default=None, metavar="MAX_LAG",
                    help="cross-correlation traveltime misfit, 1/2 the sum over traces of the squared delay at which the "
                         "correlation of synthetics and data over the lags |k| <= MAX_LAG samples peaks: grows with the "
                         "square of the time shift over any number of periods, blind to the gain of a trace "
                         "(datafit.TraveltimeL2, on the device); composes with --bands and --mute-direct, not with "
                         "--correlation, --envelope or --match-source")
    ap.add_argument("--transport", choices=sorted(datafit.OT_TRANSFORMS), default=None,
                    help="trace-by-trace optimal-transport misfit, 1/2 the sum over traces of the squared 2-Wasserstein "
                         "distance between synthetics and data made positive by the chosen transform and normalised to "
                         "densities along time: uses the whole trace, needs no pick, grows with the square of the time "
                         "shift over any number of periods (datafit.TransportW2, on the device); composes with --bands and "
                         "--mute-direct, not with --traveltime, --correlation, --envelope or --match-source")
    ap.add_argument("--transport-param", type=float, default=None, metavar="X",
                    help="the absolute parameter of --transport: b of softplus, c of linear (default: per shot from its "
                         "observed data, datafit.TransportW2.param_of, computed once and held through the run)")
    ap.add_argument("--adaptive", type=int, default=None, metavar="L",
                    help="adaptive (per-trace matching-filter) misfit, 1/2 the sum over traces of the second moment about "
                         "zero lag of the Wiener filter of 2 L + 1 samples that turns the observed trace into the synthetic "
                         "one, over the filter's energy: keeps amplitude and phase, needs no pick, grows with the square of "
                         "the time shift up to L samples, blind to the gain of a trace; not zero at equal data "
                         "(datafit.AdaptiveMatching, on the device); composes with --bands and --mute-direct, not with the "
                         "other misfits")
    ap.add_argument("--adaptive-ridge", type=float, default=None, metavar="LAM",
                    help="the ridge of --adaptive, relative to the energy of each observed trace (default 1e-2)")
    ap.add_argument("--robust", choices=datafit.ROBUST_KINDS, default=None,
                    help="robust (M-estimator) misfit of the filtered, weighted residual: quadratic up to a threshold per "
                         "trace, linear (huber, hybrid) or logarithmic (cauchy, not convex) beyond it, so that spikes and "
                         "noise bursts do not dominate the gradient (datafit.RobustMisfit, on the device); the threshold is "
                         "--robust-c times the scale of --robust-scale; composes with --bands and --mute-direct, not with "
                         "the other misfits")
    ap.add_argument("--robust-c", type=float, default=None, metavar="C",
                    help="the threshold of --robust in units of the scale (default 1.345 huber, 1.0 hybrid, 2.385 cauchy)")
    ap.add_argument("--robust-scale", default=None, metavar="{trace,gather,VALUE}",
                    help="the scale of --robust: 1.4826 times the median of the absolute residuals per trace (trace, the "
                         "default) or per shot gather (gather), taken ONCE per --bands stage at that stage's starting "
                         "model (shots.residual_scales: one more forward per shot and stage) and held through it, or an "
                         "absolute VALUE in the units of the data")
    ap.add_argument("--spectral", choices=datafit.SPECTRAL_KINDS, default=None,
                    help="frequency-domain misfit on the bins of --spectral-band: 1/2 the sum over frequencies and traces "
                         "of the squared difference of the Fourier coefficients (l2), of their phases (phase), of their "
                         "logarithmic amplitudes (logamp) or of both (log, the logarithmic misfit) "
                         "(datafit.SpectralMisfit, on the device); composes with --bands and --mute-direct, not with the "
                         "other misfits")
    ap.add_argument("--spectral-band", default=None, metavar="FMIN,FMAX",
                    help="the band of --spectral in Hz: the 1 .. 64 bins k / (nt dt) inside it (fourier.fourier_bins); "
                         "without it, with --fourier-store, the bins of the store")
    ap.add_argument("--spectral-floor-percent", type=float, default=1.0, metavar="X",
                    help="floor under the coefficients per shot: X / 100 of the largest coefficient of the shot's (weighted) "
                         "observed data (datafit.spectral_floor), computed once per evaluation from the data alone")
    ap.add_argument("--spectral-whiten", action="store_true",
                    help="frequency weights 1 / (mean power of the observed data at the frequency + 1e-4 of the largest): "
                         "the weak frequencies count like the strong ones (datafit.whitening_weights; one rank)")
    ap.add_argument("--tomography", type=int, default=0, metavar="ITERS",
                    help="before the waveform stages: ITERS L-BFGS iterations of first-arrival traveltime tomography "
                         "(shots.traveltime_fg: eikonal times and their adjoint on the device) from the starting model, "
                         "on picks taken from the eikonal times of the true model; its result starts the waveform "
                         "stages.  Takes the bounds, --smooth and --regularize / --reg-weight / --reg-eps / --reg-prior "
                         "of the run")
    ap.add_argument("--tomography-radius", type=float, default=3.0, metavar="R",
                    help="cells around each source that start at their straight-ray time (eikonal.ball)")
    ap.add_argument("--tomography-reflector", type=float, default=None, metavar="DEPTH_CELLS",
                    help="add the reflection traveltimes off a flat, fixed reflector at that depth (cells along the first "
                         "axis, rounded to the nearest node; shots.reflection_fg) to the --tomography objective, on picks "
                         "taken from the true model's reflection times; every source must lie above it")
    ap.add_argument("--tomography-newton", type=int, default=None, metavar="CG_ITERS",
                    help="the --tomography ITERS iterations are damped Gauss-Newton ones (newton.traveltime_gauss_newton: "
                         "at most CG_ITERS conjugate-gradient products per iteration, each a tangent and an adjoint "
                         "eikonal solve per shot) instead of L-BFGS; --smooth preconditions the inner iteration")
    a = ap.parse_args()
    if a.tomography_reflector is not None and (a.tomography < 1 or a.tomography_newton is not None
                                               or not a.tomography_reflector >= 0.0):
        ap.error("--tomography-reflector DEPTH_CELLS must be >= 0, needs --tomography ITERS and runs under L-BFGS only "
                 "(not with --tomography-newton)")
    if a.tomography_newton is not None and (a.tomography_newton < 1 or a.tomography < 1):
        ap.error("--tomography-newton CG_ITERS must be >= 1 and needs --tomography ITERS")
    if a.tomography < 0 or not (a.tomography_radius >= 0.0 and np.isfinite(a.tomography_radius)):
        ap.error("--tomography ITERS must be >= 0 and --tomography-radius R finite and >= 0")
    bands = [float(f) for f in a.bands.split(",")] if a.bands else None
    if a.spectral is None and (a.spectral_band is not None or a.spectral_whiten):
        ap.error("--spectral-band / --spectral-whiten need --spectral")
    if a.spectral is not None and a.spectral_band is None and a.fourier_store is None:
        ap.error("--spectral needs --spectral-band FMIN,FMAX (or --fourier-store, whose bins it then takes)")
    if not (a.spectral_floor_percent >= 0.0 and np.isfinite(a.spectral_floor_percent)):
        ap.error("--spectral-floor-percent X must be finite and >= 0")
    if a.spectral_whiten and int(os.environ.get("WORLD_SIZE", 1)) > 1:
        ap.error("--spectral-whiten takes its weights from this rank's data: it runs on one rank")
    if a.fourier_imaging is not None and a.fourier_store is None:
        ap.error("--fourier-imaging needs --fourier-store FMIN,FMAX (it images on the store's frequencies)")
    extended = None
    if a.extended_image is not None:
        if a.fourier_store is None:
            ap.error("--extended-image needs --fourier-store FMIN,FMAX (it images on the store's frequencies)")
        if a.extended_out is None:
            ap.error("--extended-image needs --extended-out PATH")
        try:
            kind, step, half = a.extended_image.split(":")
            half = int(half)
            assert kind in ("offset", "time") and half >= 0
            if kind == "offset":
                assert step in ("z", "y", "x")
                extended = ("offset", np.arange(-half, half + 1), step)
            else:
                assert np.isfinite(float(step)) and float(step) > 0
                extended = ("time", float(step) * np.arange(-half, half + 1), None)
        except (ValueError, AssertionError):
            ap.error("--extended-image takes offset:AXIS:L (AXIS z, y or x) or time:DTAU:L (DTAU > 0 seconds), L >= 0")
    elif a.extended_out is not None:
        ap.error("--extended-out needs --extended-image")
    angle = None
    if a.angle_gather is not None:
        if a.fourier_store is None:
            ap.error("--angle-gather needs --fourier-store FMIN,FMAX (it images on the store's frequencies)")
        if a.angle_out is None:
            ap.error("--angle-gather needs --angle-out PATH")
        try:
            axis, half, nang, maxdeg = a.angle_gather.split(":")
            half, nang, maxdeg = int(half), int(nang), float(maxdeg)
            assert axis in ("y", "x") and half >= 0 and nang >= 1 and 0.0 <= maxdeg < 90.0
            assert 2 * half + 1 + nang + 1 <= 256
            angle = (axis, np.arange(-half, half + 1), np.linspace(-maxdeg, maxdeg, nang) if nang > 1 else np.zeros(1))
        except (ValueError, AssertionError):
            ap.error("--angle-gather takes AXIS:L:NANG:MAXDEG (AXIS y or x, L >= 0 cells, NANG >= 1 angles, 0 <= MAXDEG "
                     "< 90 degrees; 2 L + NANG + 2 <= 256 vector slots)")
    elif a.angle_out is not None:
        ap.error("--angle-out needs --angle-gather")
    split = None
    if a.split_gradient is not None:
        if a.fourier_store is None:
            ap.error("--split-gradient needs --fourier-store FMIN,FMAX (it splits the image of the store's frequencies)")
        if a.split_out is None:
            ap.error("--split-gradient needs --split-out PATH")
        try:
            axis, half = a.split_gradient.split(":")
            assert axis in ("z", "y", "x") and 1 <= int(half) <= 64
            split = (axis, int(half))
        except (ValueError, AssertionError):
            ap.error("--split-gradient takes AXIS:R (AXIS z, y or x; 1 <= R <= 64 taps)")
    elif a.split_out is not None:
        ap.error("--split-out needs --split-gradient")
    if a.fourier_imaging == "whiten" and int(os.environ.get("WORLD_SIZE", 1)) > 1:
        ap.error("--fourier-imaging whiten takes its weights from this rank's data: it runs on one rank")
    spectral_band = None
    if a.spectral_band is not None:
        try:
            spectral_band = tuple(float(v) for v in a.spectral_band.split(","))
            assert len(spectral_band) == 2
        except (ValueError, AssertionError):
            ap.error("--spectral-band takes FMIN,FMAX in Hz")
    if bands and (a.iters < 1 or a.checkpoint or a.resume):
        ap.error("--bands needs --iters > 0 and runs without --checkpoint / --resume (one optimiser state per band)")
    if bands and (a.precondition is not None or a.smooth is not None or a.mute_sources is not None
                  or a.regularize is not None or a.host_lbfgs):
        ap.error("--bands runs the plain device L-BFGS per band: it does not combine with --precondition, --smooth, "
                 "--mute-sources, --regularize or --host-lbfgs")
    if a.match_source is not None and not 0 <= a.match_source <= datafit.L_MAX:
        ap.error("--match-source L must lie in [0, %d]" % datafit.L_MAX)
    if not (a.match_mu_percent >= 0.0 and np.isfinite(a.match_mu_percent)):
        ap.error("--match-mu-percent P must be finite and >= 0")
    misfits = [flag for flag in ("--robust", "--adaptive", "--spectral", "--transport", "--traveltime", "--correlation", "--envelope", "--match-source")
               if getattr(a, flag[2:].replace("-", "_")) is not None]
    if len(misfits) > 1:
        ap.error("%s are different misfits: choose one" % " and ".join(misfits))
    if a.transport_param is not None and a.transport is None:
        ap.error("--transport-param needs --transport")
    if a.transport_param is not None and not (a.transport_param > 0.0 and np.isfinite(a.transport_param)):
        ap.error("--transport-param X must be finite and > 0")
    if (a.robust_c is not None or a.robust_scale is not None) and a.robust is None:
        ap.error("--robust-c and --robust-scale need --robust")
    if a.robust_c is not None and not (a.robust_c > 0.0 and np.isfinite(a.robust_c)):
        ap.error("--robust-c C must be finite and > 0")
    robust_scale = a.robust_scale or "trace"
    if robust_scale not in ("trace", "gather"):
        try:
            robust_scale = float(robust_scale)
            assert robust_scale > 0.0 and np.isfinite(robust_scale)
        except (ValueError, AssertionError):
            ap.error("--robust-scale takes trace, gather or a finite VALUE > 0")
    if a.adaptive_ridge is not None and a.adaptive is None:
        ap.error("--adaptive-ridge needs --adaptive")
    if a.adaptive_ridge is not None and not (a.adaptive_ridge > 0.0 and np.isfinite(a.adaptive_ridge)):
        ap.error("--adaptive-ridge LAM must be finite and > 0")
    if a.adaptive is not None and not 1 <= a.adaptive <= datafit.AdaptiveMatching.L_MAX:
        ap.error("--adaptive L must lie in [1, %d] samples" % datafit.AdaptiveMatching.L_MAX)
    if a.traveltime is not None and not 1 <= a.traveltime <= datafit.K_MAX:
        ap.error("--traveltime MAX_LAG must lie in [1, %d] samples" % datafit.K_MAX)
    if a.correlation is not None and not (a.correlation >= 0.0 and np.isfinite(a.correlation)):
        ap.error("--correlation FLOOR_PERCENT must be finite and >= 0")
    if (a.envelope is None) != (a.hilbert_fmin is None):
        ap.error("--envelope and --hilbert-fmin go together")
    if not (a.envelope_floor_percent >= 0.0 and np.isfinite(a.envelope_floor_percent)) or (
            a.envelope == 1 and a.envelope_floor_percent == 0.0):
        ap.error("--envelope-floor-percent X must be finite and >= 0, and > 0 with --envelope 1")
    if (a.regularize is None) != (a.reg_weight is None):
        ap.error("--regularize and --reg-weight go together")
    if a.regularize is None and (a.reg_eps is not None or a.reg_prior is not None):
        ap.error("--reg-eps / --reg-prior need --regularize")
    rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    local = int(os.environ.get("LOCAL_RANK", 0))
    from full_waveform_inversion_amd import _lib as _fl
    ndev = _fl.device_count()  # a launcher may have narrowed this process to one visible GPU
    if ndev > 0:
        local %= ndev
    kw = {"nshots": a.shots} if a.shots else {}
    w = workloads.CONFIGS[a.config](a.scale, **kw)
    hilbert = None
    if a.envelope is not None:
        try:
            hilbert = datafit.hilbert_taps(datafit.hilbert_halfwidth(w.dt, a.hilbert_fmin))
        except ValueError as err:
            ap.error("--hilbert-fmin: %s" % err)
    wav = w.wavelet()
    shots = [sh.Shot(w.src_idx[i:i + 1], wav, w.rec_idx) for i in range(len(w.src_idx))]
    psize = a.pool or ((3 if a.abc == "cpml" else 2) if w.ndim == 2 else 1)  # (measured: shots.EnginePool)
    from full_waveform_inversion_amd import default_sigma_max
    sigma = default_sigma_max(float(w.c.max()), w.h, w.npml)
    uf = {} if a.update_form == "auto" else {"update_form": a.update_form}
    if a.fourier_store is not None:
        from full_waveform_inversion_amd import fourier
        try:
            fmin, fmax = (float(v) for v in a.fourier_store.split(","))
        except ValueError:
            ap.error("--fourier-store takes FMIN,FMAX in Hz")
        bins = fourier.fourier_bins(w.nt, w.dt, a.image_stride, fmin, fmax)
        if not 1 <= bins.size <= 64:
            ap.error("--fourier-store: [%g, %g] Hz holds %d bins of the sampled time axis (1 .. 64 allowed; the bins "
                     "lie 1 / (nt dt) apart)" % (fmin, fmax, bins.size))
        uf.update(fourier=bins, fourier_batch=a.fourier_batch)
    spectral_freqs = None
    if a.spectral is not None:
        from full_waveform_inversion_amd import fourier
        spectral_freqs = uf["fourier"] if spectral_band is None else fourier.fourier_bins(w.nt, w.dt, 1, *spectral_band)
        if not 1 <= spectral_freqs.size <= 64:
            ap.error("--spectral-band: the band holds %d bins of the time axis (1 .. 64 allowed; the bins lie 1 / (nt dt) "
                     "apart)" % spectral_freqs.size)
        try:
            datafit.SpectralMisfit(w.dt, spectral_freqs, a.spectral)
        except ValueError as err:
            ap.error("--spectral %s: %s" % (a.spectral, err))
    pool = sh.EnginePool(lambda: sh.inversion_engine(w.shape, w.h, w.dt, w.nt, order=w.order, npml=w.npml, device=local,
                                                     sigma_max=sigma, image_stride=a.image_stride, abc=a.abc,
                                                     launch_mode=a.launch_mode, **uf,
                                                     pml_alpha_max=(3.14159 * w.f0 if a.abc == "cpml" else 0.0)), psize)
    e = pool.primary
    ex = sh.NoExchange()
    rdzv = None
    # FWI_RUN_FORCE_EXCHANGE=1: take the N > 1 path (rendezvous, RCCL communicator, all-reduce per evaluation) with one
    # rank too -- how a one-GPU box rehearses what the driver's launch line does for N = 2, 4, 8
    if world > 1 or os.environ.get("FWI_RUN_FORCE_EXCHANGE") == "1":
        # control plane: the package's stdlib rendezvous on MASTER_ADDR / MASTER_PORT (no torch in this process)
        from full_waveform_inversion_amd.rendezvous import Rendezvous
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if os.environ.get("MASTER_ADDR", "127.0.0.1") in ("127.0.0.1", "localhost"):
            os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")
        rdzv = Rendezvous.from_env()
        e.set_model(w.c.astype(np.float32))
        ex = sh.RcclExchange(e, rdzv)  # raises on every rank if any rank's communicator fails
    sh.model_data(pool, w.c.astype(np.float32), shots, ex)
    if a.mute_direct is not None:
        for s in shots:
            if s.d_obs is not None:
                s.weights = datafit.offset_time_mute(s, w.h, w.dt, a.mute_direct, 2.0 / w.f0, int(0.5 / (w.f0 * w.dt)))
    # the misfit of the stage that is running: least squares, or its band-limited / weighted form
    match_mu = None
    if a.match_source is not None:  # data-only numbers, fixed for the run (indexed like `shots`; 0 where a rank has no data)
        match_mu = [datafit.prewhitening(s.d_obs, s.weights, a.match_mu_percent) if s.d_obs is not None else 0.0
                    for s in shots]

    spectral_fw = None
    if a.spectral_whiten:  # data-only numbers, fixed for the run: the mean power over this rank's shots
        power = [1.0 / datafit.whitening_weights(s.d_obs, w.dt, spectral_freqs, 0.0) for s in shots if s.d_obs is not None]
        power = np.mean(power, axis=0)
        spectral_fw = 1.0 / (power + 1e-4 * float(power.max()))

    # spectral imaging: the keywords every evaluation below hands to the shot loop
    imaging = {}
    if a.fourier_imaging is not None:
        imaging = {"spectral_imaging": True}
        if a.fourier_imaging == "whiten":  # data-only numbers, fixed for the run: the mean power over this rank's shots
            power = [1.0 / datafit.whitening_weights(s.d_obs, w.dt, uf["fourier"], 0.0) for s in shots if s.d_obs is not None]
            power = np.mean(power, axis=0)
            fw = 1.0 / (power + 1e-4 * float(power.max()))
            imaging["freq_weights"] = fw / float(fw.mean())

    m0 = w.c_init.astype(np.float32)
    tomo = None
    if a.tomography > 0:  # traveltime tomography first: the model it ends at starts the waveform stages
        n_local = len(sh.partition_shots(len(shots), ex.rank, ex.world))  # "solves" below counts this rank's
        per_engine = -(-n_local // len(pool.engines))
        for eng in pool.engines:  # the Gauss-Newton operator keeps every local shot's times in a slot of its own
            eng.vec_create(sh.TRAVELTIME_SLOTS + (sh.REFLECTION_SLOTS if a.tomography_reflector is not None else 0)
                           if a.tomography_newton is None else
                           max(sh.TRAVELTIME_SLOTS, sh.TraveltimeOperator.WORK_SLOTS + max(1, per_engine)))
        picks = sh.traveltime_times(pool, w.c.astype(np.float32), shots, a.tomography_radius, 0, ex)
        reflector = refl_picks = None
        if a.tomography_reflector is not None:  # the reflection's slots follow the first arrivals'
            reflector = sh.Reflector.at_depth(w.shape, a.tomography_reflector)
            refl_picks = sh.reflection_times(pool, w.c.astype(np.float32), shots, reflector, a.tomography_radius,
                                             sh.TRAVELTIME_SLOTS, ex)
        tomo_J = []

        def fg_tomo(m):
            J, g = sh.traveltime_fg(pool, np.asarray(m, np.float32), shots, picks, None, a.tomography_radius, 0, ex)
            if reflector is not None:
                Jr, gr = sh.reflection_fg(pool, np.asarray(m, np.float32), shots, refl_picks, reflector, None,
                                          a.tomography_radius, sh.TRAVELTIME_SLOTS, ex)
                J, g = J + Jr, g + gr
            tomo_J.append(J)
            return J, g
        if a.regularize is not None:
            fg_tomo = rg.regularized_fg(fg_tomo, a.reg_weight, a.regularize, 1.0,
                                        (a.reg_eps if a.reg_eps is not None else 1e-3 * float(m0.max()))
                                        if a.regularize == "tv" else None, m0 if a.reg_prior == "start" else None)
        tomo_bounds = (0.5 * float(w.c.min()), 1.5 * float(w.c.max()))
        tomo_h0 = sh.smoothing_h0(a.smooth) if a.smooth is not None else None
        if a.tomography_newton is None:
            m_tomo, _, tomo_log = lbfgs(fg_tomo, m0.astype(np.float64), maxiter=a.tomography, history=5,
                                        first_step=0.02 * float(m0.max()), bounds=tomo_bounds, h0=tomo_h0)
            tomo = {"solver": "lbfgs", "iters": a.tomography, "radius": a.tomography_radius,
                    "evaluations": len(tomo_J), "J": [float(l["f"]) for l in tomo_log],
                    "solves": {"eikonal": len(tomo_J) * n_local, "tangent": 0, "adjoint": len(tomo_J) * n_local}}
            if reflector is not None:  # two more solves of either kind per shot and evaluation
                tomo["reflector"] = {"depth_cells": a.tomography_reflector, "interface_nodes": int(reflector.gamma.sum())}
                tomo["solves"] = {"eikonal": 3 * len(tomo_J) * n_local, "tangent": 0, "adjoint": 3 * len(tomo_J) * n_local}
        else:
            reg = None if a.regularize is None else rg.Regularizer(
                a.reg_weight, a.regularize, 1.0,
                (a.reg_eps if a.reg_eps is not None else 1e-3 * float(m0.max())) if a.regularize == "tv" else None,
                m0 if a.reg_prior == "start" else None)
            m_tomo, tomo_log = nw.traveltime_gauss_newton(pool, m0.astype(np.float64), shots, picks, None, a.tomography,
                                                          a.tomography_newton, bounds=tomo_bounds,
                                                          radius=a.tomography_radius, exchange=ex, regularizer=reg,
                                                          precond=tomo_h0)
            tomo = {"solver": "gauss-newton", "iters": a.tomography, "cg_iters": a.tomography_newton,
                    "radius": a.tomography_radius, "J": [float(l["J"]) for l in tomo_log],
                    "solves": {k: int(sum(l["solves"][k] for l in tomo_log)) for k in ("eikonal", "tangent", "adjoint")}}
        m0 = np.asarray(m_tomo, np.float32)
        for eng in pool.engines:
            eng.vec_create(0)
    robust_stages = []  # per stage of --robust: the band and every shot's scale(s), as measured at its starting model

    def objective_of(taps, model=m0, band=None):
        """the misfit of one stage: a fresh object per band (a MatchedL2 keeps the shots' filters of ITS band, a
        RobustMisfit the scales measured at ``model``, the stage's starting model)"""
        if a.robust is not None:
            scale = robust_scale
            if not isinstance(scale, float):
                scale = sh.residual_scales(pool, np.asarray(model, np.float32), shots,
                                           datafit.RobustMisfit(a.robust, a.robust_c, 1.0, taps), scale == "trace", ex)
                robust_stages.append({"band_hz": band, "scales": [np.round(np.atleast_1d(v), 9).tolist() for v in scale]})
            return datafit.RobustMisfit(a.robust, a.robust_c, scale, taps)
        if a.spectral is not None:  # (the floor: a data-only number per shot, datafit.spectral_floor of its d_obs)
            return datafit.SpectralMisfit(w.dt, spectral_freqs, a.spectral, None, taps, freq_weights=spectral_fw,
                                          floor_percent=a.spectral_floor_percent)
        if a.match_source is not None:
            return datafit.MatchedL2(a.match_source, match_mu, taps)
        if a.envelope is not None:  # (the floor: a data-only number per shot, datafit.envelope_floor of its d_obs)
            return datafit.EnvelopeL2(hilbert, a.envelope, None, taps, floor_percent=a.envelope_floor_percent)
        if a.correlation is not None:  # (the floor: a data-only number per shot, datafit.correlation_floor of its d_obs)
            return datafit.NormalizedCorrelation(None, taps, floor_percent=a.correlation)
        if a.traveltime is not None:
            return datafit.TraveltimeL2(w.dt, a.traveltime, taps)
        if a.transport is not None:  # (the parameter: given, or a data-only number per shot, param_of of its d_obs)
            return datafit.TransportW2(w.dt, a.transport, a.transport_param, taps)
        if a.adaptive is not None:
            return datafit.AdaptiveMatching(w.dt, a.adaptive, 1e-2 if a.adaptive_ridge is None else a.adaptive_ridge, taps)
        return datafit.WeightedL2(taps) if (taps is not None or a.mute_direct is not None) else None

    def filters_line(o, band=None):
        """per shot of this rank, the share of the filter's energy outside lag 0: 0 = a pure scaling of the wavelet"""
        if not isinstance(o, datafit.MatchedL2):
            return
        out = {i: float(1.0 - f[o.L] ** 2 / max(float(np.sum(f * f)), 1e-300)) for i, f in sorted(o.filters.items())}
        print(json.dumps({"rank": rank, "band_hz": band, "match_filter_energy_outside_lag0": out}), flush=True)

    obj = [None if (bands and a.robust is not None) else objective_of(None)]  # (--bands measures per stage)
    t0 = time.perf_counter()
    evals = [0]

    def fg(m):
        evals[0] += 1
        return sh.misfit_and_gradient(pool, m, shots, ex, objective=obj[0], **imaging)

    eps = a.precondition
    first_H = []

    def fg_host(m):  # with --precondition: the first evaluation also returns the illumination
        if eps is None or first_H:
            return fg(m)
        evals[0] += 1
        J, g, H = sh.misfit_and_gradient(pool, m, shots, ex, objective=obj[0], illumination=True, **imaging)
        first_H.append(H)
        return J, g

    ckpt = a.checkpoint if (a.checkpoint and rank == 0) else None  # every rank holds the same state: one writer
    bounds = (0.5 * float(w.c.min()), 1.5 * float(w.c.max()))
    reg_eps = None
    if a.regularize == "tv":
        reg_eps = a.reg_eps if a.reg_eps is not None else 1e-3 * float(m0.max())
    # the prior is the starting model of the RUN: a resumed run builds the same m0 again
    reg_prior = m0 if a.reg_prior == "start" else None
    use_h0 = a.smooth is not None or a.mute_sources is not None
    h0_sigma = a.smooth if a.smooth is not None else 0.0
    mute = sh.source_mute(w.shape, shots, a.mute_sources) if a.mute_sources is not None else None
    if bands:
        def run_band(x, f_hz):  # the device L-BFGS, started afresh: curvature pairs of another band are invalid
            obj[0] = objective_of(datafit.lowpass_taps(w.dt, f_hz, a.band_halfwidth), x, f_hz)

            def fg_band(xs, gs):
                evals[0] += 1
                return sh.misfit_and_gradient_device(pool, xs, gs, shots, ex, objective=obj[0], **imaging)
            x, _, lg = lbfgs_device(e, fg_band, x, maxiter=a.iters, history=5, first_step=0.02 * float(m0.max()),
                                    bounds=bounds)
            filters_line(obj[0], f_hz)
            return x, lg
        m_final, logs = datafit.frequency_continuation(run_band, m0, bands)  # (the band itself is handed on: no taps_of)
        log = [{"band_hz": f, "log": lg} for f, lg in zip(bands, logs)]
    elif a.iters > 0 and not a.host_lbfgs:
        pslot = lbfgs_device_slots(5) if eps is not None else None
        h0 = sh.smoothing_h0_device(pool, h0_sigma, mask=mute, precond_slot=pslot) if use_h0 else None
        fg_p = (sh.preconditioned_fg_device(pool, shots, pslot, eps, ex, objective=obj[0], **imaging)
                if eps is not None else None)

        def fg_dev(xs, gs):
            evals[0] += 1
            if fg_p is not None:
                return fg_p(xs, gs)
            return sh.misfit_and_gradient_device(pool, xs, gs, shots, ex, objective=obj[0], **imaging)
        extra = 0
        if a.regularize is not None:
            xs0 = rg.prior_slot(5, pslot, h0) if reg_prior is not None else None
            extra = 0 if xs0 is None else 1
            fg_dev = rg.regularized_fg_device(pool, fg_dev, a.reg_weight, a.regularize, 1.0, reg_eps, xs0, reg_prior)
        m_final, _, log = lbfgs_device(e, fg_dev, m0, maxiter=a.iters, history=5, first_step=0.02 * float(m0.max()),
                                 bounds=bounds, checkpoint=ckpt, resume=a.resume or None, precond_slot=pslot, h0=h0,
                                 extra_slots=extra)
    elif a.iters > 0:
        pc = (lambda x, f, g: sh.illumination_preconditioner(first_H[0], eps)) if eps is not None else None
        held = {}

        def pc_keep(x, f, g):  # the optimiser builds p once (or restores it on resume); the h0 below reads it
            held["p"] = pc(x, f, g)
            return held["p"]

        def p_of_run():
            if "p" not in held:  # resumed: the optimiser took p from the state file
                from full_waveform_inversion_amd.lbfgs import load_state
                held["p"] = load_state(a.resume)["precond"]
            return held["p"]
        h0 = sh.smoothing_h0(h0_sigma, mask=mute, precond=p_of_run if eps is not None else None) if use_h0 else None
        if a.regularize is not None:
            fg_host = rg.regularized_fg(fg_host, a.reg_weight, a.regularize, 1.0, reg_eps, reg_prior)
        m_final, _, log = lbfgs(fg_host, m0, maxiter=a.iters, history=5, first_step=0.02 * float(m0.max()),
                          bounds=bounds, dot=e.dot, checkpoint=ckpt, resume=a.resume or None,
                          precond=pc_keep if pc is not None else None, h0=h0)
    else:
        fg1 = fg if a.regularize is None else rg.regularized_fg(fg, a.reg_weight, a.regularize, 1.0, reg_eps, reg_prior)
        J, g = fg1(m0)
        m_final = m0
        log = [{"iter": 0, "f": J, "gnorm": float(np.sqrt(e.dot(g, g)))}]
    el = time.perf_counter() - t0
    if extended is not None:  # the gather of the final model, with the misfit and the weights of the last stage
        from full_waveform_inversion_amd import fourier
        kind, lags, axis = extended
        _, E = sh.extended_image(pool, np.asarray(m_final, np.float32), shots, kind, lags, axis, ex, obj[0],
                                 imaging.get("freq_weights"))
        if rank == 0:
            np.savez(a.extended_out, gather=E, lags=lags, kind=kind, axis="" if axis is None else axis,
                     focusing=fourier.focusing(E, lags))
    if angle is not None:  # the angle gather of the final model, with the misfit and the weights of the last stage
        from full_waveform_inversion_amd import fourier
        axis, offsets, degrees = angle
        tangents = fourier.tangents(degrees)
        for eng in pool.engines:  # the optimiser is done with its vectors: vec_create frees them
            eng.vec_create(offsets.size + tangents.size + 1)
        _, A, E = sh.angle_gather(pool, np.asarray(m_final, np.float32), shots, axis, offsets, tangents, 0, ex, obj[0],
                                  imaging.get("freq_weights"), return_offsets=True)
        for l in range(offsets.size):  # the summed offset gather, in the primary engine's lag slots
            e.vec_upload(l, E[l].astype(e.dtype))
        moment = e.gather_moment(range(offsets.size), offsets)
        if rank == 0:
            np.savez(a.angle_out, gather=A, tangents=tangents, degrees=degrees, offsets=offsets, axis=axis,
                     gather_moment=np.array(moment))
    if split is not None:  # both parts of the final model's gradient, with the misfit and the weights of the last stage
        from full_waveform_inversion_amd import datafit as df
        axis, half = split
        J, g_same, g_opposite = sh.split_gradient(pool, np.asarray(m_final, np.float32), shots, axis, df.hilbert_taps(half),
                                                  ex, obj[0], imaging.get("freq_weights"))
        if rank == 0:
            np.savez(a.split_out, same=g_same, opposite=g_opposite, axis=axis, halfwidth=half, misfit=J)
    if not bands:
        filters_line(obj[0])
    if rank == 0:
        upd = 2 * evals[0] * len(shots) * w.updates_per_shot  # forward + adjoint sweeps
        print(json.dumps({"config": w.name, "shape": list(w.shape), "nt": w.nt, "shots": len(shots),
                          "n_gpus": world, "rccl_ranks": getattr(ex, "rccl_ranks", None), "engines_per_gpu": psize, "evaluations": evals[0], "seconds": round(el, 3),
                          "Gpts_per_s_fwd_plus_adj": round(upd / el / 1e9, 2), "kernel": e.kernel_name,
                          "update_form": e.update_form, "abc": a.abc, "launch_mode": a.launch_mode,
                          "precondition_eps": eps, "smooth_sigma": a.smooth,
                          "mute_sources_radius": a.mute_sources, "regularize": a.regularize,
                          "reg_weight": a.reg_weight, "reg_eps": reg_eps, "reg_prior": a.reg_prior, "bands_hz": bands,
                          "band_halfwidth": a.band_halfwidth if bands else None, "mute_direct": a.mute_direct,
                          "match_source": a.match_source, "correlation_floor_percent": a.correlation,
                          "traveltime_max_lag": a.traveltime, "spectral": a.spectral,
                          "spectral_freqs_hz": None if spectral_freqs is None else [float(f) for f in spectral_freqs],
                          "spectral_floor_percent": a.spectral_floor_percent if a.spectral is not None else None,
                          "spectral_whiten": a.spectral_whiten, "fourier_imaging": a.fourier_imaging,
                          "transport": a.transport, "transport_param": a.transport_param,
                          "adaptive_L": a.adaptive, "adaptive_ridge": a.adaptive_ridge,
                          "robust": a.robust,
                          "robust_c": (a.robust_c or datafit.ROBUST_C[a.robust]) if a.robust is not None else None,
                          "robust_scale": a.robust_scale or "trace" if a.robust is not None else None,
                          "robust_scales": robust_stages if a.robust is not None else None,
                          "envelope": a.envelope, "hilbert_fmin": a.hilbert_fmin,
                          "hilbert_halfwidth": len(hilbert) if hilbert is not None else None,
                          "envelope_floor_percent": a.envelope_floor_percent if a.envelope is not None else None,
                          "match_mu_percent": a.match_mu_percent if a.match_source is not None else None,
                          "tomography": tomo, "log": log}))
    pool.close()
    if rdzv is not None:
        rdzv.barrier()
        rdzv.close()


if __name__ == "__main__":
    main()
