"""What the GPU tests of the spectral misfit share (tests/test_gpu_spectral.py): the problem, the inputs
of a case, the conditions asserted on the twin's values and the rounding model that bounds device against twin.  Nothing
here needs a GPU: tests/test_spectral_host.py runs the conditions and the bounds on the twin alone.

The rounding model.  u = 2^-53, R' = 2 R + 1 with taps and 0 without.  Hats are majorants formed from absolute values of
taps and data: shat = M |B| |s|, dhat = M |B| |d|, Shat_j = sum_n shat[n,j] (|cos|, |sin| <= 1), Ohat_j likewise.  Device
and twin each compute, in fp64 and in their own order, s' = B s (R' products), sh = M s' (one), the product with a
twiddle that is itself within one rounding of the exact one (two), and an nt-term sum: each of Re S, Im S is within
(nt + R' + 3) u Shat of the exact value.  The issue states the model as sums of nt + 2 R' terms; that count is the one
used, E = (nt + 2 R' + 4) 2^-52 for the difference of the two, and
  eS = E Shat,  eO = E Ohat            per component;   dS = sqrt(2) eS, dO = sqrt(2) eO as complex numbers.
fp32 with taps: B s and B d are rounded to fp32 and a rounding boundary may fall differently in the twin, one fp32
rounding of every sample: E + 2^-23 in the place of E (as in test_gpu_correlation.py).  To first order in u:
  L2      D = S - O:  dD = dS + dO;   term 1/2 w |D|^2:  w |D| dD + 6 u term;          G = w D:  w dD + 4 u |G|
  LOGAMP  q = |S|^2 + eps^2, p = |O|^2 + eps^2:  da = |S| dS / q + |O| dO / p + 4 u (1 + |a|)   (squares, sum, quotient,
          logarithm);   term 1/2 w a^2:  w |a| da + 4 u term;   G = w a S / q:  w (da |S| / q + 3 |a| dS / q) + 4 u |G|
          (|d(S / q)| <= dS / q + 2 |S|^2 dS / q^2 <= 3 dS / q)
  PHASE   dphi = dS / |S| + dO / |O| + 8 u   (the angle of a complex number moves by at most its relative perturbation;
          the two products, the difference and atan2 add roundings relative to |S| |O| and to pi);
          term 1/2 w phi^2:  w |phi| dphi + 4 u term;   G = w phi i S / |S|^2:  w (dphi / |S| + |phi| dS / |S|^2) + 4 u |G|
          (|d(S / |S|^2)| = dS / |S|^2: it is 1 / conj S)
  LOG     the sums of both.
J adds F ntr terms, the device in the fixed order of launch_sum_partials and NumPy pairwise: F ntr 2^-52 sum |terms| more.
The source g = M sum_k (Re G cos - Im G sin) is a sum of 2 F products, then M and, with taps, B:
  |dr| <= |B| (M sum_k sqrt(2) dG_kj + (2 F + R' + 4) 2^-52 M sum_k sqrt(2) |G_kj|) =: rerr
and the gradient, which is linear in r, is checked to GRAD_TOL of test_gpu_datafit.py (168 roundings of the dtype, which
also covers the one rounding of g to the dtype) plus 4 |rerr| / |r_t|, the share of the source, with the factor 4 of
test_gpu_correlation.py.

The conditions, asserted on the twin's values and not assumed: every counted pair has |phi| <= pi - 0.2, |S|^2 and |O|^2
lie outside [eps^2 / 4, 4 eps^2] (fp32 and fp64 then fall on the same side of the counting rule), and every pair counts
unless the case names dead traces, where exactly those traces' F pairs do not."""
import numpy as np

from full_waveform_inversion_amd import datafit as df, fourier
from oracle import fwi_oracle as fo

SHAPE, H, ORDER, NPML = (40, 48), 10.0, 4, 4
SEG = 256  # SPEC_SEG of csrc/fwi_spec.h: the rows of one time segment of the analysis
NT = 70
NT_MAX = 2 * SEG + 5
SRC = (20, 24)
TAPS_R = 7
U2 = 2.0 ** -52
GRAD_TOL = {"float32": 1e-5, "float64": 1e-5 * 2.0 ** -29}  # 168 roundings of the dtype (test_gpu_datafit.py)
KINDS = ("l2", "phase", "logamp", "log")
SIZES = [(NT, n) for n in (1, 5, 63, 65, 130)] + [(SEG - 1, 65), (SEG, 65), (SEG + 1, 130), (2 * SEG + 5, 65)]
FS = (1, 3, 8, 9, 64)
FLAGS = [(m, b, fw, tw) for m in (False, True) for b in (False, True) for fw in (False, True) for tw in (False, True)]


def models(shape=SHAPE, seed=0):
    rng = np.random.default_rng(seed)
    return 2000.0 + 300.0 * rng.random(shape), np.full(shape, 2150.0)


def dt_of(shape=SHAPE, order=ORDER):
    return 0.6 * fo.cfl_dt(2300.0, H, len(shape), order)


def receivers(ntr, shape=SHAPE, src=SRC, seed=1, rmin=2.0, rmax=8.5):
    """ntr distinct nodes between rmin and rmax cells from the source: the wave has passed all of them well within 70
    steps, so that no spectrum is that of a trace the wave has not reached"""
    grids = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    nodes = np.stack([g.ravel() for g in grids], 1)
    r = np.sqrt(np.sum((nodes - np.asarray(src)) ** 2, axis=1))
    nodes = nodes[(r >= rmin) & (r <= rmax)]
    assert len(nodes) >= ntr
    return np.ascontiguousarray(nodes[np.random.default_rng(seed).permutation(len(nodes))[:ntr]], dtype=np.int32)


def weights(nt, ntr, seed=2):
    """per-sample weights in [0.2, 1]: a gain per trace, a slow swell along time and a jitter of 10 % per sample, with
    one dead time row ahead of the arrivals and no dead trace: every pair is to count.  (White weights, or a dead row
    under the peak of a trace, put notches into the spectra and turn phases by more than the conditions allow.)"""
    rng = np.random.default_rng(seed)
    n = np.arange(nt)[:, None]
    M = (0.5 + 0.5 * rng.random(ntr))[None, :] * (0.75 + 0.25 * np.sin(2.0 * np.pi * (n / nt + rng.random(ntr)[None, :])))
    M = M * (0.9 + 0.1 * rng.random((nt, ntr)))
    M[nt // 8] = 0.0
    return M


def trace_weights(ntr, seed=4):
    w = 0.25 + np.random.default_rng(seed).random(ntr)
    if ntr > 1:
        w[ntr // 3] = 0.0  # one trace that adds nothing (its pairs still count)
    return w


def freq_weights(F, seed=5):
    return 0.25 + np.random.default_rng(seed).random(F)


def freqs(nt, dt, F, fmin=20.0, fmax=70.0):
    """F distinct frequencies inside the band of the 60 Hz wavelet: evenly spaced and therefore off the bins, every third
    one moved onto the nearest bin where that bin is not taken yet"""
    f = np.array([0.5 * (fmin + fmax)]) if F == 1 else np.linspace(fmin, fmax, F)
    bins = fourier.fourier_bins(nt, dt, 1, fmin, fmax)
    for i in range(0, F, 3):
        b = bins[np.argmin(np.abs(bins - f[i]))] if len(bins) else f[i]
        if not np.any(np.delete(f, i) == b):
            f[i] = b
    assert np.unique(f).size == F
    return f


def cases():
    """a selection over sizes x kinds x F x (weights, taps, fw, tw), not the full product: every size with every kind,
    every F with every kind that takes it (F = 64: L2 and LOGAMP only), every flag on and off with every kind"""
    out = []
    for i, size in enumerate(SIZES):
        for q, kind in enumerate(KINDS):
            F = FS[(i + q) % len(FS)]
            if F == 64 and kind in ("phase", "log"):
                F = 9
            out.append((size, kind, F, FLAGS[(3 * i + 5 * q + 1) % len(FLAGS)]))
    for q, kind in enumerate(KINDS):  # all on and all off at the widest gather, the maximum of F where it is allowed
        out.append(((NT, 130), kind, 64 if kind in ("l2", "logamp") else 8, FLAGS[-1]))
        out.append(((SEG + 1, 130), kind, 9, FLAGS[0]))
    return out


def case_id(case):
    (nt, ntr), kind, F, flags = case
    return "nt%d_ntr%d_%s_F%d_%s" % (nt, ntr, kind, F, "".join(c if f else "-" for c, f in zip("MBfw", flags)))


def inputs(dtype, nt, ntr, F, flags, dt):
    """(M, taps, fw, tw, freqs) of a case"""
    weighted, with_taps, fweighted, tweighted = flags
    M = weights(nt, ntr).astype(dtype) if weighted else None
    taps = df.bandpass_taps(dt, 8.0, 150.0, TAPS_R) if with_taps else None
    return (M, taps, freq_weights(F) if fweighted else None, trace_weights(ntr) if tweighted else None,
            freqs(nt, dt, F))


def floor_of(d_obs, dt, f, M):
    """the floor of the cases: 0.02 % of the largest observed coefficient (data only)"""
    return df.spectral_floor(d_obs, dt, f, 0.02, M)


def check_conditions(obj, eps, dead=()):
    """the conditions of the module's docstring on the last call of the twin `obj`; prints what it found"""
    S, O = obj.spectra
    s2, o2 = np.abs(S) ** 2, np.abs(O) ** 2
    e2 = eps * eps
    live = np.ones(S.shape[1], bool)
    live[list(dead)] = False
    both = (s2 > e2) & (o2 > e2)
    phimax = float(np.abs(obj.phases[:, live]).max()) if live.any() else 0.0
    print("conditions: max |phi| %.3f, min |S|^2 / eps^2 %.3g, min |O|^2 / eps^2 %.3g"
          % (phimax, s2[:, live].min() / e2 if e2 else np.inf, o2[:, live].min() / e2 if e2 else np.inf))
    assert phimax <= np.pi - 0.2
    for x in (s2, o2):
        assert not np.any((x >= e2 / 4.0) & (x <= 4.0 * e2) & (x > 0.0)) and (e2 > 0.0 or np.all(x[:, live] > 0.0))
    assert both[:, live].all() and not both[:, ~live].any()
    if obj.kind in ("phase", "log"):
        assert np.array_equal(obj.counts, both)
    else:
        assert obj.counts.all()


def bounds(obj, d_syn, d_obs, M, tw, eps, dtype):
    """The rounding model of the module's docstring at the twin's values (the last call of `obj`):
    (J bound, phi bound (F, ntr), a bound (F, ntr), |rerr|)"""
    nt, ntr = np.shape(d_syn)
    F = obj.freqs.size
    taps = obj.taps
    Re = 2 * (len(taps) - 1) + 1 if taps is not None else 0
    ab = None if taps is None else np.abs(taps)
    Mw = np.ones((nt, ntr)) if M is None else np.asarray(M, np.float64)
    fw = np.ones(F) if obj.freq_weights is None else obj.freq_weights
    w = fw[:, None] * (np.ones(ntr) if tw is None else np.asarray(tw, np.float64))[None, :]
    E = (nt + 2 * Re + 4) * U2 + (2.0 ** -23 if (taps is not None and np.dtype(dtype) == np.float32) else 0.0)
    Shat = np.sum(Mw * df.fir_time(np.abs(d_syn), ab), axis=0)[None, :]
    Ohat = np.sum(Mw * df.fir_time(np.abs(d_obs), ab), axis=0)[None, :]
    dS, dO = np.sqrt(2.0) * E * Shat, np.sqrt(2.0) * E * Ohat
    S, O = obj.spectra
    aS, aO = np.abs(S), np.abs(O)
    e2 = eps * eps
    u = 0.5 * U2
    both = (aS ** 2 > e2) & (aO ** 2 > e2)
    one = np.ones_like(aS)
    q, p = np.where(aS ** 2 + e2 > 0, aS ** 2 + e2, one), np.where(aO ** 2 + e2 > 0, aO ** 2 + e2, one)
    Ss, Os = np.where(aS > 0, aS, one), np.where(aO > 0, aO, one)
    phi, a = obj.phases, obj.logamps
    da = aS * dS / q + aO * dO / p + 4 * u * (1.0 + np.abs(a))
    dphi = np.where(both, dS / Ss + dO / Os + 8 * u, 0.0)
    zero = np.zeros_like(aS)
    if obj.kind == "l2":
        D = np.abs(S - O)
        terms = 0.5 * w * D * D
        dterm = w * D * (dS + dO) + 6 * u * terms
        G, dG = w * D, w * (dS + dO) + 4 * u * w * D
    else:
        amp = one.astype(bool) if obj.kind == "logamp" else both if obj.kind == "log" else zero.astype(bool)
        ph = both if obj.kind in ("phase", "log") else zero.astype(bool)
        ta, tp = np.where(amp, 0.5 * w * a * a, 0.0), np.where(ph, 0.5 * w * phi * phi, 0.0)
        terms = ta + tp
        dterm = np.where(amp, w * np.abs(a) * da, 0.0) + np.where(ph, w * np.abs(phi) * dphi, 0.0) + 4 * u * terms
        Ga, Gp = np.where(amp, w * np.abs(a) * aS / q, 0.0), np.where(ph, w * np.abs(phi) / Ss, 0.0)
        G = Ga + Gp
        dG = (np.where(amp, w * (da * aS / q + 3.0 * np.abs(a) * dS / q), 0.0)
              + np.where(ph, w * (dphi / Ss + np.abs(phi) * dS / Ss ** 2), 0.0) + 4 * u * G)
    Jb = float(np.sum(dterm) + F * ntr * U2 * np.sum(np.abs(terms)))
    gerr = Mw * (np.sqrt(2.0) * np.sum(dG, axis=0) + (2 * F + Re + 4) * U2 * np.sqrt(2.0) * np.sum(G, axis=0))[None, :]
    rerr = float(np.linalg.norm(df.fir_time(gerr, ab)))
    return Jb, dphi, np.where(both | (obj.kind == "logamp"), da, 0.0), rerr
