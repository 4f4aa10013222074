"""The Fourier-compressed forward-term store on the GPU (include/fwi.h fwi_set_fourier_store).

1. Identity: with every bin of the sampled time axis the gradient is that of a native-store engine of the same
   configuration.  Both engines step the same fields through the same one-step kernels, so only the round-off of the two
   transforms separates them: fp64 is held to 1e-12 (the NumPy twin reaches 1e-14 on these problems, the device differs
   by its summation order); fp32 to 4 times the twin's own fp32 error (tests/_fourier.py identity_bound32), the MARGIN
   convention of tests/_pointwise.py.
2. A subset of bins, and frequencies off the bins: gradient and spectrum against the oracle with its store replaced by
   fourier.project(.) (tests/_fourier.py).  fp64 at 1e-12 (4e-15 field parity plus N 2^-53); fp32 at 4 times the fp32
   oracle's own error.  The relative measure means something only while the band-limited gradient is not small against
   the native one: within a factor 10, checked here on the CPU.
3. State: accumulators zeroed per shot, repeated adjoints, repeated calls, fwi_store_bytes.
4. Refusals: the documented code and a message that names the reason."""
import numpy as np
import pytest

import _fourier as F
from full_waveform_inversion_amd import Engine, FwiError, fourier
from oracle import fwi_oracle as fo

pytestmark = pytest.mark.gpu

TOL64 = 1e-12
MARGIN = 4.0
EINVAL, ESTATE = 1, 3
BOTH, F32 = ("float64", "float32"), ("float32",)

# id, shape, order, npml, nt, S, B, dtypes, engine options, off-grid source, native reference without the fused 2-D path
ID_CASES = [
    ("2d_31_1_4", (21, 23), 4, 3, 31, 1, 4, BOTH, {"kernel": "point"}, False, False),
    ("2d_32_1_8", (20, 24), 8, 0, 32, 1, 8, BOTH, {"kernel": "point"}, False, False),
    ("2d_33_4_4", (21, 23), 4, 3, 33, 4, 4, BOTH, {"kernel": "point"}, False, False),
    ("2d_40_4_1", (20, 24), 8, 0, 40, 4, 1, BOTH, {"kernel": "point"}, False, False),
    ("2d_N_below_B", (21, 23), 4, 3, 20, 4, 8, BOTH, {"kernel": "point"}, False, False),  # N = 5 samples, batch 8
    # a fused-capable context (natively 4 steps per launch, nt % 4 == 0; with nt = 31 the bulk fused and 3 steps single)
    # still produces the result, one step per launch through the tile kernel
    ("2d_fused_capable", (20, 24), 8, 3, 32, 1, 8, F32, {}, False, True),
    ("2d_tile", (21, 23), 4, 3, 31, 1, 4, F32, {"kernel": "stream"}, False, True),
    ("3d_stream_sponge", (12, 10, 14), 8, 3, 33, 4, 4, BOTH, {}, False, False),
    ("3d_cpml", (9, 10, 13), 4, 3, 31, 1, 4, BOTH, {"abc": "cpml", "pml_alpha_max": 30.0}, False, False),
    ("3d_increment", (12, 10, 14), 8, 3, 32, 1, 8, BOTH, {"update_form": "increment"}, False, False),
    ("3d_graph", (9, 10, 13), 8, 0, 40, 4, 1, BOTH, {"launch_mode": "graph"}, False, False),
    ("3d_off_grid", (12, 10, 14), 8, 3, 31, 1, 4, BOTH, {}, True, False),
]


def _opts_key(opts):
    return tuple(sorted(opts.items()))


def _run(e, c, src, rec, wav, res, off_grid):
    """forward(save) + adjoint(image) of one shot on engine ``e``; returns the seismograms"""
    d = e.forward_at(c, (src, wav), rec.astype(np.float64)) if off_grid else e.forward(c, (src, wav), rec)
    e.adjoint(res)
    return d


def _engine(shape, h, dt, nt, order, npml, sigma_max, dtype, opts, **kw):
    return Engine(shape, h, dt, nt, order=order, npml=npml, sigma_max=sigma_max, dtype=dtype, **opts, **kw)


ID_PARAMS = [(c, d) for c in ID_CASES for d in c[7]]  # (the 2-D stream kernels are fp32)


@pytest.mark.parametrize("case,dtype", ID_PARAMS, ids=["%s-%s" % (c[0], d) for c, d in ID_PARAMS])
def test_all_bins_give_the_native_gradient(gpu, monkeypatch, case, dtype):
    _, shape, order, npml, nt, S, B, _, opts, off_grid, unfused_ref = case
    c, h, dt, src, rec, wav, res = F.problem(shape, order, nt, off_grid)
    R = F.reference(shape, order, npml, nt, S, "float64", _opts_key(opts), off_grid)
    sig = R.p.sigma_max
    freqs = F.all_bins(nt, dt, S)
    assert freqs.size == fourier.n_samples(nt, S) // 2 + 1
    with _engine(shape, h, dt, nt, order, npml, sig, dtype, opts, image_stride=S, fourier=freqs, fourier_batch=B) as e:
        d = _run(e, c, src, rec, wav, res, off_grid)
        g = e.gradient()
        held, kname = e.store_bytes(), e.kernel_name
    if unfused_ref:
        assert kname == "step2d_fused"  # the context has the fused path, and did not take it
        monkeypatch.setenv("FWI_NO_FUSED2D", "1")  # the native run on the same one-step kernels (read by fwi_create)
    with _engine(shape, h, dt, nt, order, npml, sig, dtype, opts, image_stride=S) as e:
        d0 = _run(e, c, src, rec, wav, res, off_grid)
        g0 = e.gradient()
        held0, kname0 = e.store_bytes(), e.kernel_name
    if unfused_ref:
        assert kname0 == "step2d_tile"
    item = np.dtype(dtype).itemsize
    cx = -(-shape[-1] // 4) * 4  # row stride of the compact device arrays
    npts = int(np.prod(shape[:-1])) * cx
    assert held == (2 * freqs.size + B + 1) * npts * item and held0 == fourier.n_samples(nt, S) * npts * item
    assert np.array_equal(d, d0)  # the same fields, bit for bit
    assert np.all(np.isfinite(g)) and np.linalg.norm(g0) > 0
    err = F.rel(g, g0)
    if dtype == "float64":
        bound = TOL64
    else:
        own = F.identity_bound32(shape, order, npml, nt, S, B, _opts_key(opts), off_grid)
        bound = MARGIN * own
        assert 2.0 ** -27 < own < 1e-5, own  # an fp32 round-off, neither nothing nor everything
    print("identity %s %s: rel L2 %.3e, bound %.3e" % (case[0], dtype, err, bound))
    assert err <= bound, (err, bound)


def _subset_freqs(name, nt, dt, S):
    bins = F.all_bins(nt, dt, S)
    nyq = 1.0 / (2 * S * dt)
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


# id, frequencies, shape, order, npml, nt, S, B, options
SUB_CASES = [
    ("one_bin", "one_bin", (21, 23), 4, 3, 33, 1, 4, {"kernel": "point"}),
    ("mid_third", "mid_third", (12, 10, 14), 8, 3, 40, 1, 8, {}),
    ("off_bin_3", "off_bin_3", (9, 10, 13), 4, 3, 33, 4, 4, {"abc": "cpml", "pml_alpha_max": 30.0}),
    ("off_bin_64", "off_bin_64", (20, 24), 8, 0, 40, 1, 4, {"kernel": "point"}),
]


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("case", SUB_CASES, ids=[c[0] for c in SUB_CASES])
def test_fewer_bins_and_off_bin_frequencies_match_the_projected_oracle(gpu, case, dtype):
    _, fname, shape, order, npml, nt, S, B, opts = case
    c, h, dt, src, rec, wav, res = F.problem(shape, order, nt)
    freqs = _subset_freqs(fname, nt, dt, S)
    R = F.reference(shape, order, npml, nt, S, "float64", _opts_key(opts))
    g_ref, Q_ref = R.fourier(freqs)
    ratio = np.linalg.norm(g_ref) / np.linalg.norm(R.native)
    assert 0.1 <= ratio <= 10.0, ratio  # else the relative error below says little
    with _engine(shape, h, dt, nt, order, npml, R.p.sigma_max, dtype, opts, image_stride=S, fourier=freqs,
                 fourier_batch=B) as e:
        _run(e, c, src, rec, wav, res, False)
        g, Q = e.gradient(), e.fourier_spectrum()
    assert Q.shape == (freqs.size,) + shape
    eg, eq = F.rel(g, g_ref), F.rel(Q, Q_ref)
    if dtype == "float64":
        bg = bq = TOL64
    else:
        R32 = F.reference(shape, order, npml, nt, S, "float32", _opts_key(opts))
        g32, Q32 = R32.fourier(freqs, np.float32, B)
        bg, bq = MARGIN * F.rel(g32, g_ref), MARGIN * F.rel(Q32, Q_ref)
    print("subset %s %s: gradient %.3e (bound %.3e), spectrum %.3e (bound %.3e), |g~| / |g| = %.2f"
          % (case[0], dtype, eg, bg, eq, bq, ratio))
    assert eg <= bg and eq <= bq, (eg, bg, eq, bq)


@pytest.mark.parametrize("dtype", BOTH)
def test_state_across_shots_and_repeated_sweeps(gpu, dtype):
    shape, order, npml, S, B = (12, 10, 14), 8, 3, 4, 4
    nt_a, nt_b = 40, 33
    c, h, dt, src, rec, wav_a, res_a = F.problem(shape, order, nt_a)
    _, _, _, _, _, wav_b, res_b = F.problem(shape, order, nt_b)
    freqs = _subset_freqs("off_bin_3", nt_a, dt, S)
    sig = fo.default_sigma_max(c.max(), h, npml)
    item, npts = np.dtype(dtype).itemsize, 12 * 10 * 16
    with _engine(shape, h, dt, nt_a, order, npml, sig, dtype, {}, image_stride=S, fourier=freqs, fourier_batch=B) as e:
        assert e.store_bytes() == 0  # nothing is allocated before the first forward(save)
        e.forward(c, (src, wav_a), rec)
        assert e.store_bytes() == (2 * freqs.size + B + 1) * npts * item
        e.adjoint(res_a)
        g_a = e.gradient()
        Q_a = e.fourier_spectrum()
        # a second adjoint after the same forward: the ring is rebuilt from the accumulators, the same bits
        e.reset_gradient()
        e.adjoint(res_a)
        assert np.array_equal(e.gradient(), g_a)
        # a shorter shot on the same context: the accumulators start from zero again
        e.reset_gradient()
        e.forward(None, (src, wav_b), rec)
        e.adjoint(res_b)
        g_b, Q_b = e.gradient(), e.fourier_spectrum()
        # ... and the first shot once more: the same call gives the same bits
        e.reset_gradient()
        e.forward(None, (src, wav_a), rec)
        e.adjoint(res_a)
        assert np.array_equal(e.gradient(), g_a) and np.array_equal(e.fourier_spectrum(), Q_a)
        assert e.store_bytes() == (2 * freqs.size + B + 1) * npts * item
        # an adjoint without imaging leaves the gradient alone
        e.adjoint(res_a, image=False)
        assert np.array_equal(e.gradient(), g_a)
        # back to the configured store: everything is freed, and the native store comes with the next forward(save)
        e.set_fourier_store(None)
        assert e.store_bytes() == 0 and e.fourier_freqs is None
        with pytest.raises(FwiError) as ei:
            e.adjoint(res_a)  # what the Fourier store held is gone
        assert ei.value.code == ESTATE
        e.reset_gradient()
        e.forward(None, (src, wav_b), rec)
        assert e.store_bytes() == fourier.n_samples(nt_a, S) * npts * item  # nt_max slots
        e.adjoint(res_b)
        g_native = e.gradient()
    with _engine(shape, h, dt, nt_b, order, npml, sig, dtype, {}, image_stride=S, fourier=freqs, fourier_batch=B) as e:
        e.forward(c, (src, wav_b), rec)
        e.adjoint(res_b)
        assert np.array_equal(e.gradient(), g_b) and np.array_equal(e.fourier_spectrum(), Q_b)  # a fresh context agrees
    assert not np.array_equal(g_b, g_native) and np.linalg.norm(g_native) > 0


def test_refusals_name_their_reason(gpu):
    shape, order, nt = (12, 10, 14), 8, 32
    c, h, dt, src, rec, wav, res = F.problem(shape, order, nt)
    nyq = 1.0 / (2 * dt)
    ok = np.array([0.1, 0.2]) * nyq

    def refused(code, word, fn):
        with pytest.raises(FwiError) as ei:
            fn()
        assert ei.value.code == code and word in str(ei.value), str(ei.value)

    with Engine(shape, h, dt, nt, order=order) as e:
        for bad, word in (([-1.0], "negative"), ([np.nan], "finite"), ([np.inf], "finite"), ([1.01 * nyq], "Nyquist"),
                          ([ok[0], ok[1], ok[0]], "equal")):
            refused(EINVAL, word, lambda: e.set_fourier_store(bad))
            assert e.fourier_freqs is None  # a refused call leaves the engine as it was
        refused(EINVAL, "batch", lambda: e.set_fourier_store(ok, batch=0))
        refused(EINVAL, "batch", lambda: e.set_fourier_store(ok, batch=9))
        refused(EINVAL, "nfreq", lambda: e.set_fourier_store(np.linspace(0.0, nyq, 65)))
        e.set_fourier_store([nyq, 0.0], batch=8)  # both ends of the band are allowed
        refused(ESTATE, "fourier_spectrum", lambda: e.fourier_spectrum())  # no forward yet
        e.set_fourier_store(ok, batch=4)
        refused(EINVAL, "fwi_set_illumination", lambda: e.set_illumination(True))
        assert not e.illumination_enabled
        e.forward(c, (src, wav), rec)
        for op in ("exact", "imaging"):
            refused(ESTATE, "Fourier", lambda: e.born(np.ones(shape), operator=op))
        e.vec_create(1)
        refused(ESTATE, "Fourier", lambda: e.born_vec(0))
        e.adjoint(res)
        assert np.linalg.norm(e.gradient()) > 0
    with Engine(shape, h, dt, nt, order=order, ckpt_interval=8) as e:
        refused(EINVAL, "ckpt_interval", lambda: e.set_fourier_store(ok))
    with Engine(shape, h, dt, nt, order=order, store_dtype="bf16") as e:
        refused(EINVAL, "bf16", lambda: e.set_fourier_store(ok))
    with Engine(shape, h, dt, nt, order=order, illumination=True) as e:
        refused(EINVAL, "illumination", lambda: e.set_fourier_store(ok))
        e.set_illumination(False)
        e.set_fourier_store(ok)
    with pytest.raises(FwiError) as ei:  # at creation too
        Engine(shape, h, dt, nt, order=order, ckpt_interval=8, fourier=ok)
    assert ei.value.code == EINVAL and "ckpt_interval" in str(ei.value)
