"""Spectral imaging on the Fourier store on the GPU (include/fwi.h fwi_adjoint_spectral, fwi_fourier_*).

References, all independent of the code under test (tests/_fimage.py, tests/_fourier.py): the oracle's gradient with its
store replaced by the projection (by the identity of tests/test_fimage_host.py also the reference of the spectral
gradient), M_k from the oracle's own imaging sums against cos / sin stores, the illumination from the oracle's history.
fp64 is held to 1e-12; fp32 to MARGIN = 4 times the error of the fp32 oracle run through the fp32 / batched twin
against the fp64 reference, each such error asserted to be an fp32 round-off (2^-27 .. 1e-5).  Relative errors of a summed
band-limited gradient are asserted only where it is within a factor 10 of the native one.

1. gradient against the reference and against adjoint(image=True) on the same engine; M_k; adj_src_out bit for bit
2. per-frequency gradients and weights; the accumulator untouched by the read-outs
3. illumination: all bins against a native-store engine, a subset of bins and off-bin frequencies against the oracle
4. state across shots and repeated sweeps, store_bytes, clean padding
5. refusals: the documented code and a message that names the reason
6. the shot loop with spectral_imaging=True, illumination=True"""
import ctypes as C

import numpy as np
import pytest

import _fimage as FI
import _fourier as F
from full_waveform_inversion_amd import Engine, FwiError, _lib, fourier, shots as sh
from oracle import fwi_oracle as fo

pytestmark = pytest.mark.gpu

TOL64, MARGIN = FI.TOL64, FI.MARGIN
EINVAL, ESTATE = 1, 3


def _engine(shape, h, dt, nt, order, npml, sigma_max, dtype, opts, **kw):
    return Engine(shape, h, dt, nt, order=order, npml=npml, sigma_max=sigma_max, dtype=dtype, **opts, **kw)


def _forward(e, c, src, rec, wav, off_grid):
    return e.forward_at(c, (src, wav), rec.astype(np.float64)) if off_grid else e.forward(c, (src, wav), rec)


PARAMS = [(c, d) for c in FI.CASES for d in c[8]]


@pytest.mark.parametrize("case,dtype", PARAMS, ids=["%s-%s" % (c[0], d) for c, d in PARAMS])
def test_spectral_gradient_and_adjoint_spectrum_match_the_oracle(gpu, monkeypatch, case, dtype):
    name, fname, shape, order, npml, nt, S, B, _, opts, off_grid, fused_capable, env = case
    for k, v in env.items():
        monkeypatch.setenv(k, v)  # (read by fwi_create)
    key = FI.opts_key(opts)
    c, h, dt, src, rec, wav, res = F.problem(shape, order, nt, off_grid)
    R = F.reference(shape, order, npml, nt, S, "float64", key, off_grid)
    freqs = FI.subset_freqs(fname, nt, dt, S)
    g_ref = R.fourier(freqs)[0]
    M_ref = FI.adjoint_spectrum_ref(shape, order, npml, nt, S, freqs, key, off_grid)
    ratio = np.linalg.norm(g_ref) / np.linalg.norm(R.native)
    assert 0.1 <= ratio <= 10.0, ratio  # else the relative errors below say little
    with _engine(shape, h, dt, nt, order, npml, R.p.sigma_max, dtype, opts, image_stride=S, fourier=freqs,
                 fourier_batch=B) as e:
        _forward(e, c, src, rec, wav, off_grid)
        a0 = e.adjoint(res, image=False)
        assert np.linalg.norm(e.gradient()) == 0
        a = e.adjoint_spectral(res)
        g, M = e.gradient(), e.fourier_adjoint_spectrum()
        g_own = e.fourier_gradient()
        e.reset_gradient()
        e.adjoint(res)  # synthesis + time-domain imaging, on the same engine
        g_time = e.gradient()
        kname, dirty = e.kernel_name, e.dirty_padding()
    if fused_capable:
        # the context has the 4-steps-per-launch path, which its adjoint(image=False) takes and the spectral sweep gives up
        # for one step per launch: the two advance the same fields, bit for bit
        assert kname == "step2d_fused"
    assert np.array_equal(a, a0) and np.linalg.norm(a) > 0
    assert dirty == 0
    assert M.shape == (freqs.size,) + shape and np.all(np.isfinite(g))
    assert np.array_equal(g, g_own)  # one shot in the accumulator: the same sum, the same finalisation
    eg, em, es = F.rel(g, g_ref), F.rel(M, M_ref), F.rel(g, g_time)
    if dtype == "float64":
        bg = bm = bs = TOL64
    else:
        Q32, M32 = FI.twin32(shape, order, npml, nt, S, freqs, B, key, off_grid)
        g32 = FI.gradient_of_image(R, fourier.spectral_image(Q32, M32, nt, S, dt, freqs, dtype=np.float32))
        R32 = F.reference(shape, order, npml, nt, S, "float32", key, off_grid)
        own_g, own_m = FI.in_band(F.rel(g32, g_ref)), FI.in_band(F.rel(M32, M_ref))
        own_t = FI.in_band(F.rel(R32.fourier(freqs, np.float32, B)[0], g_ref))
        bg, bm, bs = MARGIN * own_g, MARGIN * own_m, MARGIN * (own_g + own_t)
    print("spectral %s %s: gradient %.3e (bound %.3e), M %.3e (bound %.3e), against adjoint(image) %.3e (bound %.3e), "
          "|g~| / |g| = %.2f" % (name, dtype, eg, bg, em, bm, es, bs, ratio))
    assert eg <= bg and em <= bm and es <= bs, (eg, bg, em, bm, es, bs)


WEIGHT_PARAMS = [(n, d) for n in ("mid_third", "off_bin_3") for d in FI.BOTH]


@pytest.mark.parametrize("name,dtype", WEIGHT_PARAMS, ids=["%s-%s" % p for p in WEIGHT_PARAMS])
def test_per_frequency_gradients_and_weights(gpu, name, dtype):
    _, fname, shape, order, npml, nt, S, B, _, opts, _, _, _ = FI.case(name)
    key = FI.opts_key(opts)
    c, h, dt, src, rec, wav, res = F.problem(shape, order, nt)
    R = F.reference(shape, order, npml, nt, S, "float64", key)
    freqs = FI.subset_freqs(fname, nt, dt, S)
    nf = freqs.size
    a = 0.25 + (np.arange(nf) % 3) - 1.0 * (np.arange(nf) == 1)  # (a negative weight is allowed for a gradient)
    with _engine(shape, h, dt, nt, order, npml, R.p.sigma_max, dtype, opts, image_stride=S, fourier=freqs,
                 fourier_batch=B) as e:
        e.forward(c, (src, wav), rec)
        e.adjoint_spectral(res)
        before = e.gradient()
        G, g, ga = e.fourier_gradients(), e.fourier_gradient(), e.fourier_gradient(a)
        Gm = e.fourier_gradients(wrt="slowness2")
        e.vec_create(1)
        e.fourier_gradient_vec(0, a)
        ga_vec = e.vec_download(0)
        assert np.array_equal(e.gradient(), before) and np.array_equal(before, g)  # the accumulator: read, never written
    assert G.shape == (nf,) + shape and np.array_equal(ga, ga_vec)
    if dtype == "float64":
        bound = TOL64
        bound_k = [TOL64] * nf
    else:
        Q32, M32 = FI.twin32(shape, order, npml, nt, S, freqs, B, key)
        g32 = FI.gradient_of_image(R, fourier.spectral_image(Q32, M32, nt, S, dt, freqs, dtype=np.float32))
        bound = MARGIN * FI.in_band(F.rel(g32, R.fourier(freqs)[0]))
        bound_k = []
        for k in range(nf):
            g32k = FI.gradient_of_image(R, fourier.spectral_image(Q32, M32, nt, S, dt, freqs, np.eye(nf)[k], np.float32))
            bound_k.append(MARGIN * FI.in_band(F.rel(g32k, R.fourier(freqs[[k]])[0])))
    es, ea = F.rel(G.astype(np.float64).sum(0), g), F.rel(ga, np.tensordot(a, G.astype(np.float64), axes=1))
    ek = [F.rel(G[k], R.fourier(freqs[[k]])[0]) for k in range(nf)]
    em = F.rel(Gm * (-2.0 / R.p.c ** 3), G)
    print("weights %s %s: sum of g_k %.3e, weighted %.3e (bound %.3e); g_k %s (bounds %s); slowness2 %.3e"
          % (name, dtype, es, ea, bound, ["%.2e" % v for v in ek], ["%.2e" % v for v in bound_k], em))
    assert es <= bound and ea <= bound, (es, ea, bound)
    # the two parametrisations: the same sum scaled and rounded to the field's type twice, independently
    assert em <= (TOL64 if dtype == "float64" else 2.0 * 2.0 ** -24), em
    assert all(v <= b for v, b in zip(ek, bound_k)), (ek, bound_k)


@pytest.mark.parametrize("dtype", FI.BOTH)
@pytest.mark.parametrize("name", ["3d_stream_sponge", "mid_third", "off_bin_3"])
def test_spectral_illumination(gpu, name, dtype):
    _, fname, shape, order, npml, nt, S, B, _, opts, _, _, _ = FI.case(name)
    key = FI.opts_key(opts)
    c, h, dt, src, rec, wav, res = F.problem(shape, order, nt)
    R = F.reference(shape, order, npml, nt, S, "float64", key)
    freqs = FI.subset_freqs(fname, nt, dt, S)
    a = 0.5 + np.arange(freqs.size) % 2
    with _engine(shape, h, dt, nt, order, npml, R.p.sigma_max, dtype, opts, image_stride=S, fourier=freqs,
                 fourier_batch=B) as e:
        e.forward(c, (src, wav), rec)  # nothing but the forward(save) is needed
        H = {w: e.fourier_illumination(wrt=w) for w in ("velocity", "slowness2")}
        Ha = e.fourier_illumination(a)
        e.vec_create(1)
        e.fourier_illumination_vec(0, a)
        assert np.array_equal(e.vec_download(0), Ha)
    q = np.asarray(R.q)[::S]
    Q_ref = fourier.analyse(q, nt, S, dt, freqs)
    if fname == "all":  # Parseval with every bin: the illumination of the stored term, as a native-store engine has it
        with _engine(shape, h, dt, nt, order, npml, R.p.sigma_max, dtype, opts, image_stride=S, illumination=True) as e:
            e.forward(c, (src, wav), rec)
            e.adjoint(res)
            ref = {w: e.illumination(w) for w in H}
        exact = np.sum(q * q, axis=0)
    elif fname == "mid_third":  # bins: the illumination of the band-limited term
        qt = fourier.project(R.q, nt, S, dt, freqs)[::S]
        exact = np.sum(qt * qt, axis=0)
        ref = {w: FI.illumination_of(R, exact, w) for w in H}
    else:  # off the bins: the formula, on the oracle's Q
        exact = fourier.spectral_illumination(Q_ref, nt, S, dt, freqs)
        ref = {w: FI.illumination_of(R, exact, w) for w in H}
    if dtype == "float64":
        bound = TOL64
    else:
        R32 = F.reference(shape, order, npml, nt, S, "float32", key)
        Q32 = fourier.analyse(np.asarray(R32.q)[::S], nt, S, dt, freqs, np.float32, B)
        own = F.rel(fourier.spectral_illumination(Q32, nt, S, dt, freqs, dtype=np.float32), exact)
        bound = MARGIN * FI.in_band(own)
    err = {w: F.rel(H[w], ref[w]) for w in H}
    ea = F.rel(Ha, FI.illumination_of(R, fourier.spectral_illumination(Q_ref, nt, S, dt, freqs, a)))
    print("illumination %s %s: %s, weighted %.3e (bound %.3e)" % (name, dtype, err, ea, bound))
    assert all(v <= bound for v in err.values()) and ea <= bound, (err, ea, bound)
    assert all(np.all(H[w] >= 0) and np.linalg.norm(H[w]) > 0 for w in H)


@pytest.mark.parametrize("dtype", FI.BOTH)
def test_state_across_shots_and_repeated_sweeps(gpu, dtype):
    shape, order, npml, S, B = (12, 10, 14), 8, 3, 4, 4
    nt_a, nt_b = 40, 33
    c, h, dt, src, rec, wav_a, res_a = F.problem(shape, order, nt_a)
    _, _, _, _, _, wav_b, res_b = F.problem(shape, order, nt_b)
    freqs = FI.subset_freqs("off_bin_3", nt_a, dt, S)
    nf = freqs.size
    sig = fo.default_sigma_max(c.max(), h, npml)
    vol = 12 * 10 * 16 * np.dtype(dtype).itemsize
    kw = dict(image_stride=S, fourier=freqs, fourier_batch=B)
    with _engine(shape, h, dt, nt_a, order, npml, sig, dtype, {}, **kw) as e:
        d_a = e.forward(c, (src, wav_a), rec)
        assert e.store_bytes() == (2 * nf + B + 1) * vol  # the adjoint accumulators come with the first spectral adjoint
        e.adjoint(res_a)
        g_time = e.gradient()  # today's path, before any spectral sweep
        e.reset_gradient()
        s_a = e.adjoint_spectral(res_a)
        assert e.store_bytes() == (4 * nf + B + 1) * vol
        g_a, M_a = e.gradient(), e.fourier_adjoint_spectrum()
        # a second spectral adjoint after the same forward: the same bits
        e.reset_gradient()
        assert np.array_equal(e.adjoint_spectral(res_a), s_a)
        assert np.array_equal(e.gradient(), g_a) and np.array_equal(e.fourier_adjoint_spectrum(), M_a)
        # the sweep alone, imaged afterwards with the same result; two images add
        e.reset_gradient()
        e.adjoint_spectral(res_a, image=False)
        assert np.linalg.norm(e.gradient()) == 0
        e.fourier_image()
        assert np.array_equal(e.gradient(), g_a)
        # adjoint(image=True) after a spectral sweep (which took the ring): its present result
        e.reset_gradient()
        e.adjoint(res_a)
        assert np.array_equal(e.gradient(), g_time)
        assert np.array_equal(e.fourier_adjoint_spectrum(), M_a)  # ... and M_k stays readable behind it
        # a shorter shot on the same context: both sets of accumulators start from zero again
        e.reset_gradient()
        e.forward(None, (src, wav_b), rec)
        e.adjoint_spectral(res_b)
        g_b, M_b = e.gradient(), e.fourier_adjoint_spectrum()
        # ... and the first shot once more: the same seismograms, the same bits
        e.reset_gradient()
        assert np.array_equal(e.forward(None, (src, wav_a), rec), d_a)
        e.adjoint_spectral(res_a)
        assert np.array_equal(e.gradient(), g_a) and np.array_equal(e.fourier_adjoint_spectrum(), M_a)
        assert e.store_bytes() == (4 * nf + B + 1) * vol and e.dirty_padding() == 0
        # a new set of frequencies frees everything
        e.set_fourier_store(freqs[:2])
        assert e.store_bytes() == 0
        e.forward(None, (src, wav_b), rec)
        assert e.store_bytes() == (2 * 2 + B + 1) * vol
    with _engine(shape, h, dt, nt_b, order, npml, sig, dtype, {}, **kw) as e:
        e.forward(c, (src, wav_b), rec)
        e.adjoint_spectral(res_b)
        assert np.array_equal(e.gradient(), g_b) and np.array_equal(e.fourier_adjoint_spectrum(), M_b)  # a fresh context
    assert not np.array_equal(g_b, g_a) and np.linalg.norm(g_b) > 0


def test_refusals_name_their_reason(gpu):
    shape, order, nt = (12, 10, 14), 8, 32
    c, h, dt, src, rec, wav, res = F.problem(shape, order, nt)
    ok = np.array([0.1, 0.2]) / (2 * dt)

    def refused(code, word, fn):
        with pytest.raises(FwiError) as ei:
            fn()
        assert ei.value.code == code and word in str(ei.value), str(ei.value)

    def spectrum_k(e, k):
        re, im = np.zeros(shape, e.dtype), np.zeros(shape, e.dtype)
        vp = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
        _lib.check(e._ctx, e._lib.fwi_fourier_adjoint_spectrum(e._ctx, k, vp(re), vp(im)))

    with Engine(shape, h, dt, nt, order=order) as e:  # not a Fourier context
        e.forward(c, (src, wav), rec)
        for fn in (lambda: e.adjoint_spectral(res), e.fourier_image, e.fourier_gradient, e.fourier_illumination,
                   lambda: spectrum_k(e, 0)):
            refused(ESTATE, "fwi_set_fourier_store", fn)
        e.vec_create(1)
        refused(ESTATE, "fwi_set_fourier_store", lambda: e.fourier_gradient_vec(0))
        refused(ESTATE, "fwi_set_fourier_store", lambda: e.fourier_illumination_vec(0))
        e.set_fourier_store(ok, batch=4)  # ... and no forward(save) since the store was set
        for fn in (lambda: e.adjoint_spectral(res), e.fourier_image, e.fourier_gradient, e.fourier_illumination):
            refused(ESTATE, "fwi_forward(save=1)", fn)
        e.forward(None, (src, wav), rec, save=False)
        refused(ESTATE, "fwi_forward(save=1)", lambda: e.adjoint_spectral(res))
        refused(ESTATE, "fwi_forward(save=1)", e.fourier_illumination)
        e.forward(None, (src, wav), rec)
        assert np.linalg.norm(e.fourier_illumination()) > 0  # needs only the forward
        for fn in (e.fourier_image, e.fourier_gradient, lambda: e.fourier_gradient_vec(0), e.fourier_gradients,
                   e.fourier_adjoint_spectrum):
            refused(ESTATE, "fwi_adjoint_spectral", fn)
        refused(EINVAL, "does not exist", lambda: e.fourier_gradient_vec(1))
        e.adjoint_spectral(res)
        assert np.linalg.norm(e.gradient()) > 0
        for bad in ([1.0, np.nan], [np.inf, 1.0]):
            for fn in (lambda: e.fourier_image(bad), lambda: e.fourier_gradient(bad), lambda: e.fourier_illumination(bad),
                       lambda: e.adjoint_spectral(res, bad)):
                refused(EINVAL, "finite", fn)
        refused(EINVAL, "negative", lambda: e.fourier_illumination([1.0, -1.0]))
        refused(EINVAL, "negative", lambda: e.fourier_illumination_vec(0, [1.0, -1.0]))
        e.fourier_gradient([1.0, -1.0])  # (a gradient may be weighted negatively)
        for k in (-1, 2):
            refused(EINVAL, "frequency index", lambda: spectrum_k(e, k))
        with pytest.raises(ValueError):
            e.fourier_gradient([1.0, 1.0, 1.0])
        with pytest.raises(KeyError):
            e.fourier_gradient(wrt="density")
        e.forward(None, (src, wav), rec)  # a new forward(save): the M_k of the shot before no longer go with its Q_k
        for fn in (e.fourier_image, e.fourier_gradient, e.fourier_adjoint_spectrum):
            refused(ESTATE, "fwi_adjoint_spectral", fn)
        refused(EINVAL, "fwi_set_illumination", lambda: e.set_illumination(True))  # (unchanged)


@pytest.mark.parametrize("dtype", FI.BOTH)
def test_shot_loop_with_spectral_imaging_and_illumination(gpu, dtype):
    shape, order, npml, nt, S, B = (12, 10, 14), 8, 3, 40, 1, 8
    c, h, dt, src, rec, wav, _ = F.problem(shape, order, nt)
    freqs = FI.subset_freqs("mid_third", nt, dt, S)
    a = 0.5 + np.arange(freqs.size) % 2
    sig = fo.default_sigma_max(c.max(), h, npml)
    c0 = np.full(shape, 2300.0)
    two = [sh.Shot(src, wav, rec), sh.Shot(src + 2, wav, rec)]
    with _engine(shape, h, dt, nt, order, npml, sig, dtype, {}, image_stride=S, fourier=freqs, fourier_batch=B) as e:
        sh.model_data(e, c, two)
        J, g, H = sh.misfit_and_gradient(e, c0, two, spectral_imaging=True, freq_weights=a, illumination=True)
        # ... the sum of the per-shot calls
        e.set_model(c0)
        e.reset_gradient()
        J1, H1 = 0.0, np.zeros(shape)
        for s in two:
            e.forward(None, (s.src_idx, s.wavelet), s.rec_idx)
            J1 += e.misfit_l2(s.d_obs)
            e.adjoint_spectral(None, a)
            H1 += e.fourier_illumination(a)
        assert J == J1 and np.array_equal(g, e.gradient()) and np.array_equal(H, H1)
        assert np.linalg.norm(g) > 0 and np.all(H >= 0) and np.linalg.norm(H) > 0
        # the device variant: the same gradient and illumination in vector slots
        e.vec_create(3)
        e.vec_upload(0, c0)
        Jd = sh.misfit_and_gradient_device(e, 0, 1, two, spectral_imaging=True, freq_weights=a, illum_slot=2)
        assert Jd == J and np.array_equal(e.vec_download(1), g)
        assert np.array_equal(e.vec_download(2), H.astype(dtype))
        # without the flag nothing changes: the time-domain imaging, and no illumination on a Fourier engine
        J0, g0 = sh.misfit_and_gradient(e, c0, two)
        assert J0 == J and not np.array_equal(g0, g)
        with pytest.raises(FwiError) as ei:
            sh.misfit_and_gradient(e, c0, two, illumination=True)
        assert ei.value.code == EINVAL and "fwi_set_illumination" in str(ei.value)
    with _engine(shape, h, dt, nt, order, npml, sig, dtype, {}, image_stride=S) as e:  # no Fourier store: refused
        with pytest.raises(ValueError):
            sh.misfit_and_gradient(e, c0, two, spectral_imaging=True)
