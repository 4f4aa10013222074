"""The tomographic / migration split of the Fourier-store gradient on the GPU (include/fwi.h fwi_fourier_split_image).

The reference is the NumPy twin (``fourier.split_image``, tests/test_fsplit_host.py) on the ORACLE's coefficients (Q from
its stored term, M from its own imaging sums; tests/_feximage.py).  The error of a part is ``|part - ref|`` over the norm of
the reference of ``fourier_gradient`` with the same weights and ``wrt``.  fp64 is held to ``_fimage.TOL64``.  fp32 is held
to ``_fimage.MARGIN`` times the twin's own fp32 error -- the fp32 oracle through the fp32 / batched twin of the analyses
(``_feximage.twin_spectra32``, ``_fimage.twin32``) and the fp32 twin of the split, against the fp64 reference in the same
normalisation, the largest over the three parts -- and that own error is asserted to be an fp32 round-off
(``_fimage.in_band``).  No bound comes from the engine.

1. five configurations, every axis, all three parts, unit and random non-negative weights, six tap sets (one tap, 3, 7,
   dense random, ``n - 1`` and ``n + 5`` taps); bit for bit: a repeated call, the ``_vec`` form, all-zero taps, the pad
   columns, and ``gradient()``, ``fourier_gradient()`` and an offset image before and after; ``same + opposite`` against
   ``fourier_gradient``
2. seams: one grid per axis that is two chunks of the kernel and an odd remainder long, the device against the twin on the
   device's OWN downloaded coefficients
3. refusals: the documented code and a message that names the argument
4. ``shots.split_gradient``: the fp64 sum of the per-shot parts, the J of the spectral shot loop

Measured on an MI355X (largest over the cases): parts 1.4e-14 in fp64 and 2.1e-6 in fp32 (bounds
5.7e-7 .. 1.0e-5, the closest at 0.47 of its bound); ``same + opposite`` against ``fourier_gradient`` 5.5e-16 in fp64 and
1.04e-7 in fp32, where the bound is 4 times the error of the fp32 twin's ``same + opposite`` against the fp32 twin's
gradient, 7.7e-8 .. 2.8e-7 (the closest at 0.66 of its bound); seams 3.9e-15 in fp64 and 6.1e-7 in fp32 (bounds 1.2e-6 ..
2.8e-5)."""
import functools

import numpy as np
import pytest

import _feximage as FX
import _fimage as FI
import _fourier as F
from full_waveform_inversion_amd import Engine, FwiError, datafit, fourier, shots as sh
from oracle import fwi_oracle as fo

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = 1, 3
NAMES = ("2d_33_4_4", "3d_stream_sponge", "3d_cpml", "off_bin_3", "3d_off_grid")
PARAMS = [(n, d) for n in NAMES for d in FI.case(n)[8]]
PARTS = ("same", "opposite", "hilbert")
# FSPLIT_CHUNK of csrc/fwi_fsplit.h: the cells along z or y one workgroup forms; along x a wave owns 64 vectors of 16 B,
# 256 fp32 or 128 fp64 cells.  The seam grids are two of the largest of these and an odd remainder long.
CHUNK, ROW_SEGMENT = 64, {"float32": 256, "float64": 128}
SEAMS = [("z", (151, 13), 4, {"kernel": "point"}), ("y", (6, 151, 9), 8, {}), ("x", (6, 5, 533), 8, {})]


def _engine(shape, h, dt, nt, order, npml, sigma_max, dtype, opts, **kw):
    return Engine(shape, h, dt, nt, order=order, npml=npml, sigma_max=sigma_max, dtype=dtype, **opts, **kw)


def _tap_sets(n, rng):
    return [("h1", datafit.hilbert_taps(1)), ("h3", datafit.hilbert_taps(3)), ("h7", datafit.hilbert_taps(7)),
            ("dense5", rng.uniform(-0.5, 0.5, 5)),  # every tap non-zero, a gain of the order of the Hilbert taps'
            ("n-1", datafit.hilbert_taps(n - 1)), ("n+5", datafit.hilbert_taps(n + 5))]


def _gradient_of(img, S, dt, c, wrt):
    g_m = -S * np.asarray(img, np.float64) / dt ** 2
    return g_m * (-2.0 / c ** 3) if wrt == "velocity" else g_m


def _err(a, b, norm):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / norm)


@pytest.mark.parametrize("name,dtype", PARAMS, ids=["%s-%s" % p for p in PARAMS])
def test_parts_match_the_twin_on_the_oracles_spectra(gpu, name, dtype):
    _, _, shape, order, npml, nt, S, B, _, opts, off_grid, _, _ = FI.case(name)
    c, h, dt, src, rec, wav, res = F.problem(shape, order, nt, off_grid)
    R, freqs, Q, M = FX.oracle_spectra(name)
    Q32, M32 = FX.twin_spectra32(name) if dtype == "float32" else (None, None)
    rng = np.random.default_rng(11)
    names = "zyx" if len(shape) == 3 else "zx"
    worst, worst_sum = 0.0, 0.0
    with _engine(shape, h, dt, nt, order, npml, R.p.sigma_max, dtype, opts, image_stride=S, fourier=freqs,
                 fourier_batch=B) as e:
        if off_grid:
            e.forward_at(c, (src, wav), rec.astype(np.float64))
        else:
            e.forward(c, (src, wav), rec)
        e.adjoint_spectral(res)
        e.vec_create(1)
        g_acc, g_four, e_off = e.gradient(), e.fourier_gradient(), e.fourier_offset_images(0, [1])
        for a, wrt in ((None, "velocity"), (rng.random(freqs.size), "slowness2")):
            g0 = e.fourier_gradient(a, wrt)
            g_ref = _gradient_of(fourier.spectral_image(Q, M, nt, S, R.dt, freqs, a), S, R.dt, R.p.c, wrt)
            norm = float(np.linalg.norm(g_ref))
            assert norm > 0
            for axis, n in enumerate(shape):
                for tname, t in _tap_sets(n, rng):
                    tag = "%s %s %s axis %d taps %s" % (name, dtype, wrt, axis, tname)
                    ref = {p: _gradient_of(fourier.split_image(Q, M, nt, S, R.dt, freqs, axis, t, p, a), S, R.dt, R.p.c,
                                           wrt) for p in PARTS}
                    got = {p: e.fourier_split_image(p, axis, t, a, wrt) for p in PARTS}
                    err = {p: _err(got[p], ref[p], norm) for p in PARTS}
                    esum = _err(got["same"].astype(np.float64) + got["opposite"].astype(np.float64), g0, norm)
                    if dtype == "float64":
                        bound = bound_sum = FI.TOL64
                    else:
                        own = {p: _gradient_of(fourier.split_image(Q32, M32, nt, S, R.dt, freqs, axis, t, p, a,
                                                                   np.float32), S, R.dt, R.p.c, wrt) for p in PARTS}
                        bound = FI.MARGIN * FI.in_band(max(_err(own[p], ref[p], norm) for p in PARTS))
                        # the sum of the two fp32 parts against the fp32 gradient: the twin's own error of that sum
                        own_g = _gradient_of(fourier.spectral_image(Q32, M32, nt, S, R.dt, freqs, a, np.float32), S, R.dt,
                                             R.p.c, wrt)
                        bound_sum = FI.MARGIN * FI.in_band(_err(own["same"] + own["opposite"], own_g, norm))
                    print("%s: errors %s (bound %.3e), same + opposite - gradient %.2e (bound %.3e)"
                          % (tag, {p: "%.2e" % v for p, v in err.items()}, bound, esum, bound_sum))
                    assert all(v <= bound for v in err.values()), (tag, err, bound)
                    assert esum <= bound_sum, (tag, esum, bound_sum)
                    worst, worst_sum = max(worst, *err.values()), max(worst_sum, esum)
                    assert all(got[p].shape == shape and got[p].dtype == np.dtype(dtype) for p in PARTS)
                    assert np.linalg.norm(got["hilbert"]) > 0
                    # a repeated call, the axis by name, the pair of parts and the device form: the same bits
                    tomo, mig = e.fourier_gradient_split(names[axis], t, a, wrt)
                    assert np.array_equal(tomo, got["same"]) and np.array_equal(mig, got["opposite"]), tag
                    assert np.array_equal(e.fourier_hilbert_image(axis, t, a, wrt), got["hilbert"]), tag
                    for p in PARTS:
                        e.fourier_split_image_vec(0, p, axis, t, a, wrt)
                        v = e.vec_download(0)
                        assert np.array_equal(v, got[p]), (tag, p)
                        ss = float(np.sum(v.astype(np.float64) ** 2))  # the pad columns of the slot are zeros
                        assert ss > 0 and abs(e.vec_dot(0, 0) - ss) <= 1e-13 * ss, (tag, p)
                # every tap zero: no filter, the two parts are equal bits and the filtered image is exactly zero
                z = {p: e.fourier_split_image(p, axis, np.zeros(3), a, wrt) for p in PARTS}
                assert np.array_equal(z["same"], z["opposite"]) and not np.any(z["hilbert"]), (name, axis)
                assert _err(2.0 * z["same"].astype(np.float64), g0, norm) <= (1e-15 if dtype == "float64" else 1e-7)
        print("%s %s: largest error %.3e, largest same + opposite - gradient %.3e" % (name, dtype, worst, worst_sum))
        # neither the accumulator nor Q_k, M_k were touched, and nothing was written outside the grid's cells
        assert np.array_equal(e.gradient(), g_acc) and np.array_equal(e.fourier_gradient(), g_four)
        assert np.array_equal(e.fourier_offset_images(0, [1]), e_off)
        assert e.dirty_padding() == 0


@functools.lru_cache(maxsize=None)
def _seam_problem(shape, axis, order, nt):
    """(c, h, dt, src, rec, wavelets, residual) with a source every 25 and a receiver every 12 cells in a line along
    ``axis``, so that after nt steps the forward and the adjoint coefficients overlap along the whole axis (the one source
    of ``_fourier.problem`` reaches a dozen cells, and its image would have no norm to measure a long grid against)."""
    rng = np.random.default_rng(7)
    c = 2000.0 + 600.0 * rng.random(shape)
    h = 10.0
    dt = 0.6 * fo.cfl_dt(c.max(), h, len(shape), order)

    def line(count):
        idx = np.array([[s // 2 for s in shape]] * count)
        idx[:, axis] = ((np.arange(count) + 0.5) * shape[axis] / count).astype(int)
        return idx

    nsrc, nrec = shape[axis] // 25, shape[axis] // 12
    wav = fo.ricker(nt, dt, 1.0 / (10.0 * dt), t0=12.0 * dt)[:, None] * (1.0 + 0.2 * (np.arange(nsrc) % 5))[None, :]
    return c, h, dt, line(nsrc), line(nrec), wav, rng.standard_normal((nt, nrec))


@functools.lru_cache(maxsize=None)
def _seam_oracle(shape, axis, order, npml, nt, S, B, dtype):
    """(sigma_max, freqs, Q, M) of the oracle run in ``dtype`` on ``_seam_problem``: fp64 as ``_feximage.oracle_spectra``
    (M_k from cos / sin stores), fp32 as ``_fimage.twin32`` (the samples through the fp32 / batched twin of the analyses)"""
    c, h, dt, src, rec, wav, res = _seam_problem(shape, axis, order, nt)
    p = fo.Propagator(c, h, dt, order, npml, dtype=np.dtype(dtype), image_stride=S)
    p.forward(src, wav, rec)
    q = p.q_store
    freqs = FI.subset_freqs("off_bin_3", nt, dt, S)

    def img_with(per_step):  # as _fimage._img_with
        p.q_store = np.asarray(per_step, np.float64).reshape((nt,) + (1,) * len(shape))
        p.adjoint(res)
        return np.array(p._img, np.float64)

    if dtype == "float64":
        Q = fourier.analyse(np.asarray(q)[::S], nt, S, dt, freqs)
        th = fourier.phases(nt, S, dt, freqs)
        M = np.zeros((freqs.size,) + shape, np.complex128)
        for k in range(freqs.size):
            cs, sn = np.zeros(nt), np.zeros(nt)
            cs[::S], sn[::S] = np.cos(th[k]), np.sin(th[k])
            M[k] = (img_with(cs) - 1j * img_with(sn)) / S
    else:
        Q = fourier.analyse(np.asarray(q)[::S], nt, S, dt, freqs, np.float32, B)
        N = fourier.n_samples(nt, S)
        mu = np.zeros((N,) + shape)
        for j in range(N):
            hot = np.zeros(nt)
            hot[j * S] = 1.0
            mu[j] = img_with(hot) / S
        M = fourier.adjoint_spectrum(mu, nt, S, dt, freqs, np.float32, B)
    return p.sigma_max, freqs, Q, M


@pytest.mark.parametrize("dtype", FI.BOTH)
@pytest.mark.parametrize("axis_name,shape,order,opts", SEAMS, ids=[s[0] for s in SEAMS])
def test_seams_of_the_tiling_against_the_twin_on_the_devices_own_spectra(gpu, axis_name, shape, order, opts, dtype):
    npml, nt, S, B = 3, 33, 4, 4
    axis = len(shape) - 1 if axis_name == "x" else "zy".index(axis_name)
    unit = ROW_SEGMENT[dtype] if axis_name == "x" else CHUNK
    assert shape[axis] > 2 * unit and (shape[axis] - 2 * unit) % 2 == 1
    c, h, dt, src, rec, wav, res = _seam_problem(shape, axis, order, nt)
    sigma_max, freqs, Q, M = _seam_oracle(shape, axis, order, npml, nt, S, B, "float64")
    rng = np.random.default_rng(3)
    a = rng.random(freqs.size)
    sets = [("h31", datafit.hilbert_taps(31)), ("dense9", rng.uniform(-0.5, 0.5, 9))]
    norm_o = float(np.linalg.norm(fourier.spectral_image(Q, M, nt, S, dt, freqs, a)))
    if dtype == "float32":  # the twin's own fp32 error on this grid, from the oracle
        _, _, Q32, M32 = _seam_oracle(shape, axis, order, npml, nt, S, B, "float32")
    with _engine(shape, h, dt, nt, order, npml, sigma_max, dtype, opts, image_stride=S, fourier=freqs,
                 fourier_batch=B) as e:
        e.forward(c, (src, wav), rec)
        e.adjoint_spectral(res)
        Qd, Md = e.fourier_spectrum(), e.fourier_adjoint_spectrum()
        g_ref = _gradient_of(fourier.spectral_image(Qd, Md, nt, S, dt, freqs, a), S, dt, c, "slowness2")
        norm = float(np.linalg.norm(g_ref))
        assert norm > 0
        # the image has weight, far above either bound, on either side of every seam of the tiling
        prof = np.sqrt(np.sum(np.moveaxis(g_ref, axis, 0).reshape(shape[axis], -1) ** 2, axis=1))
        assert all(np.linalg.norm(prof[lo:lo + unit]) > 1e-4 * norm for lo in range(0, shape[axis], unit)), prof
        for tname, t in sets:
            if dtype == "float64":
                bound = FI.TOL64
            else:
                own = max(_err(fourier.split_image(Q32, M32, nt, S, dt, freqs, axis, t, p, a, np.float32),
                               fourier.split_image(Q, M, nt, S, dt, freqs, axis, t, p, a), norm_o) for p in PARTS)
                bound = FI.MARGIN * FI.in_band(own)
            for p in PARTS:
                ref = _gradient_of(fourier.split_image(Qd, Md, nt, S, dt, freqs, axis, t, p, a), S, dt, c, "slowness2")
                got = e.fourier_split_image(p, axis_name, t, a, "slowness2")
                err = _err(got, ref, norm)
                print("seam %s %s %s taps %s %s: error %.2e (bound %.3e)" % (axis_name, shape, dtype, tname, p, err, bound))
                assert err <= bound, (axis_name, tname, p, err, bound)
                assert np.linalg.norm(got) > 0
        assert e.dirty_padding() == 0


def test_refusals_name_their_reason(gpu):
    shape, order, nt = (12, 10, 14), 8, 32
    c, h, dt, src, rec, wav, res = F.problem(shape, order, nt)
    ok = np.array([0.1, 0.2]) / (2 * dt)
    t = datafit.hilbert_taps(3)

    def refused(code, word, fn):
        with pytest.raises(FwiError) as ei:
            fn()
        assert ei.value.code == code and word in str(ei.value), str(ei.value)

    def calls(e):
        return (lambda: e.fourier_split_image("same", 0, t), lambda: e.fourier_split_image_vec(0, "opposite", 1, t),
                lambda: e.fourier_gradient_split("x", t), lambda: e.fourier_hilbert_image(2, t))

    with Engine(shape, h, dt, nt, order=order) as e:
        e.vec_create(1)
        e.forward(c, (src, wav), rec)
        for fn in calls(e):  # the store is off
            refused(ESTATE, "fwi_set_fourier_store", fn)
        e.set_fourier_store(ok, batch=4)
        for fn in calls(e):  # no forward(save) since the store was set
            refused(ESTATE, "fwi_forward(save=1)", fn)
        e.forward(None, (src, wav), rec)
        for fn in calls(e):  # no adjoint_spectral yet
            refused(ESTATE, "fwi_adjoint_spectral", fn)
        e.adjoint_spectral(res)
        g_four = e.fourier_gradient()
        first = e.fourier_split_image("same", 2, t)
        assert np.linalg.norm(first) > 0
        e.vec_upload(0, np.ones(shape, e.dtype))
        for axis in (3, -1):
            refused(EINVAL, "axis", lambda: e.fourier_split_image("same", axis, t))
            refused(EINVAL, "axis", lambda: e.fourier_split_image_vec(0, "same", axis, t))
        for bad in (np.zeros(0), np.zeros(fourier.SPLIT_RMAX + 1)):
            refused(EINVAL, "ntaps", lambda: e.fourier_split_image("same", 0, bad))
            refused(EINVAL, "ntaps", lambda: e.fourier_split_image_vec(0, "same", 0, bad))
        assert np.linalg.norm(e.fourier_split_image("same", 0, datafit.hilbert_taps(fourier.SPLIT_RMAX))) > 0
        for bad in ([0.5, np.nan], [np.inf], [0.1, -np.inf, 0.0]):
            refused(EINVAL, "taps", lambda: e.fourier_split_image("hilbert", 0, bad))
            refused(EINVAL, "taps", lambda: e.fourier_split_image_vec(0, "hilbert", 0, bad))
        for bad in ([1.0, np.nan], [np.inf, 1.0]):
            refused(EINVAL, "freq_weights", lambda: e.fourier_split_image("same", 0, t, bad))
            refused(EINVAL, "freq_weights", lambda: e.fourier_split_image_vec(0, "same", 0, t, bad))
        e.fourier_split_image("same", 0, t, [1.0, -1.0])  # (a negative weight is allowed, as for a gradient)
        refused(EINVAL, "part", lambda: e._chk(e._lib.fwi_fourier_split_image_vec(e._c, 0, 3, 0, 3, t.ctypes.data, None, 0)))
        refused(EINVAL, "part", lambda: e._chk(e._lib.fwi_fourier_split_image_vec(e._c, 0, -1, 0, 3, t.ctypes.data, None, 0)))
        refused(EINVAL, "parametrisation",
                lambda: e._chk(e._lib.fwi_fourier_split_image_vec(e._c, 2, 0, 0, 3, t.ctypes.data, None, 0)))
        refused(EINVAL, "null taps", lambda: e._chk(e._lib.fwi_fourier_split_image_vec(e._c, 0, 0, 0, 3, None, None, 0)))
        refused(EINVAL, "null output",
                lambda: e._chk(e._lib.fwi_fourier_split_image(e._c, 0, 0, 0, 3, t.ctypes.data, None, None)))
        for slot in (1, -1):
            refused(EINVAL, "does not exist", lambda: e.fourier_split_image_vec(slot, "same", 0, t))
        with pytest.raises(ValueError):
            e.fourier_split_image("both", 0, t)
        with pytest.raises(ValueError):
            e.fourier_split_image("same", "w", t)
        with pytest.raises(ValueError):
            e.fourier_split_image("same", 0, t, [1.0, 1.0, 1.0])
        # a refused call touched nothing: the slot, the coefficients, and the next call's bits
        assert np.array_equal(e.vec_download(0), np.ones(shape, e.dtype))
        assert np.array_equal(e.fourier_gradient(), g_four) and np.array_equal(e.fourier_split_image("same", 2, t), first)
        # the extended Born call writes its spectrum over M_k: refused until the next adjoint_spectral
        e.fourier_born_extended("time", [0.0], first[None], download=False)
        for fn in calls(e):
            refused(ESTATE, "fwi_adjoint_spectral", fn)
        e.adjoint_spectral(res)
        assert np.array_equal(e.fourier_split_image("same", 2, t), first)
        e.forward(None, (src, wav), rec)  # a new forward(save): the M_k of the shot before no longer go with its Q_k
        for fn in calls(e):
            refused(ESTATE, "fwi_adjoint_spectral", fn)
    c, h, dt, src, rec, wav, res = F.problem((21, 23), 4, nt)
    with Engine((21, 23), h, dt, nt, order=4, fourier=np.array([0.1, 0.2]) / (2 * dt), fourier_batch=4) as e:
        e.forward(c, (src, wav), rec)  # 2-D: axis 2 does not exist, "y" neither
        e.adjoint_spectral(res)
        refused(EINVAL, "axis", lambda: e.fourier_split_image("same", 2, t))
        with pytest.raises(ValueError):
            e.fourier_split_image("same", "y", t)
        assert np.array_equal(e.fourier_split_image("same", "x", t), e.fourier_split_image("same", 1, t))


@pytest.mark.parametrize("dtype", FI.BOTH)
def test_split_gradient_of_the_shot_loop(gpu, dtype):
    shape, order, npml, nt, S, B = (12, 10, 14), 8, 3, 40, 1, 8
    c, h, dt, src, rec, wav, _ = F.problem(shape, order, nt)
    freqs = FI.subset_freqs("mid_third", nt, dt, S)
    a = 0.5 + np.arange(freqs.size) % 2
    sig = fo.default_sigma_max(c.max(), h, npml)
    c0 = np.full(shape, 2300.0)
    two = [sh.Shot(src, wav, rec), sh.Shot(src + 2, wav, rec)]
    t = datafit.hilbert_taps(5)
    with _engine(shape, h, dt, nt, order, npml, sig, dtype, {}, image_stride=S, fourier=freqs, fourier_batch=B) as e:
        sh.model_data(e, c, two)
        Js, g_same, g_oppo = sh.split_gradient(e, c0, two, "z", t, freq_weights=a)
        assert np.linalg.norm(e.gradient()) == 0  # the sweeps image nothing into the accumulator
        J, g = sh.misfit_and_gradient(e, c0, two, spectral_imaging=True, freq_weights=a)
        assert Js == J
        # ... the fp64 sum of the per-shot parts
        e.set_model(c0)
        G = np.zeros((2,) + shape)
        for s in two:
            e.forward(None, (s.src_idx, s.wavelet), s.rec_idx)
            e.misfit_l2(s.d_obs)
            e.adjoint_spectral(None, image=False)
            G += np.stack(e.fourier_gradient_split(0, t, a))
        assert g_same.dtype == np.float64 and np.array_equal(g_same, G[0]) and np.array_equal(g_oppo, G[1])
        assert np.linalg.norm(g_same) > 0 and np.linalg.norm(g_oppo) > 0
        tol = 1e-12 if dtype == "float64" else 1e-6  # two roundings to fp32 per shot and part against one per sum
        assert np.linalg.norm(g_same + g_oppo - g) <= tol * np.linalg.norm(g)
        _, s2, o2 = sh.split_gradient(e, c0, two, 0, t, freq_weights=a, wrt="slowness2")
        assert np.linalg.norm(s2 * (-2.0 / c0 ** 3) - g_same) <= tol * np.linalg.norm(g_same)
    with _engine(shape, h, dt, nt, order, npml, sig, dtype, {}, image_stride=S) as e:  # no Fourier store: refused
        with pytest.raises(ValueError):
            sh.split_gradient(e, c0, two, "z", t)
