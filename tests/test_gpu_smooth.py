"""Gaussian model-space smoothing on the GPU (include/fwi.h fwi_vec_smooth) against the fp64 NumPy
restatement of tests/_smooth.py, cell by cell, and the L-BFGS drivers with a smoothing initial inverse Hessian.

Per-cell bound of one application, derived: |err| <= 2 sum_axes (2 R_a + 3) u max|x| -- every pass is a convex
combination of 2 R + 1 terms with weights rounded to the context's format (u = 2^-24 / 2^-53), passes do not amplify
(||S_a||_inf = 1), the factor 2 is the margin."""
import shutil

import numpy as np
import pytest

import _smooth as ts
from full_waveform_inversion_amd import Engine, FwiError, shots as sh, workloads
from full_waveform_inversion_amd.lbfgs import lbfgs, lbfgs_device, lbfgs_device_slots, load_state

pytestmark = pytest.mark.gpu

U = {"float32": 2.0 ** -24, "float64": 2.0 ** -53}

S2A, S2B, S3A, S3B = (37, 23), (300, 2100), (19, 21, 23), (72, 70, 300)
CASES = [  # shape, sigma (grid order)
    (S2A, (1.5, 0.0)), (S2A, (0.0, 1.5)), (S2A, (2.0, 4.0)), (S2A, (0.5, 7.5)),  # (the last: R = 23 = nx)
    (S2B, (2.0, 0.0)), (S2B, (0.0, 2.0)), (S2B, (4.0, 2.0)), (S2B, (10.8, 10.8)),
    (S3A, (1.0, 0.0, 0.0)), (S3A, (0.0, 1.0, 0.0)), (S3A, (0.0, 0.0, 1.0)), (S3A, (0.5, 2.0, 4.0)),
    (S3A, (6.2, 0.0, 0.0)),  # R = 19 = nz, the short axis
    (S3A, (6.2, 6.9, 7.5)),  # R = n on every axis
    (S3B, (2.0, 0.0, 0.0)), (S3B, (0.0, 2.0, 0.0)), (S3B, (0.0, 0.0, 2.0)), (S3B, (0.5, 2.0, 4.0)),
    (S3B, (10.8, 10.8, 10.8)),  # R = 32 on every axis
]
_inputs, _refs = {}, {}


def field(shape):
    """The test vector of a shape: fp32-representable, so that both contexts smooth the same numbers."""
    if shape not in _inputs:
        x = np.random.default_rng(sum(shape)).standard_normal(shape).astype(np.float32)
        x.setflags(write=False)
        _inputs[shape] = x
    return _inputs[shape]


def reference(shape, sigma):
    key = (shape, tuple(sigma))
    if key not in _refs:
        r = ts.gaussian_smooth(field(shape), sigma)
        r.setflags(write=False)
        _refs[key] = r
    return _refs[key]


def engine(shape, dtype="float32"):
    return Engine(shape, 10.0, 1e-3, 4, dtype=dtype)


def assert_within(y, ref, sigma, dtype, xmax, napply=1):
    err = np.abs(np.asarray(y, np.float64) - ref)  # every cell of the logical array
    b = napply * ts.bound(sigma, ref.ndim, U[dtype], xmax)
    print("max |err| = %.3e, bound %.3e" % (err.max(), b))
    assert err.shape == ref.shape and np.isfinite(err).all() and err.max() <= b, (err.max(), b)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape,sigma", CASES, ids=lambda v: "x".join(str(k) for k in v))
def test_smoothing_matches_the_restatement_at_every_cell(gpu, shape, sigma, dtype):
    x = field(shape)
    assert ts.radius(max(sigma)) <= 32
    with engine(shape, dtype) as e:
        e.vec_create(1)
        e.vec_upload(0, x)
        e.vec_smooth(0, sigma)
        y = e.vec_download(0)
    assert_within(y, reference(shape, sigma), sigma, dtype, float(np.abs(x).max()))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", [S2A, S3A])
def test_zero_width_leaves_the_vector_unchanged_and_a_scalar_width_serves_every_axis(gpu, shape, dtype):
    x = field(shape).astype(dtype)
    with engine(shape, dtype) as e:
        e.vec_create(2)
        e.vec_upload(0, x)
        e.vec_smooth(0, 0.0)
        e.vec_smooth(0, (0.0,) * len(shape))
        e.vec_smooth(0, 0.16)  # R = int(0.98) = 0
        assert np.array_equal(e.vec_download(0), x)
        e.vec_upload(1, x)
        e.vec_smooth(0, 1.5)
        e.vec_smooth(1, (1.5,) * len(shape))
        assert np.array_equal(e.vec_download(0), e.vec_download(1))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape,sigma", [(S2A, (2.0, 4.0)), (S2A, (0.0, 1.5)), (S3A, (0.5, 2.0, 4.0)),
                                         (S3A, (0.0, 2.0, 1.0))], ids=str)
def test_pad_columns_stay_zero(gpu, shape, sigma, dtype):
    """nx % 4 != 0: the compact rows carry pad columns, which vec_dot sums over and vec_download leaves out."""
    x = field(shape) + np.float32(3.0)  # far from zero mean: a pad cell that took a smoothed value would weigh in
    with engine(shape, dtype) as e:
        e.vec_create(1)
        e.vec_upload(0, x)
        e.vec_smooth(0, sigma)
        dd = e.vec_dot(0, 0)
        y = e.vec_download(0).astype(np.float64)
    ss = float(np.sum(y * y))
    assert abs(dd - ss) <= 1e-13 * ss, (dd, ss)  # fp64 round-off of two reductions over < 1e4 positive terms


def _sym_sides(e, x, y, sigma):
    e.vec_create(3)
    e.vec_upload(0, x)
    e.vec_upload(1, y)
    e.vec_copy(2, 0)
    e.vec_smooth(2, sigma)
    a = e.vec_dot(2, 1)  # <S x, y>
    e.vec_copy(2, 1)
    e.vec_smooth(2, sigma)
    return a, e.vec_dot(0, 2)  # <x, S y>


@pytest.mark.parametrize("shape,sigma", [(S2A, (2.0, 4.0)), (S3A, (0.5, 2.0, 4.0)), (S3B, (2.0, 2.0, 2.0))], ids=str)
def test_the_operator_is_symmetric_on_the_device(gpu, shape, sigma):
    x = field(shape) + np.float32(0.5)  # (a mean keeps <S x, y> away from zero: the relative test means something)
    y = np.random.default_rng(5).standard_normal(shape).astype(np.float32) + np.float32(0.5)
    with engine(shape, "float64") as e:
        a, b = _sym_sides(e, x, y, sigma)
    assert abs(a - b) <= 1e-12 * abs(a), (a, b)
    with engine(shape, "float32") as e:
        a, b = _sym_sides(e, x, y, sigma)
    # the derived per-cell bound (per unit of |x|) times sum |x| |y|
    tol = ts.bound(sigma, len(shape), U["float32"], 1.0) * float(np.sum(np.abs(x.astype(np.float64) * y)))
    print("|<Sx,y> - <x,Sy>| = %.3e, bound %.3e" % (abs(a - b), tol))
    assert abs(a - b) <= tol, (a, b, tol)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape,sigma", [(S2A, (2.0, 7.5)), (S3A, (6.2, 2.0, 4.0)), (S3B, (10.8, 2.0, 4.0))], ids=str)
def test_constants_are_preserved(gpu, shape, sigma, dtype):
    with engine(shape, dtype) as e:
        e.vec_create(1)
        e.vec_upload(0, np.ones(shape, dtype))
        e.vec_smooth(0, sigma)
        y = e.vec_download(0).astype(np.float64)
        dd = e.vec_dot(0, 0)
    assert np.abs(y - 1.0).max() <= ts.bound(sigma, len(shape), U[dtype], 1.0)
    assert abs(dd - float(np.sum(y * y))) <= 1e-13 * dd  # the pads


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape,sigma", [(S2A, (2.0, 4.0)), (S2A, (0.0, 1.5)), (S3A, (0.5, 2.0, 4.0))], ids=str)
def test_in_place_calls_chain_and_repeat_bit_for_bit(gpu, shape, sigma, dtype):
    """Two passes (even: the result is formed in the vector) and one or three (odd: in the context's spare vector and
    copied back).  The second call must see the first call's output, nothing staler; a repeat on a fresh copy must
    give the same bits."""
    x = field(shape)
    with engine(shape, dtype) as e:
        e.vec_create(3)
        for s in range(3):
            e.vec_upload(s, x)
        e.vec_smooth(0, sigma)
        once = e.vec_download(0)
        e.vec_smooth(0, sigma)
        twice = e.vec_download(0)
        e.vec_smooth(1, sigma)  # determinism: the same call on a fresh copy
        assert np.array_equal(e.vec_download(1), once)
        e.vec_upload(2, once)   # the second call, fed the first call's output through the host
        e.vec_smooth(2, sigma)
        assert np.array_equal(e.vec_download(2), twice)
    assert np.isfinite(twice).all()
    ref2 = ts.gaussian_smooth(reference(shape, sigma), sigma)
    assert_within(twice, ref2, sigma, dtype, float(np.abs(x).max()), napply=2)


def test_each_refusal_is_einval_and_names_its_argument(gpu):
    x = field(S3A)
    with engine(S3A) as e:
        e.vec_create(1)
        e.vec_upload(0, x)
        for sigma, word in [((-1.0, 0.0, 0.0), "sigma[0]"), ((0.0, float("nan"), 0.0), "sigma[1]"),
                            ((0.0, 0.0, float("inf")), "sigma[2]"), ((0.0, 0.0, 7.9), "sigma[2]"),  # R = 24 > nx = 23
                            ((6.5, 0.0, 0.0), "sigma[0]"),                                          # R = 20 > nz = 19
                            ((1.0, 1.0), "sigma"), ((1.0, 1.0, 1.0, 1.0), "sigma")]:
            with pytest.raises(FwiError) as ei:
                e.vec_smooth(0, sigma)
            assert ei.value.code == 1 and word in str(ei.value), (sigma, str(ei.value))
        with pytest.raises(FwiError) as ei:
            e.vec_smooth(1, 1.0)
        assert ei.value.code == 1 and "slot 1" in str(ei.value)
        assert np.array_equal(e.vec_download(0), x)  # nothing was touched
        e.vec_smooth(0, (1.0, 0.0, 0.0))             # and the context still works
        assert_within(e.vec_download(0), reference(S3A, (1.0, 0.0, 0.0)), (1.0, 0.0, 0.0), "float32",
                      float(np.abs(x).max()))
    with engine(S3B) as e:  # an axis long enough for the radius cap to be the reason
        e.vec_create(1)
        with pytest.raises(FwiError) as ei:
            e.vec_smooth(0, (0.0, 0.0, 10.9))  # R = 33
        assert ei.value.code == 1 and "sigma[2]" in str(ei.value) and "32" in str(ei.value)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / np.linalg.norm(b))


def _small_inversion(nshots):
    w = workloads.cfg5(0.1875, nshots=3)  # 48^3, the problem of test_device_lbfgs_matches_host_lbfgs
    wav = w.wavelet()
    shots = [sh.Shot(w.src_idx[i:i + 1], wav, w.rec_idx) for i in range(nshots)]
    return w, shots, w.c_init.astype(np.float32)


def test_device_lbfgs_with_smoothing_h0_matches_the_host_one(gpu):
    w, shots, x0 = _small_inversion(3)
    mask = sh.source_mute(w.shape, shots, 3.0)
    fixed = mask == 0.0
    assert fixed.sum() == len(shots)
    kw = dict(maxiter=3, history=3, first_step=40.0, bounds=(1000.0, 5000.0))
    with Engine(w.shape, w.h, w.dt, w.nt, order=w.order, npml=w.npml) as e:
        sh.model_data(e, w.c.astype(np.float32), shots)
        xh, fh, logh = lbfgs(lambda m: sh.misfit_and_gradient(e, m, shots), x0, dot=e.dot,
                             h0=sh.smoothing_h0(1.5, mask=mask, smooth=ts.smooth_like), **kw)
        xd, fd, logd = lbfgs_device(e, lambda xs, gs: sh.misfit_and_gradient_device(e, xs, gs, shots), x0,
                                    h0=sh.smoothing_h0_device(e, 1.5, mask=mask), **kw)
    print("host", [r["f"] for r in logh], "device", [r["f"] for r in logd])
    assert [r["evals"] for r in logd] == [r["evals"] for r in logh]
    assert abs(fd - fh) < 1e-3 * fh
    assert rel(xd, xh) < 1e-5
    assert np.array_equal(xd[fixed], x0[fixed]) and not np.array_equal(xd, x0)


class _DeviceQuadratic:
    """f = 1/2 sum d (x - x*)^2 with vector operations only, on a grid of one reduction block (npts <= 256): every
    number of the run is reproducible to the bit, which the misfit of a wave simulation (float atomics) is not."""

    def __init__(self, e, d_slot, xs_slot, fill=None):
        rng = np.random.default_rng(11)
        self.e, self.D, self.XS, self.fill = e, d_slot, xs_slot, fill
        self.d = np.logspace(0.0, 2.0, int(np.prod(e.shape))).reshape(e.shape).astype(np.float32)
        self.xs = rng.standard_normal(e.shape).astype(np.float32)
        self.p = (1.0 / np.sqrt(self.d)).astype(np.float32)

    def __call__(self, x_slot, g_slot):
        e = self.e
        e.vec_upload(self.D, self.d)
        e.vec_upload(self.XS, self.xs)
        if self.fill is not None and e.vec_absmax(self.fill) == 0.0:
            e.vec_upload(self.fill, self.p)
        e.vec_copy(g_slot, x_slot)
        e.vec_axpby(g_slot, -1.0, self.XS, 1.0)
        e.vec_mul(g_slot, self.D)
        return 0.5 * (e.vec_dot(g_slot, x_slot) - e.vec_dot(g_slot, self.XS))


QSHAPE = (12, 18)  # cx = 20: 240 compact cells, one block of the reductions


def test_h0_that_multiplies_by_the_slot_is_the_diagonal_preconditioner_bit_for_bit(gpu):
    base = lbfgs_device_slots(3)
    PC = base + 2  # the two slots below it hold the quadratic's d and x*
    x0 = np.zeros(QSHAPE, np.float32)
    kw = dict(maxiter=6, history=3, first_step=0.5, precond_slot=PC)
    with engine(QSHAPE) as e:
        fg = _DeviceQuadratic(e, base, base + 1, fill=PC)
        xa, fa, loga = lbfgs_device(e, fg, x0, **kw)
        xb, fb, logb = lbfgs_device(e, fg, x0, h0=lambda slot: e.vec_mul(slot, PC), **kw)
    assert len(loga) > 3 and fa < loga[0]["f"]
    assert np.array_equal(xa, xb) and fa == fb and loga == logb


def test_device_run_with_h0_resumes_bit_for_bit(gpu, tmp_path):
    base = lbfgs_device_slots(3)
    PC = base + 2
    x0 = np.zeros(QSHAPE, np.float32)
    mask = np.ones(QSHAPE)
    mask[3:5, 4:9] = 0.0
    mask[5, 4:9] = 0.5
    ck, ck2 = str(tmp_path / "s.npz"), str(tmp_path / "s2.npz")
    kw = dict(maxiter=6, history=3, first_step=0.5, precond_slot=PC)
    with engine(QSHAPE) as e:
        fg = _DeviceQuadratic(e, base, base + 1, fill=PC)
        h0 = sh.smoothing_h0_device(e, (1.0, 1.5), mask=mask, precond_slot=PC)
        assert h0.nslots == 1
        x_ref, f_ref, log_ref = lbfgs_device(e, fg, x0, h0=h0, checkpoint=ck,
                                             callback=lambda it, *_: it == 3 and shutil.copy(ck, ck2), **kw)
        assert load_state(ck2)["it"] == 3 and load_state(ck2)["h0"] == h0.tag and load_state(ck)["it"] == 6
        x2, f2, log2 = lbfgs_device(e, fg, None, h0=h0, resume=ck2, **kw)
        assert np.array_equal(x2, x_ref) and f2 == f_ref and log2 == log_ref
        assert np.array_equal(x_ref[mask == 0.0], x0[mask == 0.0]) and f_ref < log_ref[0]["f"]
        with pytest.raises(ValueError):
            lbfgs_device(e, fg, None, h0=sh.smoothing_h0_device(e, 2.0, mask=mask, precond_slot=PC), resume=ck2, **kw)
        with pytest.raises(ValueError):
            lbfgs_device(e, fg, None, resume=ck2, **kw)


def test_device_inversion_with_h0_resumes_from_its_state_file(gpu, tmp_path):
    """The wave-equation run of test_device_lbfgs_resumes_from_its_state_file with a smoothing h0 and a source mute: equal
    to round-off (fp32 gradients carry float atomics in the injection), at that test's tolerances."""
    w, shots, x0 = _small_inversion(2)
    mask = sh.source_mute(w.shape, shots, 3.0)
    ck, ck2 = str(tmp_path / "s.npz"), str(tmp_path / "s2.npz")
    kw = dict(maxiter=3, history=3, first_step=40.0, bounds=(1000.0, 5000.0))
    with Engine(w.shape, w.h, w.dt, w.nt, order=w.order, npml=w.npml) as e:
        sh.model_data(e, w.c.astype(np.float32), shots)
        fg = lambda xs, gs: sh.misfit_and_gradient_device(e, xs, gs, shots)  # noqa: E731
        h0 = sh.smoothing_h0_device(e, 1.5, mask=mask)
        x_ref, f_ref, log_ref = lbfgs_device(e, fg, x0, h0=h0, checkpoint=ck,
                                             callback=lambda it, *_: it == 2 and shutil.copy(ck, ck2), **kw)
        x2, f2, log2 = lbfgs_device(e, fg, None, h0=h0, resume=ck2, **kw)
    assert [r["evals"] for r in log2] == [r["evals"] for r in log_ref]
    assert abs(f2 - f_ref) <= 1e-5 * f_ref
    assert np.linalg.norm(x2 - x_ref) <= 1e-6 * np.linalg.norm(x_ref)
