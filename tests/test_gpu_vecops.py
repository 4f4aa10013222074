"""The device's vector algebra and scalar reductions (fwi_vec_* / fwi_dot / fwi_misfit_l2: dot_kernel,
residual_l2_kernel, absmax_kernel, axpby_kernel, clip_kernel, repack_kernel, vec_mul_kernel, vec_recip_kernel) against
the NumPy restatement of tests/_vecops.py: fp32 and fp64 contexts, shapes at every edge of the launches (mostly pad, less
than a wave, exactly one block, a second idle block, 3-D, past each launch's block cap so that the grid-stride loops go
round again), non-finite values, aliasing, and -- for the sums -- the BITS of the result, which are a function of the
inputs alone: the kernels add in one fixed order, tests/_vecops.py restates it, and
tests/test_vecops_host.py shows that the inputs used here make another order of the block partials visible.

The engine contexts are used for their vector slots only."""
import ctypes as C
import math

import numpy as np
import pytest

import _vecops as vo
from full_waveform_inversion_amd import Engine, FwiError, shots as sh
from full_waveform_inversion_amd.lbfgs import lbfgs, lbfgs_device
from oracle import fwi_oracle as fo

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
CASES = [(s, t) for s in vo.SHAPES for t in DTYPES]
IDS = ["%s-%s" % ("x".join(map(str, s)), np.dtype(t).name) for s, t in CASES]
on_every_shape_and_dtype = pytest.mark.parametrize("shape,dtype", CASES, ids=IDS)


def _engine(shape, dtype, slots=0):
    e = Engine(shape, 10.0, 1e-3, 2, dtype=np.dtype(dtype).name, order=2 if min(shape) < 8 else 8)
    if slots:
        e.vec_create(slots)
    return e


def _bits(x):
    return C.c_uint64.from_buffer_copy(C.c_double(x)).value


def _same_value(got, want):
    return (math.isnan(got) and math.isnan(want)) or got == want


_REF = {}


def _dot_reference(key, a, b, shape):
    """(fsum of the fp64 products, sum of their magnitudes, the sum in the kernel's order): once per input pair"""
    if key not in _REF:
        _REF[key] = vo.dot_fsum(a, b) + (vo.dot_bits(a, b, shape),)
    return _REF[key]


def _nan_patterns(dtype):
    """Quiet and signalling NaNs with payloads and both signs, as arrays of ``dtype``."""
    if np.dtype(dtype) == np.float32:
        return np.array([0x7FC12345, 0xFFC00001, 0x7F800001, 0xFFBFFFFF], np.uint32).view(np.float32)
    return np.array([0x7FF8000012345678, 0xFFF8000000000001, 0x7FF0000000000001, 0xFFF7FFFFFFFFFFFF],
                    np.uint64).view(np.float64)


# ---- upload, download, copy ------------------------------------------------------------------------------------
@on_every_shape_and_dtype
def test_upload_download_and_copy_keep_every_bit_and_zero_the_pads(gpu, shape, dtype):
    x = vo.special_values(shape, dtype)
    cells = vo.plant_cells(shape)
    for cell, nan in zip(cells, _nan_patterns(dtype)):
        x[cell] = nan
    x.reshape(-1)[x.size // 2] = -0.0
    x.reshape(-1)[x.size // 3] = -np.finfo(dtype).smallest_subnormal
    with _engine(shape, dtype, 2) as e:
        e.vec_upload(0, x)
        assert vo.same_bits(e.vec_download(0), x)
        e.vec_copy(1, 0)
        assert vo.same_bits(e.vec_download(1), x)
        e.vec_copy(0, 0)  # dst == src
        assert vo.same_bits(e.vec_download(0), x)
        # the pad columns hold zeros after an upload (over the NaNs of poisoned memory, or of the vector before)
        e.vec_copy(1, 0)
        e.vec_upload(1, np.ones(shape, dtype))
        assert e.vec_dot(1, 1) == float(np.prod(shape))
        assert e.vec_dot(1, 1) == vo.dot_bits(np.ones(shape), np.ones(shape), shape)


# ---- the sums ---------------------------------------------------------------------------------------------------
@on_every_shape_and_dtype
def test_vec_dot_is_within_the_bound_and_has_the_restated_bits(gpu, shape, dtype):
    """fp32-representable inputs in both contexts: the fp64 products are exact, so the device's sum is the restatement's
    to the bit -- with block partials added in the order of arrival this fails on the two large shapes almost surely
    (tests/test_vecops_host.py: at least 90 of 100 orders differ).  Aliased operands, the negated vector, five repeats
    and a second context (another rank's replica) give the same bits."""
    a, b = vo.vec_pair(shape, dtype)
    ref, sum_abs, want = _dot_reference(("ab", shape), a, b, shape)
    ref_aa, sum_aa, want_aa = _dot_reference(("aa", shape), a, a, shape)
    n = a.size
    with _engine(shape, dtype, 3) as e, _engine(shape, dtype, 2) as other:
        e.vec_upload(0, a)
        e.vec_upload(1, b)
        e.vec_upload(2, -a)
        got = e.vec_dot(0, 1)
        print(shape, np.dtype(dtype).name, "vec_dot", got, "restated", want, "fsum", ref, "|err|", abs(got - ref),
              "bound", vo.sum_bound(n, sum_abs, True))
        assert abs(got - ref) <= vo.sum_bound(n, sum_abs, True)
        assert _bits(got) == _bits(want)
        assert all(_bits(e.vec_dot(0, 1)) == _bits(got) for _ in range(5))
        assert _bits(e.vec_dot(1, 0)) == _bits(got)  # products commute; the order of the terms is the same
        got_aa = e.vec_dot(0, 0)  # x . x, one operand
        assert abs(got_aa - ref_aa) <= vo.sum_bound(n, sum_aa, True) and _bits(got_aa) == _bits(want_aa)
        assert _bits(e.vec_dot(0, 2)) == _bits(-got_aa)  # every term negated: the negated sum, exactly
        other.vec_upload(1, a)
        other.vec_upload(0, b)
        assert _bits(other.vec_dot(1, 0)) == _bits(got)


@pytest.mark.parametrize("shape", vo.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_vec_dot_of_full_precision_fp64_vectors_is_within_the_bound(gpu, shape):
    """fp64 values with 53-bit significands: every product is rounded once, hence n + 1"""
    rng = np.random.default_rng([21] + list(shape))
    a = rng.standard_normal(shape) * 10.0 ** rng.uniform(-3, 3, shape)
    b = rng.standard_normal(shape) * 10.0 ** rng.uniform(-3, 3, shape)
    ref, sum_abs = vo.dot_fsum(a, b)
    with _engine(shape, np.float64, 2) as e:
        e.vec_upload(0, a)
        e.vec_upload(1, b)
        got = e.vec_dot(0, 1)
        assert abs(got - ref) <= vo.sum_bound(a.size, sum_abs, True)
        assert all(_bits(e.vec_dot(0, 1)) == _bits(got) for _ in range(5))


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
def test_block_partials_that_cancel_give_exactly_zero(gpu, dtype):
    shape = (520, 509)
    x, y = vo.cancelling_pair(shape)
    with _engine(shape, dtype, 2) as e:
        e.vec_upload(0, x.astype(dtype))
        e.vec_upload(1, y.astype(dtype))
        assert _bits(e.vec_dot(0, 1)) == _bits(0.0)
        assert _bits(e.vec_dot(0, 0)) == _bits(vo.dot_bits(x, x, shape))


@pytest.fixture(scope="module")
def small_engines(gpu):
    es = {np.dtype(t): Engine((8, 8), 10.0, 1e-3, 2, dtype=np.dtype(t).name) for t in DTYPES}
    yield es
    for e in es.values():
        e.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
@pytest.mark.parametrize("n", vo.DOT_SIZES)
def test_fwi_dot_of_host_arrays_is_within_the_bound_and_has_the_restated_bits(small_engines, n, dtype):
    a, b = vo.flat_pair(n, dtype)
    e = small_engines[np.dtype(dtype)]
    ref, sum_abs = vo.dot_fsum(a, b)
    got = e.dot(a, b)
    assert abs(got - ref) <= vo.sum_bound(n, sum_abs, True)
    assert _bits(got) == _bits(vo.dot_bits(a, b))
    assert all(_bits(e.dot(a, b)) == _bits(got) for _ in range(5))
    if n:
        assert _bits(e.dot(a, -a)) == _bits(-e.dot(a, a))


MISFIT_GRID, MISFIT_NT = (24, 40), 70


def _misfit_case(dtype, nt, nrec, off_grid):
    """A small 2-D shot with ``nrec`` receivers (nodes drawn with repeats, or fractional coordinates) and wide-range
    observed data."""
    rng = np.random.default_rng([31, nt, nrec])
    c = np.full(MISFIT_GRID, 2000.0)
    wav = fo.ricker(nt, 1e-3, 250.0, t0=0.0).astype(dtype)  # (energy from the first step on: even nt = 2 records some)
    if off_grid:
        src = np.array([[11.4, 20.7]])
        rec = np.stack([rng.uniform(0.5, s - 1.5, nrec) for s in MISFIT_GRID], 1)
    else:
        src = np.array([[12, 20]])
        rec = np.stack([rng.integers(0, s, nrec) for s in MISFIT_GRID], 1)
        rec[0] = src[0]  # the node that sees the wavelet at once
    return c, src, wav, rec, vo.wide(rng, (nt, nrec), dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
@pytest.mark.parametrize("nt,nrec,off_grid", [(2, 1, False), (3, 85, False), (70, 4000, False), (3, 85, True)],
                         ids=["2x1", "3x85", "70x4000", "3x85-off-grid"])
def test_misfit_l2_is_within_the_bound_and_has_the_restated_bits(gpu, nt, nrec, off_grid, dtype):
    """J = 1/2 sum r^2 with r = d_syn - d_obs formed in the context's type.  fp32: the squares are exact in fp64 and J
    has the restatement's bits.  (A sum of squares has no cancellation, so another order of its block partials shows in
    fewer totals than a dot product's does: on the CPU 0 to 88 of 100 orders over twelve seeds of this input family, on
    the device's residual of the 70 x 4000 case 99 (fp32) and 45 (fp64).  No seed makes that a property of the inputs,
    so the count is printed, not asserted, and the at-least-90 condition of tests/test_vecops_host.py rests on the dot
    cases; this case holds the bound, the restated bits and the repeats.)"""
    c, src, wav, rec, d_obs = _misfit_case(dtype, nt, nrec, off_grid)
    with Engine(MISFIT_GRID, 10.0, 1e-3, MISFIT_NT, dtype=np.dtype(dtype).name) as e, \
            Engine(MISFIT_GRID, 10.0, 1e-3, MISFIT_NT, dtype=np.dtype(dtype).name) as other:
        run = (lambda g: g.forward_at(c, (src, wav), rec, save=False)) if off_grid else \
            (lambda g: g.forward(c, (src, wav), rec, save=False))
        d_syn = run(e)
        assert d_syn.dtype == dtype and d_syn.shape == (nt, nrec) and np.any(d_syn != 0)
        r = d_syn - d_obs
        rsq = r.astype(np.float64).ravel() ** 2
        ref, n = 0.5 * math.fsum(rsq.tolist()), nt * nrec
        J = e.misfit_l2(d_obs)
        print(nt, nrec, np.dtype(dtype).name, "J", J, "fsum", ref, "|err|", abs(J - ref), "bound",
              0.5 * vo.sum_bound(n, 2 * ref, True), "orders that change the bits:",
              vo.orders_that_change_the_bits(vo.block_partials(rsq)))
        assert abs(J - ref) <= 0.5 * vo.sum_bound(n, 2 * ref, True)
        if dtype == np.float32:
            assert _bits(J) == _bits(0.5 * vo.sumsq_bits(r))
        for _ in range(5):
            run(e)
            assert _bits(e.misfit_l2(d_obs)) == _bits(J)
        assert np.array_equal(run(other), d_syn)
        assert _bits(other.misfit_l2(d_obs)) == _bits(J)


# ---- element-wise -----------------------------------------------------------------------------------------------
AXPBY = [(2.5, -0.5), (1.0, 1.0), (-1.0, 1.0), (0.0, 0.75), (1.7, 0.0)]


@on_every_shape_and_dtype
def test_vec_axpby_is_fp64_arithmetic_rounded_once(gpu, shape, dtype):
    """|got - ref64| <= u_T |ref64| + 3 2^-53 (|a x| + |b y|) + tiny_T: an implementation that computes in fp32 fails.
    IEEE semantics for non-finite values: 0 * NaN and 0 * inf are NaN, as in the host optimiser."""
    x, y = vo.vec_pair(shape, dtype)
    xs, ys = x.copy(), y.copy()
    cells = vo.plant_cells(shape)
    xs[cells[0]], xs[cells[1]], ys[cells[2]], ys[cells[3]] = np.nan, np.inf, -np.inf, np.nan
    with _engine(shape, dtype, 2) as e:
        for a, b in AXPBY:
            for u, v in ((x, y), (xs, ys)):
                e.vec_upload(0, u)
                e.vec_upload(1, v)
                e.vec_axpby(1, a, 0, b)
                got, ref = e.vec_download(1).astype(np.float64), vo.axpby(a, u, b, v)
                assert vo.same_bits(e.vec_download(0), u)
                fin = np.isfinite(ref)
                assert np.array_equal(np.isnan(got), np.isnan(ref)), (a, b)
                assert np.array_equal(got[np.isinf(ref)], ref[np.isinf(ref)]), (a, b)
                assert np.all(np.abs(got[fin] - ref[fin]) <= vo.axpby_bound(a, u, b, v, dtype)[fin]), (a, b)
            # y == x: the in-place scaling of lbfgs_device (a x + b x)
            e.vec_upload(0, x)
            e.vec_axpby(0, a, 0, b)
            got = e.vec_download(0).astype(np.float64)
            assert np.all(np.abs(got - vo.axpby(a, x, b, x)) <= vo.axpby_bound(a, x, b, x, dtype)), (a, b)
        e.vec_upload(0, xs)
        e.vec_axpby(0, 0.0, 0, 0.5)
        got = e.vec_download(0)
        assert np.isnan(got[cells[0]]) and np.isnan(got[cells[1]])  # 0 * NaN + .., 0 * inf + ..


@on_every_shape_and_dtype
def test_vec_mul_is_numpys_product_in_the_contexts_type(gpu, shape, dtype):
    x, y = (v.copy() for v in vo.vec_pair(shape, dtype))
    cells = vo.plant_cells(shape)
    tiny = float(np.finfo(dtype).tiny)
    x[cells[0]], y[cells[0]] = -0.0, 3.0
    x[cells[1]], y[cells[1]] = tiny * 8, 1.0 / 64 + 1.0 / 1024   # a denormal product, rounded
    x[cells[2]], y[cells[2]] = np.inf, -2.0
    x[cells[3]], y[cells[3]] = float(np.finfo(dtype).max), 2.0   # overflows to inf
    with _engine(shape, dtype, 2) as e:
        e.vec_upload(0, y)
        e.vec_upload(1, x)
        e.vec_mul(0, 1)
        assert vo.same_bits(e.vec_download(0), vo.mul(x, y))
        assert vo.same_bits(e.vec_download(1), x)
        e.vec_mul(1, 1)  # y == x
        assert vo.same_bits(e.vec_download(1), vo.mul(x, x))


@on_every_shape_and_dtype
def test_vec_recip_is_fp64_arithmetic_rounded_once_and_keeps_the_pads_zero(gpu, shape, dtype):
    y = vo.vec_pair(shape, dtype)[1]
    a, b = 2.0, 0.5
    with _engine(shape, dtype, 1) as e:
        e.vec_upload(0, y)
        e.vec_recip(0, a, b)
        got, ref = e.vec_download(0), vo.recip(y, a, b)
        assert np.all(np.isfinite(ref))
        assert np.all(np.abs(got.astype(np.float64) - ref) <= vo.recip_bound(y, a, b, dtype))
        # a pad column would hold a / (0 + b): the sum over the compact array is the logical one
        sq, sum_sq = vo.dot_fsum(got, got)
        assert abs(e.vec_dot(0, 0) - sq) <= vo.sum_bound(y.size, sum_sq, True)
        for sign in (1.0, -1.0):  # y + b == 0 is +0: the infinity has the sign of a, as in NumPy
            z = y.copy()
            cells = vo.plant_cells(shape)
            for cell in cells:
                z[cell] = -b
            e.vec_upload(0, z)
            e.vec_recip(0, sign * a, b)
            got, ref = e.vec_download(0), vo.recip(z, sign * a, b)
            assert all(got[cell] == sign * np.inf and ref[cell] == sign * np.inf for cell in cells)
            fin = np.isfinite(ref)
            assert np.all(np.abs(got.astype(np.float64)[fin] - ref[fin]) <= vo.recip_bound(z, sign * a, b, dtype)[fin])


CLIPS = [(-1.0, 2.0), (0.0, 2.0), (-0.0, 0.0), (0.25, 0.25), (0.1, 0.7)]


@on_every_shape_and_dtype
def test_vec_clip_is_numpys_clip_bit_for_bit(gpu, shape, dtype):
    """A NaN stays a NaN (with its payload), infinities are clipped, a zero keeps its sign; lo == hi; lo > hi refused;
    the pad columns stay out of the result."""
    x = vo.special_values(shape, dtype)
    for cell, v in zip(vo.plant_cells(shape), (_nan_patterns(dtype)[0], np.inf, -np.inf, _nan_patterns(dtype)[1])):
        x[cell] = v
    with _engine(shape, dtype, 1) as e:
        for lo, hi in CLIPS:
            e.vec_upload(0, x)
            e.vec_clip(0, lo, hi)
            assert vo.same_bits(e.vec_download(0), vo.clip(x, lo, hi)), (lo, hi)
        e.vec_upload(0, x)
        for lo, hi in ((0.5, 0.25), (np.nan, 1.0), (0.0, np.nan)):
            with pytest.raises(FwiError) as ei:
                e.vec_clip(0, lo, hi)
            assert ei.value.code == 1
        assert vo.same_bits(e.vec_download(0), x)
        # a clamp away from zero: the pads stay zero
        y = vo.special_values(shape, dtype)
        e.vec_upload(0, y)
        e.vec_clip(0, 0.25, 0.5)
        want = vo.clip(y, 0.25, 0.5)
        assert vo.same_bits(e.vec_download(0), want)
        sq, sum_sq = vo.dot_fsum(want, want)
        assert abs(e.vec_dot(0, 0) - sq) <= vo.sum_bound(y.size, sum_sq, True)


@on_every_shape_and_dtype
def test_vec_absmax_is_numpys_abs_max_nan_and_inf_included(gpu, shape, dtype):
    """The maximum, an infinity or a NaN planted in turn in the first cell, the last logical cell, the last cell before
    a pad column and a cell that the largest shape reaches only in the second trip of its grid-stride loop."""
    base = vo.vec_pair(shape, dtype)[0]
    cells = vo.plant_cells(shape)
    with _engine(shape, dtype, 1) as e:
        e.vec_upload(0, base)
        assert e.vec_absmax(0) == vo.absmax(base)
        for cell in cells:
            for v in (-7.0e5, 7.0e5, np.inf, -np.inf, np.nan, -_nan_patterns(dtype)[0]):
                x = base.copy()
                x[cell] = v
                e.vec_upload(0, x)
                assert _same_value(e.vec_absmax(0), vo.absmax(x)), (cell, v)
        x = base.copy()
        for k, cell in enumerate(cells):  # a NaN wins over an infinity wherever the two lie
            x[...] = base
            x[cell], x[cells[(k + 1) % len(cells)]] = np.nan, np.inf
            e.vec_upload(0, x)
            assert math.isnan(e.vec_absmax(0)) and math.isnan(vo.absmax(x))
        e.vec_upload(0, np.zeros(shape, dtype))
        assert e.vec_absmax(0) == 0.0


# ---- error paths ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "float64"])
def test_errors_are_reported_and_leave_the_vectors_untouched(gpu, dtype):
    shape = (8, 33)
    a, b = vo.vec_pair(shape, dtype)
    with _engine(shape, dtype, 2) as e:
        e.vec_upload(0, a)
        e.vec_upload(1, b)
        calls = [lambda: e.vec_dot(0, 2), lambda: e.vec_dot(-1, 0), lambda: e.vec_absmax(2), lambda: e.vec_copy(2, 0),
                 lambda: e.vec_copy(0, 2), lambda: e.vec_axpby(2, 1.0, 0, 1.0), lambda: e.vec_axpby(0, 1.0, 2, 1.0),
                 lambda: e.vec_clip(2, 0.0, 1.0), lambda: e.vec_mul(0, 2), lambda: e.vec_mul(2, 0),
                 lambda: e.vec_recip(2, 1.0, 0.0), lambda: e.vec_upload(2, a), lambda: e.vec_download(2),
                 lambda: e._chk(e._lib.fwi_vec_upload(e._ctx, 0, None)),
                 lambda: e._chk(e._lib.fwi_vec_download(e._ctx, 0, None)),
                 lambda: e._chk(e._lib.fwi_vec_dot(e._ctx, 0, 1, None)),
                 lambda: e._chk(e._lib.fwi_vec_absmax(e._ctx, 0, None)),
                 lambda: e._chk(e._lib.fwi_dot(e._ctx, None, None, C.c_int64(4), None)),
                 lambda: e.vec_create(257)]
        for k, call in enumerate(calls):
            with pytest.raises(FwiError) as ei:
                call()
            assert ei.value.code == 1, k
        with pytest.raises(ValueError):  # a host array of another shape never reaches the library
            e.vec_upload(0, np.zeros((8, 32), dtype))
        with pytest.raises(ValueError):
            e.dot(np.zeros(4, dtype), np.zeros(5, dtype))
        assert vo.same_bits(e.vec_download(0), a) and vo.same_bits(e.vec_download(1), b)
        assert _bits(e.vec_dot(0, 1)) == _bits(vo.dot_bits(a, b, shape))


# ---- two consequences, end to end -------------------------------------------------------------------------------
def test_a_partly_nan_illumination_is_refused_on_the_device_as_on_the_host(gpu):
    shape = (24, 40)
    H = (1.0 + np.random.default_rng(4).random(shape)).astype(np.float32)
    H[13, 17] = np.nan
    with pytest.raises(ValueError):
        sh.illumination_preconditioner(H)
    with _engine(shape, np.float32, 1) as e:
        e.vec_upload(0, H)
        with pytest.raises(ValueError):
            sh.illumination_preconditioner_vec(e, 0)
        assert vo.same_bits(e.vec_download(0), H)  # refused before anything was written
        H[13, 17] = 1.5
        e.vec_upload(0, H)
        sh.illumination_preconditioner_vec(e, 0)
        assert np.all(np.isfinite(e.vec_download(0)))


def test_a_nan_in_the_start_model_stops_the_bounded_device_optimiser_as_it_stops_the_host_one(gpu):
    """bounds= clips the start model: a NaN must come out of the clip as a NaN, so that the engine refuses the model,
    and not as the lower bound, from which the optimiser would carry on."""
    shape, nt = (32, 40), 40
    c = np.full(shape, 2000.0, np.float32)
    c[16:, :] = 2200.0
    wav = fo.ricker(nt, 1e-3, 60.0).astype(np.float32)
    shots = [sh.Shot(np.array([[2, 20]]), wav, np.stack([np.full(10, 3), np.arange(2, 40, 4)], 1))]
    x0 = np.full(shape, 2100.0, np.float32)
    x0[20, 11] = np.nan
    bounds = (1500.0, 3000.0)
    with Engine(shape, 10.0, 1e-3, nt) as e:
        sh.model_data(e, c, shots)
        done = []

        def fg_device(xs, gs):
            f = sh.misfit_and_gradient_device(e, xs, gs, shots)
            done.append(f)
            return f

        def fg_host(x):
            f, g = sh.misfit_and_gradient(e, x, shots)
            done.append(f)
            return f, g

        with pytest.raises((FwiError, FloatingPointError)) as ei:
            lbfgs_device(e, fg_device, x0, maxiter=2, history=2, first_step=20.0, bounds=bounds)
        assert isinstance(ei.value, FloatingPointError) or "velocity must be finite" in str(ei.value)
        with pytest.raises((FwiError, FloatingPointError)) as ei:
            lbfgs(fg_host, x0, maxiter=2, history=2, first_step=20.0, bounds=bounds)
        assert isinstance(ei.value, FloatingPointError) or "velocity must be finite" in str(ei.value)
        assert done == []  # no evaluation was reported as successful
        # the same run from a finite start model goes through
        x0[20, 11] = 2100.0
        _, f, log = lbfgs_device(e, fg_device, x0, maxiter=1, history=2, first_step=20.0, bounds=bounds)
        assert np.isfinite(f) and len(done) >= 2 and log[-1]["f"] <= log[0]["f"]
