"""The NumPy restatement of the device's sums (tests/_vecops.py) and the NaN semantics the host and the device optimiser
share, without a GPU:

* the restatement is a sum of the same terms in some order, so it lies within the standard bound of ``math.fsum``;
* it adds in the order the kernels are written in (a thread-by-thread emulation in plain Python says the same);
* the inputs of the GPU suite's large sum cases make the order of the block partials visible in the total's bits --
  without that, a bit-for-bit comparison with the device would pass whatever the order;
* ``np.clip`` and ``np.abs(x).max()``, which the host optimiser uses, do what include/fwi.h specifies for
  ``fwi_vec_clip`` and ``fwi_vec_absmax``."""
import math

import numpy as np
import pytest

import _vecops as vo


@pytest.mark.parametrize("shape", vo.SHAPES, ids=str)
def test_restated_grid_sum_is_within_the_any_order_bound_of_fsum(shape):
    a, b = vo.vec_pair(shape)
    ref, sum_abs = vo.dot_fsum(a, b)
    got = vo.dot_bits(a, b, shape)
    print(shape, got, ref, abs(got - ref), vo.sum_bound(a.size, sum_abs))
    assert abs(got - ref) <= vo.sum_bound(a.size, sum_abs)
    ref2, sum_sq = vo.dot_fsum(a, a)
    assert abs(vo.sumsq_bits(vo.compact(a, shape)) - ref2) <= vo.sum_bound(a.size, sum_sq)


@pytest.mark.parametrize("n", vo.DOT_SIZES)
def test_restated_flat_sum_is_within_the_any_order_bound_of_fsum(n):
    a, b = vo.flat_pair(n)
    ref, sum_abs = vo.dot_fsum(a, b)
    got = vo.dot_bits(a, b)
    assert abs(got - ref) <= vo.sum_bound(n, sum_abs)
    assert n > 0 or got == 0.0


def _emulated(terms, max_blocks):
    """The kernels' sum, thread by thread and lane by lane in plain Python floats (IEEE doubles)."""
    n = len(terms)
    blocks = max(1, min(max_blocks, (n + 255) // 256))
    partials = []
    for blk in range(blocks):
        acc = []
        for t in range(256):
            s, i = 0.0, blk * 256 + t
            while i < n:
                s += terms[i]
                i += blocks * 256
            acc.append(s)
        waves = []
        for w in range(4):
            lane = acc[64 * w:64 * w + 64]
            off = 32
            while off:
                lane = [lane[k] + (lane[k + off] if k + off < 64 else lane[k]) for k in range(64)]  # __shfl_down
                off //= 2
            waves.append(lane[0])
        partials.append((waves[0] + waves[1]) + (waves[2] + waves[3]))
    red = []
    for t in range(256):
        s = 0.0
        for i in range(t, blocks, 256):
            s += partials[i]
        red.append(s)
    s = 128
    while s:
        for t in range(s):
            red[t] += red[t + s]
        s //= 2
    return red[0]


@pytest.mark.parametrize("n,max_blocks", [(1, 1024), (40, 1024), (256, 1024), (288, 1024), (1500, 1024), (1500, 2), (2049, 3),
                                          (300 * 256 + 7, 1024)])
def test_restatement_adds_in_the_order_of_a_thread_by_thread_emulation(monkeypatch, n, max_blocks):
    """(a small block cap makes the grid-stride loop go round several times at a size plain Python can walk; the last
    case has more than 256 partials, so that the final kernel's strided loop goes round, too)"""
    monkeypatch.setattr(vo, "MAX_BLOCKS", max_blocks)
    rng = np.random.default_rng(n)
    a, b = vo.wide(rng, n), vo.wide(rng, n)
    terms = vo.products(a, b)
    assert vo.dot_bits(a, b) == _emulated(terms.tolist(), max_blocks)


def test_products_of_the_input_family_are_exact_in_fp64():
    """fp32 values, also when held as fp64: 24 x 24 bits fit in 53, so no product is rounded and an FMA adds what a
    multiply and an add do."""
    from fractions import Fraction
    for dtype in (np.float32, np.float64):
        a, b = vo.vec_pair((20, 17, 23), dtype)
        assert a.dtype == dtype and not a.flags.writeable
        assert np.array_equal(a.astype(np.float32).astype(dtype), a)
        p = vo.products(a, b)
        for i in range(0, p.size, 97):
            assert Fraction(float(p[i])) == Fraction(float(a.ravel()[i])) * Fraction(float(b.ravel()[i]))


@pytest.mark.parametrize("case", vo.LARGE_SHAPES + vo.LARGE_DOT_SIZES, ids=str)
def test_inputs_of_the_large_sum_cases_make_the_order_visible(case):
    """At least 90 of 100 random orders of the 1024 block partials change the bits of the total: a device that added
    them in the order of arrival would be caught by the bit comparison.  A condition on the inputs: a case that
    misses it takes another seed (_vecops.SEEDS), the 90 stays."""
    if isinstance(case, tuple):
        a, b = vo.vec_pair(case)
        partials = vo.block_partials(vo.products(a, b, case))
    else:
        a, b = vo.flat_pair(case)
        partials = vo.block_partials(vo.products(a, b))
    assert partials.size == 1024
    changed = vo.orders_that_change_the_bits(partials, trials=100)
    print(case, "orders that change the bits:", changed, "of 100")
    assert changed >= 90


def test_cancelling_block_partials_sum_to_exactly_zero_in_the_restatement():
    x, y = vo.cancelling_pair((520, 509))
    p = vo.block_partials(vo.products(x, y, (520, 509)))
    assert np.count_nonzero(p) == p.size and vo.final_sum(p) == 0.0


# ---- the NaN semantics of include/fwi.h, stated without NumPy's own clip / max -----------------------------------
def _spec_clip(x, lo, hi):
    """fwi_vec_clip: a NaN stays; a value below lo becomes lo, one above hi becomes hi; everything else is untouched"""
    out = x.copy().ravel()
    for i, v in enumerate(out.tolist()):
        if v < lo:
            out[i] = lo
        elif v > hi:
            out[i] = hi
    return out.reshape(x.shape)


def _spec_absmax(x):
    """fwi_vec_absmax: NaN if any element is NaN, +inf if any is infinite and none NaN, else the largest magnitude"""
    v = [abs(t) for t in x.ravel().tolist()]
    if any(math.isnan(t) for t in v):
        return math.nan
    return max(v)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", [(5, 7), (8, 33), (20, 17, 23)], ids=str)
def test_numpy_clip_and_absmax_do_what_the_device_contract_says(shape, dtype):
    base = vo.special_values(shape, dtype)
    for where in vo.plant_cells(shape):
        for value in (np.nan, np.inf, -np.inf, -0.0, float(np.finfo(dtype).smallest_subnormal), -3.5):
            x = base.copy()
            x[where] = value
            for lo, hi in ((-1.0, 2.0), (0.0, 2.0), (-0.0, 0.0), (0.25, 0.25), (0.1, 0.7)):
                assert vo.same_bits(vo.clip(x, lo, hi), _spec_clip(x, dtype(lo), dtype(hi))), (where, value, lo, hi)
            got, want = vo.absmax(x), _spec_absmax(x)
            assert (math.isnan(got) and math.isnan(want)) or got == want, (where, value)
    x = base.copy()
    x[vo.plant_cells(shape)[0]], x[vo.plant_cells(shape)[1]] = np.inf, np.nan
    assert math.isnan(vo.absmax(x))  # a NaN wins over an infinity, wherever the two lie
    x[vo.plant_cells(shape)[0]], x[vo.plant_cells(shape)[1]] = np.nan, np.inf
    assert math.isnan(vo.absmax(x))


def test_the_host_optimisers_finite_check_sees_what_the_device_returns():
    from full_waveform_inversion_amd.lbfgs import _require_finite
    g = np.ones((5, 7), np.float32)
    g[2, 3] = np.nan
    with pytest.raises(FloatingPointError):
        _require_finite(1.0, vo.absmax(g), 1.0, 0)       # max |g| alone gives the NaN away ...
    with pytest.raises(FloatingPointError):
        _require_finite(1.0, 1.0, float(np.sum(g.astype(np.float64) ** 2)), 0)  # ... and g.g is checked as well
    _require_finite(1.0, 1.0, 35.0, 0)


def test_host_illumination_preconditioner_refuses_a_partly_nan_illumination():
    from full_waveform_inversion_amd import shots as sh
    H = np.ones((5, 7))
    H[1, 2] = np.nan
    with pytest.raises(ValueError):
        sh.illumination_preconditioner(H)
