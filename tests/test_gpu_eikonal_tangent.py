"""The tangent of the first-arrival traveltimes on the GPU (include/fwi.h fwi_eikonal_tangent;
csrc/fwi_eikonal_tangent.hip), ``shots.TraveltimeOperator`` and ``newton.traveltime_gauss_newton`` on the device.  The
oracle is the NumPy twin that defines the tangent (full_waveform_inversion_amd/eikonal.py), fed the model rounded to the
engine's dtype.

Shapes: (37, 41) and (19, 22, 27) -- three tiles per axis (16 cells in 2-D, 8 in 3-D) with ragged last tiles and pad
columns (nx not a multiple of 4); (9, 10, 11) and (7, 41): a single tile on an axis.

Bounds.  dT: the twin is evaluated IN THE ENGINE'S DTYPE on the device's own downloaded T, as tests/test_gpu_eikonal.py
holds lambda ("T_i < G_i" and the upwind choice are decisions of that arithmetic); fp64 1e-12 of max |dT|, fp32 four
times the fp32 twin's own error against the fp64 twin, each on its own times.  Equal bits are expected (the kernel does
the twin's operations in the twin's order) and the number of cells whose bits differ is printed.  Transposition,
<w, J v> against <J^T w, v> by the device's fp64-accumulating dot: fp64 1e-12 of the larger side; fp32 four times the
defect of the fp32 twin on the same inputs (its products summed in fp64).  Operator and Gauss-Newton parity against the
stand-in in fp64: 1e-10.  Repetition and K: bit for bit.

Every comparison prints its error / bound; see DESIGN.md s.4x for the record."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from _eikonal import layered_model, smooth_model  # noqa: E402
from full_waveform_inversion_amd import Engine, FwiError, _lib, eikonal as ek, newton as nw, shots as sh  # noqa: E402

pytestmark = pytest.mark.gpu

H = 10.0
SHAPES = [(37, 41), (19, 22, 27), (9, 10, 11), (7, 41)]
DTYPES = ["float64", "float32"]
EINVAL, ESTATE = 1, 3
T, SC, D, X, B, L, G = range(7)


def engine(shape, dtype, c=None, nslots=7, nt_max=4):
    e = Engine(shape, H, 1e-3, nt_max, order=4, npml=0, dtype=dtype)
    if c is not None:
        e.set_model(c)
    e.vec_create(nslots)
    return e


def sources(shape):
    """(src, radius): off-grid with a ball of 0 and of 2 cells"""
    off = tuple(0.45 * n + 0.3 for n in shape)
    return [(off, 0.0), (off, 2.0)]


def padded_sum_matches(e, slot):
    """the pad columns of the slot are zero: the device's dot over the whole compact array equals the sum over the
    grid's cells"""
    a = e.vec_download(slot).astype(np.float64)
    want, got = float(np.sum(a * a)), e.vec_dot(slot, slot)
    return abs(got - want) <= 1e-12 * max(want, 1e-300)


def with_k(k, fn):
    os.environ["FWI_EIKONAL_K"] = str(k)
    try:
        return fn()
    finally:
        del os.environ["FWI_EIKONAL_K"]


_TWIN = {}


def twin_own_error(shape, kind, src, radius, wrt, dm, w):
    """the fp32 twin against the fp64 twin, each on its own times, on the model rounded to fp32: (the largest
    difference of dT, the fp32 twin's transposition defect), computed once"""
    key = (shape, kind, radius, wrt)
    if key not in _TWIN:
        c32 = (smooth_model if kind == "smooth" else layered_model)(shape).astype(np.float32)
        c64 = c32.astype(np.float64)
        init = ek.ball(src, shape, H, radius)
        d32, w32 = dm.astype(np.float32), w.astype(np.float32)
        t64 = ek.solve(c64, H, init)
        x64 = ek.tangent(t64, c64, H, d32.astype(np.float64), init, wrt)
        t32 = ek.solve(c32, H, init, dtype="float32")
        x32 = ek.tangent(t32, c32, H, d32, init, wrt)
        g32 = ek.gradient(t32, ek.adjoint(t32, c32, H, w32), c32, H, init, wrt)
        a = float(np.sum(w32.astype(np.float64) * x32.astype(np.float64)))
        b = float(np.sum(g32.astype(np.float64) * d32.astype(np.float64)))
        _TWIN[key] = (float(np.abs(x32.astype(np.float64) - x64).max()), abs(a - b))
    return _TWIN[key]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_tangent_matches_the_twin_and_is_the_transpose(gpu, shape, dtype):
    kind = "layered" if len(shape) == 2 else "smooth"
    c = (smooth_model if kind == "smooth" else layered_model)(shape).astype(dtype)
    rng = np.random.default_rng(9)
    dm, w = rng.standard_normal(shape), rng.standard_normal(shape)
    worst, worst_t, differ = 0.0, 0.0, 0
    with engine(shape, dtype, c) as e:
        e.vec_upload(D, dm.astype(dtype))
        e.vec_upload(B, w.astype(dtype))
        d_dev, w_dev = e.vec_download(D), e.vec_download(B)
        for src, radius in sources(shape):
            init = e.eikonal(src, T, SC, radius=radius)
            t_dev = e.vec_download(T)
            for wrt in ek.WRT:
                e.eikonal_tangent(T, D, X, SC, init, wrt=wrt)
                n1 = e.last_eikonal_launches
                x = e.vec_download(X)
                ref = ek.tangent(t_dev, c, H, d_dev, init, wrt)  # in the engine's dtype, on the engine's times
                assert ref.dtype == np.dtype(dtype) and x.dtype == ref.dtype
                if dtype == "float64":
                    bound, tbound = 1e-12 * float(np.abs(ref).max()), None
                else:
                    own, defect = twin_own_error(shape, kind, src, radius, wrt, dm, w)
                    bound, tbound = 4.0 * own, 4.0 * defect
                    assert bound > 0.0 and tbound > 0.0
                err = float(np.abs(x.astype(np.float64) - ref.astype(np.float64)).max())
                worst = max(worst, err / bound)
                differ += int(np.count_nonzero(x != ref))
                assert np.all(np.isfinite(x[np.isfinite(t_dev)])) and np.all(np.isfinite(t_dev))
                assert err <= bound, (src, radius, wrt, err, bound)
                # read only, both halves of the pair hold the result, pad columns are zero everywhere
                assert np.array_equal(e.vec_download(T), t_dev) and np.array_equal(e.vec_download(D), d_dev)
                assert np.array_equal(e.vec_download(SC), x)
                assert all(padded_sum_matches(e, s) for s in (T, SC, D, X)) and e.dirty_padding() == 0
                # the same call again: the same bits and the same number of launches
                e.eikonal_tangent(T, D, X, SC, init, wrt=wrt)
                assert np.array_equal(e.vec_download(X), x) and e.last_eikonal_launches == n1 and n1 >= 2
                # one inner sweep per launch: the same bits, in more launches
                with_k(1, lambda: e.eikonal_tangent(T, D, X, SC, init, wrt=wrt))
                assert np.array_equal(e.vec_download(X), x) and e.last_eikonal_launches > n1
                # <w, J v> against <J^T w, v> on the device
                a = e.vec_dot(B, X)
                e.eikonal_adjoint(T, B, L, SC)
                e.eikonal_gradient(T, L, G, init, wrt=wrt)
                b = e.vec_dot(G, D)
                if tbound is None:
                    tbound = 1e-12 * max(abs(a), abs(b))
                worst_t = max(worst_t, abs(a - b) / tbound)
                assert abs(a - b) <= tbound, (src, radius, wrt, a, b, tbound)
                assert np.array_equal(e.vec_download(B), w_dev)
    print("eikonal tangent %s %s: dT error / bound %.2e, cells whose bits differ from the twin's: %d, transposition "
          "defect / bound %.2e" % (shape, dtype, worst, differ, worst_t))


def _survey(shape):
    rng = np.random.default_rng(2)
    rec = np.unique(np.array([[int(rng.integers(0, n)) for n in shape] for _ in range(14)]), axis=0)
    pts = np.array([[rng.uniform(0.0, n - 1.0) for n in shape] for _ in range(5)])
    wav = np.zeros(4)
    return [sh.Shot(np.array([[n // 4 for n in shape]]), wav, rec),
            sh.Shot.at_coordinates([[0.45 * n + 0.3 for n in shape]], wav, pts, shape),
            sh.Shot(np.array([[3 * n // 4 for n in shape]]), wav, rec)]


@pytest.mark.parametrize("shape", [(37, 41), (9, 10, 11)])
def test_operator_and_gauss_newton_match_the_stand_in(gpu, shape):
    c, c_true = layered_model(shape), smooth_model(shape)
    shots = _survey(shape)
    v = np.random.default_rng(5).standard_normal(shape)
    nslots = 6 + len(shots)
    tw = ek.TwinEngine(shape, H)
    tw.vec_create(nslots)
    picks = sh.traveltime_times(tw, c_true, shots, radius=2.0)
    w = [np.linspace(0.5, 1.5, len(p)) for p in picks]
    picks[0][2] = np.nan
    kw = dict(radius=2.0, pick_weights=w, picks=picks)
    want = {wrt: sh.TraveltimeOperator(tw, c, shots, wrt=wrt, **kw).hvp(v) for wrt in ek.WRT}
    m_want, log_want = nw.traveltime_gauss_newton(tw, c, shots, picks, w, iters=1, cg_iters=3, radius=2.0,
                                                  bounds=(1000.0, 4000.0))

    def held(what, got, ref):
        err = float(np.abs(got - ref).max() / np.abs(ref).max())
        print("traveltime operator %s, %s: device against the stand-in %.1e (bound 1e-10)" % (shape, what, err))
        assert err <= 1e-10

    with engine(shape, "float64", c, nslots=nslots) as e:
        for wrt in ek.WRT:
            for keep in (True, False):
                op = sh.TraveltimeOperator(e, c, shots, wrt=wrt, keep_times=keep, **kw)
                assert op.slots_needed(len(shots)) <= nslots
                held("hvp %s keep_times=%s" % (wrt, keep), op.hvp(v), want[wrt])
        m, log = nw.traveltime_gauss_newton(e, c, shots, picks, w, iters=1, cg_iters=3, radius=2.0,
                                            bounds=(1000.0, 4000.0))
        held("one Gauss-Newton iteration", m, m_want)
        assert len(log) == 2 and abs(log[1]["J"] - log_want[1]["J"]) <= 1e-10 * log_want[1]["J"] < log_want[0]["J"]
        assert log[1]["solves"] == log_want[1]["solves"] and e.dirty_padding() == 0
    with sh.EnginePool(lambda: engine(shape, "float64", c, nslots=nslots), 2) as pool:
        op = sh.TraveltimeOperator(pool, c, shots, **kw)
        assert op.slots_needed(len(shots)) == 8
        held("hvp on a pool of two", op.hvp(v), want["velocity"])
        m, log = nw.traveltime_gauss_newton(pool, c, shots, picks, w, iters=1, cg_iters=3, radius=2.0,
                                            bounds=(1000.0, 4000.0))
        held("one Gauss-Newton iteration on a pool of two", m, m_want)


def _sweep(e, c):
    """a small forward + adjoint + gradient: what a tangent call must leave untouched"""
    nt = 30
    wav = np.sin(np.arange(nt) * 0.4) * np.exp(-((np.arange(nt) - 10.0) / 5.0) ** 2)
    src = np.array([[n // 2 for n in e.shape]])
    rec = np.array([[n // 3 for n in e.shape], [2 * n // 3 for n in e.shape]])
    e.reset_gradient()
    d = e.forward(c, (src, wav.astype(e.dtype)), rec, save=True)
    a = e.adjoint(0.5 * d)
    return d, a, e.gradient()


def _raw(e, wrt, slots, init, null=None):
    """fwi_eikonal_tangent itself: what Engine.eikonal_tangent refuses before the call (an unknown wrt, a null pointer)"""
    _, (n, pidx, pdist, pref) = e._init_args(init)
    ptr = {"init_idx": pidx, "init_dist": pdist, "ref_idx": pref}
    if null is not None:
        ptr[null] = None
    cnt = C.c_int32(0)
    _lib.check(e._ctx, e._lib.fwi_eikonal_tangent(e._c, wrt, *[int(s) for s in slots], n, ptr["init_idx"],
                                                  ptr["init_dist"], ptr["ref_idx"], 0, C.byref(cnt)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(37, 41), (19, 22, 27)])
def test_refusals_cap_and_non_interference(gpu, shape, dtype):
    c = smooth_model(shape).astype(dtype)
    nd = len(shape)
    with engine(shape, dtype, c, nt_max=30) as fresh:
        want = _sweep(fresh, c)
    node = np.array([[n // 2 for n in shape]])
    twice = np.concatenate([node, node + 1, node])
    init = ek.ball([n // 2 for n in shape], shape, H, 1.0)
    outside = (np.array([[n for n in shape]]), np.zeros(1), np.zeros(nd, np.int32))
    ref_outside = (init[0], init[1], np.array(shape, np.int32))
    empty = (np.zeros((0, nd), np.int32), np.zeros(0), np.zeros(nd, np.int32))
    rng = np.random.default_rng(1)
    four = (T, D, X, SC)
    with engine(shape, dtype, c, nt_max=30) as e:
        e.eikonal(init, T, SC)
        e.vec_upload(D, rng.standard_normal(shape).astype(dtype))
        e.vec_upload(X, rng.standard_normal(shape).astype(dtype))
        e.vec_upload(SC, rng.standard_normal(shape).astype(dtype))
        before = [e.vec_download(s) for s in four]
        cases = [  # (the call, a word of the message that names the argument)
            (lambda: e.eikonal_tangent(T, D, X, 9, init), "slot 9"),                       # a slot that does not exist
            (lambda: e.eikonal_tangent(-1, D, X, SC, init), "slot -1"),
            (lambda: e.eikonal_tangent(T, T, X, SC, init), "dm_slot"),                     # any two of the four equal
            (lambda: e.eikonal_tangent(T, D, T, SC, init), "out_slot"),
            (lambda: e.eikonal_tangent(T, D, X, T, init), "scratch_slot"),
            (lambda: e.eikonal_tangent(T, D, D, SC, init), "out_slot"),
            (lambda: e.eikonal_tangent(T, D, X, D, init), "scratch_slot"),
            (lambda: e.eikonal_tangent(T, D, X, X, init), "scratch_slot"),
            (lambda: e.eikonal_tangent(T, D, X, SC, empty), "n_init"),                     # an empty list
            (lambda: e.eikonal_tangent(T, D, X, SC, outside), "init_idx"),                 # outside the grid
            (lambda: e.eikonal_tangent(T, D, X, SC, ref_outside), "ref_idx"),
            (lambda: e.eikonal_tangent(T, D, X, SC, (twice, np.zeros(3), node[0])), "init_idx"),  # listed twice
            (lambda: e.eikonal_tangent(T, D, X, SC, (init[0], -init[1] - 1.0, init[2])), "init_dist"),
            (lambda: e.eikonal_tangent(T, D, X, SC, (init[0], init[1] + np.inf, init[2])), "init_dist"),
            (lambda: e.eikonal_tangent(T, D, X, SC, (init[0], init[1] * np.nan, init[2])), "init_dist"),
            (lambda: _raw(e, 7, four, init), "wrt"),                                       # an unknown wrt
            (lambda: _raw(e, _lib.WRT_VELOCITY, four, init, null="init_idx"), "init_idx"),  # a null pointer
            (lambda: _raw(e, _lib.WRT_VELOCITY, four, init, null="init_dist"), "init_dist"),
            (lambda: _raw(e, _lib.WRT_VELOCITY, four, init, null="ref_idx"), "ref_idx"),
        ]
        for n, (call, word) in enumerate(cases):
            with pytest.raises(FwiError) as err:
                call()
            assert err.value.code == EINVAL and word in str(err.value), (n, str(err.value))
            assert all(np.array_equal(e.vec_download(s), b) for s, b in zip(four, before)), n
        with pytest.raises(ValueError):
            e.eikonal_tangent(T, D, X, SC, init, wrt="impedance")
        # a cap of one launch: FWI_ESTATE, one launch counted, the inputs untouched
        with pytest.raises(FwiError) as err:
            e.eikonal_tangent(T, D, X, SC, init, max_sweeps=1)
        assert err.value.code == ESTATE and e.last_eikonal_launches == 1
        assert np.array_equal(e.vec_download(T), before[0]) and np.array_equal(e.vec_download(D), before[1])
        assert all(padded_sum_matches(e, s) for s in four)
        # after a complete call the sweeps return the bits of a fresh context
        e.eikonal_tangent(T, D, X, SC, init)
        x = e.vec_download(X)
        got = _sweep(e, c)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        assert np.array_equal(e.vec_download(X), x) and e.dirty_padding() == 0
    with engine(shape, dtype, None, nt_max=30) as bare:  # no model set
        with pytest.raises(FwiError) as err:
            bare.eikonal_tangent(T, D, X, SC, init)
        assert err.value.code == ESTATE and "model" in str(err.value)
        got = _sweep(bare, c)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
