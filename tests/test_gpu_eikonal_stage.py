"""Walled, slot-started eikonal solves, the handover, the stage tangent and reflection tomography on the GPU
(include/fwi.h fwi_eikonal_stage, fwi_eikonal_handover, fwi_eikonal_gradient_field, fwi_eikonal_tangent_stage;
csrc/fwi_eikonal_stage.hip), ``shots.reflection_fg`` and ``shots.ReflectionOperator`` on the device.  The oracle is the
NumPy twin that defines them (full_waveform_inversion_amd/eikonal.py), fed the model rounded to the engine's dtype.

Shapes: (37, 41) and (19, 22, 27) -- three tiles per axis (16 cells in 2-D, 8 in 3-D) with ragged last tiles and pad
columns (nx not a multiple of 4); (5, 23): a single ragged tile on the first axis.  The reflector is curved
(tests/_eikonal_stage.py), the source off-grid with a ball of two cells.

Bounds, the project's standing ones.  Times: fp64 1e-12 of max T against the twin; fp32 four times the fp32 twin's own
error against the fp64 twin.  The twin of stage 2 starts from the DEVICE's stage-1 times on the interface, in the
engine's dtype, so stage 2 is held on its own.  Handover: equal bits against the twin's decision on the device's own
times.  Stage tangent and lambda: the twin in the engine's dtype on the device's own times; fp64 1e-12 of max |x|, fp32
four times the fp32 twin's own error against the fp64 twin (each on its own times).  ``reflection_fg`` against the
stand-in engine in fp64: 1e-10.  The fp64 gradient against central differences of the device's own J (relative step
1e-5, two random directions): 1e-6, the bound of the host test, where the twin gives at most 4.1e-8 on these surveys.
``<w, J v>`` against ``<J^T w, v>`` by the device's fp64-accumulating dot in fp64: 1e-10.  A list and no wall against
``fwi_eikonal``, repetition and K: bit for bit.

Every comparison prints its error / bound; see DESIGN.md s.4y for the record."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from _eikonal import smooth_model  # noqa: E402
from _eikonal_stage import H, curved_reflector, source, survey  # noqa: E402
from full_waveform_inversion_amd import Engine, FwiError, _lib, eikonal as ek, shots as sh  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(37, 41), (19, 22, 27), (5, 23)]
DTYPES = ["float64", "float32"]
EINVAL, ESTATE = 1, 3
W, S0, T1, T2, SC, B, L2, HO, L1, G, D, X1, X2 = range(13)
NSLOTS = 13
RADIUS = 2.0


def engine(shape, dtype, c=None, nslots=NSLOTS, nt_max=4):
    e = Engine(shape, H, 1e-3, nt_max, order=4, npml=0, dtype=dtype)
    if c is not None:
        e.set_model(c)
    e.vec_create(nslots)
    return e


def with_k(k, fn):
    os.environ["FWI_EIKONAL_K"] = str(k)
    try:
        return fn()
    finally:
        del os.environ["FWI_EIKONAL_K"]


def raw_stage(e, t_slot, scratch_slot, wall_slot, init=None, max_sweeps=0):
    """fwi_eikonal_stage itself; returns the launches"""
    args = (0, None, None, None) if init is None else e._init_args(init)[1]
    n = C.c_int32(0)
    _lib.check(e._ctx, e._lib.fwi_eikonal_stage(e._c, int(t_slot), int(scratch_slot), int(wall_slot), *args,
                                                int(max_sweeps), C.byref(n)))
    return int(n.value)


def raw_tangent_stage(e, wrt, t_slot, dm_slot, b0_slot, out_slot, scratch_slot, init=None):
    args = (0, None, None, None) if init is None else e._init_args(init)[1]
    n = C.c_int32(0)
    _lib.check(e._ctx, e._lib.fwi_eikonal_tangent_stage(e._c, int(wrt), int(t_slot), int(dm_slot), int(b0_slot),
                                                        int(out_slot), int(scratch_slot), *args, 0, C.byref(n)))
    return int(n.value)


_TWIN = {}


def twin(shape):
    """the fp64 and the fp32 twin of both stages, their adjoint chain and their tangent chain on the model rounded to
    fp32, each on its own times; computed once.  The fp32 twin's own errors bound the fp32 device."""
    if shape not in _TWIN:
        c32 = smooth_model(shape).astype(np.float32)
        refl = sh.Reflector.at_depth(shape, curved_reflector(shape))
        rng = np.random.default_rng(9)
        dm, w = rng.standard_normal(shape), np.where(refl.wall, 0.0, rng.standard_normal(shape))
        out = {"dm": dm, "w": w, "refl": refl}
        for dtype in DTYPES:
            c = c32.astype(dtype)
            t1, t2, init = ek.reflection_solve(c, H, source(shape), refl.gamma, refl.wall, RADIUS, dtype=dtype)
            lam2 = ek.adjoint(t2, c, H, w.astype(dtype))
            lam1 = ek.adjoint(t1, c, H, ek.handover(t2, c, H, lam2))
            out[dtype] = dict(t1=t1, t2=t2, lam2=lam2, lam1=lam1)
            for wrt in ek.WRT:
                x1 = ek.tangent(t1, c, H, dm.astype(dtype), init, wrt)
                out[dtype].update({
                    "x2 " + wrt: ek.tangent(t2, c, H, dm.astype(dtype), None, wrt, b0=ek.handover(t2, c, H, x1)),
                    "x1b " + wrt: ek.tangent(t1, c, H, dm.astype(dtype), init, wrt, b0=w.astype(dtype)),
                    "x2n " + wrt: ek.tangent(t2, c, H, dm.astype(dtype), None, wrt),
                    "g2 " + wrt: ek.gradient(t2, lam2, c, H, None, wrt)})
        free = ~refl.wall
        out["own"] = {k: float(np.abs(out["float32"][k][free].astype(np.float64) - out["float64"][k][free]).max())
                      for k in out["float64"]}
        _TWIN[shape] = out
    return _TWIN[shape]


def held(what, got, ref, dtype, own, mask):
    """`got` against `ref` on `mask`: fp64 1e-12 of max |ref|, fp32 four times the fp32 twin's own error"""
    bound = 1e-12 * float(np.abs(ref[mask]).max()) if dtype == "float64" else 4.0 * own
    assert bound > 0.0, what
    err = float(np.abs(got[mask].astype(np.float64) - ref[mask].astype(np.float64)).max())
    differ = int(np.count_nonzero(got[mask] != ref[mask]))
    print("eikonal stage %s: error / bound %.2e, cells whose bits differ from the twin's: %d" % (what, err / bound, differ))
    assert err <= bound, (what, err, bound)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_a_list_and_no_wall_is_fwi_eikonal_bit_for_bit(gpu, shape, dtype):
    c = smooth_model(shape).astype(dtype)
    with engine(shape, dtype, c) as e:
        for radius in (0.0, RADIUS):
            init = e.eikonal(source(shape), T1, SC, radius=radius)
            n = e.last_eikonal_launches
            t, sc = e.vec_download(T1), e.vec_download(SC)
            assert raw_stage(e, T2, B, -1, init) == n and n >= 2
            assert np.array_equal(e.vec_download(T2), t) and np.array_equal(e.vec_download(B), sc)
            # restarted from the list's own start: the same fixed point, whatever K
            e.vec_upload(T2, ek.init_times(c, H, init, dtype=dtype))
            e.eikonal_restart(T2, B)
            assert np.array_equal(e.vec_download(T2), t) and np.array_equal(e.vec_download(B), t)
            assert e.last_eikonal_launches == n
            e.vec_upload(T2, ek.init_times(c, H, init, dtype=dtype))
            with_k(1, lambda: e.eikonal_restart(T2, B))
            assert np.array_equal(e.vec_download(T2), t) and e.last_eikonal_launches > n
            # a wall that walls nothing
            e.vec_upload(W, np.zeros(shape, dtype))
            e.eikonal(init, T2, B, wall_slot=W)
            assert np.array_equal(e.vec_download(T2), t) and e.last_eikonal_launches == n
        assert e.dirty_padding() == 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_both_stages_their_adjoint_and_tangent_match_the_twin(gpu, shape, dtype):
    tw = twin(shape)
    refl, own = tw["refl"], tw["own"]
    gamma, wall, free = refl.gamma, refl.wall, ~refl.wall
    c = smooth_model(shape).astype(np.float32).astype(dtype)
    with engine(shape, dtype, c) as e:
        refl.upload(e, W, S0)
        init = refl.solve(e, source(shape), RADIUS, W, S0, T1, T2, SC)
        t1, t2 = e.vec_download(T1), e.vec_download(T2)
        assert np.all(np.isposinf(t1[wall])) and np.all(np.isposinf(t2[wall]))
        assert np.all(np.isfinite(t1[free])) and np.all(np.isfinite(t2[free]))
        assert np.array_equal(e.vec_download(SC), t2) and e.dirty_padding() == 0
        held("%s %s stage 1" % (shape, dtype), t1, ek.solve(c, H, init, dtype=dtype, wall=wall), dtype, own["t1"], free)
        ref2 = ek.solve_from(c, H, np.where(gamma, t1, np.inf), wall, dtype=dtype)  # from the device's own stage 1
        held("%s %s stage 2" % (shape, dtype), t2, ref2, dtype, own["t2"], free)
        assert np.array_equal(t2[gamma], t1[gamma])
        # the same again, and with one inner sweep per launch: the same bits
        n2 = e.last_eikonal_launches
        refl.solve(e, source(shape), RADIUS, W, S0, X1, X2, SC)
        assert np.array_equal(e.vec_download(X1), t1) and np.array_equal(e.vec_download(X2), t2)
        assert e.last_eikonal_launches == n2
        with_k(1, lambda: refl.solve(e, source(shape), RADIUS, W, S0, X1, X2, SC))
        assert np.array_equal(e.vec_download(X1), t1) and np.array_equal(e.vec_download(X2), t2)
        assert e.last_eikonal_launches > n2
        # the handover: the twin's decision on the device's own times, bit for bit; beta adds
        e.vec_upload(B, tw["w"].astype(dtype))
        w_dev = e.vec_download(B)
        e.eikonal_handover(T2, B, HO)
        want = ek.handover(t2, c, H, w_dev)
        assert np.array_equal(e.vec_download(HO), want) and np.count_nonzero(want[gamma]) == gamma.sum()
        e.eikonal_handover(T2, B, HO, beta=-0.5)
        assert np.array_equal(e.vec_download(HO), np.dtype(dtype).type(-0.5) * want + want)
        assert np.array_equal(e.vec_download(T2), t2) and np.array_equal(e.vec_download(B), w_dev)
        # the adjoint chain
        e.eikonal_adjoint(T2, B, L2, SC)
        lam2 = e.vec_download(L2)
        held("%s %s lambda 2" % (shape, dtype), lam2, ek.adjoint(t2, c, H, w_dev), dtype, own["lam2"], free)
        e.eikonal_handover(T2, L2, HO)
        b1 = e.vec_download(HO)
        assert np.array_equal(b1, ek.handover(t2, c, H, lam2))
        e.eikonal_adjoint(T1, HO, L1, SC)
        held("%s %s lambda 1" % (shape, dtype), e.vec_download(L1), ek.adjoint(t1, c, H, b1), dtype, own["lam1"], free)
        # the tangent chain
        e.vec_upload(D, tw["dm"].astype(dtype))
        d_dev = e.vec_download(D)
        for wrt in ek.WRT:
            e.eikonal_tangent(T1, D, X1, SC, init, wrt=wrt)
            x1 = e.vec_download(X1)
            e.eikonal_handover(T2, X1, HO)
            b0 = e.vec_download(HO)
            assert np.array_equal(b0, ek.handover(t2, c, H, x1))
            e.eikonal_tangent(T2, D, X2, SC, None, wrt=wrt, b0_slot=HO)
            n1 = e.last_eikonal_launches
            x2 = e.vec_download(X2)
            assert np.all(np.isfinite(x2)) and np.array_equal(e.vec_download(SC), x2)
            held("%s %s stage tangent %s" % (shape, dtype, wrt), x2, ek.tangent(t2, c, H, d_dev, None, wrt, b0=b0), dtype,
                 own["x2 " + wrt], free)
            with_k(1, lambda: e.eikonal_tangent(T2, D, X2, SC, None, wrt=wrt, b0_slot=HO))
            assert np.array_equal(e.vec_download(X2), x2) and e.last_eikonal_launches >= n1
            # a list and b0 together (stage 1 with something added), and neither
            e.eikonal_tangent(T1, D, X2, SC, init, wrt=wrt, b0_slot=B)
            held("%s %s tangent with a list and b0, %s" % (shape, dtype, wrt), e.vec_download(X2),
                 ek.tangent(t1, c, H, d_dev, init, wrt, b0=w_dev), dtype, own["x1b " + wrt], free)
            e.eikonal_tangent(T2, D, X2, SC, None, wrt=wrt)
            held("%s %s tangent without a list, %s" % (shape, dtype, wrt), e.vec_download(X2),
                 ek.tangent(t2, c, H, d_dev, None, wrt), dtype, own["x2n " + wrt], free)
            # the gradient without the source term
            e.eikonal_gradient(T2, L2, G, None, wrt=wrt)
            held("%s %s field gradient %s" % (shape, dtype, wrt), e.vec_download(G),
                 ek.gradient(t2, lam2, c, H, None, wrt), dtype, own["g2 " + wrt], free)
        assert all(np.array_equal(e.vec_download(s), a) for s, a in ((T1, t1), (T2, t2), (D, d_dev), (B, w_dev)))
        assert e.dirty_padding() == 0


@pytest.mark.parametrize("shape", SHAPES)
def test_reflection_fg_gradient_and_transpose_on_the_device(gpu, shape):
    c = smooth_model(shape)
    refl = sh.Reflector.at_depth(shape, curved_reflector(shape))
    shots = survey(shape)
    nslots = sh.ReflectionOperator.WORK_SLOTS + 2 * len(shots)
    tw = ek.TwinEngine(shape, H)
    tw.vec_create(nslots)
    picks = sh.reflection_times(tw, 1.03 * c, shots, refl, radius=RADIUS)
    w = [np.linspace(0.5, 1.5, len(p)) for p in picks]
    picks[0][2] = np.nan
    kw = dict(pick_weights=w, radius=RADIUS)
    rng = np.random.default_rng(4)
    v, u = rng.standard_normal(shape), rng.standard_normal(shape)

    def close(what, got, ref, bound=1e-10):
        err = float(np.abs(np.asarray(got) - np.asarray(ref)).max() / np.abs(ref).max())
        print("reflection %s, %s: device against the stand-in %.1e (bound %.0e)" % (shape, what, err, bound))
        assert err <= bound

    with engine(shape, "float64", c, nslots=nslots) as e:
        got_t = sh.reflection_times(e, 1.03 * c, shots, refl, radius=RADIUS)
        close("times", np.concatenate(got_t), np.concatenate(sh.reflection_times(tw, 1.03 * c, shots, refl, radius=RADIUS)))
        for wrt in ek.WRT:
            J, g = sh.reflection_fg(e, c, shots, picks, refl, wrt=wrt, **kw)
            Jw, gw = sh.reflection_fg(tw, c, shots, picks, refl, wrt=wrt, **kw)
            assert abs(J - Jw) <= 1e-10 * Jw
            close("gradient %s" % wrt, g, gw)
        # central differences of the device's own J
        J, g = sh.reflection_fg(e, c, shots, picks, refl, **kw)
        for k in range(2):
            d = rng.standard_normal(shape)
            d /= np.abs(d).max()
            eps = 1e-5 * float(c.max())
            fd = (sh.reflection_fg(e, c + eps * d, shots, picks, refl, **kw)[0]
                  - sh.reflection_fg(e, c - eps * d, shots, picks, refl, **kw)[0]) / (2.0 * eps)
            err = abs(fd - float(np.sum(g * d))) / abs(fd)
            print("reflection %s: device gradient against central differences of the device's J %.1e (bound 1e-6)"
                  % (shape, err))
            assert err <= 1e-6
        # the operator: the stand-in's products, and <w, J v> = <J^T w, v> on the device
        for wrt in ek.WRT:
            want = sh.ReflectionOperator(tw, c, shots, refl, radius=RADIUS, wrt=wrt, pick_weights=w, picks=picks).hvp(v)
            for keep in (True, False):
                op = sh.ReflectionOperator(e, c, shots, refl, radius=RADIUS, wrt=wrt, pick_weights=w, picks=picks,
                                           keep_times=keep)
                assert op.slots_needed(len(shots)) <= nslots
                close("hvp %s keep_times=%s" % (wrt, keep), op.hvp(v), want)
            Jv = op.jvp(v)
            r = [rng.standard_normal(len(x)) for x in Jv]
            a, b = float(sum(np.dot(x, y) for x, y in zip(r, Jv))), float(np.sum(op.vjp(r) * v))
            print("reflection %s %s: device transposition %.1e (bound 1e-10)" % (shape, wrt, abs(a - b) / max(abs(a), abs(b))))
            assert abs(a - b) <= 1e-10 * max(abs(a), abs(b))
            a, b = float(np.sum(u * op.hvp(v))), float(np.sum(v * op.hvp(u)))
            assert abs(a - b) <= 1e-10 * max(abs(a), abs(b))
        assert e.dirty_padding() == 0
    if shape == (37, 41):
        with sh.EnginePool(lambda: engine(shape, "float64", c, nslots=nslots), 2) as pool:
            J2, g2 = sh.reflection_fg(pool, c, shots, picks, refl, **kw)
            Jw, gw = sh.reflection_fg(tw, c, shots, picks, refl, **kw)
            assert abs(J2 - Jw) <= 1e-10 * Jw
            close("gradient on a pool of two", g2, gw)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(37, 41), (19, 22, 27)])
def test_refusals_and_the_cap(gpu, shape, dtype):
    c = smooth_model(shape).astype(dtype)
    refl = sh.Reflector.at_depth(shape, curved_reflector(shape))
    init = ek.ball(source(shape), shape, H, 1.0)
    nd = len(shape)
    outside = (np.array([[n for n in shape]]), np.zeros(1), np.zeros(nd, np.int32))
    node = np.array([[n // 2 for n in shape]])
    twice = (np.concatenate([node, node + 1, node]), np.zeros(3), node[0])
    rng = np.random.default_rng(1)
    start = np.where(refl.gamma, 0.25, np.inf)
    slots = (W, S0, T1, T2, SC, B, HO)
    V, ST = _lib.WRT_VELOCITY, S0
    with engine(shape, dtype, c) as e:
        e.vec_upload(W, refl.wall.astype(dtype))
        e.vec_upload(T1, start.astype(dtype))
        for s in (T2, SC, B, HO):
            e.vec_upload(s, rng.standard_normal(shape).astype(dtype))
        e.vec_upload(S0, np.full(shape, np.inf, dtype))                               # no finite entry
        before = [e.vec_download(s) for s in slots]
        nan_start, neg_start = X1, X2
        e.vec_upload(nan_start, np.where(node_mask(shape, node[0]), np.nan, start).astype(dtype))
        e.vec_upload(neg_start, np.where(node_mask(shape, node[0]), -1.0, start).astype(dtype))
        keep = [e.vec_download(s) for s in (nan_start, neg_start)]
        cases = [  # (the call, a word of the message that names the argument)
            (lambda: raw_stage(e, 19, SC, -1), "slot 19"),                              # a slot that does not exist
            (lambda: raw_stage(e, T1, -1, -1), "slot -1"),
            (lambda: raw_stage(e, T1, SC, 19), "wall_slot"),
            (lambda: raw_stage(e, T1, SC, -2), "wall_slot"),
            (lambda: raw_stage(e, T1, T1, -1), "scratch_slot"),                         # two arguments naming one slot
            (lambda: raw_stage(e, T1, SC, T1), "wall_slot"),
            (lambda: raw_stage(e, T1, SC, SC), "wall_slot"),
            (lambda: raw_stage(e, ST, SC, -1), "t_slot"),                               # no finite entry
            (lambda: raw_stage(e, ST, SC, W), "t_slot"),
            (lambda: raw_stage(e, nan_start, SC, -1), "t_slot"),                        # a NaN
            (lambda: raw_stage(e, neg_start, SC, W), "t_slot"),                         # a negative entry
            (lambda: raw_stage(e, T2, SC, W, outside), "init_idx"),                     # a bad list, as fwi_eikonal
            (lambda: raw_stage(e, T2, SC, W, twice), "init_idx"),
            (lambda: raw_stage(e, T2, SC, W, (init[0], -init[1] - 1.0, init[2])), "init_dist"),
            (lambda: e.eikonal_handover(T1, B, 19), "slot 19"),
            (lambda: e.eikonal_handover(T1, T1, HO), "in_slot"),
            (lambda: e.eikonal_handover(T1, B, B), "out_slot"),
            (lambda: e.eikonal_handover(T1, B, T1), "out_slot"),
            (lambda: e.eikonal_handover(T1, B, HO, beta=np.nan), "beta"),
            (lambda: e.eikonal_gradient(T1, B, 19), "slot 19"),
            (lambda: e.eikonal_gradient(T1, B, T1), "out_slot"),
            (lambda: e.eikonal_gradient(T1, B, B), "out_slot"),
            (lambda: _lib.check(e._ctx, e._lib.fwi_eikonal_gradient_field(e._c, 7, T1, B, HO, 0.0)), "wrt"),
            (lambda: raw_tangent_stage(e, V, T1, B, 19, HO, SC), "b0_slot"),
            (lambda: raw_tangent_stage(e, V, T1, B, -2, HO, SC), "b0_slot"),
            (lambda: raw_tangent_stage(e, V, T1, B, T2, 19, SC), "slot 19"),
            (lambda: raw_tangent_stage(e, V, T1, B, T1, HO, SC), "b0_slot"),
            (lambda: raw_tangent_stage(e, V, T1, B, B, HO, SC), "b0_slot"),
            (lambda: raw_tangent_stage(e, V, T1, B, T2, T2, SC), "out_slot"),
            (lambda: raw_tangent_stage(e, V, T1, B, T2, HO, T2), "scratch_slot"),
            (lambda: raw_tangent_stage(e, V, T1, B, -1, HO, HO), "scratch_slot"),
            (lambda: raw_tangent_stage(e, V, T1, T1, -1, HO, SC), "dm_slot"),
            (lambda: raw_tangent_stage(e, 7, T1, B, T2, HO, SC), "wrt"),
            (lambda: raw_tangent_stage(e, V, T1, B, T2, HO, SC, outside), "init_idx"),
        ]
        for n, (call, word) in enumerate(cases):
            with pytest.raises(FwiError) as err:
                call()
            assert err.value.code == EINVAL and word in str(err.value), (n, str(err.value))
            assert all(np.array_equal(e.vec_download(s), b, equal_nan=True) for s, b in zip(slots, before)), n
        assert all(np.array_equal(e.vec_download(s), b, equal_nan=True) for s, b in zip((nan_start, neg_start), keep))
        # whatever the start says inside the wall: a NaN there is no reason to refuse
        e.vec_upload(X1, np.where(refl.wall, np.nan, start).astype(dtype))
        e.eikonal_restart(X1, SC, wall_slot=W)
        full = e.vec_download(X1)
        assert np.all(np.isposinf(full[refl.wall])) and np.all(np.isfinite(full[~refl.wall]))
        # a cap of one launch: FWI_ESTATE, one launch counted, an upper bound in the slot, the wall in place
        e.vec_upload(X2, start.astype(dtype))
        with pytest.raises(FwiError) as err:
            e.eikonal_restart(X2, SC, wall_slot=W, max_sweeps=1)
        assert err.value.code == ESTATE and e.last_eikonal_launches == 1
        part = e.vec_download(X2)
        assert np.all(part >= full) and np.any(part > full) and np.all(np.isposinf(part[refl.wall]))
        with pytest.raises(FwiError) as err:
            e.eikonal(init, X2, SC, max_sweeps=1, wall_slot=W)
        assert err.value.code == ESTATE and e.last_eikonal_launches == 1
        e.vec_upload(B, rng.standard_normal(shape).astype(dtype))
        with pytest.raises(FwiError) as err:
            e.eikonal_tangent(X1, B, HO, SC, None, b0_slot=T2, max_sweeps=1)
        assert err.value.code == ESTATE and e.last_eikonal_launches == 1
        assert e.dirty_padding() == 0
    with engine(shape, dtype, None) as bare:  # no model set
        bare.vec_upload(T1, start.astype(dtype))
        for call in (lambda: bare.eikonal_restart(T1, SC), lambda: bare.eikonal_handover(T1, B, HO),
                     lambda: bare.eikonal_gradient(T1, B, HO), lambda: bare.eikonal_tangent(T1, B, HO, SC, None),
                     lambda: bare.eikonal(init, T2, SC, wall_slot=W)):
            with pytest.raises(FwiError) as err:
                call()
            assert err.value.code == ESTATE and "model" in str(err.value)
        assert np.array_equal(bare.vec_download(T1), start.astype(dtype))


def node_mask(shape, node):
    m = np.zeros(shape, bool)
    m[tuple(node)] = True
    return m
