"""Born modelling (include/fwi.h fwi_born) and the Gauss-Newton products built on it, on the GPU, against the NumPy
restatement tests/_born.py (validated on its own by tests/test_born_oracle.py): parity over every kind of context,
the derivative of the engine's own forward, adjointness with the gradient, exact (bitwise) invariants, H_GN over shots
and pools, a small linear inversion by conjugate gradients, and the error paths.

Parity tolerance (data dd = J dc, relative L2).  fp64: 1e-10.  fp32: the project's flat 1e-5 for every case whose
REFERENCE error -- tests/_born.py run in fp32 against itself in fp64, computed here on the CPU -- is <= 5e-6; a case
above that keeps its inputs and gets 2 x its own reference error.  Both figures of every case go to
profiles/r05_born_parity.json.  Contexts with a fused Born path (3-D fp32 O(8) stream kernel without the CPML) run
every case in both modes with ``born_path`` asserted; everywhere else "fused" must be refused.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import _born
from full_waveform_inversion_amd import Engine, FwiError, _lib, newton, shots as sh
from full_waveform_inversion_amd.points import Spread
from oracle import fwi_oracle as fo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY_JSON = os.path.join(ROOT, "profiles", "r05_born_parity.json")
TOL32, TOL64 = 1e-5, 1e-10
REF32_LIMIT = 5e-6
AUTO_PATH = "fused"  # what FWI_BORN_AUTO resolves to where both paths exist (by measurement: DESIGN.md s.4e)
CPML2, CPML3 = {"abc": "cpml", "pml_alpha_max": 40.0}, {"abc": "cpml", "pml_alpha_max": 30.0}
INC = {"update_form": "increment"}
S3 = (40, 36, 44)

CASES = [  # id, shape, order, npml, nt, dtype, kernel name, engine / oracle options, FWI_STREAM_TY
    ("2d_fused_nt80", (192, 256), 8, 8, 80, "float32", "step2d_fused", {}, None),
    ("2d_fused_nt82", (192, 256), 8, 8, 82, "float32", "step2d_fused", {}, None),
    ("2d_fused_cpml", (192, 256), 8, 8, 80, "float32", "step2d_fused", CPML2, None),
    ("2d_tile_cpml", (72, 96), 8, 12, 60, "float32", "step2d_tile", CPML2, None),
    ("3d_stream", S3, 8, 6, 60, "float32", "step3d_stream", {}, None),
    ("3d_stream_increment", S3, 8, 6, 60, "float32", "step3d_stream", INC, None),
    ("3d_stream_cpml", S3, 8, 6, 60, "float32", "step3d_stream", CPML3, None),
    ("3d_stream_cpml_increment", S3, 8, 6, 60, "float32", "step3d_stream", {**CPML3, **INC}, None),
    ("3d_point", S3, 8, 6, 60, "float32", "step_point", {"kernel": "point"}, None),
    ("3d_fp64_o4", (33, 29, 50), 4, 5, 50, "float64", "step3d_stream", {}, None),
    ("3d_stream_ty8", S3, 8, 6, 60, "float32", "step3d_stream", {}, 8),
    ("3d_stream_increment_ty8", S3, 8, 6, 60, "float32", "step3d_stream", INC, 8),
    ("3d_stream_cpml_ty8", S3, 8, 6, 60, "float32", "step3d_stream", CPML3, 8),
    ("3d_stream_cpml_increment_ty8", S3, 8, 6, 60, "float32", "step3d_stream", {**CPML3, **INC}, 8),
    ("3d_point_ty8", S3, 8, 6, 60, "float32", "step_point", {"kernel": "point"}, 8),
    ("3d_fp64_o4_ty8", (33, 29, 50), 4, 5, 50, "float64", "step3d_stream", {}, 8),
    ("3d_full_tiles", (12, 16, 256), 8, 4, 60, "float32", "step3d_stream", {}, None),
    ("3d_full_tiles_increment_ty8", (12, 16, 256), 8, 4, 60, "float32", "step3d_stream", INC, 8),
]
ORACLE_KEYS = ("abc", "pml_alpha_max")


def _has_fused(shape, order, dtype, opts):
    return len(shape) == 3 and order == 8 and dtype == "float32" and opts.get("kernel") != "point" and "abc" not in opts


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / np.linalg.norm(b))


def _problem(shape, order, nt, seed=0):
    """Model, sources (one duplicate node) and wavelets as ``_problem`` of tests/test_gpu_illumination.py; the receivers
    are drawn within 0.5 c_min nt dt of the first source, where the wave has arrived; dc = 30 m/s x standard normal."""
    rng = np.random.default_rng(seed)
    c = 2000.0 + 600.0 * rng.random(shape)
    h = 10.0
    dt = 0.6 * fo.cfl_dt(c.max(), h, len(shape), order)
    src = np.array([[s // 2 for s in shape], [s // 3 for s in shape], [s // 2 for s in shape]])  # a duplicate node
    wav = np.stack([fo.ricker(nt, dt, 0.12 / dt / 8) * a for a in (1.0, 0.7, -0.4)], 1)
    radius = 0.5 * c.min() * nt * dt / h  # cells
    rec = []
    while len(rec) < 8:
        off = rng.integers(-int(radius), int(radius) + 1, len(shape))
        node = src[0] + off
        if np.linalg.norm(off) <= radius and np.all(node >= 0) and np.all(node < np.array(shape)):
            rec.append(node)
    dc = 30.0 * rng.standard_normal(shape)
    return c, h, dt, src, np.array(rec), wav, dc


def _assert_the_reference_sees_the_wave(d, J):
    peaks = np.abs(d).max(axis=0)
    assert peaks.min() >= 1e-3 * peaks.max(), peaks
    assert np.linalg.norm(J) >= 1e-3 * np.linalg.norm(d), (np.linalg.norm(J), np.linalg.norm(d))


def _record(case_id, entry):
    os.makedirs(os.path.dirname(PARITY_JSON), exist_ok=True)
    try:
        data = json.load(open(PARITY_JSON))
    except (OSError, ValueError):
        data = {}
    data[case_id] = entry
    with open(PARITY_JSON, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")


def _tolerance(dtype, ref32):
    if np.dtype(dtype) == np.float64:
        return TOL64
    return TOL32 if ref32 <= REF32_LIMIT else 2.0 * ref32


def _reference(c, h, dt, order, npml, opts, forward, dc, dtype):
    """J dc (velocity) and J dm (slowness^2, dm = -2 dc / c^3: the same data) from tests/_born.py in fp64, the error of
    the same computation in fp32 (fp32 engines), and the data d."""
    ok = {k: v for k, v in opts.items() if k in ORACLE_KEYS}
    p = fo.Propagator(c, h, dt, order, npml, **ok)
    d = forward(p)
    J = {"velocity": _born.born(p, dc), "slowness2": _born.born(p, -2.0 * dc / c ** 3, "slowness2")}
    ref32 = 0.0
    if np.dtype(dtype) == np.float32:
        p32 = fo.Propagator(c, h, dt, order, npml, sigma_max=p.sigma_max, dtype=np.float32, **ok)
        forward(p32)
        ref32 = rel(_born.born(p32, dc), J["velocity"])
    return p, d, J, ref32


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_born_matches_the_numpy_restatement(gpu, monkeypatch, case):
    cid, shape, order, npml, nt, dtype, kname, opts, ty = case
    if ty:
        monkeypatch.setenv("FWI_STREAM_TY", str(ty))
    c, h, dt, src, rec, wav, dc = _problem(shape, order, nt)
    p, d, J, ref32 = _reference(c, h, dt, order, npml, opts, lambda q: q.forward(src, wav, rec), dc, dtype)
    _assert_the_reference_sees_the_wave(d, J["velocity"])
    tol = _tolerance(dtype, ref32)
    errs = {}
    with Engine(shape, h, dt, nt, order=order, npml=npml, sigma_max=p.sigma_max, dtype=dtype, **opts) as e:
        assert e.born_path == "none"
        e.forward(c, (src, wav), rec, save=True)
        assert e.kernel_name == kname
        fused = _has_fused(shape, order, dtype, opts)
        for mode in ("auto", "scatter") + (("fused",) if fused else ()):
            errs["velocity/" + mode] = rel(e.born(dc, mode=mode), J["velocity"])
            assert e.born_path == (mode if mode != "auto" else AUTO_PATH if fused else "scatter")
            errs["slowness2/" + mode] = rel(e.born(-2.0 * dc / c ** 3, "slowness2", mode=mode), J["slowness2"])
        if not fused:
            with pytest.raises(FwiError) as ei:
                e.born(dc, mode="fused")
            assert ei.value.code == 1
    print(cid, "reference fp32-vs-fp64 %.3g" % ref32, "tolerance %.3g" % tol, errs)
    _record(cid, {"gpu_rel_l2": errs, "reference_fp32_vs_fp64": ref32, "tolerance": tol, "dtype": dtype,
                  "dd_over_d": float(np.linalg.norm(J["velocity"]) / np.linalg.norm(d))})
    assert max(errs.values()) <= tol, (errs, tol)


@pytest.mark.parametrize("opts", [{}, INC, CPML3], ids=["standard", "increment", "cpml"])
def test_born_with_off_grid_sources_and_receivers(gpu, opts):
    shape, order, npml, nt = S3, 8, 6, 60
    c, h, dt, src, rec, wav, dc = _problem(shape, order, nt)
    rng = np.random.default_rng(4)
    sxyz = np.array([[20.3, 17.6, 21.2], [20.7, 17.6, 21.9], [13.0, 12.5, 14.0]])  # the first two share nodes
    rxyz = np.clip(rec + rng.random(rec.shape), 0.0, np.array(shape) - 1.0)
    S, R = Spread(sxyz, shape), Spread(rxyz, shape)
    fwd = lambda q: R.gather(q.forward(S.idx, S.scatter(wav), R.idx))  # noqa: E731
    p, d, J, ref32 = _reference(c, h, dt, order, npml, opts, fwd, dc, "float32")
    Jv = R.gather(J["velocity"])
    _assert_the_reference_sees_the_wave(d, Jv)
    tol = _tolerance("float32", ref32)
    with Engine(shape, h, dt, nt, order=order, npml=npml, sigma_max=p.sigma_max, **opts) as e:
        e.forward_at(c, (sxyz, wav), rxyz, save=True)
        if _has_fused(shape, order, "float32", opts):
            assert rel(e.born(dc, mode="fused"), Jv) <= tol and e.born_path == "fused"
        got = e.born(dc, mode="scatter")
        assert got.shape == (nt, len(rxyz)) and e.born_path == "scatter"
        err = rel(got, Jv)
        # the per-point data stay on the device as the residual: J^T J dc, against the adjoint of the downloaded copy
        e.adjoint(None)
        g1 = e.gradient()
        e.reset_gradient()
        e.adjoint(got)
        assert np.array_equal(g1, e.gradient())
    cid = "3d_off_grid_" + ("_".join(sorted(opts)) or "standard")
    print(cid, "reference fp32-vs-fp64 %.3g" % ref32, "tolerance %.3g" % tol, err)
    _record(cid, {"gpu_rel_l2": {"velocity/auto": err}, "reference_fp32_vs_fp64": ref32, "tolerance": tol,
                  "dtype": "float32", "dd_over_d": float(np.linalg.norm(Jv) / np.linalg.norm(d))})
    assert err <= tol, (err, tol)


@pytest.mark.parametrize("shape,order,npml,nt,opts", [((72, 96), 8, 8, 80, {}), ((72, 96), 8, 8, 80, CPML2),
                                                      ((33, 29, 50), 4, 5, 50, {}), ((33, 29, 50), 4, 5, 50, CPML3)],
                         ids=["2d_sponge", "2d_cpml", "3d_sponge", "3d_cpml"])
def test_born_is_the_derivative_of_the_engines_forward(gpu, shape, order, npml, nt, opts):
    """fp64, central difference with eps = 1e-3: 1e-7 (truncation O(eps^2) plus round-off over 2 eps ||dd|| / ||d||)."""
    c, h, dt, src, rec, wav, dc = _problem(shape, order, nt)
    sigma = fo.default_sigma_max(c.max(), h, npml)
    eps = 1e-3
    with Engine(shape, h, dt, nt, order=order, npml=npml, sigma_max=sigma, dtype="float64", **opts) as e:
        dp = e.forward(c + eps * dc, (src, wav), rec, save=False)
        dm = e.forward(c - eps * dc, (src, wav), rec, save=False)
        e.forward(c, (src, wav), rec, save=True)
        J = e.born(dc)
    err = rel(J, (dp - dm) / (2 * eps))
    print("finite difference", shape, opts, err)
    assert err <= 1e-7, err


@pytest.mark.parametrize("case", [c for c in CASES if c[0] in (
    "2d_fused_nt82", "2d_fused_cpml", "3d_stream", "3d_stream_increment", "3d_stream_cpml_increment", "3d_point",
    "3d_fp64_o4")], ids=lambda c: c[0])
def test_born_and_gradient_are_adjoint(gpu, case):
    """<J dc, r> = <dc, J^T r>: fp64 1e-10; fp32 1e-4, the bound the F / F^T identity of the full-size 3-D test uses."""
    cid, shape, order, npml, nt, dtype, _, opts, _ = case
    c, h, dt, src, rec, wav, dc = _problem(shape, order, nt)
    r = np.random.default_rng(7).standard_normal((nt, len(rec)))
    sigma = fo.default_sigma_max(c.max(), h, npml)
    with Engine(shape, h, dt, nt, order=order, npml=npml, sigma_max=sigma, dtype=dtype, **opts) as e:
        e.forward(c, (src, wav), rec, save=True)
        modes = ("scatter", "fused") if _has_fused(shape, order, dtype, opts) else ("scatter",)
        for wrt, v, mode in [(w, v, m) for w, v in (("velocity", dc), ("slowness2", -2.0 * dc / c ** 3)) for m in modes]:
            J = e.born(v, wrt, mode=mode)
            e.reset_gradient()
            e.adjoint(r)
            lhs = float(np.vdot(J.astype(np.float64), r))
            rhs = float(np.vdot(np.asarray(v, np.float64), e.gradient(wrt).astype(np.float64)))
            print(cid, wrt, mode, abs(lhs - rhs) / abs(lhs))
            assert abs(lhs - rhs) <= (1e-10 if dtype == "float64" else 1e-4) * abs(lhs)


@pytest.mark.parametrize("case", [c for c in CASES if c[0] in (
    "2d_fused_nt82", "2d_fused_cpml", "3d_stream", "3d_stream_increment", "3d_stream_cpml", "3d_stream_cpml_increment",
    "3d_point", "3d_full_tiles_increment_ty8")], ids=lambda c: c[0])
def test_exact_invariants(gpu, monkeypatch, case):
    cid, shape, order, npml, nt, dtype, _, opts, ty = case
    for mode in ("scatter", "fused") if _has_fused(shape, order, dtype, opts) else ("scatter",):
        _exact_invariants(monkeypatch, mode, shape, order, npml, nt, dtype, opts, ty)


def _exact_invariants(monkeypatch, mode, shape, order, npml, nt, dtype, opts, ty):
    if ty:
        monkeypatch.setenv("FWI_STREAM_TY", str(ty))
    c, h, dt, src, rec, wav, dc = _problem(shape, order, nt)
    dc = dc.astype(np.float32)
    r = np.random.default_rng(7).standard_normal((nt, len(rec))).astype(np.float32)
    sigma = fo.default_sigma_max(c.max(), h, npml)
    with Engine(shape, h, dt, nt, order=order, npml=npml, sigma_max=sigma, dtype=dtype, **opts) as e:
        e.forward(c, (src, wav), rec, save=True)
        e.adjoint(r)
        g_plain = e.gradient()
        e.reset_gradient()
        e.forward(None, (src, wav), rec, save=True)
        J1 = e.born(dc, mode=mode)
        assert e.born_path == mode and e.dirty_padding() == 0
        assert np.array_equal(e.born(dc, mode=mode), J1)            # a second sweep: the same bytes
        assert np.array_equal(e.born(2.0 * dc, mode=mode), 2.0 * J1)  # linear, exactly (a power of two)
        e.vec_create(1)
        e.vec_upload(0, dc)
        assert np.array_equal(e.born_vec(0, mode=mode), J1)         # dm from a device vector
        assert e.born_vec(0, mode=mode, download=False) is None
        assert e.dirty_padding() == 0
        e.adjoint(r)                                                # the store is untouched by the Born sweeps
        assert np.array_equal(e.gradient(), g_plain)
        assert e.dirty_padding() == 0
        # the data stay on the device as the next adjoint's residual: J^T (J dc) either way
        e.reset_gradient()
        e.born(dc, mode=mode)
        e.adjoint(None)
        g_dev = e.gradient()
        e.reset_gradient()
        e.adjoint(J1)
        assert np.array_equal(g_dev, e.gradient())


def _two_shots(dtype, shape=(72, 96), order=8, npml=8, nt=80):
    c, h, dt, src, rec, wav, dc = _problem(shape, order, nt)
    shots = [sh.Shot(src[:1], wav[:, 0], rec), sh.Shot(src[1:2] + 3, wav[:, 1], rec)]
    sigma = fo.default_sigma_max(c.max(), h, npml)
    mk = lambda: Engine(shape, h, dt, nt, order=order, npml=npml, sigma_max=sigma, dtype=dtype)  # noqa: E731
    return c, shots, dc, mk


def test_gauss_newton_hvp_fp64(gpu):
    c, shots, v, mk = _two_shots("float64")
    u = np.random.default_rng(11).standard_normal(v.shape) * 30.0
    with mk() as e:
        Hv = sh.gauss_newton_hvp(e, c, shots, v)
        Hu = sh.gauss_newton_hvp(e, None, shots, u)
        by_hand, jj = 0.0, 0.0
        for s in shots:
            e.reset_gradient()
            s.forward(e, save=True)
            J = e.born(v)
            jj += float(np.sum(J ** 2))
            e.adjoint(J)
            by_hand = by_hand + e.gradient()
        assert rel(Hv, by_hand) <= 1e-12  # (the accumulator is scaled once, the sum by hand once per shot)
        assert abs(np.vdot(u, Hv) - np.vdot(v, Hu)) <= 1e-10 * abs(np.vdot(u, Hv))
        assert np.vdot(v, Hv) >= 0.0 and abs(np.vdot(v, Hv) - jj) <= 1e-10 * jj
        e.vec_create(3)
        e.vec_upload(0, c)
        e.vec_upload(1, v)
        sh.gauss_newton_hvp_device(e, 0, 1, 2, shots)
        assert np.array_equal(e.vec_download(2), Hv)


def test_gauss_newton_hvp_on_an_engine_pool_matches_the_single_engine(gpu):
    c, shots, v, mk = _two_shots("float32")
    with mk() as e:
        H1 = sh.gauss_newton_hvp(e, c, shots, v)
    with sh.EnginePool(mk, 2) as pool:
        H2 = sh.gauss_newton_hvp(pool, c, shots, v)
        pool.primary.vec_create(3)
        pool.primary.vec_upload(0, c)
        pool.primary.vec_upload(1, v)
        sh.gauss_newton_hvp_device(pool, 0, 1, 2, shots)
        H3 = pool.primary.vec_download(2)
    assert rel(H2, H1) <= 1e-6 and rel(H3, H1) <= 1e-6, (rel(H2, H1), rel(H3, H1))


def _linear_inversion(mk_engine, dtype):
    """CG on H_GN x = J^T d for 8 iterations; returns ||J x_k - d|| / ||d||, k = 0 .. 8."""
    shape, h, order, npml, nt = (96, 128), 10.0, 8, 8, 300
    c = 2000.0 + 8.0 * np.arange(shape[0], dtype=np.float64)[:, None] * np.ones(shape)
    dt = 0.6 * fo.cfl_dt(c.max(), h, 2, order)
    wav = fo.ricker(nt, dt, 12.0)
    rec = np.stack([np.full(32, 10), np.arange(0, 128, 4)], 1)
    shots = [sh.Shot(np.array([[10, x]]), wav, rec) for x in (16, 48, 80, 112)]
    dc_true = np.zeros(shape)
    dc_true[40:56, 50:80] = 60.0
    sigma = fo.default_sigma_max(c.max(), h, npml)
    e = mk_engine(shape, h, dt, nt, order, npml, sigma)
    try:
        e.set_model(c)

        def J(x):
            out = []
            for s in shots:
                s.forward(e, save=True)
                out.append(np.asarray(s.born(e, np.asarray(x, dtype)), np.float64))
            return np.stack(out)

        d = J(dc_true)
        e.reset_gradient()
        for s, ds in zip(shots, d):
            s.forward(e, save=True)
            s.adjoint(e, ds.astype(dtype))
        b = np.asarray(e.gradient(), np.float64)
        curve = []
        newton.cg(lambda v: sh.gauss_newton_hvp(e, None, shots, np.asarray(v, dtype)), b, maxiter=8, rtol=0.0,
                  callback=lambda k, x: curve.append(float(np.linalg.norm(J(x) - d) / np.linalg.norm(d))))
    finally:
        e.close()
    return curve


def test_linear_inversion_follows_the_reference_curve(gpu):
    """8 CG iterations on the normal equations of a 4-shot 2-D reflection survey.  CG on H x = J^T d minimises
    ||J x - d|| over the Krylov space, so the data residual never increases (1e-5 relative slack per step in fp32), and
    every ||J x_k - d|| / ||d|| is within 1e-3 relative of the same iteration on the NumPy engine in fp64 (reference
    alone: 1.000, 0.775, 0.753, 0.727, 0.702, 0.678, 0.636, 0.611, 0.584; the GPU's operators are within 1e-5 of the
    reference per application, which leaves two orders)."""
    ref = _linear_inversion(lambda shape, h, dt, nt, order, npml, sigma: _born.BornOracleEngine(
        shape, h, dt, nt, order=order, npml=npml, sigma_max=sigma), np.float64)
    got = _linear_inversion(lambda shape, h, dt, nt, order, npml, sigma: Engine(
        shape, h, dt, nt, order=order, npml=npml, sigma_max=sigma), np.float32)
    print("reference", ["%.4f" % v for v in ref])
    print("gpu      ", ["%.4f" % v for v in got])
    assert len(got) == len(ref) == 9 and ref[0] == 1.0 and got[0] == 1.0
    for a, b in zip(got, got[1:]):
        assert b <= a * (1.0 + 1e-5), got
    for g, r in zip(got, ref):
        assert abs(g - r) <= 1e-3 * r, (got, ref)


def test_born_errors(gpu):
    shape, order, npml, nt = (40, 36, 44), 8, 6, 24
    c, h, dt, src, rec, wav, dc = _problem(shape, order, nt)
    kw = dict(order=order, npml=npml, sigma_max=50.0)
    with Engine(shape, h, dt, nt, **kw) as e:
        e.set_model(c)
        e._nt, e._nrec = nt, len(rec)
        with pytest.raises(FwiError) as ei:  # before any forward
            e.born(dc)
        assert ei.value.code == 3
        e.forward(None, (src, wav), rec, save=False)
        with pytest.raises(FwiError) as ei:  # a forward that kept nothing
            e.born(dc)
        assert ei.value.code == 3
        e.forward(None, (src, wav), rec, save=True)
        with pytest.raises(ValueError):
            e.born(dc[:-1])
        with pytest.raises(KeyError):
            e.born(dc, wrt="density")
        dcp = np.ascontiguousarray(dc, np.float32).ctypes.data_as(C.c_void_p)
        for args in ((5, dcp, 0, None), (0, dcp, 7, None), (0, None, 0, None)):
            assert e._lib.fwi_born(e._ctx, *args) == 1, args
            assert b"fwi_born" in e._lib.fwi_last_error(e._ctx)
        assert e._lib.fwi_born_vec(e._ctx, 0, 0, 0, None) == 1  # no such vector slot
        e.born(dc)
        with pytest.raises(FwiError) as ei:  # the forward's synthetics are gone
            e.misfit_l2(np.zeros((nt, len(rec)), np.float32))
        assert ei.value.code == 3
        e.set_model(c)
        with pytest.raises(FwiError) as ei:  # a new model invalidates the store
            e.born(dc)
        assert ei.value.code == 3
    for opts in ({"kernel": "point"}, {"abc": "cpml"}, {"dtype": "float64"}):  # contexts without a fused path refuse it
        with Engine(shape, h, dt, nt, **{**kw, "order": 4 if "dtype" in opts else order}, **opts) as e:
            e.forward(c, (src, wav), rec, save=True)
            with pytest.raises(FwiError) as ei:
                e.born(dc, mode="fused")
            assert ei.value.code == 1 and "FWI_BORN_FUSED" in str(ei.value), opts
            e.born(dc)
            assert e.born_path == "scatter"
    for opts, word in (({"image_stride": 4}, "image_stride"), ({"store_dtype": "bf16"}, "bf16"),
                       ({"ckpt_interval": 8}, "ckpt_interval")):
        with Engine(shape, h, dt, nt, **kw, **opts) as e:
            e.forward(c, (src, wav), rec, save=True)
            with pytest.raises(FwiError) as ei:
                e.born(dc)
            assert ei.value.code == 1 and word in str(ei.value), (opts, str(ei.value))
            e.adjoint(np.ones((nt, len(rec)), np.float32))  # the context still works


MIB = 1 << 20


def _free_bytes():
    hip = C.CDLL("libamdhip64.so")
    fr, tot = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(fr), C.byref(tot)) == 0
    return fr.value


def _cycles(n, born):
    shape, order, nt = (96, 96, 128), 8, 12
    c, h, dt, src, rec, wav, dc = _problem(shape, order, nt, seed=3)
    lib = _lib.load()
    for i in range(n):
        with Engine(shape, h, dt, nt, order=order, npml=8, sigma_max=900.0) as e:
            d = e.forward(c, (src, wav), rec, save=True)
            if born:
                e.born(dc, download=False)
                e.adjoint(None)
            else:
                e.adjoint(d)
            e.gradient()
        msg = lib.fwi_last_error(None) or b""
        assert not msg.startswith(b"fwi_destroy:"), (i, msg.decode())


def test_destroy_gives_back_the_born_array(gpu):
    """Six create -> forward(save) -> born -> adjoint(None) -> destroy cycles at (96, 96, 128) end with free device
    memory within 14 MiB of where it was after a warm-up cycle, and fwi_destroy reports no refused free.  The w array of
    that grid is 4.5 MiB: one leaked per cycle is 27 MiB.  Six cycles without born run first as the control: if those
    move by more, another tenant of the device did it."""
    drift = {}
    for born in (False, True):
        _cycles(1, born)  # warm-up: the runtime's own first-use allocations are not leaks
        start = _free_bytes()
        _cycles(6, born)
        drift[born] = start - _free_bytes()
    print("free-memory drift over six cycles: control %.1f MiB, with born %.1f MiB" % (drift[False] / MIB, drift[True] / MIB))
    if abs(drift[False]) > 14 * MIB:
        pytest.fail("the control cycles moved free memory by %.1f MiB: another tenant is allocating on this device"
                    % (drift[False] / MIB))
    assert abs(drift[True]) <= 14 * MIB, drift
