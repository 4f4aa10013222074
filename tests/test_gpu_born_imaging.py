"""The imaging Born operator (include/fwi.h fwi_born_imaging; ``Engine.born(operator="imaging")``) on the GPU, on the
three stores the exact ``fwi_born`` refuses -- image_stride > 1, the bf16 store, ckpt_interval > 0 -- against the NumPy
restatement tests/_born_imaging.py (validated on its own by tests/test_born_imaging_oracle.py).

Every context is held to: the data dd = J_img dm against the restatement in fp64 (both parametrisations, every path the
context has, ``born_path`` asserted); <J_img dm, r> = <dm, gradient> after adjoint(r) on the same context; the exact
(bitwise) invariants; clean padding after every sweep.

Bounds.  dd, relative L2: fp32 1e-5 (the project's flat bound), fp64 1e-10.  bf16 store: 2e-4 + half the relative
difference between the restatement's bf16 and native data (the bound of the bf16 gradient test, tests/test_gpu_parity.py:
an fp32 and an fp64 value of C L u that straddle a bf16 rounding boundary round apart by a whole bf16 ulp), and the
engine's data must lie nearer the bf16 restatement than the native one.  The adjoint identity is exact in the operator
whatever the store holds: fp32 1e-4, fp64 1e-10 in every mode, bf16 included.  Checkpointed against store-all on the
same engine: fp32 1e-6, fp64 1e-12.  nt = 37 is a multiple of no stride or interval used: last slots and segments are
short.
"""
import functools

import numpy as np
import pytest

import _born
import _born_imaging as bi
from full_waveform_inversion_amd import Engine, FwiError, newton, shots as sh
from oracle import fwi_oracle as fo

pytestmark = pytest.mark.gpu

TOL32, TOL64 = 1e-5, 1e-10
ADJ32, ADJ64 = 1e-4, 1e-10
CPML2, CPML3 = {"abc": "cpml", "pml_alpha_max": 40.0}, {"abc": "cpml", "pml_alpha_max": 30.0}
INC = {"update_form": "increment"}
G3, G3ODD, G2 = (20, 22, 36), (19, 21, 30), (40, 48)  # 19 x 21 x 30: nx % 4 != 0, the compact rows are padded
ORACLE_KEYS = ("abc", "pml_alpha_max")


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / np.linalg.norm(b))


@functools.lru_cache(maxsize=None)
def _problem(shape, order, nt):
    """Random model, three sources of which two share a node, a wavelet that peaks within the run, receivers within reach
    of the first source's wave, dc = 30 m/s x standard normal, a random residual."""
    rng = np.random.default_rng(0)
    c = 2000.0 + 600.0 * rng.random(shape)
    h = 10.0
    dt = 0.6 * fo.cfl_dt(c.max(), h, len(shape), order)
    src = np.array([[s // 2 for s in shape], [s // 3 for s in shape], [s // 2 for s in shape]])  # a duplicate node
    f0 = 0.5 / dt / 8
    wav = np.stack([fo.ricker(nt, dt, f0, t0=1.0 / f0) * a for a in (1.0, 0.7, -0.4)], 1)
    radius = max(2.0, 0.5 * c.min() * nt * dt / h)  # cells
    rec = []
    while len(rec) < 8:
        off = rng.integers(-int(radius), int(radius) + 1, len(shape))
        node = src[0] + off
        if np.linalg.norm(off) <= radius and np.all(node >= 0) and np.all(node < np.array(shape)):
            rec.append(node)
    dc = 30.0 * rng.standard_normal(shape)
    r = rng.standard_normal((nt, 8))
    return c, h, dt, src, np.array(rec), wav, dc, r


@functools.lru_cache(maxsize=None)
def _reference(shape, order, npml, nt, okeys, stride=1, store="native"):
    """J_img dc (velocity) and J_img dm (slowness^2, dm = -2 dc / c^3: the same data) of tests/_born_imaging.py in fp64,
    computed once per configuration and shared (read-only) by the tests."""
    c, h, dt, src, rec, wav, dc, _ = _problem(shape, order, nt)
    p = fo.Propagator(c, h, dt, order, npml, image_stride=stride, store_dtype=store, **dict(okeys))
    d = p.forward(src, wav, rec)
    J = {"velocity": bi.born_imaging(p, dc), "slowness2": bi.born_imaging(p, -2.0 * dc / c ** 3, "slowness2")}
    for v in J.values():
        v.setflags(write=False)
    peaks = np.abs(J["velocity"]).max(axis=0)
    assert peaks.min() > 0.0 and np.linalg.norm(J["velocity"]) >= 1e-4 * np.linalg.norm(d), (peaks, np.linalg.norm(d))
    return p.sigma_max, J


def _okeys(opts):
    return tuple(sorted((k, v) for k, v in opts.items() if k in ORACLE_KEYS))


def _has_fused(shape, order, dtype, opts):
    return len(shape) == 3 and order == 8 and dtype == "float32" and opts.get("kernel") != "point" and "abc" not in opts


def _check_context(monkeypatch, shape, order, npml, nt, dtype, opts, ty, store_opts, J, sigma, tol, near=None,
                   kernel=None):
    """Everything a context is held to (module docstring).  ``store_opts``: the engine's store mode; ``near``: data the
    engine's must be FARTHER from than from ``J`` (bf16 store: the native restatement)."""
    if ty:
        monkeypatch.setenv("FWI_STREAM_TY", str(ty))
    c, h, dt, src, rec, wav, dc, r = _problem(shape, order, nt)
    f64 = dtype == "float64"
    dcv = {"velocity": dc, "slowness2": -2.0 * dc / c ** 3}
    fused = _has_fused(shape, order, dtype, opts)
    modes = ("scatter", "fused") if fused else ("scatter",)
    rt = r.astype(dtype)
    with Engine(shape, h, dt, nt, order=order, npml=npml, sigma_max=sigma, dtype=dtype, **opts, **store_opts) as e:
        e.forward(c, (src, wav), rec, save=True)
        if kernel:
            assert e.kernel_name == kernel
        e.adjoint(rt)
        g_plain = {w: e.gradient(w) for w in dcv}
        assert e.dirty_padding() == 0
        e.vec_create(1)
        for mode in modes:
            for wrt, v in dcv.items():
                vt = np.asarray(v, dtype)
                e.reset_gradient()
                e.forward(None, (src, wav), rec, save=True)
                Jg = e.born(vt, wrt, mode=mode, operator="imaging")
                assert e.born_path == mode and e.dirty_padding() == 0
                err = rel(Jg, J[wrt])
                print(shape, opts, store_opts, ty, mode, wrt, "dd %.3g (bound %.3g)" % (err, tol))
                assert err <= tol, (mode, wrt, err, tol)
                if near is not None:
                    assert np.linalg.norm(Jg - J[wrt]) < np.linalg.norm(Jg - near[wrt]), (mode, wrt)
                # exact invariants: a second sweep, linearity in a power of two, dm from a device vector
                assert np.array_equal(e.born(vt, wrt, mode=mode, operator="imaging"), Jg)
                assert np.array_equal(e.born(2.0 * vt, wrt, mode=mode, operator="imaging"), 2.0 * Jg)
                e.vec_upload(0, vt)
                assert np.array_equal(e.born_vec(0, wrt, mode=mode, operator="imaging"), Jg)
                assert e.born_vec(0, wrt, mode=mode, download=False, operator="imaging") is None
                assert e.dirty_padding() == 0
                # the store (and the snapshots) are untouched by the Born sweeps: the gradient of the same residual
                e.adjoint(rt)
                assert e.dirty_padding() == 0
                g = e.gradient(wrt)
                assert np.array_equal(g, g_plain[wrt]), (mode, wrt)
                # <J_img dm, r> = <dm, J_img^T r>, both sides from this context
                lhs = float(np.vdot(Jg.astype(np.float64), rt.astype(np.float64)))
                rhs = float(np.vdot(vt.astype(np.float64), g.astype(np.float64)))
                print(shape, opts, store_opts, ty, mode, wrt, "adjoint identity %.3g" % (abs(lhs - rhs) / abs(lhs)))
                assert abs(lhs - rhs) <= (ADJ64 if f64 else ADJ32) * abs(lhs), (mode, wrt, lhs, rhs)
        e.born(np.asarray(dc, dtype), operator="imaging")  # "auto": fused where it exists (by measurement)
        assert e.born_path == ("fused" if fused else "scatter")
        if not fused:
            with pytest.raises(FwiError) as ei:
                e.born(np.asarray(dc, dtype), mode="fused", operator="imaging")
            assert ei.value.code == 1
        with pytest.raises(FwiError) as ei:  # the exact operator keeps refusing this store
            e.born(np.asarray(dc, dtype))
        assert ei.value.code == 1 and "fwi_born_imaging" in str(ei.value)


# ---- strided store ---------------------------------------------------------------------------------------------------
STRIDED = [  # id, shape, order, npml, nt, dtype, engine options, FWI_STREAM_TY, kernel name
    ("3d_stream", G3, 8, 4, 37, "float32", {}, None, "step3d_stream"),
    ("3d_stream_increment", G3, 8, 4, 37, "float32", INC, None, "step3d_stream"),
    ("3d_stream_cpml", G3, 8, 4, 37, "float32", CPML3, None, "step3d_stream"),
    ("3d_stream_cpml_increment", G3, 8, 4, 37, "float32", {**CPML3, **INC}, None, "step3d_stream"),
    ("3d_stream_ty8", G3, 8, 4, 37, "float32", {}, 8, "step3d_stream"),
    ("3d_stream_increment_ty8", G3, 8, 4, 37, "float32", INC, 8, "step3d_stream"),
    ("3d_stream_cpml_ty8", G3, 8, 4, 37, "float32", CPML3, 8, "step3d_stream"),
    ("3d_stream_cpml_increment_ty8", G3, 8, 4, 37, "float32", {**CPML3, **INC}, 8, "step3d_stream"),
    ("3d_padded_rows", G3ODD, 8, 4, 37, "float32", {}, None, "step3d_stream"),
    ("2d_fused_nt82", G2, 8, 4, 82, "float32", {}, None, "step2d_fused"),
    ("2d_fused_nt82_cpml", G2, 8, 4, 82, "float32", CPML2, None, None),
    ("3d_point", G3, 8, 4, 37, "float32", {"kernel": "point"}, None, "step_point"),
    ("3d_fp64_o4", G3, 4, 4, 37, "float64", {}, None, "step3d_stream"),
]


@pytest.mark.parametrize("stride", [3, 4])
@pytest.mark.parametrize("case", STRIDED, ids=[c[0] for c in STRIDED])
def test_strided_store(gpu, monkeypatch, case, stride):
    _, shape, order, npml, nt, dtype, opts, ty, kernel = case
    sigma, J = _reference(shape, order, npml, nt, _okeys(opts), stride=stride)
    _check_context(monkeypatch, shape, order, npml, nt, dtype, opts, ty, {"image_stride": stride}, J, sigma,
                   TOL64 if dtype == "float64" else TOL32, kernel=kernel)


# ---- bf16 store ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("ty", [4, 8])
@pytest.mark.parametrize("npml", [4, 0], ids=["sponge", "no_border"])
@pytest.mark.parametrize("shape", [G3, G3ODD], ids=["20x22x36", "19x21x30"])
def test_bf16_store(gpu, monkeypatch, shape, npml, ty, stride):
    """(The problem's first and third source share a node: the source's exact share is summed over them.)"""
    sigma, J = _reference(shape, 8, npml, 37, (), stride=stride, store="bf16")
    _, Jn = _reference(shape, 8, npml, 37, (), stride=stride)
    quant = rel(J["velocity"], Jn["velocity"])
    print("bf16 against native restatement: %.3g" % quant)
    _check_context(monkeypatch, shape, 8, npml, 37, "float32", {}, ty, {"store_dtype": "bf16", "image_stride": stride}, J,
                   sigma, 2e-4 + 0.5 * quant, near=Jn, kernel="step3d_stream")


# ---- checkpointed store ----------------------------------------------------------------------------------------------
CKPT = [  # id, shape, order, npml, nt, dtype, engine options, FWI_STREAM_TY, K
    ("3d_stream", G3, 8, 4, 37, "float32", {}, None, 8),
    ("3d_stream_increment", G3, 8, 4, 37, "float32", INC, None, 8),
    ("3d_stream_cpml", G3, 8, 4, 37, "float32", CPML3, None, 8),
    ("3d_stream_cpml_increment", G3, 8, 4, 37, "float32", {**CPML3, **INC}, None, 8),
    ("3d_stream_ty8", G3, 8, 4, 37, "float32", {}, 8, 8),
    ("3d_stream_cpml_increment_ty8", G3, 8, 4, 37, "float32", {**CPML3, **INC}, 8, 8),
    ("3d_padded_rows", G3ODD, 8, 4, 37, "float32", {}, None, 8),
    ("2d_fused_nt82", G2, 8, 4, 82, "float32", {}, None, 8),        # nt % 4 != 0: the recomputation steps one by one
    ("2d_fused_nt80", G2, 8, 4, 80, "float32", {}, None, 8),        # ... four steps per launch
    ("2d_fused_nt80_k6", G2, 8, 4, 80, "float32", {}, None, 6),     # K % 4 != 0: one by one again
    ("2d_fused_nt80_cpml", G2, 8, 4, 80, "float32", CPML2, None, 8),
    ("2d_fused_nt80_increment", G2, 8, 4, 80, "float32", INC, None, 8),
    ("2d_cpml_increment_nt82", G2, 8, 4, 82, "float32", {**CPML2, **INC}, None, 8),
    ("3d_point", G3, 8, 4, 37, "float32", {"kernel": "point"}, None, 8),
    ("3d_fp64_o4", G3, 4, 4, 37, "float64", {}, None, 8),
]


@pytest.mark.parametrize("case", CKPT, ids=[c[0] for c in CKPT])
def test_checkpointed_store(gpu, monkeypatch, case):
    _, shape, order, npml, nt, dtype, opts, ty, K = case
    sigma, J = _reference(shape, order, npml, nt, _okeys(opts))
    f64 = dtype == "float64"
    _check_context(monkeypatch, shape, order, npml, nt, dtype, opts, ty, {"ckpt_interval": K}, J, sigma,
                   TOL64 if f64 else TOL32)
    # against the same engine with every step stored (recomputed q^n = stored q^n up to the launch sequence)
    c, h, dt, src, rec, wav, dc, _ = _problem(shape, order, nt)
    out = {}
    for K_ in (0, K):
        with Engine(shape, h, dt, nt, order=order, npml=npml, sigma_max=sigma, dtype=dtype, ckpt_interval=K_, **opts) as e:
            e.forward(c, (src, wav), rec, save=True)
            out[K_] = {m: e.born(np.asarray(dc, dtype), mode=m, operator="imaging")
                       for m in (("scatter", "fused") if _has_fused(shape, order, dtype, opts) else ("scatter",))}
    for m in out[0]:
        err = rel(out[K][m], out[0][m])
        print(case[0], m, "checkpointed against store-all %.3g" % err)
        assert err <= (1e-12 if f64 else 1e-6), (m, err)


def test_stride_and_checkpointing_together_stay_refused(gpu):
    with pytest.raises(FwiError):
        Engine(G3, 10.0, 1e-3, 37, npml=4, sigma_max=50.0, image_stride=3, ckpt_interval=8)


# ---- plain contexts: the imaging operator IS the exact one -----------------------------------------------------------
@pytest.mark.parametrize("shape,order,nt,dtype,opts", [
    (G3, 8, 37, "float32", {}), (G3, 8, 37, "float32", INC), (G3, 8, 37, "float32", CPML3), (G2, 8, 82, "float32", {}),
    (G2, 8, 82, "float32", CPML2), (G3, 8, 37, "float32", {"kernel": "point"}), (G3, 4, 37, "float64", {})],
    ids=["3d_stream", "3d_increment", "3d_cpml", "2d_fused", "2d_cpml", "3d_point", "3d_fp64_o4"])
def test_imaging_born_equals_born_on_a_plain_context_bitwise(gpu, shape, order, nt, dtype, opts):
    c, h, dt, src, rec, wav, dc, _ = _problem(shape, order, nt)
    dc = np.asarray(dc, dtype)
    with Engine(shape, h, dt, nt, order=order, npml=4, sigma_max=fo.default_sigma_max(c.max(), h, 4), dtype=dtype,
                **opts) as e:
        e.forward(c, (src, wav), rec, save=True)
        e.vec_create(1)
        e.vec_upload(0, dc)
        for mode in ("auto", "scatter") + (("fused",) if _has_fused(shape, order, dtype, opts) else ()):
            for wrt, v in (("velocity", dc), ("slowness2", np.asarray(-2.0 * dc / c ** 3, dtype))):
                J = e.born(v, wrt, mode=mode)
                path = e.born_path
                assert np.any(J) and np.array_equal(e.born(v, wrt, mode=mode, operator="imaging"), J)
                assert e.born_path == path
            assert np.array_equal(e.born_vec(0, mode=mode, operator="imaging"), e.born_vec(0, mode=mode))
        with pytest.raises(ValueError):
            e.born(dc, operator="approximate")


@pytest.mark.parametrize("store", [{"image_stride": 3}, {"store_dtype": "bf16"}, {"ckpt_interval": 8},
                                   {"ckpt_interval": 8, **CPML3, **INC}], ids=["stride3", "bf16", "ckpt8", "ckpt8_cpml_increment"])
def test_a_captured_sweep_repeats_the_submitted_one_bitwise(gpu, store):
    """launch_mode: the sweep captured into one graph (snapshot restores and recomputation included) launches what the
    launch-by-launch sweep submits, and is timed like it."""
    shape, order, npml, nt = G3, 8, 4, 37
    c, h, dt, src, rec, wav, dc, _ = _problem(shape, order, nt)
    out = {}
    for lm in ("stream", "graph"):
        with Engine(shape, h, dt, nt, order=order, npml=npml, sigma_max=fo.default_sigma_max(c.max(), h, npml),
                    launch_mode=lm, **store) as e:
            e.forward(c, (src, wav), rec, save=True)
            out[lm] = {m: e.born(dc.astype(np.float32), mode=m, operator="imaging")
                       for m in (("scatter", "fused") if "abc" not in store else ("scatter",))}
            assert e.last_loop_ms() > 0.0 and e.dirty_padding() == 0
    for m in out["stream"]:
        assert np.any(out["stream"][m]) and np.array_equal(out["graph"][m], out["stream"][m]), m


# ---- H = J_img^T J_img -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", [{"image_stride": 4}, {"store_dtype": "bf16"}, {"store_dtype": "bf16", "image_stride": 3},
                                   {"ckpt_interval": 8}], ids=["stride4", "bf16", "bf16_stride3", "ckpt8"])
def test_gauss_newton_hvp_is_symmetric(gpu, store):
    """<u, H v> = <v, H u> through shots.gauss_newton_hvp, fp32 1e-4: the exact J paired with a strided J^T misses it
    (tests/test_born_imaging_oracle.py shows by how much)."""
    shape, order, npml, nt = G3, 8, 4, 37
    c, h, dt, src, rec, wav, dc, _ = _problem(shape, order, nt)
    shots = [sh.Shot(src[:1], wav[:, 0], rec), sh.Shot(src[1:2], wav[:, 1], rec)]
    v = dc.astype(np.float32)
    u = (30.0 * np.random.default_rng(11).standard_normal(shape)).astype(np.float32)
    with Engine(shape, h, dt, nt, order=order, npml=npml, sigma_max=fo.default_sigma_max(c.max(), h, npml), **store) as e:
        Hv = sh.gauss_newton_hvp(e, c, shots, v).astype(np.float64)
        Hu = sh.gauss_newton_hvp(e, None, shots, u).astype(np.float64)
        a, b = float(np.vdot(u, Hv)), float(np.vdot(v, Hu))
        print(store, "<u, H v> %.6g <v, H u> %.6g relative %.3g" % (a, b, abs(a - b) / abs(a)))
        assert abs(a - b) <= 1e-4 * abs(a)
        assert np.vdot(v, Hv) > 0.0
        e.vec_create(3)
        e.vec_upload(0, c)
        e.vec_upload(1, v)
        sh.gauss_newton_hvp_device(e, 0, 1, 2, shots)
        assert np.array_equal(e.vec_download(2).astype(np.float64), Hv)


def _linear_inversion(mk_engine, dtype):
    """CG on H x = J_img^T d for 8 iterations; returns ||J_img x_k - d|| / ||d||, k = 0 .. 8 (the survey of
    tests/test_gpu_born.py, on an engine with image_stride = 4)."""
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
                out.append(np.asarray(s.born(e, np.asarray(x, dtype), operator="imaging"), np.float64))
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


def test_linear_inversion_on_a_strided_engine_follows_the_reference_curve(gpu):
    """8 CG iterations on the normal equations of a 4-shot 2-D reflection survey with image_stride = 4.  H is exactly
    J_img^T J_img, so CG minimises ||J_img x - d|| over the Krylov space: the data residual never increases (1e-5
    relative slack per step in fp32), and every ||J_img x_k - d|| / ||d|| is within 1e-3 relative of the same iteration
    on the NumPy engine of tests/_born_imaging.py in fp64 -- the 4 digits tests/test_gpu_born.py asks of the store-all
    twin."""
    ref = _linear_inversion(lambda shape, h, dt, nt, order, npml, sigma: bi.ImagingOracleEngine(
        shape, h, dt, nt, order=order, npml=npml, sigma_max=sigma, image_stride=4), np.float64)
    got = _linear_inversion(lambda shape, h, dt, nt, order, npml, sigma: Engine(
        shape, h, dt, nt, order=order, npml=npml, sigma_max=sigma, image_stride=4), np.float32)
    print("reference", ["%.4f" % v for v in ref])
    print("gpu      ", ["%.4f" % v for v in got])
    assert len(got) == len(ref) == 9 and ref[0] == 1.0 and got[0] == 1.0
    for a, b in zip(got, got[1:]):
        assert b <= a * (1.0 + 1e-5), got
    for g, r in zip(got, ref):
        assert abs(g - r) <= 1e-3 * r, (got, ref)
