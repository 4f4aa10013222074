"""Born modelling and Gauss-Newton products without a GPU: the three C-ABI symbols and their argument checks, the
conjugate-gradient solver on systems with a known answer, ``shots.gauss_newton_hvp`` over a NumPy engine (oracle +
tests/_born.py) against the explicit sum over shots -- alone and in a host-exchange world of two -- and the code object
of the Born kernels (fwi_born.o)."""
import ctypes as C
import os
import socket
import sys
import threading

import numpy as np
import pytest

import _born
from full_waveform_inversion_amd import _lib, newton, shots as sh
from oracle import fwi_oracle as fo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import code_objects as co  # noqa: E402

FWI_EINVAL = 1


def test_the_born_calls_are_declared_bound_and_exported_at_abi_14():
    lib = _lib.load()
    assert lib.fwi_abi_version() == _lib.ABI_VERSION == 14
    header = open(os.path.join(ROOT, "include", "fwi.h")).read()
    for name in ("fwi_born", "fwi_born_vec", "fwi_born_path"):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and name + "(" in header
    assert "FWI_BORN_AUTO = 0, FWI_BORN_SCATTER = 1, FWI_BORN_FUSED = 2" in header
    assert _lib.BORN_MODES == {"auto": 0, "scatter": 1, "fused": 2}


def test_born_calls_reject_a_null_context():
    lib = _lib.load()
    buf = np.zeros(16, np.float32)
    vp = buf.ctypes.data_as(C.c_void_p)
    for wrt in (_lib.WRT_VELOCITY, _lib.WRT_SLOWNESS2, 7):
        for mode in (0, 1, 2, 9):
            assert lib.fwi_born(None, wrt, vp, mode, vp) == FWI_EINVAL
            assert lib.fwi_born_vec(None, wrt, 0, mode, None) == FWI_EINVAL
    assert lib.fwi_born_path(None) == b""


# ---- newton.cg ------------------------------------------------------------------------------------------------------
def _spd(n=60, cond=1e4):
    d = np.logspace(0, np.log10(cond), n)
    x_star = np.linspace(-1.0, 2.0, n)
    return d, x_star, d * x_star


def _iterations_to(log, rtol):
    for e in log:
        if e["rnorm"] <= rtol * log[0]["rnorm"]:
            return e["iter"]
    return None


def test_cg_with_the_exact_diagonal_preconditioner_converges_at_once():
    d, x_star, b = _spd()
    xp, lp = newton.cg(lambda v: d * v, b, precond=1.0 / d, maxiter=60, rtol=1e-10)
    xu, lu = newton.cg(lambda v: d * v, b, maxiter=60, rtol=1e-10)
    kp, ku = _iterations_to(lp, 1e-10), _iterations_to(lu, 1e-10)
    assert kp is not None and kp <= 2, lp
    assert ku is None or ku > 5, lu
    assert np.allclose(xp, x_star, rtol=1e-9, atol=1e-9) and lp[-1]["stop"] == "converged"
    # a callable preconditioner and a starting point
    xc, lc = newton.cg(lambda v: d * v, b, precond=lambda r: r / d, x0=0.5 * x_star, maxiter=60, rtol=1e-10)
    assert np.allclose(xc, x_star, rtol=1e-9, atol=1e-9) and _iterations_to(lc, 1e-10) <= 2


def test_cg_solves_a_dense_spd_system_with_known_inverse_and_reports_every_iterate():
    rng = np.random.default_rng(5)
    Q, _ = np.linalg.qr(rng.standard_normal((60, 60)))
    A = Q @ np.diag(np.linspace(1.0, 30.0, 60)) @ Q.T
    b = rng.standard_normal(60)
    seen = []
    x, log = newton.cg(lambda v: A @ v, b, maxiter=200, rtol=1e-12, callback=lambda k, xk: seen.append((k, xk.copy())))
    assert np.allclose(x, np.linalg.solve(A, b), rtol=1e-9, atol=1e-10)
    assert [k for k, _ in seen] == [e["iter"] for e in log] and not np.any(seen[0][1])
    for (k, xk), e in zip(seen, log):  # the logged residual is the true one
        assert abs(np.linalg.norm(b - A @ xk) - e["rnorm"]) <= 1e-9 * log[0]["rnorm"]
    # CG minimises the energy norm of the error over the Krylov space: it decreases monotonically
    xs = np.linalg.solve(A, b)
    en = [float((xk - xs) @ A @ (xk - xs)) for _, xk in seen]
    assert all(b_ <= a_ * (1 + 1e-12) for a_, b_ in zip(en, en[1:]))
    assert newton.cg(lambda v: A @ v, b, maxiter=3)[1][-1]["stop"] == "maxiter"


def test_cg_stops_on_an_indefinite_matrix():
    d = np.concatenate([np.linspace(1.0, 4.0, 30), -np.linspace(1.0, 4.0, 30)])
    b = np.ones(60)
    x, log = newton.cg(lambda v: d * v, b, maxiter=50)
    assert log[-1]["stop"] == "negative_curvature" and log[-1]["curvature"] <= 0.0
    assert np.all(np.isfinite(x)) and len(log) < 50


# ---- shots.gauss_newton_hvp over the NumPy engine -------------------------------------------------------------------
def _survey(seed=2):
    shape, order, npml, nt = (36, 44), 4, 6, 70
    rng = np.random.default_rng(seed)
    c = 2000.0 + 500.0 * rng.random(shape)
    h = 10.0
    dt = 0.6 * fo.cfl_dt(c.max(), h, 2, order)
    wav = fo.ricker(nt, dt, 0.12 / dt / 8)
    rec = np.stack([np.full(10, 8), np.arange(4, 44, 4)], 1)
    shots = [sh.Shot(np.array([[7, x]]), wav, rec) for x in (8, 20, 34)]
    v = 30.0 * rng.standard_normal(shape)
    mk = lambda: _born.BornOracleEngine(shape, h, dt, nt, order=order, npml=npml)  # noqa: E731
    return c, shots, v, mk


def _explicit_hvp(mk, c, shots, v, wrt):
    H = 0.0
    for s in shots:
        e = mk()
        s.forward(e.set_model(c) or e, save=True)
        e.adjoint(e.born(v, wrt))
        H = H + e.gradient(wrt)
    return H


@pytest.mark.parametrize("wrt", ["velocity", "slowness2"])
def test_gauss_newton_hvp_is_the_explicit_sum_over_shots(wrt):
    c, shots, v, mk = _survey()
    if wrt == "slowness2":
        v = v * 1e-9
    want = _explicit_hvp(mk, c, shots, v, wrt)
    e = mk()
    e._g = np.ones(e.shape)  # the accumulator is overwritten, not added to
    got = sh.gauss_newton_hvp(e, c, shots, v, wrt=wrt)
    assert np.allclose(got, want, rtol=1e-12, atol=1e-12 * np.abs(want).max())
    # symmetric and positive: <u, H v> = <v, H u>, <v, H v> = sum ||J_s v||^2
    u = np.random.default_rng(9).standard_normal(v.shape) * np.abs(v).max()
    Hu = sh.gauss_newton_hvp(e, None, shots, u, wrt=wrt)
    assert abs(np.vdot(u, got) - np.vdot(v, Hu)) <= 1e-10 * abs(np.vdot(u, got))
    jj = 0.0
    for s in shots:
        s.forward(e, save=True)
        jj += float(np.sum(e.born(v, wrt) ** 2))
    assert abs(np.vdot(v, got) - jj) <= 1e-10 * jj
    with sh.EnginePool(mk, 2) as pool:
        assert np.allclose(sh.gauss_newton_hvp(pool, c, shots, v, wrt=wrt), want, rtol=1e-12,
                           atol=1e-12 * np.abs(want).max())


def test_gauss_newton_hvp_in_a_host_exchange_world_of_two():
    from full_waveform_inversion_amd.rendezvous import Rendezvous
    c, shots, v, mk = _survey()
    want = _explicit_hvp(mk, c, shots, v, "velocity")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out, err = [None, None], []

    def rank(r):
        try:
            rdzv = Rendezvous(r, 2, port=port, timeout=60.0)
            try:
                out[r] = sh.gauss_newton_hvp(mk(), c, shots, v, exchange=sh.HostExchange(rdzv))
            finally:
                rdzv.close()
        except BaseException as ex:  # noqa: BLE001  (re-raised below)
            err.append(ex)

    ts = [threading.Thread(target=rank, args=(r,)) for r in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(180)
    assert not err, err
    for r in range(2):
        assert np.allclose(out[r], want, rtol=1e-12, atol=1e-12 * np.abs(want).max())


def test_gauss_newton_step_solves_the_normal_equations_of_a_linear_problem():
    c, shots, v, mk = _survey()
    e = mk()
    H = lambda x: sh.gauss_newton_hvp(e, c, shots, x)  # noqa: E731
    g = -H(v)  # the gradient at which the exact Gauss-Newton step is v
    seen = []
    p, log = newton.gauss_newton_step(e, c, shots, g, maxiter=6, rtol=1e-8, callback=lambda k, x: seen.append(k))
    assert seen == [e_["iter"] for e_ in log] and len(log) >= 2
    assert all(b["rnorm"] < 1.0001 * log[0]["rnorm"] for b in log) and log[-1]["rnorm"] < 0.5 * log[0]["rnorm"]
    # the model-space error in the H-norm falls monotonically (the property CG has)
    # (checked through the quadratic it minimises: phi(p) = 1/2 p^T H p + g^T p)
    phi = lambda x: 0.5 * float(np.vdot(x, H(x))) + float(np.vdot(g, x))  # noqa: E731
    assert phi(p) < 0.0 and phi(p) >= phi(v) - 1e-9 * abs(phi(v))
    pd, _ = newton.gauss_newton_step(e, c, shots, g, maxiter=6, rtol=1e-8, damping=1e3 * np.abs(H(v)).max())
    assert np.linalg.norm(pd) < np.linalg.norm(p)


# ---- the code object -------------------------------------------------------------------------------------------------
# born_weight <fp32, fp64>, born_scatter <fp32, fp64> x <standard, increment form>
BORN_KERNELS = 6


def test_born_object_has_no_scratch_and_a_pinned_kernel_count():
    path = os.path.join(co.CSRC, "fwi_born.o")
    if not co.tools_present() or not os.path.exists(path):
        pytest.skip("ROCm LLVM tools or the built objects are missing (run `make -C full_waveform_inversion_amd/csrc`)")
    ks = co.kernels([path])
    bad = [k["name"] for k in ks if k.get("private_segment_fixed_size", 0) > 0 or k.get("vgpr_spill_count", 0) > 0]
    assert not bad, bad
    assert len(ks) == BORN_KERNELS, [k["name"] for k in ks]
    assert sum("born_scatter<" in k["name"] for k in ks) == 4


# step3d_stream Born variants: <4, 8 rows> x <sponge, none> x <full, partial tiles> x <standard, increment form>
BORN3D_KERNELS = 16


def test_fused_born_object_has_no_scratch_and_a_pinned_kernel_count():
    path = os.path.join(co.CSRC, "fwi_born3d.o")
    if not co.tools_present() or not os.path.exists(path):
        pytest.skip("ROCm LLVM tools or the built objects are missing (run `make -C full_waveform_inversion_amd/csrc`)")
    ks = co.kernels([path])
    bad = [k["name"] for k in ks if k.get("private_segment_fixed_size", 0) > 0 or k.get("vgpr_spill_count", 0) > 0]
    assert not bad, bad
    assert len(ks) == BORN3D_KERNELS and all("step3d_stream<" in k["name"] for k in ks), [k["name"] for k in ks]
