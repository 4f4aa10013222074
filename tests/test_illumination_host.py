"""Source-illumination preconditioning without a GPU: the C-ABI's argument checks, the preconditioned L-BFGS on a
problem whose exact inverse Hessian is known, its checkpoint / resume, the host exchange of H, and the code object of
the illumination kernels (fwi_illum.o)."""
import ctypes as C
import os
import socket
import sys
import threading

import numpy as np
import pytest

from full_waveform_inversion_amd import _lib, shots as sh
from full_waveform_inversion_amd.lbfgs import lbfgs, lbfgs_device_slots

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import code_objects as co  # noqa: E402

FWI_EINVAL = 1


def test_abi_14_declares_the_illumination_calls():
    lib = _lib.load()
    assert lib.fwi_abi_version() == _lib.ABI_VERSION == 14
    for name in ("fwi_set_illumination", "fwi_illumination", "fwi_illumination_vec", "fwi_allreduce_illumination",
                 "fwi_vec_mul", "fwi_vec_recip"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)


def test_illumination_calls_reject_a_null_context():
    lib = _lib.load()
    buf = np.zeros(16, np.float32)
    vp = buf.ctypes.data_as(C.c_void_p)
    assert lib.fwi_set_illumination(None, 1) == FWI_EINVAL
    assert lib.fwi_set_illumination(None, 0) == FWI_EINVAL
    for wrt in (_lib.WRT_VELOCITY, _lib.WRT_SLOWNESS2, 7, -1):  # (an unknown wrt never gets past the null context)
        assert lib.fwi_illumination(None, wrt, vp) == FWI_EINVAL
        assert lib.fwi_illumination_vec(None, wrt, 0) == FWI_EINVAL
    assert lib.fwi_allreduce_illumination(None) == FWI_EINVAL
    assert lib.fwi_vec_mul(None, 0, 1) == FWI_EINVAL
    assert lib.fwi_vec_recip(None, 0, 1.0, 0.0) == FWI_EINVAL


def _quadratic(n=60, cond=1e4):
    d = np.logspace(0, np.log10(cond), n)
    x_star = np.linspace(-1.0, 2.0, n)

    def fg(x):
        r = x - x_star
        return 0.5 * float(np.sum(d * r * r)), d * r

    return d, x_star, fg


def _iterations_to(log, f0, rtol):
    for e in log:
        if e["f"] <= rtol * f0:
            return e["iter"]
    return None


def test_preconditioned_lbfgs_converges_at_once_on_a_diagonal_quadratic():
    d, x_star, fg = _quadratic()
    x0 = np.zeros_like(x_star)
    f0 = fg(x0)[0]
    first = float(np.abs(x_star).max())  # the largest change the exact Newton step makes
    _, _, lp = lbfgs(fg, x0, maxiter=10, first_step=first, precond=1.0 / d)
    _, _, lu = lbfgs(fg, x0, maxiter=10, first_step=first)
    kp, ku = _iterations_to(lp, f0, 1e-10), _iterations_to(lu, f0, 1e-10)
    assert kp is not None and kp <= 2, lp
    assert ku is None or ku > 5, lu
    # the callable form: built once, from the first evaluation, like the illumination
    calls = []

    def build(x, f, g):
        calls.append(f)
        return 1.0 / d

    _, _, lc = lbfgs(fg, x0, maxiter=10, first_step=first, precond=build)
    assert calls == [f0] and [e["f"] for e in lc] == [e["f"] for e in lp]


def test_precond_none_is_the_unpreconditioned_iteration():
    d, x_star, fg = _quadratic(cond=1e3)
    x0 = np.zeros_like(x_star)
    a = lbfgs(fg, x0, maxiter=6, first_step=0.5)
    b = lbfgs(fg, x0, maxiter=6, first_step=0.5, precond=None)
    assert np.array_equal(a[0], b[0]) and a[2] == b[2]


def test_preconditioned_checkpoint_and_resume_are_bit_identical(tmp_path):
    d, x_star, fg = _quadratic(cond=1e3)
    p = 1.0 / np.sqrt(d)  # an inexact preconditioner: the run takes several iterations
    x0 = np.zeros_like(x_star)
    full = lbfgs(fg, x0, maxiter=6, first_step=0.5, precond=p)
    path = str(tmp_path / "state.npz")
    lbfgs(fg, x0, maxiter=3, first_step=0.5, precond=p, checkpoint=path)
    resumed = lbfgs(fg, None, maxiter=6, first_step=0.5, precond=p, resume=path)
    assert np.array_equal(full[0], resumed[0]) and full[1] == resumed[1] and full[2] == resumed[2]
    # a callable resumes with the p of the state, without calling it
    again = lbfgs(fg, None, maxiter=6, first_step=0.5, precond=lambda *a: pytest.fail("rebuilt"), resume=path)
    assert np.array_equal(full[0], again[0])
    with pytest.raises(ValueError):
        lbfgs(fg, None, maxiter=6, first_step=0.5, precond=p * 2.0, resume=path)
    with pytest.raises(ValueError):
        lbfgs(fg, None, maxiter=6, first_step=0.5, resume=path)
    plain = str(tmp_path / "plain.npz")
    lbfgs(fg, x0, maxiter=2, first_step=0.5, checkpoint=plain)
    with pytest.raises(ValueError):
        lbfgs(fg, None, maxiter=6, first_step=0.5, precond=p, resume=plain)


def test_precond_must_be_positive_and_model_shaped():
    d, x_star, fg = _quadratic()
    with pytest.raises(ValueError):
        lbfgs(fg, np.zeros_like(x_star), maxiter=2, precond=-1.0 / d)
    with pytest.raises(ValueError):
        lbfgs(fg, np.zeros_like(x_star), maxiter=2, precond=np.ones(3))


def test_illumination_preconditioner_definition():
    H = np.array([[4.0, 1.0], [0.0, 0.04]])
    p = sh.illumination_preconditioner(H, eps=0.01)
    assert np.allclose(p, 1.0 / (H / 4.0 + 0.01))
    with pytest.raises(ValueError):
        sh.illumination_preconditioner(np.zeros((2, 2)))
    assert lbfgs_device_slots(5) == 19


class _HostEngine:
    def __init__(self, H):
        self.H = H
        self.uploaded = None

    def illumination(self, wrt="velocity"):
        return self.H[wrt]

    def vec_upload(self, slot, a):
        self.uploaded = (slot, np.array(a))


def test_host_exchange_sums_the_illumination_over_a_world_of_two():
    from full_waveform_inversion_amd.rendezvous import Rendezvous
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    rng = np.random.default_rng(3)
    parts = [{w: rng.random((5, 7)) for w in ("velocity", "slowness2")} for _ in range(2)]
    out, err = [None, None], []

    def rank(r):
        try:
            rdzv = Rendezvous(r, 2, port=port, timeout=60.0)
            try:
                ex = sh.HostExchange(rdzv)
                eng = _HostEngine(parts[r])
                out[r] = (ex.reduce_illumination(eng, "slowness2"), ex.reduce_illumination(eng, "velocity", slot=3),
                          eng.uploaded)
            finally:
                rdzv.close()
        except BaseException as ex:  # noqa: BLE001  (re-raised below)
            err.append(ex)

    ts = [threading.Thread(target=rank, args=(r,)) for r in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    assert not err, err
    for r in range(2):
        H, none, (slot, up) = out[r]
        assert np.allclose(H, parts[0]["slowness2"] + parts[1]["slowness2"])
        assert none is None and slot == 3 and np.allclose(up, parts[0]["velocity"] + parts[1]["velocity"])


# accumulate <fp32, bf16, fp64 store>, bf16 source correction, finalize x2, vec_mul x2, vec_recip x2
ILLUM_KERNELS = 10


def test_illumination_object_has_no_scratch_and_a_pinned_kernel_count():
    path = os.path.join(co.CSRC, "fwi_illum.o")
    if not co.tools_present() or not os.path.exists(path):
        pytest.skip("ROCm LLVM tools or the built objects are missing (run `make -C full_waveform_inversion_amd/csrc`)")
    ks = co.kernels([path])
    bad = [k["name"] for k in ks if k.get("private_segment_fixed_size", 0) > 0 or k.get("vgpr_spill_count", 0) > 0]
    assert not bad, bad
    assert len(ks) == ILLUM_KERNELS, [k["name"] for k in ks]
    assert sum("illum_accumulate<" in k["name"] for k in ks) == 3
