"""The imaging Born operator without a GPU: its NumPy restatement (tests/_born_imaging.py) is the exact transpose of the
oracle's ``adjoint`` + ``gradient`` under ``image_stride`` and the bf16 store, equals ``_born.born`` on a lossless store,
and makes ``shots.gauss_newton_hvp`` symmetric on a strided engine; the two C-ABI symbols; the code objects of the new
kernels (fwi_born_bf16.o, fwi_born3d_bf16.o)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import _born
import _born_imaging as bi
from full_waveform_inversion_amd import _lib, shots as sh
from oracle import fwi_oracle as fo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import code_objects as co  # noqa: E402

FWI_EINVAL = 1
NT, ORDER, NPML = 37, 8, 4
CPML = {"abc": "cpml", "pml_alpha_max": 40.0}
CASES = [  # id, shape, propagator options
    ("2d_s3_sponge", (20, 24), {"image_stride": 3}),
    ("2d_s4_cpml", (20, 24), {"image_stride": 4, **CPML}),
    ("3d_s2", (12, 14, 16), {"image_stride": 2}),
    ("3d_bf16", (12, 14, 16), {"store_dtype": "bf16"}),
    ("3d_bf16_s3", (12, 14, 16), {"store_dtype": "bf16", "image_stride": 3}),
]


def _setup(shape, opts, seed=0):
    rng = np.random.default_rng(seed)
    c = 2000.0 + 600.0 * rng.random(shape)
    h = 10.0
    dt = 0.6 * fo.cfl_dt(c.max(), h, len(shape), ORDER)
    src = np.array([[s // 2 for s in shape], [s // 3 for s in shape], [s // 2 for s in shape]])  # a duplicate node
    wav = np.stack([fo.ricker(NT, dt, 0.25 / dt / 8) * a for a in (1.0, 0.7, -0.4)], 1)
    rec = np.stack([rng.integers(0, s, 6) for s in shape], 1)
    p = fo.Propagator(c, h, dt, ORDER, NPML, **opts)
    p.forward(src, wav, rec, save=True)
    dc = 30.0 * rng.standard_normal(shape)
    r = rng.standard_normal((NT, len(rec)))
    return p, c, dc, r


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_imaging_born_is_the_transpose_of_the_oracles_adjoint_and_gradient(case):
    """<J_img dm, r> = <dm, gradient(wrt)> after adjoint(r), fp64: 1e-12 relative (round-off of two 37-step sweeps)."""
    _, shape, opts = case
    p, c, dc, r = _setup(shape, opts)
    p.adjoint(r)
    for wrt, v in (("velocity", dc), ("slowness2", -2.0 * dc / c ** 3)):
        J = bi.born_imaging(p, v, wrt)
        assert np.linalg.norm(J) > 0.0
        lhs, rhs = float(np.vdot(J, r)), float(np.vdot(v, p.gradient(wrt)))
        print(case[0], wrt, abs(lhs - rhs) / abs(lhs))
        assert abs(lhs - rhs) <= 1e-12 * abs(lhs)


def test_the_exact_born_is_not_that_transpose_on_a_strided_store():
    """What the imaging operator is for: the exact J against the strided J^T misses the identity by far more."""
    p, c, dc, r = _setup((20, 24), {"image_stride": 3})
    p.adjoint(r)
    lhs, rhs = float(np.vdot(_born.born(p, dc), r)), float(np.vdot(dc, p.gradient()))
    assert abs(lhs - rhs) > 1e-6 * abs(lhs)


@pytest.mark.parametrize("shape,opts", [((20, 24), {}), ((20, 24), CPML), ((12, 14, 16), {})],
                         ids=["2d_sponge", "2d_cpml", "3d"])
def test_imaging_born_equals_born_on_a_lossless_store_bitwise(shape, opts):
    p, c, dc, _ = _setup(shape, opts)
    for wrt, v in (("velocity", dc), ("slowness2", -2.0 * dc / c ** 3)):
        assert np.array_equal(bi.born_imaging(p, v, wrt), _born.born(p, v, wrt))


def test_gauss_newton_hvp_is_symmetric_on_a_strided_oracle_engine():
    shape, order, npml, nt = (36, 44), 4, 6, 70
    rng = np.random.default_rng(2)
    c = 2000.0 + 500.0 * rng.random(shape)
    h = 10.0
    dt = 0.6 * fo.cfl_dt(c.max(), h, 2, order)
    wav = fo.ricker(nt, dt, 0.12 / dt / 8)
    rec = np.stack([np.full(10, 8), np.arange(4, 44, 4)], 1)
    shots = [sh.Shot(np.array([[7, x]]), wav, rec) for x in (8, 34)]
    u, v = 30.0 * rng.standard_normal(shape), 30.0 * rng.standard_normal(shape)
    e = bi.ImagingOracleEngine(shape, h, dt, nt, order=order, npml=npml, image_stride=3)
    Hv = sh.gauss_newton_hvp(e, c, shots, v)
    Hu = sh.gauss_newton_hvp(e, None, shots, u)
    a, b = float(np.vdot(u, Hv)), float(np.vdot(v, Hu))
    print("<u, H v> - <v, H u> relative", abs(a - b) / abs(a))
    assert abs(a - b) <= 1e-12 * abs(a)
    # H = sum_s J_img^T J_img: <v, H v> is the sum of the squared imaging Born data
    jj = 0.0
    for s in shots:
        s.forward(e, save=True)
        jj += float(np.sum(s.born(e, v, operator="imaging") ** 2))
    assert abs(np.vdot(v, Hv) - jj) <= 1e-10 * jj
    # a Shot passes the operator on only to an engine that names it (tests/_born.py's engine takes no keyword)
    e0 = _born.BornOracleEngine(shape, h, dt, nt, order=order, npml=npml)
    e0.set_model(c)
    shots[0].forward(e0, save=True)
    assert np.array_equal(shots[0].born(e0, v, operator="imaging"), shots[0].born(e0, v))


def test_the_imaging_born_calls_are_declared_bound_and_exported_at_abi_14():
    lib = _lib.load()
    assert lib.fwi_abi_version() == _lib.ABI_VERSION == 14
    header = open(os.path.join(ROOT, "include", "fwi.h")).read()
    for name in ("fwi_born_imaging", "fwi_born_imaging_vec"):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and name + "(" in header
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.replace("_imaging", "")]


def test_the_imaging_born_calls_reject_a_null_context():
    lib = _lib.load()
    buf = np.zeros(16, np.float32)
    vp = buf.ctypes.data_as(C.c_void_p)
    for wrt in (_lib.WRT_VELOCITY, _lib.WRT_SLOWNESS2, 7):
        for mode in (0, 1, 2, 9):
            assert lib.fwi_born_imaging(None, wrt, vp, mode, vp) == FWI_EINVAL
            assert lib.fwi_born_imaging_vec(None, wrt, 0, mode, None) == FWI_EINVAL


# ---- the code objects ------------------------------------------------------------------------------------------------
# born_weight_strided <fp32, fp64>, born_scatter_bf16, born_source_share
BORN_BF16_KERNELS = 4
# step3d_stream Born variants on the bf16 store (standard form only): <4, 8 rows> x <sponge, none> x <full, partial tiles>
BORN3D_BF16_KERNELS = 8


def _object(name):
    path = os.path.join(co.CSRC, name)
    if not co.tools_present() or not os.path.exists(path):
        pytest.skip("ROCm LLVM tools or the built objects are missing (run `make -C full_waveform_inversion_amd/csrc`)")
    ks = co.kernels([path])
    bad = [k["name"] for k in ks if k.get("private_segment_fixed_size", 0) > 0 or k.get("vgpr_spill_count", 0) > 0]
    assert not bad, bad
    return ks


def test_bf16_born_object_has_no_scratch_and_a_pinned_kernel_count():
    ks = _object("fwi_born_bf16.o")
    assert len(ks) == BORN_BF16_KERNELS, [k["name"] for k in ks]
    assert sum("born_scatter_bf16" in k["name"] for k in ks) == 1


def test_fused_bf16_born_object_has_no_scratch_and_fits_its_launch_bounds():
    ks = _object("fwi_born3d_bf16.o")
    assert len(ks) == BORN3D_BF16_KERNELS and all("step3d_stream<" in k["name"] for k in ks), [k["name"] for k in ks]
    for k in ks:  # 8-row tiles are 512 threads = 2 waves per SIMD: at most 256 VGPRs per lane; 4-row tiles 512
        args = k["name"].split("step3d_stream<")[1].split(">")[0].split(", ")
        ty, image, qb = int(args[2]), int(args[5]), args[9]
        assert image == 3 and qb == "true", k["name"]
        assert k["vgpr_count"] + k.get("agpr_count", 0) <= (256 if ty == 8 else 512), k
