"""Angle-domain common-image gathers on the CPU: the NumPy twin (``fourier.shift_sum``, ``fourier.angle_gather``,
``fourier.angle_gather_adjoint``, ``fourier.tangents``) that tests/test_gpu_slant.py holds the device to.

1. identities of the twin: the transpose, ``S_0``, integer shifts, a gather that is zero away from ``h = 0``
2. a dipping event in the offset gather stacks best at its own tangent, at its own depth
3. a two-layer reflection experiment through the oracle: the reflector's depth is flat across the angles at the true
   background and is not at a background 10 % too slow
4. the binding, the header and the driver's flags"""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _feximage as FX
from full_waveform_inversion_amd import _lib, fourier
from oracle import fwi_oracle as fo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(9, 13), (9, 5, 13), (7, 4)]
OFFSETS, TANGENTS = np.arange(-4, 5), fourier.tangents(np.linspace(-50.0, 50.0, 11))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(k) for k in s))
@pytest.mark.parametrize("taper", [False, True], ids=["ones", "taper"])
def test_transpose_identity(shape, taper):
    rng = np.random.default_rng(3)
    E, A = rng.standard_normal((OFFSETS.size,) + shape), rng.standard_normal((TANGENTS.size,) + shape)
    t = 0.5 + 0.5 * np.cos(np.pi * OFFSETS / 10.0) if taper else None
    TE, TtA = fourier.angle_gather(E, OFFSETS, TANGENTS, t), fourier.angle_gather_adjoint(A, OFFSETS, TANGENTS, t)
    assert TE.shape == A.shape and TtA.shape == E.shape and TE.dtype == np.float64
    lhs, rhs = float(np.vdot(A, TE)), float(np.vdot(TtA, E))
    print("<A, T E> = %.17g, <T^T A, E> = %.17g" % (lhs, rhs))
    assert lhs != 0 and abs(lhs - rhs) <= 1e-13 * abs(lhs)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(k) for k in s))
def test_shift_identities_bit_for_bit(shape):
    rng = np.random.default_rng(4)
    a = rng.standard_normal((3,) + shape)
    nz = shape[0]
    assert np.array_equal(fourier.shift_sum(a[:1], [0.0]), a[0])  # S_0 is the identity
    for s in (1, -1, 2, -3, nz - 1, 1 - nz, nz, -nz, nz + 1, 10 ** 9, -10 ** 9):  # whole planes, or nothing
        assert np.array_equal(fourier.shift_sum(a[:1], [float(s)]), FX.shifted(a[:1], 0, s)[0]), s
    # a tap outside the grid contributes zero and the other still counts
    half = fourier.shift_sum(a[:1], [nz - 0.5])
    assert np.array_equal(half[0], 0.5 * a[0][nz - 1]) and not np.any(half[1:])
    half = fourier.shift_sum(a[:1], [-(nz - 0.5)])
    assert np.array_equal(half[nz - 1], 0.5 * a[0][0]) and not np.any(half[:nz - 1])
    assert not np.any(fourier.shift_sum(a[:1], [nz + 0.5])) and not np.any(fourier.shift_sum(a[:1], [-nz - 0.5]))
    # beta == 0 does not read dst; beta != 0 does, also with every source outside the grid
    nan = np.full(shape, np.nan)
    assert np.array_equal(fourier.shift_sum(a, [0.5, -1.25, 2.0], [1.0, -2.0, 0.5], 0.0, nan),
                          fourier.shift_sum(a, [0.5, -1.25, 2.0], [1.0, -2.0, 0.5]))
    assert np.array_equal(fourier.shift_sum(a[:1], [1e9], None, -0.5, a[1]), -0.5 * a[1])
    # linear interpolation between the two planes
    got = fourier.shift_sum(a[:1], [2.25], [3.0])
    ref = 3.0 * (0.75 * FX.shifted(a[:1], 0, 2)[0] + 0.25 * FX.shifted(a[:1], 0, 3)[0])
    assert np.allclose(got, ref, rtol=0, atol=1e-15 * np.abs(a).max() * 3)
    # a gather whose only non-zero lag is h = 0: every angle image is E_0
    E = np.zeros((OFFSETS.size,) + shape)
    E[4] = a[2]
    A = fourier.angle_gather(E, OFFSETS, TANGENTS)
    assert all(np.array_equal(Aj, a[2]) for Aj in A)


def test_twin_arguments():
    a = np.zeros((2, 5, 4))
    for bad in (lambda: fourier.shift_sum(a, [0.0]), lambda: fourier.shift_sum(a, [0.0, np.nan]),
                lambda: fourier.shift_sum(a, [0.0, 1.0], [1.0]), lambda: fourier.shift_sum(a, [0.0, 1.0], [1.0, np.inf]),
                lambda: fourier.shift_sum(a, [0.0, 1.0], None, np.nan), lambda: fourier.shift_sum(a, [0.0, 1.0], None, 1.0),
                lambda: fourier.shift_sum(a, [0.0, 1.0], None, 1.0, np.zeros((4, 4))),
                lambda: fourier.angle_gather(a, [0, 1, 2], [0.0]), lambda: fourier.angle_gather(a, [0, 0.5], [0.0]),
                lambda: fourier.angle_gather(a, [0, 1], [0.0], [1.0]),
                lambda: fourier.angle_gather_adjoint(a, [0, 1], [0.0]),
                lambda: fourier.tangents([90.0]), lambda: fourier.tangents([[1.0]])):
        with pytest.raises(ValueError):
            bad()
    assert np.allclose(fourier.tangents([-45, 0, 45]), [-1, 0, 1], atol=1e-15) and fourier.tangents(30.0).shape == (1,)


def test_a_dipping_event_stacks_at_its_own_tangent_and_depth():
    nz, z0, p0 = 64, 30, 0.5
    h = np.arange(-8, 9)
    tang = np.linspace(-1.0, 1.0, 9)
    z = np.arange(nz)
    E = np.stack([np.exp(-0.5 * ((z - z0 - p0 * hl) / 1.5) ** 2) for hl in h])[:, :, None] * np.ones((1, 1, 3))
    A = fourier.angle_gather(E, h, tang)
    j0 = int(np.argmin(np.abs(tang - p0)))
    peak = A[:, :, 1].max(axis=1)
    print("peak per tangent:", np.round(peak, 2))
    assert tang[j0] == p0 and int(np.argmax(peak)) == j0 and np.all(np.delete(peak, j0) < peak[j0])
    assert int(np.argmax(A[j0, :, 1])) == z0 and peak[j0] <= h.size


# -- the two-layer experiment (the one of tests/test_fsplit_host.py, six shots) ----------------------------------------

@functools.lru_cache(maxsize=None)
def _peak_depths():
    """Per background (true, 10 % too slow): the depth in cells of the reflector's peak in every angle image, at x = 50"""
    shape, h, order, npml, nt, stride = (96, 100), 10.0, 4, 12, 420, 2
    dt = 0.6 * fo.cfl_dt(2600.0, h, 2, order)
    c_true = np.full(shape, 2000.0)
    c_true[60:] = 2600.0
    f0 = 1.0 / (16.0 * dt)
    wav = fo.ricker(nt, dt, f0, t0=24.0 * dt)[:, None]
    rec = np.stack([np.full(40, 16), np.arange(10, 90, 2)], 1)
    srcs = [np.array([[16, x]]) for x in range(20, 81, 12)]
    offsets, tang = np.arange(-8, 9), np.linspace(-0.6, 0.6, 13)
    freqs = fourier.fourier_bins(nt, dt, stride, 0.3 * f0, 2.5 * f0)
    assert freqs.size == 58
    # the reflection alone: the data of the two layers less those of the upper layer's velocity everywhere
    data = [np.asarray(fo.Propagator(c_true, h, dt, order, npml).forward(s, wav, rec, save=False))
            - np.asarray(fo.Propagator(np.full(shape, 2000.0), h, dt, order, npml).forward(s, wav, rec, save=False))
            for s in srcs]
    out = []
    for c_bg in (2000.0, 1800.0):
        E = np.zeros((offsets.size,) + shape)
        for s, r in zip(srcs, data):
            p = fo.Propagator(np.full(shape, c_bg), h, dt, order, npml, image_stride=stride)
            p.forward(s, wav, rec)
            Q = fourier.analyse(np.asarray(p.q_store)[::stride], nt, stride, dt, freqs)
            p.src_flat = np.arange(shape[0] * shape[1])  # the adjoint field itself, recorded at every cell
            mu = np.asarray(p.adjoint(r, image=False)).reshape((nt,) + shape)[::stride]
            M = fourier.adjoint_spectrum(mu, nt, stride, dt, freqs)
            for l, hl in enumerate(offsets):
                E[l] += fourier.offset_image(Q, M, nt, stride, dt, freqs, 1, hl)
        col = np.abs(fourier.angle_gather(E, offsets, tang)[:, 30:90, 50])
        z = []
        for cj in col:  # the peak below the acquisition, refined by the parabola through its neighbours
            k = int(np.argmax(cj))
            assert 0 < k < cj.size - 1
            z.append(30 + k + 0.5 * (cj[k - 1] - cj[k + 1]) / (cj[k - 1] - 2.0 * cj[k] + cj[k + 1]))
        out.append(np.array(z))
    return tuple(out)


def test_the_reflector_is_flat_across_angles_only_in_the_true_background():
    true, slow = _peak_depths()
    st, ss = float(true.max() - true.min()), float(slow.max() - slow.min())
    print("depth of the reflector's peak per angle, true background: %s\n... 10 %% too slow: %s\nspread %.2f against %.2f "
          "cells" % (np.round(true, 2), np.round(slow, 2), st, ss))
    assert abs(np.median(true) - 59.5) <= 0.5  # the interface lies between rows 59 and 60
    assert np.median(slow) < np.median(true) - 3.0  # too slow: too shallow
    assert ss > st  # 5.59 against 0.26 cells measured


# -- the binding, the header, the driver --------------------------------------------------------------------------------

def test_binding_and_header_declare_the_call_under_the_same_abi():
    header = open(os.path.join(ROOT, "include", "fwi.h")).read()
    name = "fwi_vec_shift_sum"
    assert name in _lib.SIGNATURES
    assert re.search(r"^int %s\(fwi_ctx \*ctx, int32_t dst, int32_t nsrc, const int32_t \*src_slots," % name, header, re.M)
    assert "#define FWI_ABI_VERSION 14" in header and _lib.ABI_VERSION == 14
    assert "#define FWI_SHIFT_SUM_MAX %d" % _lib.SHIFT_SUM_MAX in header
    assert fourier.SHIFT_SUM_MAX == _lib.SHIFT_SUM_MAX == 64
    lib = _lib.load()
    assert lib.fwi_abi_version() == 14
    assert lib.fwi_vec_shift_sum(None, 0, 1, None, None, None, 0.0) == 1  # null context: refused without a device
    makefile = open(os.path.join(ROOT, "full_waveform_inversion_amd", "csrc", "Makefile")).read()
    # the object is built, and rebuilt when fwi_slant.h (or any header it includes) changes: the compiler writes the
    # dependencies of every object beside it and the Makefile reads them back
    assert " fwi_slant.o " in makefile
    assert re.search(r"^%\.o: %\.hip\n\t.* -MMD -MP -c \$< -o \$@$", makefile, re.M)
    assert re.search(r"^-include \$\(OBJS:\.o=\.d\)$", makefile, re.M)


def test_the_engine_and_the_shot_loop_have_the_methods():
    from full_waveform_inversion_amd import Engine, shots
    assert all(callable(getattr(Engine, m)) for m in ("vec_shift_sum", "angle_gather_vec", "gather_moment"))
    assert callable(shots.angle_gather)


def test_run_config_knows_the_angle_flags_and_refuses_bad_combinations():
    """tools/run_config.py --angle-gather / --angle-out: checked before any engine exists"""
    tool = os.path.join(ROOT, "tools", "run_config.py")
    out = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--angle-gather" in out.stdout and "--angle-out" in out.stdout
    store = ["--fourier-store", "2,12"]
    for bad, word in ((["--angle-gather", "x:8:33:50", "--angle-out", "a.npz"], "--fourier-store"),
                      (["--angle-gather", "x:8:33:50"] + store, "--angle-out"),
                      (["--angle-out", "a.npz"] + store, "--angle-gather"),
                      (["--angle-gather", "z:8:33:50", "--angle-out", "a.npz"] + store, "AXIS:L:NANG:MAXDEG"),
                      (["--angle-gather", "x:-1:33:50", "--angle-out", "a.npz"] + store, "AXIS:L:NANG:MAXDEG"),
                      (["--angle-gather", "x:8:0:50", "--angle-out", "a.npz"] + store, "AXIS:L:NANG:MAXDEG"),
                      (["--angle-gather", "x:8:33:90", "--angle-out", "a.npz"] + store, "AXIS:L:NANG:MAXDEG"),
                      (["--angle-gather", "x:100:60:50", "--angle-out", "a.npz"] + store, "AXIS:L:NANG:MAXDEG"),
                      (["--angle-gather", "x:8:33", "--angle-out", "a.npz"] + store, "AXIS:L:NANG:MAXDEG")):
        out = subprocess.run([sys.executable, tool] + bad, capture_output=True, text=True)
        assert out.returncode == 2 and word in out.stderr, (bad, out.stderr[-400:])
