"""The yardstick's own ladder: tests/_born.py (NumPy Born modelling on the oracle) against things that do not depend on
it -- a central finite difference of ``Propagator.forward`` and the dot-product identity with ``adjoint`` +
``gradient`` -- on 2-D / 3-D, sponge / CPML, O(4) / O(8) problems with random heterogeneous models.  These pass with or
without the engine's Born path.

Bounds.  Finite difference, 1e-7 relative L2: central differences with eps = 1e-3 of a dc of ~30 m/s rms leave
truncation O(eps^2) plus fp64 round-off over 2 eps ||dd|| / ||d||; measured <= 3.4e-9.  Dot-product identity and the
agreement of the two parametrisations, 1e-12: the oracle ladder's own bound (tests/test_oracle.py); measured <= 1.4e-15.
"""
import numpy as np
import pytest

import _born
from oracle import fwi_oracle as fo

CASES = [  # id, shape, order, npml, nt, options
    ("2d_sponge_o8", (48, 56), 8, 8, 90, {}),
    ("2d_cpml_o4", (44, 52), 4, 8, 90, {"abc": "cpml", "pml_alpha_max": 40.0}),
    ("3d_sponge_o4", (20, 18, 22), 4, 4, 50, {}),
    ("3d_cpml_o8", (20, 18, 22), 8, 5, 50, {"abc": "cpml", "pml_alpha_max": 30.0}),
]


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / np.linalg.norm(b))


def _setup(shape, order, nt, seed=0):
    rng = np.random.default_rng(seed)
    c = 2000.0 + 600.0 * rng.random(shape)
    h = 10.0
    dt = 0.6 * fo.cfl_dt(c.max(), h, len(shape), order)
    src = np.array([[s // 2 for s in shape], [s // 3 for s in shape]])
    rec = np.stack([np.clip(s // 2 + rng.integers(-6, 7, 6), 0, s - 1) for s in shape], 1)
    wav = np.stack([fo.ricker(nt, dt, 0.12 / dt / 8) * a for a in (1.0, -0.6)], 1)
    dc = 30.0 * rng.standard_normal(shape)
    return c, h, dt, src, rec, wav, dc, rng


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_born_is_the_derivative_of_forward(case):
    _, shape, order, npml, nt, opts = case
    c, h, dt, src, rec, wav, dc, _ = _setup(shape, order, nt)
    p = fo.Propagator(c, h, dt, order, npml, **opts)
    d = p.forward(src, wav, rec)
    J = _born.born(p, dc)
    assert np.linalg.norm(J) >= 1e-3 * np.linalg.norm(d)  # the perturbation is seen
    eps = 1e-3
    dp = fo.Propagator(c + eps * dc, h, dt, order, npml, sigma_max=p.sigma_max, **opts).forward(src, wav, rec)
    dm = fo.Propagator(c - eps * dc, h, dt, order, npml, sigma_max=p.sigma_max, **opts).forward(src, wav, rec)
    e = rel(J, (dp - dm) / (2 * eps))
    print(case[0], "fd", e)
    assert e <= 1e-7, e


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_born_is_the_transpose_of_the_gradient_and_both_parametrisations_agree(case):
    _, shape, order, npml, nt, opts = case
    c, h, dt, src, rec, wav, dc, rng = _setup(shape, order, nt)
    p = fo.Propagator(c, h, dt, order, npml, **opts)
    p.forward(src, wav, rec)
    J = _born.born(p, dc)
    r = rng.standard_normal(J.shape)
    p.adjoint(r)
    lhs, rhs = float(np.vdot(J, r)), float(np.vdot(dc, p.gradient("velocity")))
    print(case[0], "dot", abs(lhs - rhs) / abs(lhs))
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)
    assert rel(_born.born(p, -2.0 * dc / c ** 3, "slowness2"), J) <= 1e-12
    dm = rng.standard_normal(shape) * 1e-9
    assert abs(float(np.vdot(_born.born(p, dm, "slowness2"), r)) - float(np.vdot(dm, p.gradient("slowness2")))) \
        <= 1e-12 * abs(float(np.vdot(_born.born(p, dm, "slowness2"), r)))

