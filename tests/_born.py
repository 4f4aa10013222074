"""Tests-only NumPy restatement of Born modelling on top of the CPU oracle (``oracle/`` is frozen; like ``_mms.py``).

With the oracle's scheme (oracle/fwi_oracle.py, header), C = dt^2 c^2 and q^n the forward term ``Propagator.forward``
stores:

    w        = dC / C = 2 dc / c  (wrt velocity)   or   -c^2 dm  (wrt m = 1 / c^2)
    dq^n     = C (L du^n + CPML terms of du^n) + w q^n          (no point source)
    du^{n+1} = A (2 du^n - B du^{n-1} + dq^n),   du^0 = du^{-1} = 0
    dd^n     = R du^{n+1},   n = 0 .. nt - 1

the exact derivative of the discrete ``forward`` along dc (dm), whose exact transpose is ``adjoint`` + ``gradient``.
tests/test_born_oracle.py checks both statements against things that do not depend on this file.  Never imported by the
product package.
"""
import numpy as np


def weight(p, dm, wrt="velocity"):
    dm = np.asarray(dm, np.float64)
    if dm.shape != p.shape:
        raise ValueError("perturbation must be model-shaped")
    if wrt == "velocity":
        return 2.0 * dm / p.c
    if wrt == "slowness2":
        return -(p.c ** 2) * dm
    raise ValueError("wrt must be 'velocity' or 'slowness2'")


def born(p, dm, wrt="velocity"):
    """``J dm`` as ``(nt, nrec)`` for the last ``p.forward(..., save=True)``, in ``p.dtype``."""
    if p.q_store is None:
        raise RuntimeError("forward(..., save=True) must precede born")
    dt_ = p.dtype
    w = weight(p, dm, wrt).astype(dt_)
    u_prev = np.zeros(p.shape, dt_)
    u_cur = np.zeros(p.shape, dt_)
    rec = np.zeros((p.nt, len(p.rec_flat)), dt_)
    aux = [(np.zeros(p.shape, dt_), np.zeros(p.shape, dt_)) for _ in range(p.ndim)] if p.cpml else None
    for n in range(p.nt):
        extra = p._cpml_term(u_cur, aux, False) if p.cpml else 0.0
        dq = p.C * (p.laplacian(u_cur) + extra) + w * p.q_store[n]
        u_next = p.A * (2 * u_cur - p.B * u_prev + dq)
        rec[n] = u_next.reshape(-1)[p.rec_flat]
        u_prev, u_cur = u_cur, u_next
    return rec


class BornOracleEngine:
    """Engine interface over the NumPy oracle with ``born``: lets the host code of ``shots.gauss_newton_hvp`` and
    ``newton`` run without a GPU, and is the fp64 reference of the GPU tests' inversion."""

    def __init__(self, shape, h, dt, nt_max, order=8, npml=0, sigma_max=None, dtype=np.float64, **opts):
        from oracle import fwi_oracle as fo
        self._fo = fo
        self.shape, self.h, self.dt, self.order, self.npml = tuple(shape), h, dt, order, npml
        self.sigma_max, self.dtype, self._opts = sigma_max, np.dtype(dtype), opts
        self._p = None
        self._g = np.zeros(self.shape)

    def set_model(self, model):
        self._p = self._fo.Propagator(np.asarray(model, np.float64), self.h, self.dt, self.order, self.npml,
                                      sigma_max=self.sigma_max, dtype=self.dtype, **self._opts)

    def reset_gradient(self):
        self._g = np.zeros(self.shape)

    def forward(self, model, src, rec, save=True):
        if model is not None:
            self.set_model(model)
        return self._p.forward(src[0], src[1], rec, save=save)

    def born(self, dm, wrt="velocity"):
        return born(self._p, dm, wrt)

    def adjoint(self, residual, image=True):
        a = self._p.adjoint(residual, image=image)
        if image:
            self._g = self._g + self._p.gradient("slowness2")
        return a

    def gradient(self, wrt="velocity"):
        return self._g if wrt == "slowness2" else self._g * (-2.0 / self._p.c ** 3)

    def gradient_add_from(self, other):
        self._g = self._g + other._g

    def close(self):
        pass
