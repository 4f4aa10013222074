"""Tests-only NumPy restatement of the IMAGING Born operator (include/fwi.h, fwi_born_imaging) on top of the CPU oracle
(``oracle/`` is frozen; like ``_born.py``, whose loop this is with one line changed).

``Propagator.adjoint(image)`` + ``gradient`` of a propagator with ``image_stride = S`` pair the adjoint field with the
store on the steps n % S == 0 only, weight S; with ``store_dtype="bf16"`` the store holds bf16(C L u^n) + C src^n.  They
are the exact transpose of the operator that takes its scattering source from that same store:

    dq^n     = C (L du^n + CPML terms of du^n) + [n % S == 0] S w q~^n,    q~^n = p.q_store[n]
    du^{n+1} = A (2 du^n - B du^{n-1} + dq^n),   du^0 = du^{-1} = 0;   dd^n = R du^{n+1}

On a lossless store (S = 1, native type) this is ``_born.born`` bit for bit.  tests/test_born_imaging_oracle.py checks
the transpose statement with nothing but the oracle.  Never imported by the product package.
"""
import numpy as np

import _born


def born_imaging(p, dm, wrt="velocity"):
    """``J_img dm`` as ``(nt, nrec)`` for the last ``p.forward(..., save=True)``, in ``p.dtype``."""
    if p.q_store is None:
        raise RuntimeError("forward(..., save=True) must precede born_imaging")
    dt_ = p.dtype
    w = _born.weight(p, dm, wrt).astype(dt_)
    u_prev = np.zeros(p.shape, dt_)
    u_cur = np.zeros(p.shape, dt_)
    rec = np.zeros((p.nt, len(p.rec_flat)), dt_)
    aux = [(np.zeros(p.shape, dt_), np.zeros(p.shape, dt_)) for _ in range(p.ndim)] if p.cpml else None
    for n in range(p.nt):
        extra = p._cpml_term(u_cur, aux, False) if p.cpml else 0.0
        dq = p.C * (p.laplacian(u_cur) + extra)
        if p.image_stride == 1:
            dq = dq + w * p.q_store[n]  # (the expression of _born.born: the same bits)
        elif n % p.image_stride == 0:
            dq += p.image_stride * w * p.q_store[n]
        u_next = p.A * (2 * u_cur - p.B * u_prev + dq)
        rec[n] = u_next.reshape(-1)[p.rec_flat]
        u_prev, u_cur = u_cur, u_next
    return rec


class ImagingOracleEngine(_born.BornOracleEngine):
    """``_born.BornOracleEngine`` with the signature of ``Engine.born``: ``image_stride`` and ``store_dtype`` go to the
    oracle's propagator, ``operator="imaging"`` is :func:`born_imaging`, "exact" stays ``_born.born``."""

    born_operators = ("exact", "imaging")

    def __init__(self, shape, h, dt, nt_max, order=8, npml=0, sigma_max=None, dtype=np.float64, image_stride=1,
                 store_dtype="native", **opts):
        super().__init__(shape, h, dt, nt_max, order=order, npml=npml, sigma_max=sigma_max, dtype=dtype,
                         image_stride=image_stride, store_dtype=store_dtype, **opts)

    def born(self, dm, wrt="velocity", mode="auto", download=True, operator="exact"):
        if operator not in self.born_operators:
            raise ValueError("operator must be 'exact' or 'imaging'")
        d = born_imaging(self._p, dm, wrt) if operator == "imaging" else _born.born(self._p, dm, wrt)
        return d if download else None
