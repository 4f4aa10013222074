"""Model-space penalty terms: first-order Tikhonov and smoothed isotropic total variation, each with a prior model.

The objective becomes ``J(m) + lam R(m - m_prior)``.  With ``d = x - x0`` (``d = x`` without a prior), per axis ``a`` of
the grid order and weight ``w_a >= 0`` (cell units)::

    (D_a d)_i = d_{i+e_a} - d_i  for i_a < n_a - 1,   0 on the last cell of the axis,
    s_i = sum_a w_a (D_a d)_i^2,
    tikhonov  R = 1/2 sum_i s_i,                     k_i = 1,
    tv        R = sum_i (sqrt(s_i + eps^2) - eps),   k_i = 1 / sqrt(s_i + eps^2),   eps > 0,
    L(d; v) = sum_a w_a D_a' diag(k(d)) D_a v.

``L(d; d)`` is the gradient of R; for fixed d, L is symmetric positive semi-definite in v (the exact Hessian of
Tikhonov, the lagged-diffusivity one of TV) and annihilates constants.  The device form is ``Engine.vec_regularizer``
(``fwi_vec_regularizer``, ``csrc/fwi_reg.hip``); this module holds its fp64 NumPy twin and the wrappers that add the
term to an ``fg`` of :func:`lbfgs.lbfgs` / :func:`lbfgs.lbfgs_device` and to the Gauss-Newton products of
:func:`newton.gauss_newton_step`.  No reference counterpart.
"""
from __future__ import annotations

import numpy as np

KINDS = ("tikhonov", "tv")


def _weights(weight, ndim):
    w = np.atleast_1d(np.asarray(weight, np.float64))
    if w.ndim != 1 or w.size not in (1, ndim):
        raise ValueError("weight must be a scalar or %d weights, got shape %r" % (ndim, tuple(np.shape(weight))))
    w = np.broadcast_to(w, (ndim,))
    if not (np.isfinite(w).all() and (w >= 0.0).all()):
        raise ValueError("weight must be finite and >= 0, got %r" % (w.tolist(),))
    return [float(v) for v in w]


def _checked(kind, eps):
    if kind not in KINDS:
        raise ValueError("unknown kind %r (one of %s)" % (kind, list(KINDS)))
    if kind == "tv" and not (eps is not None and np.isfinite(eps) and eps > 0.0):
        raise ValueError("total variation needs a finite eps > 0, got %r" % (eps,))
    return 0.0 if kind == "tikhonov" else float(eps)


def _diff(d, ax):
    """D_a d: forward difference, zero on the last cell of the axis."""
    out = np.zeros_like(d)
    lo = [slice(None)] * d.ndim
    hi = list(lo)
    lo[ax], hi[ax] = slice(0, -1), slice(1, None)
    out[tuple(lo)] = d[tuple(hi)] - d[tuple(lo)]
    return out


def _diff_t(f, ax):
    """D_a' f: (D' f)_j = f_{j-e_a} - f_j, with f on the last cell of the axis taken as zero."""
    lo = [slice(None)] * f.ndim
    hi = list(lo)
    lo[ax], hi[ax] = slice(0, -1), slice(1, None)
    out = np.zeros_like(f)
    out[tuple(lo)] = -f[tuple(lo)]
    out[tuple(hi)] += f[tuple(lo)]
    return out


def _difference(x, x0):
    d = np.asarray(x, np.float64)
    if x0 is not None:
        x0 = np.asarray(x0, np.float64)
        if x0.shape != d.shape:
            raise ValueError("x0 has shape %r, x %r" % (x0.shape, d.shape))
        d = d - x0
    return d


def _s(d, w):
    s = np.zeros_like(d)
    for ax, wa in enumerate(w):
        if wa:
            s += wa * _diff(d, ax) ** 2
    return s


def value(x, kind="tv", weight=1.0, eps=None, x0=None):
    """R(x - x0) in fp64."""
    eps = _checked(kind, eps)
    d = _difference(x, x0)
    s = _s(d, _weights(weight, d.ndim))
    if kind == "tikhonov":
        return 0.5 * float(np.sum(s))
    return float(np.sum(s / (np.sqrt(s + eps * eps) + eps)))  # sqrt(s + eps^2) - eps without the cancellation


def apply(x, v=None, kind="tv", weight=1.0, eps=None, x0=None):
    """L(x - x0; v) in fp64 (``v=None``: v = x - x0, the gradient of R)."""
    eps = _checked(kind, eps)
    d = _difference(x, x0)
    w = _weights(weight, d.ndim)
    if v is None:
        v = d
    else:
        v = np.asarray(v, np.float64)
        if v.shape != d.shape:
            raise ValueError("v has shape %r, x %r" % (v.shape, d.shape))
    k = 1.0 if kind == "tikhonov" else 1.0 / np.sqrt(_s(d, w) + eps * eps)
    out = np.zeros_like(d)
    for ax, wa in enumerate(w):
        if wa:
            out += wa * _diff_t(k * _diff(v, ax), ax)
    return out


def value_and_gradient(x, kind="tv", weight=1.0, eps=None, x0=None):
    """``(R(x - x0), dR/dx)`` in fp64."""
    return value(x, kind, weight, eps, x0), apply(x, None, kind, weight, eps, x0)


class Regularizer:
    """``lam R(m - x0)`` as one object: what ``newton.gauss_newton_step(regularizer=)`` takes."""

    def __init__(self, lam, kind="tv", weight=1.0, eps=None, x0=None):
        if not (np.isfinite(lam) and lam >= 0.0):
            raise ValueError("lam must be finite and >= 0, got %r" % (lam,))
        _checked(kind, eps)
        self.lam, self.kind, self.weight, self.eps = float(lam), kind, weight, eps
        self.x0 = None if x0 is None else np.array(x0, np.float64)

    def value_and_gradient(self, model):
        r, g = value_and_gradient(model, self.kind, self.weight, self.eps, self.x0)
        return self.lam * r, self.lam * g

    def hvp(self, model, v):
        """``lam L(model - x0; v)``: symmetric positive semi-definite in v."""
        return self.lam * apply(model, v, self.kind, self.weight, self.eps, self.x0)


def regularized_fg(fg, lam, kind="tv", weight=1.0, eps=None, x0=None):
    """``fg(x) -> (f, g)`` of :func:`lbfgs.lbfgs` with the penalty added: ``(f + lam R(x - x0), g + lam L(d; d))``, the
    sum formed in fp64 and returned in g's dtype.  ``lam == 0`` returns ``fg`` itself."""
    if not (np.isfinite(lam) and lam >= 0.0):
        raise ValueError("lam must be finite and >= 0, got %r" % (lam,))
    if lam == 0.0:
        return fg
    reg = Regularizer(lam, kind, weight, eps, x0)

    def fg_reg(x):
        f, g = fg(x)
        r, gr = reg.value_and_gradient(x)
        g = np.asarray(g)
        return f + r, (g.astype(np.float64) + gr).astype(g.dtype)

    return fg_reg


def prior_slot(history=5, precond_slot=None, h0=None):
    """The first of the ``extra_slots`` of :func:`lbfgs.lbfgs_device`: where a prior model can live."""
    from .lbfgs import lbfgs_device_slots
    base = lbfgs_device_slots(history) if precond_slot is None else int(precond_slot) + 1
    return base + int(getattr(h0, "nslots", 0))


def regularized_fg_device(engine, fg, lam, kind="tv", weight=1.0, eps=None, x0_slot=None, x0=None):
    """``fg(x_slot, g_slot) -> f`` of :func:`lbfgs.lbfgs_device` with the penalty added by ONE device call,
    ``g_slot := lam L(d; d) + g_slot`` (no further slot), returning ``f + lam R``.  ``x0_slot``: the slot of the prior
    model (None: none); with a host array ``x0`` as well, the wrapper uploads it there before its first evaluation
    (``lbfgs_device`` creates its slots anew: ask it for ``extra_slots=1`` and take ``prior_slot(...)``).
    ``lam == 0`` returns ``fg`` itself."""
    from .shots import engine_of
    if not (np.isfinite(lam) and lam >= 0.0):
        raise ValueError("lam must be finite and >= 0, got %r" % (lam,))
    if lam == 0.0:
        return fg
    _checked(kind, eps)
    if x0 is not None and x0_slot is None:
        raise ValueError("a prior model needs a slot (x0_slot)")
    e = engine_of(engine)
    todo = [] if x0 is None else [np.array(x0)]

    def fg_reg(x_slot, g_slot):
        if todo:
            e.vec_upload(x0_slot, todo.pop())
        f = fg(x_slot, g_slot)
        return f + lam * e.vec_regularizer(x_slot, out=g_slot, kind=kind, x0=x0_slot, alpha=lam, beta=1.0,
                                           weight=weight, eps=eps)

    return fg_reg
