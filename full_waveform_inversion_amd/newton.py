"""Gauss-Newton steps: conjugate gradients on the Hessian-vector products of :mod:`shots`.

``H_GN = sum_s J_s^T J_s`` is applied matrix-free (``shots.gauss_newton_hvp``: three sweeps per shot and product), so an
inner iteration costs about one and a half gradient evaluations.  Host arrays are enough at this size of problem; the
products themselves run on the device.  No reference counterpart.

Traveltime tomography has the same two layers on ``shots.TraveltimeOperator`` (one tangent and one adjoint eikonal solve
per shot and product): :func:`traveltime_newton_step` and :func:`traveltime_gauss_newton`.
"""
from __future__ import annotations

import numpy as np


def cg(hvp, b, x0=None, precond=None, maxiter=20, rtol=1e-6, callback=None):
    """Preconditioned conjugate gradients for ``H x = b`` with ``H`` symmetric positive (semi-)definite, given as
    ``hvp(p) -> H p`` on arrays of ``b``'s shape.  ``precond``: None, an array applied elementwise (an approximate
    inverse diagonal, e.g. ``shots.illumination_preconditioner``) or a callable ``r -> M^-1 r``.

    Stops when ``||r|| <= rtol ||r_0||``, after ``maxiter`` products, or on a direction of non-positive curvature
    ``p^T H p <= 0`` (the iterate reached so far is returned; a Gauss-Newton Hessian has none up to round-off).
    Returns ``(x, log)``: one entry per iterate k = 0, 1, ... with ``iter``, ``rnorm`` = ||b - H x_k|| and, from k = 1
    on, ``curvature`` = p^T H p and ``alpha`` of the step that led there; the last entry carries ``stop`` =
    "converged" | "maxiter" | "negative_curvature".  ``callback(k, x_k)`` is called for every iterate.
    """
    b = np.asarray(b, np.float64)
    apply_m = (lambda r: r) if precond is None else precond if callable(precond) else \
        (lambda r, m=np.asarray(precond, np.float64): m * r)
    x = np.zeros_like(b) if x0 is None else np.array(x0, np.float64)
    r = b - np.asarray(hvp(x), np.float64) if x0 is not None else b.copy()
    z = np.asarray(apply_m(r), np.float64)
    p = z.copy()
    rz = float(np.vdot(r, z))
    r0 = float(np.linalg.norm(r))
    log = [{"iter": 0, "rnorm": r0}]
    if callback:
        callback(0, x)
    if r0 == 0.0:
        log[-1]["stop"] = "converged"
        return x, log
    for k in range(1, int(maxiter) + 1):
        Hp = np.asarray(hvp(p), np.float64)
        curv = float(np.vdot(p, Hp))
        if not curv > 0.0:
            log[-1]["stop"] = "negative_curvature"
            log[-1]["curvature"] = curv
            return x, log
        alpha = rz / curv
        x = x + alpha * p
        r = r - alpha * Hp
        rn = float(np.linalg.norm(r))
        log.append({"iter": k, "rnorm": rn, "curvature": curv, "alpha": alpha})
        if callback:
            callback(k, x)
        if rn <= rtol * r0:
            log[-1]["stop"] = "converged"
            return x, log
        z = np.asarray(apply_m(r), np.float64)
        rz_new = float(np.vdot(r, z))
        p = z + (rz_new / rz) * p
        rz = rz_new
    log[-1]["stop"] = "maxiter"
    return x, log


def gauss_newton_step(engine, model, shots, g, exchange=None, wrt="velocity", precond=None, maxiter=10, rtol=1e-2,
                      damping=0.0, callback=None, regularizer=None, objective=None):
    """The (truncated) Gauss-Newton step ``p``: ``(H_GN + damping I) p = -g`` at ``model`` by :func:`cg`, with ``g``
    the gradient ``shots.misfit_and_gradient`` returned there (same ``wrt``).  ``precond`` as in :func:`cg`; the
    illumination preconditioner of ``shots.illumination_preconditioner`` fits (the illumination is the diagonal of the
    pseudo-Hessian).  Every inner iteration is one ``shots.gauss_newton_hvp``: three sweeps per shot, and the engine's
    gradient accumulator is overwritten.  Returns ``(p, log)`` (``log`` as :func:`cg`).

    ``regularizer``: a ``regularizers.Regularizer``; its symmetric positive semi-definite term ``lam L(model - x0; v)``
    is added to every product (host fp64), for a ``g`` that already holds its gradient
    (``regularizers.regularized_fg``).  None: no such term.

    ``objective``: the ``datafit.WeightedL2`` that ``g`` was computed with; every product then carries its weight,
    ``H_GN = sum_s J_s^T B M_s^2 B J_s`` (``shots.gauss_newton_hvp``), or the ``datafit.RobustMisfit``: the weight is then
    its IRLS one at ``model``, ``B (tw M_s^2 psi(e_s)) B``, positive semi-definite for every kind (each product forms it
    anew from the shot's residual: one more misfit call per shot, no further sweep).  None: plain least squares."""
    from .shots import _engines, gauss_newton_hvp
    for e in _engines(engine):
        e.set_model(model)
    g = np.asarray(g, np.float64)

    def hvp(v):
        dtype = getattr(_engines(engine)[0], "dtype", np.float64)
        kw = {} if objective is None else {"objective": objective}
        Hv = np.asarray(gauss_newton_hvp(engine, None, shots, np.asarray(v, dtype), exchange, wrt, **kw), np.float64)
        Hv = Hv + damping * v if damping else Hv
        return Hv if regularizer is None else Hv + regularizer.hvp(model, v)

    return cg(hvp, -g, precond=precond, maxiter=maxiter, rtol=rtol, callback=callback)


def traveltime_newton_step(op, g, damping=0.0, maxiter=10, rtol=1e-2, precond=None, regularizer=None, callback=None):
    """The (truncated) Gauss-Newton step of traveltime tomography: ``(H + damping I [+ lam L]) p = -g`` by :func:`cg`,
    ``H = sum_s J_s^T W_s J_s`` applied by ``op`` (a ``shots.TraveltimeOperator`` at the model where
    ``shots.traveltime_fg`` returned ``g``, same ``wrt`` and weights): per inner iteration one tangent and one adjoint
    solve per shot.  ``precond`` as in :func:`cg`; ``regularizer`` as in :func:`gauss_newton_step` (the operator must
    have been given its model).
    Returns ``(p, log)`` (``log`` as :func:`cg`)."""
    g = np.asarray(g, np.float64)
    if regularizer is not None and op.model is None:
        raise ValueError("traveltime_newton_step: a regularizer needs the operator's model (TraveltimeOperator(model=...))")
    if regularizer is not None and op.wrt != "velocity":
        raise ValueError("traveltime_newton_step: a regularizer acts on the velocity model; use wrt='velocity' with it")

    def hvp(v):
        Hv = np.asarray(op.hvp(v), np.float64)
        Hv = Hv + damping * v if damping else Hv
        return Hv if regularizer is None else Hv + regularizer.hvp(op.model, v)

    return cg(hvp, -g, precond=precond, maxiter=maxiter, rtol=rtol, callback=callback)


def traveltime_gauss_newton(engine, model0, shots, picks, pick_weights=None, iters=3, cg_iters=6, rtol=1e-2,
                            rel_damping=1e-2, bounds=None, radius=0.0, slot0=0, exchange=None, wrt="velocity",
                            regularizer=None, precond=None):
    """Damped Gauss-Newton traveltime tomography from the velocity ``model0``: ``(model, log)``.  Per iteration: the
    operator at the model (``shots.TraveltimeOperator``, times kept); ``mu = rel_damping (g.Hg) / (g.g)`` (one
    product); ``p`` from :func:`traveltime_newton_step` with ``damping = mu`` (``cg_iters`` products at most); then
    ``t = 1``, halved while ``J`` (``shots.traveltime_fg`` at ``model + t p`` clipped to ``bounds``, with the
    regulariser's value) does not fall -- after 10 halvings the iterations stop at the model reached.  The ``(J, g)``
    of the accepted trial start the next iteration.  With ``wrt="slowness2"`` the step is taken in ``1 / c^2`` and
    turned back into a velocity.  ``log[0]`` holds the starting ``J``; ``log[k]`` the ``J`` after iteration k, its
    ``t``, ``mu``, the :func:`cg` log and the eikonal / tangent / adjoint solves of the iteration on this rank (those of
    ``log[0]``: the first evaluation).  ``regularizer`` and ``precond`` as in :func:`traveltime_newton_step` (the
    regulariser's value and gradient are added to ``J`` and ``g``; it acts on the velocity model, so it is refused
    with ``wrt="slowness2"``).  The engines need ``max(shots.TRAVELTIME_SLOTS, op.slots_needed(n_local))``
    vector slots from ``slot0`` on."""
    from .shots import NoExchange, TraveltimeOperator, partition_shots, traveltime_fg
    if regularizer is not None and wrt != "velocity":
        raise ValueError("traveltime_gauss_newton: a regularizer acts on the velocity model; use wrt='velocity' with it")
    ex = exchange or NoExchange()
    n_local = len(partition_shots(len(shots), ex.rank, ex.world))
    count = {"eikonal": 0, "tangent": 0, "adjoint": 0}

    def fg(m):
        J, g = traveltime_fg(engine, m, shots, picks, pick_weights, radius=radius, slot0=slot0, exchange=exchange,
                             wrt=wrt)
        count["eikonal"] += n_local
        count["adjoint"] += n_local
        if regularizer is not None:
            r, gr = regularizer.value_and_gradient(m)
            J, g = J + r, g + gr
        return J, np.asarray(g, np.float64)

    def moved(m, step):
        if wrt == "slowness2":
            m = np.maximum(1.0 / m ** 2 + step, np.finfo(np.float64).tiny) ** -0.5
        else:
            m = m + step
        return m if bounds is None else np.clip(m, bounds[0], bounds[1])

    def taken():
        out = dict(count)
        for k in count:
            count[k] = 0
        return out

    m = np.array(model0, np.float64)
    J, g = fg(m)
    log = [{"iter": 0, "J": J, "solves": taken()}]
    for it in range(1, int(iters) + 1):
        op = TraveltimeOperator(engine, m, shots, radius=radius, slot0=slot0, exchange=exchange, wrt=wrt,
                                pick_weights=pick_weights, picks=picks, keep_times=True)
        gg = float(np.vdot(g, g))
        if gg == 0.0:
            log[-1]["stop"] = "zero_gradient"
            break
        mu = float(rel_damping) * float(np.vdot(g, op.hvp(g))) / gg
        p, cglog = traveltime_newton_step(op, g, damping=mu, maxiter=cg_iters, rtol=rtol, precond=precond,
                                          regularizer=regularizer)
        for k in ("eikonal", "tangent", "adjoint"):
            count[k] += op.solves[k]
        t = 1.0
        for _ in range(11):
            mt = moved(m, t * p)
            Jt, gt = fg(mt)
            if Jt < J:
                break
            t *= 0.5
        else:
            log[-1]["stop"] = "line_search"
            log[-1]["solves_after"] = taken()
            break
        m, J, g = mt, Jt, gt
        log.append({"iter": it, "J": J, "t": t, "mu": mu, "cg": cglog, "solves": taken()})
    return m, log
