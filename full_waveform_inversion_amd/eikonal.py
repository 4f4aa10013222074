"""First-arrival traveltimes on the engine's grid and their discrete adjoint: the NumPy twin of ``fwi_eikonal*`` and the
DEFINITION of what those calls compute.

``|grad T| = s``, ``s = 1 / c``, by the first-order Godunov upwind scheme.  For cell ``i`` and axis ``d``,
``t_d = min(T[i - e_d], T[i + e_d])`` (a neighbour outside the grid counts as ``+inf``; on a tie the lower-index one is
"the" upwind neighbour).  With the ``t_d`` sorted ``a <= b <= c`` and ``f = s_i h``, the local solution ``G_i`` is

    a + f                                               if that is <= b,
    a + (b' + sqrt(2 f^2 - b'^2)) / 2                   else, if that is <= c   (b' = b - a; the last case in 2-D),
    a + (S + sqrt(S^2 - 3 (Q - f^2))) / 3               else                    (S = b' + c', Q = b'^2 + c'^2, c' = c - a),

the usual roots ``(a + b + sqrt(2 f^2 - (a - b)^2)) / 2`` and ``(S + sqrt(S^2 - 3 (Q - f^2))) / 3`` written with the
smallest time taken out, so that the square root's argument is formed from differences of the order of ``f`` and not
from squares of whole traveltimes.  The source is an init list (nodes, their distances ``d_i`` in metres and one
reference node): ``T_init = s_ref d_i`` on the listed nodes, ``+inf`` elsewhere, and the solution is the limit of
``T <- min(T, T_init, G(T))`` from ``+inf``.  There is no mask: a listed node is *source-determined* exactly when its
final ``T_i < G_i``.

The adjoint differentiates that fixed point.  With the active axes ``D = {d : t_d < T_i}``,

    dG_i/dt_d = (T_i - t_d) / sum_{e in D} (T_i - t_e),      dG_i/ds_i = s_i h^2 / sum_{e in D} (T_i - t_e),

both zero where ``T_i < G_i``; ``lambda = b + A^T lambda`` with ``A_ij = dG_i/dT_j`` (strictly causal, so the Jacobi
iteration stops bit-exactly), ``g_s = (dG/ds) lambda`` plus ``sum_i d_i lambda_i`` over the source-determined listed
nodes at ``ref``.

The tangent (``fwi_eikonal_tangent``) differentiates the same fixed point forwards: with
``ds = -dm / c^2`` (or ``dm c / 2`` for ``m = 1 / c^2``), ``b = (dG/ds) ds`` and ``b_i = d_i ds[ref]`` on the
source-determined listed nodes, ``x = b + A x`` in gather form, by the same Jacobi iteration.  It is the exact transpose
of the adjoint followed by the gradient.

Reflections off a FIXED interface are two such solves in a row.  A *wall* is a boolean array of the
grid's shape: a walled cell holds ``+inf`` from start to end and is, to every other cell, a neighbour outside the grid
(``f = +inf`` in the local solver: ``G = +inf``).  :func:`solve_from` is the limit of ``T <- min(T, G(T))`` from any
``T_init`` (finite and ``>= 0`` on the secondary sources, ``+inf`` elsewhere); a node is *source-determined* when its
final ``T_i`` is finite and ``< G_i``, and then ``T_i = T_init,i``.  Stage 1 runs from the source inside the wall, stage
2 restarts from the interface nodes with the times they just got; :func:`handover` carries a field across on the
source-determined nodes, which is all the adjoint and the tangent of the chain need beside the pieces above
(:func:`reflection_gradient`, :func:`reflection_tangent`: exact transposes).  The adjoint needs no wall: a walled
cell is not live and never anybody's upwind neighbour.

Out of scope: the factored eikonal equation, second-order stencils, anisotropy; of the later arrivals everything but
reflections off a fixed, node-rounded interface -- the reflector's depth is not an unknown and has no sub-cell position
(its staircase is part of the first-order error), head waves, multiples and transmitted conversions are not separate
arrivals.  The scheme is first
order: 0.3 - 1.2 % of ``max T`` on 101^2 - 401^2 grids (the table in DESIGN.md), most of it from the source's
neighbourhood, which a ball of a few cells (``radius``) reduces.

No reference counterpart.
"""
from __future__ import annotations

import itertools

import numpy as np

WRT = ("velocity", "slowness2")


def ball(coords, shape, h, radius=0.0):
    """The init list of a source at fractional grid coordinates ``coords`` (cells): ``(idx (n, ndim) int32, dist (n,)
    float64 metres, ref (ndim,) int32)``.  Every node within ``radius`` cells is listed, in ascending flat order; at
    ``radius`` 0 the nearest node alone.  ``ref`` is the nearest node, the lowest index on a tie."""
    shape = tuple(int(n) for n in shape)
    x = np.asarray(coords, np.float64).reshape(-1)
    if x.size != len(shape):
        raise ValueError("coords must hold %d coordinates, got %r" % (len(shape), np.shape(coords)))
    if np.any(x < 0.0) or np.any(x > np.array(shape) - 1.0):
        raise ValueError("the source must lie inside the grid [0, n - 1] on every axis")
    if not (np.isfinite(radius) and radius >= 0.0):
        raise ValueError("radius = %r must be finite and >= 0" % (radius,))
    R = float(radius) + 1.0  # the nearest node is at most sqrt(ndim) / 2 < 1 away
    rng = [np.arange(max(0, int(np.floor(x[d] - R))), min(shape[d] - 1, int(np.ceil(x[d] + R))) + 1)
           for d in range(len(shape))]
    nodes = np.array(list(itertools.product(*rng)), dtype=np.int64).reshape(-1, len(shape))  # ascending flat order
    r = np.sqrt(((nodes - x) ** 2).sum(axis=1))
    ref = int(np.argmin(r))  # the first of equal minima: the lowest index
    keep = r <= float(radius)
    keep[ref] = True
    return (np.ascontiguousarray(nodes[keep], dtype=np.int32), np.ascontiguousarray(r[keep] * float(h)),
            np.ascontiguousarray(nodes[ref], dtype=np.int32))


def _source(src, shape, h, radius):
    """``src`` as an init list: already one (a 3-tuple), or coordinates for :func:`ball`"""
    if isinstance(src, tuple) and len(src) == 3 and np.ndim(src[0]) == 2:
        idx, dist, ref = src
        return (np.ascontiguousarray(idx, dtype=np.int32), np.ascontiguousarray(dist, dtype=np.float64),
                np.ascontiguousarray(np.reshape(ref, -1), dtype=np.int32))
    return ball(src, shape, h, radius)


def _shift(T, d, k, fill):
    """``T[i + k e_d]``, ``fill`` outside the grid"""
    out = np.full_like(T, fill)
    n = T.shape[d]
    src = [slice(None)] * T.ndim
    dst = [slice(None)] * T.ndim
    if k > 0:
        src[d], dst[d] = slice(k, n), slice(0, n - k)
    else:
        src[d], dst[d] = slice(0, n + k), slice(-k, n)
    out[tuple(dst)] = T[tuple(src)]
    return out


def upwind(T):
    """Per axis ``(t_d, lower)``: the smaller neighbour's time and whether it is the lower-index one (ties: yes)"""
    out = []
    for d in range(T.ndim):
        lo, hi = _shift(T, d, -1, np.inf), _shift(T, d, +1, np.inf)
        out.append((np.minimum(lo, hi), lo <= hi))
    return out


def local_solution(t, f):
    """``G`` from the per-axis upwind times ``t`` (a list of ndim arrays) and ``f = s h``, in their dtype"""
    two, three = f.dtype.type(2), f.dtype.type(3)
    srt = np.sort(np.stack(t), axis=0)
    a, b = srt[0], srt[1]
    c = srt[2] if len(t) == 3 else np.full_like(a, np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        x1 = a + f
        bp = b - a
        x2 = a + (bp + np.sqrt(two * f * f - bp * bp)) / two
        cp = c - a
        S, Q = bp + cp, bp * bp + cp * cp
        x3 = a + (S + np.sqrt(S * S - three * (Q - f * f))) / three
    return np.where(x1 <= b, x1, np.where(x2 <= c, x2, x3))


def _slowness(c, dtype):
    c = np.asarray(c, dtype=dtype)
    return dtype.type(1) / c


def init_times(c, h, init, dtype=np.float64):
    """``T_init``: ``s_ref d_i`` on the listed nodes, ``+inf`` elsewhere"""
    dtype = np.dtype(dtype)
    idx, dist, ref = init
    s = _slowness(c, dtype)
    T0 = np.full(s.shape, np.inf, dtype)
    T0[tuple(idx.T)] = s[tuple(ref)] * dist.astype(dtype)
    return T0


def _wall(wall, shape):
    if wall is None:
        return None
    wall = np.asarray(wall)
    if wall.shape != tuple(shape):
        raise ValueError("wall must have the grid's shape %r, got %r" % (tuple(shape), wall.shape))
    return wall != 0


def sweep(T, s, h, wall=None):
    """One Jacobi sweep ``min(T, G(T))`` (``T_init`` is in ``T`` from the start and ``min`` keeps it); a walled cell
    (``wall``: booleans of the grid's shape) is never updated"""
    f = s * s.dtype.type(h)
    Tn = np.minimum(T, local_solution([t for t, _ in upwind(T)], f))
    return Tn if wall is None else np.where(wall, T, Tn)


def _fixed_point(T, s, h, wall, max_sweeps, return_sweeps, who):
    if wall is not None:
        T = np.where(wall, T.dtype.type(np.inf), T)
    cap = 4 * sum(T.shape) if max_sweeps is None else int(max_sweeps)
    for n in range(1, cap + 1):
        Tn = sweep(T, s, h, wall)
        if np.array_equal(Tn, T):
            return (T, n) if return_sweeps else T
        T = Tn
    raise RuntimeError("eikonal.%s: no fixed point after %d sweeps" % (who, cap))


def solve(c, h, src, radius=0.0, dtype=np.float64, max_sweeps=None, return_sweeps=False, wall=None):
    """First-arrival times of the model ``c`` (m/s) for the source ``src`` (coordinates in cells, or an init list):
    plain Jacobi from ``+inf`` until a sweep changes no bit.  ``wall``: cells the front may not enter (``+inf``)."""
    dtype = np.dtype(dtype)
    c = np.asarray(c)
    init = _source(src, c.shape, h, radius)
    return _fixed_point(init_times(c, h, init, dtype), _slowness(c, dtype), h, _wall(wall, c.shape), max_sweeps,
                        return_sweeps, "solve")


def check_start(T_init, wall=None):
    """What a slot-started solve refuses: ``ValueError`` unless ``T_init`` is free of NaNs and of negative entries and
    holds a finite one, on the cells that are not walled"""
    T_init = np.asarray(T_init)
    free = T_init if wall is None else T_init[~wall]
    if np.any(np.isnan(free)) or np.any(free < 0):
        raise ValueError("T_init holds a NaN or a negative entry")
    if not np.any(np.isfinite(free)):
        raise ValueError("T_init holds no finite entry: there is no source")


def solve_from(c, h, T_init, wall=None, dtype=np.float64, max_sweeps=None, return_sweeps=False):
    """The limit of ``T <- min(T, G(T))`` from ``T = T_init`` (finite and ``>= 0`` on the secondary sources, ``+inf``
    elsewhere; walled cells ``+inf`` whatever it says there).  With ``T_init = init_times(c, h, init)`` and no wall it
    is :func:`solve`, bit for bit."""
    dtype = np.dtype(dtype)
    c = np.asarray(c)
    T0 = np.array(T_init, dtype=dtype)
    if T0.shape != c.shape:
        raise ValueError("T_init must have the grid's shape %r, got %r" % (c.shape, T0.shape))
    wall = _wall(wall, c.shape)
    check_start(T0, wall)
    return _fixed_point(T0, _slowness(c, dtype), h, wall, max_sweeps, return_sweeps, "solve_from")


def solve_blocks(c, h, src, radius=0.0, tile=8, inner=4, dtype=np.float64, wall=None, T_init=None):
    """The same fixed point by block Jacobi, as the device runs it: per outer step every ``tile``-cell block takes
    ``inner`` sweeps with the cells around it frozen, all blocks reading the same input.  Returns ``(T, outer steps)``.
    ``wall``: cells that are never updated; ``T_init``: the start of :func:`solve_from` instead of ``src``."""
    dtype = np.dtype(dtype)
    c = np.asarray(c)
    s = _slowness(c, dtype)
    T = init_times(c, h, _source(src, c.shape, h, radius), dtype) if T_init is None else np.array(T_init, dtype=dtype)
    wall = _wall(wall, c.shape)
    if wall is not None:
        T = np.where(wall, dtype.type(np.inf), T)
    f = s * dtype.type(h)
    nd = c.ndim
    for n in range(1, 4 * sum(c.shape) + 1):
        Tn = T.copy()
        for org in itertools.product(*[range(0, m, tile) for m in c.shape]):
            lo = [max(0, o - 1) for o in org]
            hi = [min(m, o + tile + 1) for o, m in zip(org, c.shape)]
            box = tuple(slice(a, b) for a, b in zip(lo, hi))
            own = tuple(slice(o - a, min(o + tile, m) - a) for o, a, m in zip(org, lo, c.shape))
            P = np.full([b - a + 2 for a, b in zip(lo, hi)], np.inf, dtype)  # the box with +inf around it
            ins = tuple(slice(1, -1) for _ in range(nd))
            P[ins] = T[box]
            F = np.ones(P.shape, dtype)
            F[ins] = f[box]
            keep = np.ones(P.shape, bool)  # everything but the block's own cells is frozen
            keep[tuple(slice(o.start + 1, o.stop + 1) for o in own)] = False
            if wall is not None:
                keep[ins] |= wall[box]
            for _ in range(inner):
                Pn = np.minimum(P, local_solution([t for t, _ in upwind(P)], F))
                P = np.where(keep, P, Pn)
            Tn[tuple(slice(o, min(o + tile, m)) for o, m in zip(org, c.shape))] = P[ins][own]
        if np.array_equal(Tn, T):
            return T, n
        T = Tn
    raise RuntimeError("eikonal.solve_blocks: no fixed point")


def derivatives(T, c, h):
    """At the fixed point ``T``: ``(W, lower, dGds)`` with ``W[d] = dG_i/dt_d`` (0 on inactive axes and where
    ``T_i < G_i``), ``lower[d]`` whether the upwind neighbour on axis ``d`` is the lower-index one, and ``dG_i/ds_i``."""
    dtype = T.dtype
    s = _slowness(c, dtype)
    hh = dtype.type(h)
    up = upwind(T)
    G = local_solution([t for t, _ in up], s * hh)
    live = np.isfinite(T) & ~(T < G)
    with np.errstate(invalid="ignore", divide="ignore"):
        diff = [np.where(live & (t < T), T - t, dtype.type(0)) for t, _ in up]
        den = diff[0]
        for x in diff[1:]:
            den = den + x
        ok = den > 0
        W = [np.where(ok, x / den, dtype.type(0)) for x in diff]
        dGds = np.where(ok, s * hh * hh / den, dtype.type(0))
    return W, [lo for _, lo in up], dGds


def adjoint_sweep(lam, b, W, lower):
    """``b + A^T lam`` in gather form, the terms of a cell added axis by axis, lower neighbour first"""
    zero = lam.dtype.type(0)
    out = b.copy()
    for d in range(lam.ndim):
        # cell i = j - e_d hands lam_i to j when its upwind neighbour on d is the upper one; i = j + e_d when the lower
        out = out + _shift(np.where(lower[d], zero, W[d] * lam), d, -1, zero)
        out = out + _shift(np.where(lower[d], W[d] * lam, zero), d, +1, zero)
    return out


def adjoint(T, c, h, b, return_sweeps=False):
    """``lambda = b + A^T lambda`` by Jacobi from ``lambda = b``, recomputed in full until a sweep changes no bit"""
    W, lower, _ = derivatives(T, c, h)
    b = np.asarray(b, dtype=T.dtype)
    lam = b.copy()
    for n in range(1, 4 * sum(T.shape) + 1):
        ln = adjoint_sweep(lam, b, W, lower)
        if np.array_equal(ln, lam):
            return (lam, n) if return_sweeps else lam
        lam = ln
    raise RuntimeError("eikonal.adjoint: no fixed point")


def adjoint_matrix(T, c, h):
    """The dense ``A`` (``A[i, j] = dG_i/dT_j``, flat indices) of a SMALL grid, for tests"""
    W, lower, _ = derivatives(T, c, h)
    n = T.size
    A = np.zeros((n, n))
    flat = np.arange(n).reshape(T.shape)
    for d in range(T.ndim):
        for i in np.ndindex(*T.shape):
            if W[d][i] != 0:
                j = list(i)
                j[d] += -1 if lower[d][i] else 1
                A[flat[i], flat[tuple(j)]] = W[d][i]
    return A


def gradient(T, lam, c, h, init, wrt="velocity", ball_term=True):
    """The gradient of ``sum_i b_i T_i`` with respect to the model: ``g_s = (dG/ds) lambda`` plus the source term at
    ``ref``, then ``g_c = -g_s / c^2`` (``wrt="velocity"``) or ``g_m = g_s c / 2`` (``"slowness2"``, ``m = 1 / c^2``)"""
    if wrt not in WRT:
        raise ValueError("wrt must be one of %r" % (WRT,))
    dtype = T.dtype
    c = np.asarray(c, dtype=dtype)
    _, _, dGds = derivatives(T, c, h)
    gs = dGds * lam
    if ball_term and init is not None:
        idx, dist, ref = init
        s = _slowness(c, dtype)
        G = local_solution([t for t, _ in upwind(T)], s * dtype.type(h))
        acc = dtype.type(0)
        for k in range(len(dist)):  # in list order, as the device's one thread
            i = tuple(idx[k])
            if T[i] < G[i]:
                acc = acc + dtype.type(dist[k]) * lam[i]
        gs[tuple(ref)] += acc
    return -gs / (c * c) if wrt == "velocity" else gs * c / dtype.type(2)


def tangent_sweep(x, b, W, lower):
    """``b + A x`` in gather form: cell ``i`` reads its own upwind neighbour on every axis (the lower-index one where
    ``lower[d]``), the terms added axis by axis in ascending order after ``b``"""
    zero = x.dtype.type(0)
    out = b.copy()
    for d in range(x.ndim):
        out = out + W[d] * np.where(lower[d], _shift(x, d, -1, zero), _shift(x, d, +1, zero))
    return out


def tangent_rhs(T, c, h, dm, init, wrt="velocity", ball_term=True):
    """``(b, W, lower)`` of :func:`tangent`: ``b = (dG/ds) ds`` with ``ds = -dm / c^2`` (``wrt="velocity"``) or
    ``dm c / 2`` (``"slowness2"``), the transposes of the two conversions of :func:`gradient`, and
    ``b_i = dist_k ds[ref]`` on the listed nodes that are source-determined (``T_i < G_i``)"""
    if wrt not in WRT:
        raise ValueError("wrt must be one of %r" % (WRT,))
    dtype = T.dtype
    c = np.asarray(c, dtype=dtype)
    dm = np.asarray(dm, dtype=dtype)
    if dm.shape != T.shape:
        raise ValueError("dm must have the grid's shape %r, got %r" % (T.shape, dm.shape))
    W, lower, dGds = derivatives(T, c, h)
    ds = -dm / (c * c) if wrt == "velocity" else dm * c / dtype.type(2)
    b = dGds * ds
    if ball_term and init is not None:
        idx, dist, ref = init
        G = local_solution([t for t, _ in upwind(T)], _slowness(c, dtype) * dtype.type(h))
        for k in range(len(dist)):
            i = tuple(idx[k])
            if T[i] < G[i]:
                b[i] = dtype.type(dist[k]) * ds[tuple(ref)]
    return b, W, lower


def source_determined(T, c, h):
    """Where ``T_i`` is finite and ``T_i < G_i``: the nodes whose time is their start's, not their neighbours'"""
    G = local_solution([t for t, _ in upwind(T)], _slowness(c, T.dtype) * T.dtype.type(h))
    return np.isfinite(T) & (T < G)


def handover(T, c, h, x):
    """``x`` on the source-determined nodes of the fixed point ``T`` and 0 elsewhere: what one stage of a multi-stage
    solve hands to the stage before it (the adjoint variable) or receives from it (the tangent)"""
    x = np.asarray(x, dtype=T.dtype)
    return np.where(source_determined(T, c, h), x, T.dtype.type(0))


def tangent(T, c, h, dm, init, wrt="velocity", return_sweeps=False, ball_term=True, max_sweeps=None, b0=None):
    """The derivative of the fixed point ``T`` along the model perturbation ``dm``, in ``T``'s dtype:
    ``x = b + A x`` (``A`` and ``b`` of :func:`tangent_rhs`) by Jacobi from ``x = b``, recomputed in full until a sweep
    changes no bit (``A`` is strictly causal: it stops after the longest dependency chain).  Where ``T_i = +inf`` or
    the cell is not live, ``x_i = b_i``.  ``max_sweeps=None``: ``4 * sum(shape)``; ``RuntimeError`` beyond the cap.  The
    exact transpose of :func:`adjoint` followed by :func:`gradient`; on the
    non-differentiable set the same one-sided choice.  ``init=None``: no source term.  ``b0``: any array of the grid's
    shape, added to ``b`` (after ``b_i``, before the axis terms): ``x = b(dm) + b0 + A x``, the tangent of a solve
    whose start moves by ``b0`` with the model."""
    b, W, lower = tangent_rhs(T, c, h, dm, init, wrt, ball_term)
    if b0 is not None:
        b0 = np.asarray(b0, dtype=T.dtype)
        if b0.shape != T.shape:
            raise ValueError("b0 must have the grid's shape %r, got %r" % (T.shape, b0.shape))
        b = b + b0
    x = b.copy()
    cap = 4 * sum(T.shape) if max_sweeps is None else int(max_sweeps)
    for n in range(1, cap + 1):
        xn = tangent_sweep(x, b, W, lower)
        if np.array_equal(xn, x):
            return (x, n) if return_sweeps else x
        x = xn
    raise RuntimeError("eikonal.tangent: no fixed point after %d sweeps" % cap)


def times_at(T, rec):
    """Times at receivers: node indices ``(n, ndim)`` or a ``points.Spread`` (multilinear weights)"""
    if hasattr(rec, "pt_start"):
        v = T[tuple(np.asarray(rec.idx).T)].astype(np.float64) * rec.weights
        return np.add.reduceat(v, rec.pt_start[:-1]) if len(v) else np.zeros(0)
    return T[tuple(np.asarray(rec, dtype=np.int64).reshape(-1, T.ndim).T)].astype(np.float64)


def exact_constant(shape, h, c0, coords):
    """``s r`` of a constant medium"""
    ax = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    r = np.sqrt(sum((a - x) ** 2 for a, x in zip(ax, np.asarray(coords, np.float64)))) * h
    return r / c0


def exact_gradient(shape, h, c0, g, coords):
    """``acosh(1 + g^2 r^2 / (2 c c0)) / g`` of ``c = c0 + g (z - z_src)``, depth the first axis; ``c0`` the velocity at
    the source"""
    x = np.asarray(coords, np.float64)
    ax = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    r2 = sum((a - xs) ** 2 for a, xs in zip(ax, x)) * h * h
    c = c0 + g * (ax[0] - x[0]) * h
    return np.arccosh(1.0 + g * g * r2 / (2.0 * c * c0)) / g


def interface(shape, depth):
    """``(gamma, wall)`` of a reflector at ``depth`` cells along the first axis, one value per column (an array of
    ``shape[1:]``, or a scalar): ``gamma`` marks the node nearest to it in every column (the lower index on a tie),
    ``wall`` everything below that node.  Both boolean, of the grid's shape."""
    shape = tuple(int(n) for n in shape)
    d = np.broadcast_to(np.asarray(depth, np.float64), shape[1:])
    if not np.all(np.isfinite(d)) or np.any(d < 0.0) or np.any(d > shape[0] - 1.0):
        raise ValueError("the reflector must lie inside the grid [0, %d] on the first axis" % (shape[0] - 1))
    node = np.ceil(d - 0.5).astype(np.int64)  # nearest, the lower index on a tie
    z = np.arange(shape[0]).reshape((-1,) + (1,) * (len(shape) - 1))
    return z == node[None], z > node[None]


def exact_reflection_constant(shape, h, c0, src, rec, Z):
    """The reflection time off a flat reflector at depth ``Z`` (cells, first axis) in a constant medium, by the image
    source: ``|x_r - x_s'| / c0`` with ``x_s'`` the source mirrored at ``Z``; ``rec``: ``(n, ndim)`` coordinates"""
    xs = np.asarray(src, np.float64).reshape(-1).copy()
    xs[0] = 2.0 * float(Z) - xs[0]
    r = np.asarray(rec, np.float64).reshape(-1, len(shape))
    return np.sqrt(((r - xs) ** 2).sum(axis=1)) * float(h) / float(c0)


def reflection_solve(c, h, src, gamma, wall, radius=0.0, dtype=np.float64):
    """Both stages of the reflection off the nodes ``gamma`` inside ``wall``: ``(T1, T2, init)`` with ``T1`` the first
    arrivals from ``src`` and ``T2`` the solve restarted from ``gamma`` with ``T1``'s times there"""
    dtype = np.dtype(dtype)
    init = _source(src, np.shape(c), h, radius)
    T1 = solve(c, h, init, dtype=dtype, wall=wall)
    T2 = solve_from(c, h, np.where(gamma, T1, dtype.type(np.inf)), wall, dtype=dtype)
    return T1, T2, init


def reflection_gradient(T1, T2, c, h, init, b2, wrt="velocity", with_handover=True):
    """The gradient of ``sum_i b2_i T2_i`` with respect to the model, through both stages.  ``with_handover=False``
    drops stage 1 (tests: the check against differences must then fail)."""
    lam2 = adjoint(T2, c, h, b2)
    g = gradient(T2, lam2, c, h, None, wrt)
    if with_handover:
        lam1 = adjoint(T1, c, h, handover(T2, c, h, lam2))
        g = g + gradient(T1, lam1, c, h, init, wrt)
    return g


def reflection_tangent(T1, T2, c, h, init, dm, wrt="velocity"):
    """``dT2`` along the model perturbation ``dm``: the exact transpose of :func:`reflection_gradient`"""
    x1 = tangent(T1, c, h, dm, init, wrt)
    return tangent(T2, c, h, dm, None, wrt, b0=handover(T2, c, h, x1))


class TwinEngine:
    """The engine calls ``shots.traveltime_fg`` and ``shots.TraveltimeOperator`` need, backed by this module on the CPU
    (tests, prototypes): model and slots are host arrays."""

    def __init__(self, shape, h, dtype=np.float64):
        self.shape, self.h, self.dtype = tuple(shape), float(h), np.dtype(dtype)
        self.ndim = len(self.shape)
        self.c = None
        self.vecs = []
        self.last_eikonal_launches = 0
        self._init = {}

    def set_model(self, model):
        self.c = np.array(model, dtype=self.dtype).reshape(self.shape)

    def vec_create(self, count):
        self.vecs = [np.zeros(self.shape, self.dtype) for _ in range(count)]

    def vec_download(self, slot):
        return self.vecs[slot].copy()

    def vec_upload(self, slot, a):
        self.vecs[slot] = np.array(a, dtype=self.dtype).reshape(self.shape)

    def vec_copy(self, dst, src):
        self.vecs[dst] = self.vecs[src].copy()

    def _slots(self, who, **slots):
        """what the C ABI refuses with FWI_EINVAL: a slot that does not exist, two arguments naming one slot"""
        for name, s in slots.items():
            if not 0 <= int(s) < len(self.vecs):
                raise ValueError("%s: %s = %d does not exist" % (who, name, s))
        if len(set(int(s) for s in slots.values())) != len(slots):
            raise ValueError("%s: %s must be %d different slots, got %r"
                             % (who, ", ".join(slots), len(slots), tuple(slots.values())))

    def _wall_of(self, wall_slot):
        return None if wall_slot is None else self.vecs[wall_slot] != 0

    def eikonal(self, src, t_slot, scratch_slot, radius=0.0, max_sweeps=None, wall_slot=None):
        init = _source(src, self.shape, self.h, radius)
        if wall_slot is not None:
            self._slots("eikonal", t_slot=t_slot, scratch_slot=scratch_slot, wall_slot=wall_slot)
        self.vecs[t_slot], self.last_eikonal_launches = solve(self.c, self.h, init, dtype=self.dtype,
                                                              max_sweeps=max_sweeps, return_sweeps=True,
                                                              wall=self._wall_of(wall_slot))
        self._init[t_slot] = init
        return init

    def eikonal_restart(self, t_slot, scratch_slot, wall_slot=None, max_sweeps=None):
        """As ``Engine.eikonal_restart``: the slot holds ``T_init``; what ``fwi_eikonal_stage`` refuses is a
        ``ValueError`` here"""
        slots = dict(t_slot=t_slot, scratch_slot=scratch_slot)
        if wall_slot is not None:
            slots["wall_slot"] = wall_slot
        self._slots("eikonal_restart", **slots)
        wall = self._wall_of(wall_slot)
        try:
            check_start(self.vecs[t_slot], wall)
        except ValueError as err:
            raise ValueError("eikonal_restart: t_slot: %s" % err)
        if self.c is None:
            raise ValueError("eikonal_restart: no model set")
        self.vecs[t_slot], self.last_eikonal_launches = solve_from(self.c, self.h, self.vecs[t_slot], wall,
                                                                   dtype=self.dtype, max_sweeps=max_sweeps,
                                                                   return_sweeps=True)

    def eikonal_handover(self, t_slot, in_slot, out_slot, beta=0.0):
        self._slots("eikonal_handover", t_slot=t_slot, in_slot=in_slot, out_slot=out_slot)
        if self.c is None:
            raise ValueError("eikonal_handover: no model set")
        v = handover(self.vecs[t_slot], self.c, self.h, self.vecs[in_slot])
        self.vecs[out_slot] = v if beta == 0.0 else self.dtype.type(beta) * self.vecs[out_slot] + v

    def eikonal_times(self, t_slot, rec):
        return times_at(self.vecs[t_slot], rec)

    def vec_scatter_points(self, slot, idx, values, beta=0.0):
        a = self.dtype.type(beta) * self.vecs[slot] if beta != 0.0 else np.zeros(self.shape, self.dtype)
        a[tuple(np.asarray(idx).reshape(-1, self.ndim).T)] += np.asarray(values, dtype=self.dtype)
        self.vecs[slot] = a

    def vec_gather_points(self, slot, idx):
        return self.vecs[slot][tuple(np.asarray(idx).reshape(-1, self.ndim).T)].astype(np.float64)

    def eikonal_adjoint(self, t_slot, rhs_slot, lam_slot, scratch_slot, max_sweeps=None):
        self.vecs[lam_slot], self.last_eikonal_launches = adjoint(self.vecs[t_slot], self.c, self.h, self.vecs[rhs_slot],
                                                                  return_sweeps=True)

    def eikonal_gradient(self, t_slot, lam_slot, out_slot, init=None, beta=0.0, wrt="velocity"):
        g = gradient(self.vecs[t_slot], self.vecs[lam_slot], self.c, self.h, init, wrt)
        self.vecs[out_slot] = g if beta == 0.0 else self.dtype.type(beta) * self.vecs[out_slot] + g

    def eikonal_tangent(self, t_slot, dm_slot, out_slot, scratch_slot, init=None, wrt="velocity", max_sweeps=None,
                        b0_slot=None):
        """As ``Engine.eikonal_tangent``; what ``fwi_eikonal_tangent`` (``fwi_eikonal_tangent_stage`` with
        ``init=None`` or a ``b0_slot``) refuses is a ``ValueError`` here"""
        if init is None or b0_slot is not None:
            return self._tangent_stage(t_slot, dm_slot, out_slot, scratch_slot, init, wrt, max_sweeps, b0_slot)
        slots = (t_slot, dm_slot, out_slot, scratch_slot)
        for name, s in zip(("t_slot", "dm_slot", "out_slot", "scratch_slot"), slots):
            if not 0 <= int(s) < len(self.vecs):
                raise ValueError("eikonal_tangent: %s = %d does not exist" % (name, s))
        if len(set(int(s) for s in slots)) != 4:
            raise ValueError("eikonal_tangent: t_slot, dm_slot, out_slot and scratch_slot must be four different slots, "
                             "got %r" % (slots,))
        if wrt not in WRT:
            raise ValueError("eikonal_tangent: wrt must be one of %r, got %r" % (WRT, wrt))
        idx, dist, ref = _source(init, self.shape, self.h, 0.0)
        if len(idx) < 1 or dist.shape != (len(idx),) or ref.shape != (self.ndim,):
            raise ValueError("eikonal_tangent: the init list is empty or ill-shaped (%d nodes, distances %r, reference %r)"
                             % (len(idx), dist.shape, ref.shape))
        n = np.array(self.shape)
        if np.any(idx < 0) or np.any(idx >= n) or np.any(ref < 0) or np.any(ref >= n):
            raise ValueError("eikonal_tangent: init_idx or ref_idx lies outside the grid")
        if len(np.unique(idx, axis=0)) != len(idx):
            raise ValueError("eikonal_tangent: init_idx names a node twice")
        if not np.all(np.isfinite(dist) & (dist >= 0.0)):
            raise ValueError("eikonal_tangent: init_dist must be finite and >= 0")
        if self.c is None:
            raise ValueError("eikonal_tangent: no model set")
        self.vecs[out_slot], self.last_eikonal_launches = tangent(self.vecs[t_slot], self.c, self.h, self.vecs[dm_slot],
                                                                  (idx, dist, ref), wrt, return_sweeps=True,
                                                                  max_sweeps=max_sweeps)

    def _tangent_stage(self, t_slot, dm_slot, out_slot, scratch_slot, init, wrt, max_sweeps, b0_slot):
        slots = dict(t_slot=t_slot, dm_slot=dm_slot, out_slot=out_slot, scratch_slot=scratch_slot)
        if b0_slot is not None:
            slots["b0_slot"] = b0_slot
        self._slots("eikonal_tangent", **slots)
        if wrt not in WRT:
            raise ValueError("eikonal_tangent: wrt must be one of %r, got %r" % (WRT, wrt))
        if init is not None:
            init = _source(init, self.shape, self.h, 0.0)
        if self.c is None:
            raise ValueError("eikonal_tangent: no model set")
        self.vecs[out_slot], self.last_eikonal_launches = tangent(
            self.vecs[t_slot], self.c, self.h, self.vecs[dm_slot], init, wrt, return_sweeps=True, max_sweeps=max_sweeps,
            b0=None if b0_slot is None else self.vecs[b0_slot])
