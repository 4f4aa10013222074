"""L-BFGS (two-loop recursion, Armijo backtracking + Wolfe-curvature expansion, box projection) for the model update.

The reference has no optimiser (its "optimiser" is exhaustive random search,
full_waveform_inversion.py:713); BASELINE.json configs[4] asks for 5 L-BFGS
iterations on the all-reduced gradient, which is what this drives.
"""
from __future__ import annotations

import json
import os

import numpy as np


def save_state(path, it, x, f, g, S, Y, log, evals, history=None, bounds=None, precond=None, h0=None):
    """Optimiser state after iteration ``it`` (SURVEY.md s.5 "checkpoint / resume": "optimiser state save per L-BFGS
    iteration"): model, misfit, gradient, the curvature pairs oldest first, the log, and the settings a continuation
    must share (``history``, ``bounds``, the diagonal preconditioner ``precond``).  Written to a temporary file and renamed, so an interrupted run never leaves
    a torn file behind.  In a multi-rank job only ONE rank should pass a path (every rank holds the same state).
    ``h0``: the tag of the run's initial-inverse-Hessian operator (:func:`lbfgs`), recorded when there is one."""
    tmp = "%s.tmp.%d.npz" % (path, os.getpid())
    arrays = {"x": np.asarray(x), "g": np.asarray(g)}
    for i, (s, y) in enumerate(zip(S, Y)):
        arrays["s%d" % i] = np.asarray(s)
        arrays["y%d" % i] = np.asarray(y)
    if precond is not None:
        arrays["precond"] = np.asarray(precond)
    meta = {"history": None if history is None else int(history),
            "bounds": None if bounds is None else [float(bounds[0]), float(bounds[1])]}
    if h0 is not None:
        meta["h0"] = str(h0)
    np.savez(tmp, it=np.int64(it), f=np.float64(f), evals=np.int64(evals), npairs=np.int64(len(S)),
             log=np.frombuffer(json.dumps(log).encode(), np.uint8),
             meta=np.frombuffer(json.dumps(meta).encode(), np.uint8), **arrays)
    os.replace(tmp, path)


def load_state(path):
    """The dict :func:`save_state` wrote: ``it, f, evals, x, g, S, Y, log, precond`` (+ ``history``, ``bounds`` when
    the file holds them; ``precond`` is None when the run had none)."""
    with np.load(path) as z:
        n = int(z["npairs"])
        st = {"it": int(z["it"]), "f": float(z["f"]), "evals": int(z["evals"]), "x": z["x"].copy(), "g": z["g"].copy(),
              "S": [z["s%d" % i].copy() for i in range(n)], "Y": [z["y%d" % i].copy() for i in range(n)],
              "log": json.loads(bytes(z["log"]).decode()),
              "precond": z["precond"].copy() if "precond" in z.files else None}
        if "meta" in z.files:
            st.update(json.loads(bytes(z["meta"]).decode()))
        return st


def _checked_resume(resume, history, bounds, shape=None, precond=None, check_precond=True, h0=None):
    """Load and validate a state for continuation: the bit-for-bit promise holds only if the continuation runs with
    the settings of the run that wrote the file, so differing ``history`` / ``bounds`` (when the file records them)
    and arrays of the wrong shape are errors, not silent changes; more pairs than ``history`` are trimmed (oldest
    first), which is what the writing run would have done."""
    st = load_state(resume) if isinstance(resume, (str, os.PathLike)) else dict(resume)
    if st.get("history") is not None and int(st["history"]) != int(history):
        raise ValueError("resume: the state was written with history=%d, this run has history=%d"
                         % (st["history"], int(history)))
    if "bounds" in st:
        b = None if bounds is None else [float(bounds[0]), float(bounds[1])]
        if st["bounds"] != b:
            raise ValueError("resume: the state was written with bounds=%r, this run has bounds=%r" % (st["bounds"], b))
    if st.get("h0") != (None if h0 is None else str(h0)):
        raise ValueError("resume: the state was written with h0=%r, this run has h0=%r" % (st.get("h0"), h0))
    sp = st.get("precond")
    if check_precond:  # (precond: an array, or None for none)
        if (sp is None) != (precond is None) or (sp is not None and not np.array_equal(np.asarray(sp), np.asarray(precond))):
            raise ValueError("resume: the state was written with preconditioner %s, this run has %s"
                             % ("None" if sp is None else "p", "None" if precond is None else "another p"))
    elif sp is None:
        raise ValueError("resume: this run wants a preconditioner, the state was written without one")
    x = np.asarray(st["x"])
    if shape is not None and tuple(x.shape) != tuple(shape):
        raise ValueError("resume: the state holds a model of shape %r, the engine's grid is %r" % (x.shape, tuple(shape)))
    for name, a in [("g", st["g"])] + [("s%d" % i, s) for i, s in enumerate(st["S"])] + \
                   [("y%d" % i, y) for i, y in enumerate(st["Y"])] + ([("precond", sp)] if sp is not None else []):
        if np.asarray(a).shape != x.shape:
            raise ValueError("resume: %s has shape %r, the model %r" % (name, np.asarray(a).shape, x.shape))
    if len(st["S"]) != len(st["Y"]):
        raise ValueError("resume: %d s-vectors but %d y-vectors" % (len(st["S"]), len(st["Y"])))
    st["S"], st["Y"] = list(st["S"])[-int(history):], list(st["Y"])[-int(history):]
    return st


def _search_failed(log):
    return bool(log) and log[-1].get("note") == "line search failed"


def lbfgs(fg, x0, maxiter=5, history=5, first_step=None, bounds=None, dot=None, c1=1e-4, max_ls=8,
          gtol=0.0, callback=None, c2=0.9, checkpoint=None, resume=None, precond=None, h0=None):
    """Minimise ``f`` given ``fg(x) -> (f, g)``.

    Line search: backtracking (safeguarded quadratic interpolation) until the Armijo condition holds; while no backtracking was needed and the slope
    along the direction is still steeper than ``c2`` times the initial one (the weak Wolfe curvature condition
    fails: the step is too short, typical of the first, hand-scaled iteration) the step is doubled instead, as
    long as the misfit keeps decreasing.  ``c2=None`` switches the expansion off (plain Armijo).

    ``first_step``: largest change of any component in the first trial step (the gradient of
    an FWI misfit has no natural scale).  ``dot(a, b)``: inner product (pass ``Engine.dot``
    for the GPU wave-shuffle reduction).  Returns ``(x, f, log)``.

    ``checkpoint``: path of a state file rewritten after every completed iteration (:func:`save_state`); in a
    multi-rank job pass it on ONE rank only (every rank holds the same state).
    ``resume``: such a path (or the dict of :func:`load_state`): the run continues after the iteration it holds --
    ``x0`` is ignored and no misfit is re-evaluated -- and, ``fg`` being deterministic, reproduces the
    uninterrupted run bit for bit (``maxiter`` counts iterations of the whole run, not of this call).

    ``precond``: a fixed diagonal preconditioner p > 0 (an array shaped like ``x``, or a callable ``precond(x, f, g)``
    called once after the first evaluation, so that p can be built from that evaluation's illumination at no extra
    cost; see ``shots.illumination_preconditioner``).  The initial inverse Hessian of every iteration becomes
    ``gamma * diag(p)`` with ``gamma = s.y / (y.(p y))``; the first step (and a restart) is ``p g`` scaled so that
    ``first_step`` bounds the largest change.  p is part of the checkpoint; resuming with another p is an error.
    ``None`` leaves the iteration exactly as without this argument.

    ``h0``: a callable ``h0(q) -> B q`` applying a symmetric positive semi-definite operator B (one with a spatial
    extent, e.g. ``shots.smoothing_h0``).  Wherever the iteration multiplies by p it applies B instead: the initial
    inverse Hessian is ``gamma B`` with ``gamma = s.y / (y.(B y))``, the first step and a restart are ``B g`` scaled by
    ``first_step / max |B g|``.  With ``precond`` as well, p keeps its bookkeeping (built once, saved, checked on
    resume) and ``h0`` is responsible for using it.  A ``tag`` attribute of ``h0`` (a string naming the operator) is
    recorded in the state file; resuming with another tag is an error.  ``None`` leaves the iteration bit for bit as
    it is without this argument.
    """
    h0_tag = getattr(h0, "tag", None)
    dot = dot or (lambda a, b: float(np.sum(np.multiply(a, b, dtype=np.float64))))  # no BLAS threads
    if int(history) < 1:
        raise ValueError("history must be >= 1")
    lo, hi = bounds if bounds is not None else (None, None)

    def project(x):
        return np.clip(x, lo, hi) if bounds is not None else x

    pc = None if precond is None or callable(precond) else np.asarray(precond)
    if resume is not None:
        st = _checked_resume(resume, history, bounds, None if x0 is None else np.shape(x0), pc,
                             check_precond=not callable(precond), h0=h0_tag)
        if callable(precond):
            pc = np.asarray(st["precond"])
        x, f, g, S, Y = st["x"], st["f"], st["g"], list(st["S"]), list(st["Y"])
        log, evals, it0 = list(st["log"]), st["evals"], st["it"]
        if _search_failed(log):
            return x, f, log  # the run ended on a failed search: a continuation would only repeat it
    else:
        x = project(np.array(x0, copy=True))
        f, g = fg(x)
        _require_finite(f, float(np.abs(g).max()), dot(g, g), 0)
        S, Y, log = [], [], [{"iter": 0, "f": f, "evals": 1}]
        evals, it0 = 1, 0
        if callable(precond):
            pc = np.asarray(precond(x, f, g))
        if pc is not None and not (pc.shape == np.shape(g) and np.all(pc > 0) and np.all(np.isfinite(pc))):
            raise ValueError("precond must be finite, > 0 and shaped like the model")
        if checkpoint:
            save_state(checkpoint, 0, x, f, g, S, Y, log, evals, history, bounds, pc, h0_tag)
    for it in range(it0 + 1, maxiter + 1):
        if not float(np.abs(g).max()) > gtol:
            break  # stationary (or projected onto a bound everywhere)
        q = np.array(g, copy=True)
        al = []
        for s, y in zip(reversed(S), reversed(Y)):
            rho = 1.0 / dot(y, s)
            a = rho * dot(s, q)
            q -= a * y
            al.append((a, rho))
        if h0 is not None:  # initial inverse Hessian gamma B
            q = np.array(h0(q), copy=True)
            if S:
                q *= dot(S[-1], Y[-1]) / dot(Y[-1], h0(Y[-1]))
            else:
                q *= (first_step if first_step is not None else 1.0) / float(np.abs(q).max())
        elif pc is not None:  # initial inverse Hessian gamma diag(p)
            q *= pc
            if S:
                q *= dot(S[-1], Y[-1]) / dot(Y[-1], pc * Y[-1])
            else:
                q *= (first_step if first_step is not None else 1.0) / float(np.abs(q).max())
        elif S:
            q *= dot(S[-1], Y[-1]) / dot(Y[-1], Y[-1])
        else:
            gmax = float(np.abs(g).max())
            q *= (first_step if first_step is not None else 1.0) / gmax
        for (s, y), (a, rho) in zip(zip(S, Y), reversed(al)):
            b = rho * dot(y, q)
            q += s * (a - b)
        p = -q
        gp = dot(g, p)
        if not gp < 0.0:  # not a descent direction: restart from steepest descent
            S, Y = [], []
            p = -h0(g) if h0 is not None else -g if pc is None else -(pc * g)
            p = p * ((first_step if first_step is not None else 1.0) / float(np.abs(p).max()))
            gp = dot(g, p)
        t, best, shrunk = 1.0, None, False
        for _ in range(max_ls):
            xn = project(x + t * p)
            fn, gn = fg(xn)
            evals += 1
            if fn <= f + c1 * t * gp and (best is None or fn < best[1]):
                best = (t, fn, xn, gn)
                if shrunk or c2 is None or not dot(gn, p) < c2 * gp:
                    break  # Armijo holds and (after backtracking, or by the slope) the step is long enough
                t *= 2.0   # still descending steeply: the step is too short
            elif best is not None:
                break      # the doubled step overshot: keep the last good one
            else:
                t = _backtrack(t, f, gp, fn)
                shrunk = True
        if best is None:
            log.append({"iter": it, "f": f, "evals": evals, "note": "line search failed"})
            if checkpoint:  # the terminal entry too: a resumed run must not repeat the failed search
                save_state(checkpoint, it - 1, x, f, g, S, Y, log, evals, history, bounds, pc, h0_tag)
            break
        t, fn, xn, gn = best
        s, y = xn - x, gn - g
        if dot(s, y) > 1e-12 * np.sqrt(dot(s, s) * dot(y, y)):
            S.append(s)
            Y.append(y)
            if len(S) > history:
                S.pop(0)
                Y.pop(0)
        x, f, g = xn, fn, gn
        _require_finite(f, float(np.abs(g).max()), dot(g, g), it)
        log.append({"iter": it, "f": f, "evals": evals, "step": t})
        if checkpoint:
            save_state(checkpoint, it, x, f, g, S, Y, log, evals, history, bounds, pc, h0_tag)
        if callback:
            callback(it, x, f, g)
    return x, f, log


def _backtrack(t, f0, gp, ft):
    """Next trial step after ``t`` failed the Armijo test: the minimiser of the parabola through ``f(0) = f0``,
    ``f'(0) = gp`` and ``f(t) = ft``, kept inside ``[t / 10, t / 2]`` (a misfit evaluation is a full sweep over
    the shots, so a badly scaled first step should cost two or three of them, not one per halving)."""
    curv = ft - f0 - gp * t
    tq = -gp * t * t / (2.0 * curv) if np.isfinite(curv) and curv > 0.0 else 0.5 * t
    return min(max(tq, 0.1 * t), 0.5 * t)


def _require_finite(f, gmax, gg, it):
    """A blown-up propagation must not pass for convergence.  ``max |g|`` is NaN when any entry is (``np.abs(g).max()``
    on the host, ``fwi_vec_absmax`` on the device: the same semantics); the squared norm is checked as well, which also
    catches finite entries whose squares overflow."""
    if not (np.isfinite(f) and np.isfinite(gmax) and np.isfinite(gg)):
        raise FloatingPointError("L-BFGS iteration %d: non-finite misfit or gradient (f=%r, max|g|=%r, g.g=%r); "
                                 "check the time step against the CFL limit of the current model" % (it, f, gmax, gg))


def lbfgs_device_slots(history=5):
    """Vector slots :func:`lbfgs_device` uses for itself: a ``precond_slot`` must be this or higher."""
    return 7 + 2 * (int(history) + 1)


def lbfgs_device(engine, fg, x0, maxiter=5, history=5, first_step=None, bounds=None, c1=1e-4, max_ls=8,
                 gtol=0.0, callback=None, c2=0.9, checkpoint=None, resume=None, precond_slot=None, h0=None,
                 extra_slots=0):
    """The same iteration as :func:`lbfgs` with every model-sized vector resident on the GPU
    (``Engine.vec_*`` slots): per iteration only scalars cross PCIe.

    ``fg(x_slot, g_slot) -> f`` evaluates the misfit at the model in ``x_slot`` and leaves the
    gradient in ``g_slot`` (see ``shots.misfit_and_gradient_device``).  Returns ``(x, f, log)``
    with ``x`` downloaded once at the end.

    ``checkpoint`` / ``resume``: as in :func:`lbfgs` (the state file is the same: a run may be saved by one and
    resumed by the other); saving downloads the model, the gradient and the curvature pairs once per iteration
    (2 + 2 x history model-sized arrays over PCIe: ~0.1 s at 256^3 against ~7 s of shots per evaluation).

    ``precond_slot``: the vector slot (``>= lbfgs_device_slots(history)``; created here, zeroed) of the diagonal
    preconditioner p of :func:`lbfgs`.  ``fg`` fills it during the first evaluation
    (``shots.preconditioned_fg_device``); it stays fixed afterwards, is saved with the state and, on resume, is
    restored from it before any evaluation.

    ``h0``: the operator B of :func:`lbfgs` as a callable ``h0(slot)`` that applies it to a vector slot in place
    (``shots.smoothing_h0_device``); it takes the place of the multiplication by p in the same three spots, and with
    ``precond_slot`` as well the slot keeps its bookkeeping while ``h0`` is responsible for reading it.  An ``h0`` that
    needs vector slots of its own says how many in an ``nslots`` attribute: they are created behind the optimiser's
    (and the preconditioner's), and ``h0.setup(first_slot)`` is called once after ``vec_create`` -- on resume too --
    to fill them.  ``h0.tag`` is recorded and checked as in :func:`lbfgs`.

    ``extra_slots``: that many more slots, zeroed, are created behind all of these for ``fg``'s own use (the prior model
    of ``regularizers.regularized_fg_device``: ``regularizers.prior_slot`` says which).
    """
    m = int(history)
    if m < 1:
        raise ValueError("history must be >= 1")
    X, G, XN, GN, P, XB, GB = 0, 1, 2, 3, 4, 5, 6  # XB / GB: the best trial point of the line search so far
    # m + 1 pair slots: the candidate pair is formed in a spare slot, so the oldest pair is evicted only
    # once the candidate has passed the curvature test
    S0, Y0 = 7, 7 + (m + 1)
    nslots = lbfgs_device_slots(m)
    PC = precond_slot
    if PC is not None:
        if int(PC) < nslots:
            raise ValueError("precond_slot must be >= %d (the optimiser's own slots come first)" % nslots)
        PC = int(PC)
        nslots = PC + 1
    h0_tag = getattr(h0, "tag", None)
    engine.vec_create(nslots + int(getattr(h0, "nslots", 0)) + int(extra_slots))
    if hasattr(h0, "setup"):
        h0.setup(nslots)
    if h0 is not None:
        B = h0
    elif PC is not None:
        def B(slot):
            engine.vec_mul(slot, PC)
    else:
        B = None
    pairs = []  # ring of (s_slot, y_slot), oldest first
    free = list(range(m + 1))

    def save(it, f, log, evals):
        save_state(checkpoint, it, engine.vec_download(X), f, engine.vec_download(G),
                   [engine.vec_download(s) for s, _ in pairs], [engine.vec_download(y) for _, y in pairs], log, evals,
                   m, bounds, None if PC is None else engine.vec_download(PC), h0_tag)

    if resume is not None:
        st = _checked_resume(resume, m, bounds, getattr(engine, "shape", None), check_precond=PC is None, h0=h0_tag)
        if _search_failed(st["log"]):
            return np.asarray(st["x"]), st["f"], list(st["log"])
        if PC is not None:
            engine.vec_upload(PC, st["precond"])
        engine.vec_upload(X, st["x"])
        engine.vec_upload(G, st["g"])
        for s_h, y_h in list(zip(st["S"], st["Y"]))[-m:]:
            k = free.pop(0)
            engine.vec_upload(S0 + k, s_h)
            engine.vec_upload(Y0 + k, y_h)
            pairs.append((S0 + k, Y0 + k))
        f, log, evals, it0 = st["f"], list(st["log"]), st["evals"], st["it"]
    else:
        engine.vec_upload(X, x0)
        if bounds is not None:
            engine.vec_clip(X, *bounds)
        f = fg(X, G)
        _require_finite(f, engine.vec_absmax(G), engine.vec_dot(G, G), 0)
        if PC is not None and not engine.vec_absmax(PC) > 0.0:
            raise ValueError("precond_slot %d is empty after the first evaluation: fg must fill it "
                             "(shots.preconditioned_fg_device)" % PC)
        log = [{"iter": 0, "f": f, "evals": 1}]
        evals, it0 = 1, 0
        if checkpoint:
            save(0, f, log, evals)
    for it in range(it0 + 1, maxiter + 1):
        gmax = engine.vec_absmax(G)
        if not gmax > gtol:
            break
        engine.vec_copy(P, G)  # P holds q; the search direction is -P
        al = []
        for s, y in reversed(pairs):
            rho = 1.0 / engine.vec_dot(y, s)
            a = rho * engine.vec_dot(s, P)
            engine.vec_axpby(P, -a, y, 1.0)
            al.append((a, rho))
        if B is not None:  # initial inverse Hessian gamma diag(p) or gamma B; GN is free until the line search
            B(P)
            if pairs:
                s, y = pairs[-1]
                engine.vec_copy(GN, y)
                B(GN)
                engine.vec_axpby(P, 0.0, P, engine.vec_dot(s, y) / engine.vec_dot(y, GN))
            else:
                engine.vec_axpby(P, 0.0, P, (first_step if first_step is not None else 1.0) / engine.vec_absmax(P))
        elif pairs:
            s, y = pairs[-1]
            engine.vec_axpby(P, 0.0, P, engine.vec_dot(s, y) / engine.vec_dot(y, y))
        else:
            engine.vec_axpby(P, 0.0, P, (first_step if first_step is not None else 1.0) / gmax)
        for (s, y), (a, rho) in zip(pairs, reversed(al)):
            b = rho * engine.vec_dot(y, P)
            engine.vec_axpby(P, a - b, s, 1.0)
        gp = -engine.vec_dot(G, P)
        if not gp < 0.0:  # not a descent direction: restart from steepest descent
            free += [s - S0 for s, _ in pairs]
            pairs = []
            engine.vec_copy(P, G)
            if B is not None:
                B(P)
            engine.vec_axpby(P, 0.0, P, (first_step if first_step is not None else 1.0)
                             / (gmax if B is None else engine.vec_absmax(P)))
            gp = -engine.vec_dot(G, P)
        t, best, shrunk = 1.0, None, False
        for _ in range(max_ls):  # the same search as lbfgs(): Armijo backtracking, Wolfe-curvature expansion
            engine.vec_copy(XN, X)
            engine.vec_axpby(XN, -t, P, 1.0)
            if bounds is not None:
                engine.vec_clip(XN, *bounds)
            fn = fg(XN, GN)
            evals += 1
            if fn <= f + c1 * t * gp and (best is None or fn < best[1]):
                best = (t, fn)
                XB, XN = XN, XB
                GB, GN = GN, GB
                if shrunk or c2 is None or not -engine.vec_dot(GB, P) < c2 * gp:
                    break
                t *= 2.0
            elif best is not None:
                break
            else:
                t = _backtrack(t, f, gp, fn)
                shrunk = True
        if best is None:
            log.append({"iter": it, "f": f, "evals": evals, "note": "line search failed"})
            if checkpoint:
                save(it - 1, f, log, evals)
            break
        t, fn = best
        XN, XB = XB, XN
        GN, GB = GB, GN
        k = free.pop(0)  # never empty: at most m of the m + 1 slots hold history
        s, y = S0 + k, Y0 + k
        engine.vec_copy(s, XN)
        engine.vec_axpby(s, -1.0, X, 1.0)
        engine.vec_copy(y, GN)
        engine.vec_axpby(y, -1.0, G, 1.0)
        sy = engine.vec_dot(s, y)
        if sy > 1e-12 * np.sqrt(engine.vec_dot(s, s) * engine.vec_dot(y, y)):
            pairs.append((s, y))
            if len(pairs) > m:  # the new pair is good: now the oldest one goes
                s_old, _ = pairs.pop(0)
                free.append(s_old - S0)
        else:
            free.append(k)
        X, XN = XN, X
        G, GN = GN, G
        f = fn
        _require_finite(f, engine.vec_absmax(G), engine.vec_dot(G, G), it)
        log.append({"iter": it, "f": f, "evals": evals, "step": t})
        if checkpoint:
            save(it, f, log, evals)
        if callback:
            callback(it, X, f, G)
    return engine.vec_download(X), f, log
