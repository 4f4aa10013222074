"""Per-cell comparison of the Born sweeps and of the illumination with the oracle (tests only; no test in this file).
The harness of tests/_pointwise.py -- its problems, its majorant, its comparator -- carried over to ``J dc`` observed at
EVERY cell (``forward(save=True)`` with every cell a receiver, then ``born``) and to the illumination ``H``.

The Born majorant
-----------------
With q^n the stored forward term, the Born field obeys the forward recursion with the distributed source ``w q^n`` in
place of the point source (tests/_born.py).  Its majorant ``M_B[n, cell]`` is therefore the :class:`_pointwise.Majorant`
recursion with the source ``|w| M_q[n]``, ``M_q`` from ``Majorant.sweep`` of the forward problem, ``|w| = |2 dc / c|``
(``|c^2 dm|`` for ``wrt="slowness2"``); under ``image_stride = S`` the source acts on the steps ``n % S == 0`` with
weight S (tests/_born_imaging.py).  The CPML is the same ``_cpml_term`` with ``+`` throughout.  ``M_B[n]`` is recorded
as ``_born.born`` records ``du^{n+1}`` at step n.  ``|du_fp64| <= M_B`` at every sample (tests/test_pointwise_born_host.py).

The factor
----------
An engine's Born sweep errs in two ways.  (a) Its own rounding: per cell update the operations of a forward step and
three more -- forming ``w``, its product with ``q``, its addition -- so ``1.01 nt (f + 3)`` by the running-error
argument of _pointwise.py.  (b) The stored ``q`` it reads already differs from the exact one by up to ``T_rig u M_q``
(the forward bound applied to the stored term); that error enters through ``|w|`` as a source below ``T_rig u |w| M_q``
and is carried by an operator the majorant dominates: at most ``T_rig u M_B``.  Hence

    T_rig_born = t_rig(forward case) + 1.01 nt (flops + 3)

and a case is held to ``T_born = min(T_rig_born, MARGIN x own)``, ``own`` the largest err / (u M_B) of the fp32 ORACLE
(``Propagator(dtype=float32)`` + ``_born.born``, stored term and all) against fp64 on that very case.  fp64 engines:
``u = 2^-53``, ``T = T_rig_born``.  No factor is ever derived from an engine's output.

``dc = 30 m/s x standard normal`` is rounded to the engine's type once, ``dm = -2 dc / c^3`` likewise, and the rounded
arrays go to engine, oracle and majorant alike: input rounding is no part of the error.

Coverage: ``M_B[n0:] > 0`` at every cell, ``n0 = ceil(nt / 2)``, on the majorant alone.

The illumination
----------------
``H_m = (S / dt^4) sum_{n % S == 0} q^n(x)^2``.  With ``|q_gpu - q64| <= T_fwd u M_q`` the sum of squares differs by at
most ``T_fwd u E`` to first order, ``E = (S / dt^4) sum 2 |q64| M_q``; squaring, adding nt terms in the engine's type
and scaling add ``(nt + 3) u H_m``.  Bound per cell: ``|h - H_m| <= T_fwd u E + (nt + 3) u H_m``, ``T_fwd`` the forward
factor of ``_pointwise.factors``.  This catches a skipped or doubled step, a cell or row never accumulated, a wrong
weight S; it does NOT catch a 1e-3 error in one ``q`` (E adds magnitudes; the Born cases hold the stored ``q``).

The bf16 store is not held to the oracle per cell: a flipped bf16 rounding of one stored value is a 2^-8 effect at that
cell, against which ``T u M_B`` says nothing.  Its two paths read the SAME rounded store, so they are compared with each
other (``2 T_born u M_B``: each is within ``T_born u M_B`` of the exact sweep over that store); the store itself stays
with the norm-wise tests of tests/test_gpu_born_imaging.py.
"""
import contextlib
import functools
from collections import namedtuple

import numpy as np

import _born
import _born_imaging
import _pointwise as pw
from oracle import fwi_oracle as fo

WRTS = ("velocity", "slowness2")
BornCase = namedtuple("BornCase", "case modes operator")   # case: a _pointwise.Case (its ``what`` is not used)


def has_fused(c):
    """fwi_api.hip born_fused_supported: 3-D fp32 O(8) stream contexts without the CPML."""
    return (len(c.shape) == 3 and c.order == 8 and c.dtype == "float32" and c.kernel == "step3d_stream"
            and c.abc == "sponge")


def _bcase(path, shape, order, npml, kernel, operator="exact", **k):
    c = pw._case(path, shape, order, npml, kernel, what=(), **k)
    return BornCase(c, ("scatter", "fused") if has_fused(c) else ("scatter",), operator)


def _born_cases():
    out = []
    S3, F2, T2 = "step3d_stream", "step2d_fused", "step2d_tile"
    ty = [({}, 4), ({"FWI_STREAM_TY": "8"}, 8)]
    forms = [{}, {"update_form": "increment"}]
    for env, t in ty:
        for kw in forms:
            out.append(_bcase("born fused damped partial", (20, 17, 23), 8, 4, S3, kw=kw, env=env, tile=(0, t, 256)))
            out.append(_bcase("born fused damped full", (12, 16, 256), 8, 4, S3, kw=kw, env=env, tile=(0, t, 256)))
            out.append(_bcase("born fused undamped partial", (24, 20, 32), 8, 0, S3, kw=kw, env=env, tile=(0, t, 256)))
        out.append(_bcase("born fused two x tiles", (10, 9, 264), 8, 4, S3, env=env, tile=(0, t, pw._tx(264))))
    out.append(_bcase("born fused undamped full", (12, 16, 256), 8, 0, S3, tile=(0, 4, 256)))
    for zc in (5, 16):
        out.append(_bcase("born fused z chunks", (30, 12, 24), 8, 4, S3, kw={"zchunk": zc}, tile=(zc, 4, 256)))
    for shape, order, npml in [((12, 40, 36), 2, 3), ((33, 29, 50), 4, 5)]:
        out.append(_bcase("born stream other orders", shape, order, npml, S3, tile=(0, 4, 256)))
    for shape, npml, alpha in [((24, 20, 32), 8, 30.0), ((22, 20, 30), 6, 0.0)]:
        lanes = int(pw.xpml_in_lanes(shape, 8, npml, pw._tx(shape[2])))
        for form in ("standard", "increment"):
            out.append(_bcase("born cpml3d " + form + (" lanes" if lanes else " slabs"), shape, 8, npml, S3, abc="cpml",
                              alpha=alpha, kw={"update_form": form}, tile=(0, 4, pw._tx(shape[2])),
                              ctx={"x-in-kernel": lanes, "line-axes": 3}))
    for shape, npml, dtype in [((20, 17, 23), 4, "float32"), ((20, 17, 23), 4, "float64"), ((33, 47), 6, "float64")]:
        out.append(_bcase("born point", shape, 8, npml, "step_point", dtype=dtype, kw={"kernel": "point"}))
    out.append(_bcase("born stream fp64", (20, 17, 23), 8, 4, S3, dtype="float64", tile=(0, 4, pw._tx(23, 128, 2))))
    for shape, nt in [((70, 52), 12), ((70, 52), 10), ((133, 260), 12)]:
        out.append(_bcase("born fused2d sponge", shape, 8, 6, F2, nt=nt, tile=(64, 64)))
    out.append(_bcase("born tile2d sponge", (40, 131), 8, 5, T2, env={"FWI_NO_FUSED2D": "1"}, tile=(8, 256)))
    out.append(_bcase("born fused2d cpml", (150, 216), 8, 6, F2, abc="cpml", tile=(64, 64)))
    out.append(_bcase("born tile2d cpml slabs", (70, 90), 8, 8, T2, abc="cpml", alpha=40.0, tile=(8, 256)))
    out.append(_bcase("born store image_stride", (20, 17, 23), 8, 4, S3, operator="imaging", kw={"image_stride": 3},
                      tile=(0, 4, 256)))
    return out


BORN_CASES = _born_cases()


def born_case_id(b):
    c = b.case
    inc = c.kw.get("update_form") == "increment" and "increment" not in c.path
    return pw.case_id(c) + ("-increment" if inc else "")


# (shape, npml, ty): the contexts of test_bf16_store_paths_agree_at_every_cell
BF16_CASES = [_bcase("born bf16 store", shape, 8, npml, "step3d_stream", operator="imaging", kw={"store_dtype": "bf16"},
                     env=env, tile=(0, t, 256))
              for shape, npml in (((20, 17, 23), 4), ((24, 20, 32), 0))
              for env, t in (({}, 4), ({"FWI_STREAM_TY": "8"}, 8))]


def _icase(path, shape, order, npml, kernel, **k):
    return pw._case(path, shape, order, npml, kernel, what=(), **k)


def _illum_cases():
    S3, F2 = "step3d_stream", "step2d_fused"
    G = (20, 17, 23)
    return [
        _icase("illum stream3d", G, 8, 4, S3, tile=(0, 4, 256)),
        _icase("illum stream3d", G, 8, 4, S3, env={"FWI_STREAM_TY": "8"}, tile=(0, 8, 256)),
        _icase("illum stream3d full tile", (12, 16, 256), 8, 4, S3, tile=(0, 4, 256)),
        _icase("illum cpml3d", (24, 20, 32), 8, 8, S3, abc="cpml", alpha=30.0, tile=(0, 4, 256)),
        _icase("illum point", G, 8, 4, "step_point", kw={"kernel": "point"}),
        _icase("illum fused2d sponge", (70, 52), 8, 6, F2, nt=12, tile=(64, 64)),
        _icase("illum fused2d sponge", (70, 52), 8, 6, F2, nt=10, tile=(64, 64)),
        _icase("illum fused2d cpml", (150, 216), 8, 6, F2, abc="cpml", tile=(64, 64)),
        _icase("illum store image_stride", G, 8, 4, S3, kw={"image_stride": 3}, tile=(0, 4, 256)),
        _icase("illum store checkpoints", G, 8, 4, S3, kw={"ckpt_interval": 5}, tile=(0, 4, 256)),
        _icase("illum stream3d fp64", G, 8, 4, S3, dtype="float64", tile=(0, 4, pw._tx(23, 128, 2))),
    ]


ILLUM_CASES = _illum_cases()


# ---------------------------------------------------------------------------------------------------------------------
# inputs, majorant and references (one per distinct problem)
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def perturbation(key):
    """{"velocity": dc, "slowness2": dm} for the problem ``key``, each rounded to the engine's type once."""
    pb = pw.problem(key)
    shape, order, npml, nt = key[:4]
    rng = np.random.default_rng([0xB0, len(shape), order, npml, nt] + list(shape))
    dc = (30.0 * rng.standard_normal(shape)).astype(pb["dtype"])
    dm = (-2.0 * dc.astype(np.float64) / pb["c"].astype(np.float64) ** 3).astype(pb["dtype"])
    for a in (dc, dm):
        a.setflags(write=False)
    return {"velocity": dc, "slowness2": dm}


def majorant_q(pb):
    """``M_q[n, cell]`` of the forward problem, model-shaped per step."""
    m = pw.Majorant(pb["c"], pb["h"], pb["dt"], **pb["okw"])
    _, Mq = m.sweep(fo._ravel_idx(pb["src"], pb["shape"]), pb["w"], 1.0 / pb["h"] ** pb["nd"], False)
    return Mq


def born_majorant(pb, absw, Mq):
    """``M_B[n, cell]``: the majorant recursion with no point source and the distributed source ``|w| M_q[n]`` (every
    S-th step with weight S under ``image_stride``), recorded as ``_born.born`` records ``du^{n+1}`` at step n."""
    m = pw.Majorant(pb["c"], pb["h"], pb["dt"], **pb["okw"])
    nt, S = pb["nt"], pb["stride"]
    absw = np.abs(np.asarray(absw, np.float64)).reshape(m.shape)
    up, uc = np.zeros(m.shape), np.zeros(m.shape)
    out = np.zeros((nt,) + m.shape)
    aux = [(np.zeros(m.shape), np.zeros(m.shape)) for _ in range(m.ndim)] if m.cpml else None
    for n in range(nt):
        extra = m._cpml_term(uc, aux, False) if m.cpml else 0.0
        q = m.C * (m.laplacian(uc) + extra)
        if n % S == 0:
            q = q + S * absw * Mq[n].reshape(m.shape)
        un = m.A * (2 * uc + m.B * up + q)
        out[n] = un
        up, uc = uc, un
    return out.reshape(nt, -1)


def oracle_born(pb, dtype, pert, mutate=None, mutate_store=None, wrts=WRTS):
    """{wrt: J d(wrt) at every cell, (nt, N), fp64 array} of the oracle in ``dtype`` and the propagator that holds the
    store.  ``mutate(p)`` may alter the propagator before the forward, ``mutate_store(p)`` its store after it."""
    p = fo.Propagator(pb["c"], pb["h"], pb["dt"], dtype=dtype, **pb["okw"])
    if mutate:
        mutate(p)
    p.forward(pb["src"], pb["w"], pb["cells"], save=True)
    if mutate_store:
        mutate_store(p)
    f = _born_imaging.born_imaging if pb["stride"] > 1 else _born.born
    return {wrt: np.asarray(f(p, pert[wrt], wrt), np.float64) for wrt in wrts}, p


def abs_weight(pb, pert, wrt):
    c = pb["c"].astype(np.float64)
    v = pert[wrt].astype(np.float64)
    return np.abs(2.0 * v / c) if wrt == "velocity" else np.abs(c ** 2 * v)


def t_rig_born(nt, order, ndim, abc="sponge", form="standard"):
    return pw.t_rig(nt, order, ndim, abc, form) + 1.01 * nt * (pw.flops(order, ndim, abc, form) + 3)


@functools.lru_cache(maxsize=4)
def born_reference(key):
    """fp64 Born fields at every cell, their majorants, and for fp32 problems the fp32 oracle's fields and its own
    err / (u M_B), per parametrisation, for the problem ``key``; also the fp64 store and ``M_q`` (the illumination's
    reference and scale).  Shared by every test that asks for it: never modified."""
    pb = pw.problem(key)
    pert = perturbation(key)
    u = pw.U[pb["dtype"]]
    Mq = majorant_q(pb)
    ref, p64 = oracle_born(pb, np.float64, pert)
    maj = {wrt: born_majorant(pb, abs_weight(pb, pert, wrt), Mq) for wrt in WRTS}
    o32 = own = None
    if pb["dtype"] == "float32":
        o32, _ = oracle_born(pb, np.float32, pert)
        own = {wrt: pw.ratio(o32[wrt], ref[wrt], maj[wrt], u) for wrt in WRTS}
    q64 = np.asarray(p64.q_store, np.float64).reshape(pb["nt"], -1)
    return dict(pb=pb, pert=pert, ref=ref, maj=maj, u=u, o32=o32, own=own, order=key[1], abc=key[5], Mq=Mq, q64=q64)


def born_factors(R, form="standard"):
    """{wrt: T_born, "rig": T_rig_born}: min(T_rig_born, 4 x the fp32 oracle's own ratio); fp64: T_rig_born."""
    pb = R["pb"]
    rig = t_rig_born(pb["nt"], R["order"], pb["nd"], R["abc"], form)
    T = {wrt: rig for wrt in WRTS}
    T["rig"] = rig
    if R["own"] is not None:
        T.update({wrt: min(rig, pw.MARGIN * R["own"][wrt]) for wrt in WRTS})
    return T


def born_coverage(R):
    n0 = -(-R["pb"]["nt"] // 2)
    for wrt in WRTS:
        assert (R["maj"][wrt][n0:] > 0).all(), "Born majorant (%s): cells the scattered field has not reached by step %d" % (
            wrt, n0)


# ---------------------------------------------------------------------------------------------------------------------
# the illumination's reference
# ---------------------------------------------------------------------------------------------------------------------
def illumination_reference(R):
    """(H_m, E) per cell from the fp64 oracle's store and ``M_q``: ``H_m = (S / dt^4) sum q64^2`` and its scale
    ``E = (S / dt^4) sum 2 |q64| M_q``, both over the imaged steps."""
    pb = R["pb"]
    S, k = pb["stride"], pb["stride"] / pb["dt"] ** 4
    q = R["q64"][::S]
    return k * np.sum(q * q, axis=0), k * np.sum(2.0 * np.abs(q) * R["Mq"][::S], axis=0)


def illumination_bound(R, T_fwd, Hm, E):
    return T_fwd * R["u"] * E + (R["pb"]["nt"] + 3) * R["u"] * Hm


def check_illumination(h, R, T_fwd, what, shape=None):
    """Assert at every cell ``|h - H_m| <= T_fwd u E + (nt + 3) u H_m``, ``h == 0`` where ``E == 0`` and ``h`` finite;
    returns the largest err / bound and the largest err / (u E)."""
    Hm, E = illumination_reference(R)
    h = np.asarray(h, np.float64).reshape(-1)
    assert np.isfinite(h).all(), "%s: %d non-finite cells" % (what, (~np.isfinite(h)).sum())
    bad = (E == 0) & (h != 0)
    assert not bad.any(), "%s: %d cells accumulated where the field never arrived" % (what, bad.sum())
    bound = illumination_bound(R, T_fwd, Hm, E)
    err = np.abs(h - Hm)
    ok = bound > 0
    share = float(np.max(err[ok] / bound[ok])) if ok.any() else 0.0
    if (err > bound).any():
        k = int(np.argmax(np.where(ok, err / np.where(ok, bound, 1.0), 0.0)))
        at = tuple(int(i) for i in np.unravel_index(k, shape)) if shape is not None else k
        raise AssertionError("%s: %d cells beyond the illumination bound; worst at cell %s of %s: got %.9g, oracle %.9g, "
                             "err / bound = %.2f (err / (u E) = %.2f, T_fwd = %.1f)" % (
                                 what, (err > bound).sum(), at, shape, h[k], Hm[k], err[k] / bound[k],
                                 err[k] / (R["u"] * E[k]), T_fwd))
    pos = E > 0
    return share, (float(np.max(err[pos] / (R["u"] * E[pos]))) if pos.any() else 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# the engine's side
# ---------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def open_context(case, pb, **extra):
    """An engine context for ``case`` created under the case's hooks and FWI_DEBUG_PML=1, with the model set; asserts
    the kernel's name and the context's own report of its path exactly as ``_pointwise.engine_fields`` does.  Yields
    (engine, reported path)."""
    from full_waveform_inversion_amd import Engine
    kw = dict(order=case.order, npml=case.npml, sigma_max=pb["okw"]["sigma_max"], dtype=case.dtype)
    if case.abc == "cpml":
        kw.update(abc="cpml", pml_alpha_max=case.alpha)
    kw.update(case.kw)
    kw.update(extra)
    lines = []
    with contextlib.ExitStack() as stack:
        stack.enter_context(pw.environment(dict(case.env, FWI_DEBUG_PML="1")))
        with pw.context_report(lines):
            e = stack.enter_context(Engine(case.shape, pb["h"], pb["dt"], pb["nt"], **kw))
        e.set_model(pb["c"])
        path = pw.context_path(lines)
        assert e.kernel_name == case.kernel, (e.kernel_name, case.kernel)
        assert path["cpml"] == int(case.abc == "cpml"), path
        for k, v in case.ctx.items():
            assert path[k] == v, "%s: the context reports %s = %d, the case is meant for %d (%s)" % (
                pw.case_id(case), k, path[k], v, path)
        assert path["pair3d"] == 0, path
        assert path["fused2d"] == int(case.kernel == "step2d_fused"), path
        if "FWI_STREAM_TY" in case.env:
            assert path["ty"] == int(case.env["FWI_STREAM_TY"]), path
        elif len(case.shape) == 3 and case.kernel == "step3d_stream" and case.tile:
            assert path["ty"] == case.tile[1], path
        if len(case.shape) == 3 and case.kernel == "step3d_stream":
            assert not case.kw.get("zchunk") or path["zchunk"] == case.kw["zchunk"], path
        yield e, path


def engine_born(b, R):
    """{(wrt, mode): J d(wrt) at every cell as an fp64 (nt, N) array} from ONE context (closed on return), and the
    context's report of its path.  Asserts ``born_path`` after every sweep, clean padding after every sweep, and that
    "fused" is refused with code 1 where the context has no fused path."""
    from full_waveform_inversion_amd import FwiError
    case, pb = b.case, R["pb"]
    out = {}
    with open_context(case, pb) as (e, path):
        e.forward(None, (pb["src"], pb["w"]), pb["cells"], save=True)
        assert e.dirty_padding() == 0
        for mode in b.modes:
            for wrt in WRTS:
                d = e.born(R["pert"][wrt], wrt, mode=mode, operator=b.operator)
                assert e.born_path == mode, (e.born_path, mode)
                assert e.dirty_padding() == 0, (wrt, mode)
                out[wrt, mode] = np.asarray(d, np.float64)
        if not has_fused(case):
            try:
                e.born(R["pert"]["velocity"], mode="fused", operator=b.operator)
            except FwiError as err:
                assert err.code == 1, err
            else:
                raise AssertionError("%s: mode='fused' was not refused" % pw.case_id(case))
    return out, path


def judge_born(b, fields, R):
    """Every Born field of ``fields`` through ``_pointwise.check``; returns {(wrt, mode): (err / (u M_B), T)}."""
    case = b.case
    T = born_factors(R, case.kw.get("update_form", "standard"))
    res = {}
    for (wrt, mode), x in fields.items():
        res[wrt, mode] = (pw.check(x, R["ref"][wrt], R["maj"][wrt], R["u"], T[wrt],
                                   "%s, born %s %s" % (pw.case_id(case), wrt, mode), case.shape, case.tile), T[wrt])
    return res


def engine_bf16_paths(b, R):
    """{mode: J_img dc at every cell} of the two paths of ONE bf16-store context after one forward."""
    case, pb = b.case, R["pb"]
    out = {}
    with open_context(case, pb) as (e, path):
        e.forward(None, (pb["src"], pb["w"]), pb["cells"], save=True)
        for mode in ("scatter", "fused"):
            d = e.born(R["pert"]["velocity"], mode=mode, operator="imaging")
            assert e.born_path == mode and e.dirty_padding() == 0, (e.born_path, mode)
            out[mode] = np.asarray(d, np.float64)
    return out, path


def engine_illumination(case, R):
    """(h_m, h_c, h_c through illumination_vec) of ONE ``illumination=True`` context, through the calls of
    tests/test_gpu_illumination.py: forward(save=True), adjoint(r), illumination."""
    pb = R["pb"]
    with open_context(case, pb, illumination=True) as (e, path):
        e.forward(None, (pb["src"], pb["w"]), pb["rec"], save=True)
        e.adjoint(pb["r"])
        hm, hc = e.illumination("slowness2"), e.illumination("velocity")
        e.vec_create(1)
        e.illumination_vec(0, "velocity")
        hv = e.vec_download(0)
        assert e.dirty_padding() == 0
    return hm, hc, hv, path


def check_conversion(hm, hc, pb, u, what):
    """``illumination("velocity") = illumination("slowness2") x (2 / c^3)^2`` at every cell, evaluated from the rounded
    c: relative error <= 8 u (c^2, c^3, the division, its square, the product: five rounded operations, one spare for the
    division form, one for the final rounding).  fp32 engines: the product in fp64.  An fp64 evaluation errs as much as
    an fp64 engine's kernel does, so there the product and the relative error are formed exactly, in rationals.  Returns
    the largest relative error in u."""
    c = pb["c"].astype(np.float64).reshape(-1)
    hm = np.asarray(hm, np.float64).reshape(-1)
    got = np.asarray(hc, np.float64).reshape(-1)
    assert np.isfinite(got).all(), what
    assert (got[hm == 0] == 0).all(), what
    ok = np.flatnonzero(hm != 0)
    if u == pw.U["float64"]:
        from fractions import Fraction
        rel = np.zeros(len(ok))
        for j, i in enumerate(ok):
            want = Fraction(float(hm[i])) * 4 / Fraction(float(c[i])) ** 6
            rel[j] = float(abs(Fraction(float(got[i])) - want) / want / Fraction(u))
    else:
        want = hm[ok] * (2.0 / c[ok] ** 3) ** 2
        rel = np.abs(got[ok] - want) / np.abs(want) / u
    worst = float(rel.max()) if len(ok) else 0.0
    assert worst <= 8.0, "%s: velocity illumination %.2f u from slowness2 x (2 / c^3)^2 at cell %d" % (
        what, worst, int(ok[int(np.argmax(rel))]))
    return worst
