"""Per-cell comparison of a stepping kernel with the oracle (tests only; no test in this file).

A relative L2 norm over a few receivers cannot see an error confined to a few cells that carry little energy: a border
corner, a masked lane, a tile seam.  Here the WHOLE field is observed, at every cell and step, and every sample is judged
against its own round-off scale.

Dense observation goes through the ordinary entry points: ``forward(c, (src, w), rec=all cells)`` is the forward field;
``forward(c, (all cells, zeros), rec)`` followed by ``adjoint(r, image=False)`` returns ``P^T mu / h^D`` at every cell,
i.e. the adjoint field after a multiplication by ``h^D``; the gradient covers every cell anyway.

The majorant
------------
:class:`Majorant` is the oracle's recursion with every coefficient replaced by its absolute value and every subtraction
by an addition (``|a_k|``, ``|d_k|``, ``|B|``, the CPML's ``|a|``; ``D_d`` sums its two sides; the leapfrog is
``A (2 M + |B| M_prev + q)``; the adjoint CPML recursion has ``+`` throughout; ``|w|`` is injected).  Its fields ``M`` (forward),
``M_mu`` (adjoint), ``M_q`` (the stored term) and ``G = sum_n M_mu M_q / dt^2`` (the gradient; every S-th step with
weight S under ``image_stride``) bound the magnitude of every intermediate of the exact recursion, cell by cell.

Running-error bound: let one cell update consist of at most ``f`` rounded operations.  Its local error at step k is then
at most ``f u (1 + O(u))`` times the majorant of that update, ``M[k]``; the exact recursion carries it to step n with an
operator that the majorant recursion dominates entrywise, and the majorant recursion applied to ``M[k]`` gives at most
``M[n]`` (sources only add).  Summing the n local errors: any correctly rounded evaluation of the scheme, in any order of
summation, with or without fused multiply-adds, differs from the exact result by at most ``T u M[n, i]`` at cell i of
step n, with ``T = 1.01 n f`` (the 1.01 takes the higher-order terms).  The increment form ``v' = A (B v + q)``,
``u' = u + v'`` has a majorant below the standard form's, so the same ``M`` serves it.  One form is NOT under ``M`` as it
stands: the stream kernels take differences from the centre, ``sum_k a_k (u+ + u- - 2 u)``, whose intermediates reach
``sum_k |a_k| (M+ + M- + 2 M)`` where the majorant's star has ``|a_0| M + sum_k |a_k| (M+ + M-)``, and ``|a_0| < 2 sum |a_k|``
for alternating weights.  That is at most ``rho = 2 sum_k |a_k| / |a_0|`` times the majorant's star (1 for O(2), 1.134 for
O(4), 1.284 for O(8)), so the star's operations are counted ``rho`` times over, rounded up.

Rounded operations per cell update, ``f`` (r = order / 2, D = ndim; forming a coefficient counts like an operation on
the field, which bounds the depth of every path from above):

  star            r (2D + 1) + 1       per shell 2D - 1 additions, a multiplication, an addition; the centre's multiplication
                  + (r + 1)            the weights a_k / h^2;  S = ceil(rho (r (2D + 2) + 2)) in all
  source          2                    w / h^D, its addition
  C               4                    dt^2, c^2, their product, the multiplication by it
  sponge A, B     5D + 2               D profiles of 4 operations, D - 1 additions, 1 + d, the division, 1 - d
  leapfrog        4                    B u_prev, the subtraction, + q, the multiplication by A
  increment form  + 2                  v' = A (B v + q) and u + v' instead: one operation more, one spare
  CPML, per axis  15 r + 12            the adjoint recursion, the longer of the two: zt (2), alpha (1), pt (two first
                                       differences of 4r each, 3), beta (1), E alpha (3r + 1), D beta (4r), 2 additions,
                                       a and b (formed in fp64, rounded once each: 2); A = B = 1, the leapfrog is 2

  sponge:  f = S + 5D + 12     (O(8), 3-D: 71; O(8), 2-D: 56; O(2), 3-D: 37)
  CPML:    f = S + 8 + D (15 r + 12)      (O(8), 3-D: 268)

The factor a case is held to is the smaller of this rigorous ``T_rig`` and four times the largest ``err / (u M)`` the
ORACLE ITSELF reaches in the engine's precision on that very case (``Propagator(dtype=float32)`` against fp64) -- four,
because a kernel sums in another order, fuses multiply-adds and forms A, B, C and the star weights by its own fp32
expressions.  For the gradient the fp32 oracle accumulates its image in fp64 and so understates an engine's
accumulation error: ``T_grad = T_fwd + T_adj + nt``.  fp64 engines: ``u = 2^-53``, ``T = T_rig``.  No factor is ever
derived from an engine's output.

Coverage is a condition on the majorant alone: from step ceil(nt / 2) of each sweep on, ``M > 0`` and ``M_mu > 0`` at
every cell, and ``G > 0`` at every cell -- every cell of every case is then compared with a non-zero field.  Lattices of
sources and receivers with independent random series reach it; ``nt`` stays at 8 .. 12 because the majorant belongs to an
unstable operator and grows geometrically (median M / |u| near 1e3 after 12 steps, 1e15 after 40).
"""
import contextlib
import functools
import os
from collections import namedtuple

import numpy as np

from oracle import fwi_oracle as fo

U = {"float32": 2.0 ** -24, "float64": 2.0 ** -53}
TINY = {2.0 ** -24: float(np.finfo(np.float32).tiny), 2.0 ** -53: float(np.finfo(np.float64).tiny)}
MARGIN = 4.0      # over the fp32 oracle's own err / (u M)
GLOBAL_TOL = 1e-5  # the relative L2 bar of the norm-wise suites (tests/test_gpu_parity.py TOL32)


# ---------------------------------------------------------------------------------------------------------------------
# the majorant
# ---------------------------------------------------------------------------------------------------------------------
class Majorant(fo.Propagator):
    """The oracle with every coefficient its absolute value and every subtraction an addition, in fp64."""

    def __init__(self, *a, **k):
        k["dtype"] = np.float64
        super().__init__(*a, **k)
        self.coef = [abs(x) for x in self.coef]
        self.B = np.abs(self.B)
        if self.cpml:
            self.cpml = [(np.abs(a_), np.abs(b_)) for a_, b_ in self.cpml]
            self.dcoef = [abs(x) for x in self.dcoef]

    def _d1(self, u, ax):
        r, n = self.r, self.shape[ax]
        pad = [(0, 0)] * self.ndim
        pad[ax] = (r, r)
        p = np.pad(u, pad)
        out = np.zeros(self.shape)
        for k in range(1, r + 1):
            hi = [slice(None)] * self.ndim
            lo = [slice(None)] * self.ndim
            hi[ax] = slice(r + k, r + k + n)
            lo[ax] = slice(r - k, r - k + n)
            out = out + self.dcoef[k - 1] * (p[tuple(hi)] + p[tuple(lo)])
        return out

    def _cpml_term(self, u, aux, reverse):
        term = np.zeros(self.shape)
        for ax, (a, b) in enumerate(self.cpml):
            p_, z_ = aux[ax]
            if not reverse:
                p_ = b * p_ + a * self._d1(u, ax)
                z_ = b * z_ + a * (self._d2(u, ax) + self._d1(p_, ax))
                term = term + self._d1(p_, ax) + z_
            else:
                z_ = b * z_ + u
                al = a * z_
                p_ = b * p_ + self._d1(u, ax) + self._d1(al, ax)
                term = term + self._d2(al, ax) + self._d1(a * p_, ax)
            aux[ax] = (p_, z_)
        return term

    def sweep(self, inj_flat, amp, scale, reverse):
        """(M[n, cell], M_q[n, cell]) of a sweep that injects ``|amp[n]| * scale`` at ``inj_flat``."""
        nt = len(amp)
        up, uc = np.zeros(self.shape), np.zeros(self.shape)
        out, qs = np.zeros((nt,) + self.shape), np.zeros((nt,) + self.shape)
        aux = [(np.zeros(self.shape), np.zeros(self.shape)) for _ in range(self.ndim)] if self.cpml else None
        for n in (range(nt - 1, -1, -1) if reverse else range(nt)):
            s = np.zeros(self.shape)
            np.add.at(s.reshape(-1), inj_flat, np.abs(np.asarray(amp[n], np.float64)) * scale)
            extra = self._cpml_term(uc, aux, reverse) if self.cpml else 0.0
            q = self.C * (self.laplacian(uc) + extra + s)
            un = self.A * (2 * uc + self.B * up + q)
            out[n], qs[n] = un, q
            up, uc = uc, un
        return out.reshape(nt, -1), qs.reshape(nt, -1)


def flops(order, ndim, abc="sponge", form="standard"):
    """Rounded operations of one cell update (module docstring)."""
    r = order // 2
    rho = 2.0 * sum(abs(a) for a in fo.COEFFS[order][1:]) / abs(fo.COEFFS[order][0])
    f = int(np.ceil(rho * (r * (2 * ndim + 2) + 2) - 1e-9)) + 2 + 4
    if abc == "cpml":
        return f + 2 + ndim * (15 * r + 12)
    return f + 5 * ndim + 2 + 4 + (2 if form == "increment" else 0)


def t_rig(nt, order, ndim, abc="sponge", form="standard"):
    return 1.01 * nt * flops(order, ndim, abc, form)


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
# path: the row of the table in DESIGN.md; kw: Engine options; env: creation-time hooks; tile: the tile shape in use
# (z, y, x or z, x; 0 = not tiled along that axis), for the failure message; what: the quantities compared
Case = namedtuple("Case", "path shape order npml nt dtype abc alpha kw env tile kernel what ctx")
ALL = ("forward", "adjoint", "gradient")


def _case(path, shape, order, npml, kernel, nt=12, dtype="float32", abc="sponge", alpha=0.0, kw=None, env=None,
          tile=None, what=ALL, ctx=None):
    return Case(path, tuple(shape), order, npml, nt, dtype, abc, alpha, dict(kw or {}), dict(env or {}),
                tile, kernel, tuple(what), dict(ctx or {}))


def xpml_in_lanes(shape, order, npml, tile_x):
    """fwi_kernels.hip stream_xpml_supported for a 3-D fp32 grid: step3d_stream carries the x border in its lanes."""
    nx, r = shape[2], order // 2
    if r != 4 or npml < 4 or npml % 2 or nx % 4 or nx < 2 * (npml + r):
        return False
    nxt = -(-nx // tile_x)
    return tile_x >= npml + r and nx - (nxt - 1) * tile_x >= npml + r


def xpml_masked(shape, order, npml, tile_x):
    """... with one lane per side astride the border's inner edge, whose stores are masked (stream_xpml_partial)."""
    return xpml_in_lanes(shape, order, npml, tile_x) and npml % 4 == 2


def _tx(nx, full=256, vl=4):
    """Columns per x tile of the 3-D stream kernel: nx split into equal tiles, rounded up to the lane vector."""
    nxt = -(-nx // full)
    return -(-(-(-nx // nxt)) // vl) * vl


def _cases():
    out = []
    S3 = "step3d_stream"
    ty = [({}, 4), ({"FWI_STREAM_TY": "8"}, 8)]   # rows per workgroup: the tuned shape of these grids, and the HBM regime's
    for env, t in ty:
        for shape, order, npml in [((20, 17, 23), 8, 4), ((9, 8, 8), 8, 0), ((12, 40, 36), 2, 3), ((33, 29, 50), 4, 5)]:
            out.append(_case("stream3d sponge", shape, order, npml, S3, env=env, tile=(0, t, 256)))
        for shape in [(10, 9, 264), (12, 16, 256)]:  # two x tiles of 132 columns; one FULL 256-column tile
            out.append(_case("stream3d x tiles", shape, 8, 4, S3, env=env, tile=(0, t, _tx(shape[2]))))
        for shape in [(20, 17, 23), (12, 16, 256)]:
            out.append(_case("stream3d increment", shape, 8, 4, S3, kw={"update_form": "increment"}, env=env,
                             tile=(0, t, 256)))
    for zc in (5, 16):
        out.append(_case("stream3d z chunks", (30, 12, 24), 8, 4, S3, kw={"zchunk": zc}, tile=(zc, 4, 256)))
    for zc in (None, "7"):   # (the hooks of test_two_steps_per_pass_3d_matches_the_oracle)
        env = {"FWI_STREAM_PAIR": "1"}
        if zc:
            env["FWI_PAIR_ZCHUNK"] = zc
        out.append(_case("pair3d", (24, 20, 32), 8, 0, S3, env=env, tile=(int(zc or 0), 0, 256), what=("forward_nosave",),
                         ctx={"pair3d": 1}))
    for shape, order in [((20, 17, 23), 8), ((22, 9, 30), 2)]:
        out.append(_case("stream3d fp64", shape, order, 4, S3, dtype="float64", tile=(0, 4, _tx(shape[2], 128, 2))))
    for dtype in ("float32", "float64"):
        out.append(_case("point", (20, 17, 23), 8, 4, "step_point", dtype=dtype, kw={"kernel": "point"}))
        out.append(_case("point", (33, 47), 8, 6, "step_point", dtype=dtype, kw={"kernel": "point"}))
    # 3-D CPML: x border in the lanes (npml, nx multiples of 4); border even, not a multiple of 4 (masked stores);
    # y borders that overlap; two x tiles
    # (22, 20, 32) npml 6: the lane astride the border's inner edge; (22, 20, 30): nx off the lane vector, the x border
    # runs as slab phases around the step kernel.  ctx: what the context must report about its path (context_path)
    C3 = [((24, 20, 32), 8, 8, 30.0), ((22, 20, 32), 8, 6, 0.0), ((22, 20, 30), 8, 6, 0.0), ((22, 9, 30), 2, 5, 0.0),
          ((20, 18, 300), 8, 8, 0.0)]
    for shape, order, npml, alpha in C3:
        lanes = int(xpml_in_lanes(shape, order, npml, _tx(shape[2])))
        for form in ("standard", "increment"):
            for env, t in ty:
                out.append(_case("cpml3d " + form + (" lanes" if lanes else " slabs"), shape, order, npml, S3, abc="cpml",
                                 alpha=alpha, kw={"update_form": form}, env=env, tile=(0, t, _tx(shape[2])),
                                 ctx={"x-in-kernel": lanes, "line-axes": 3}))
    out.append(_case("cpml3d FWI_NO_PML_LINES", (24, 20, 32), 8, 8, S3, abc="cpml", alpha=30.0,
                     env={"FWI_NO_PML_LINES": "1"}, tile=(0, 4, 256), ctx={"x-in-kernel": 0, "line-axes": 0}))
    out.append(_case("cpml3d FWI_NO_STREAM_XPML", (24, 20, 32), 8, 8, S3, abc="cpml", alpha=30.0,
                     env={"FWI_NO_STREAM_XPML": "1"}, tile=(0, 4, 256), ctx={"x-in-kernel": 0, "line-axes": 3}))
    F2 = "step2d_fused"
    for shape in [(133, 260), (70, 52)]:
        for ft in (None, "32", "16"):
            for nt in (12, 10):   # three 4-step launches; two and a 2-step remainder through the tile kernel
                out.append(_case("fused2d sponge", shape, 8, 6, F2, nt=nt, env={"FWI_FUSED2D_TILE": ft} if ft else {},
                                 tile=(int(ft or 64),) * 2))
    for shape, order, npml in [((40, 131), 8, 5), ((70, 91), 2, 7)]:
        out.append(_case("tile2d sponge", shape, order, npml, "step2d_tile", env={"FWI_NO_FUSED2D": "1"}, tile=(8, 256)))
    for shape, npml, alpha in [((150, 216), 6, 0.0), ((149, 216), 6, 0.0), ((130, 250), 16, 30.0)]:
        for nt in (12, 10):
            out.append(_case("fused2d cpml", shape, 8, npml, F2, nt=nt, abc="cpml", alpha=alpha, tile=(64, 64)))
    for shape, npml, alpha in [((60, 216), 6, 0.0), ((70, 90), 8, 40.0)]:
        out.append(_case("tile2d cpml slabs", shape, 8, npml, "step2d_tile", abc="cpml", alpha=alpha, tile=(8, 256)))
    out.append(_case("store image_stride", (20, 17, 23), 8, 4, S3, kw={"image_stride": 3}, tile=(0, 4, 256),
                     what=("gradient",)))
    out.append(_case("store checkpoints", (20, 17, 23), 8, 4, S3, kw={"ckpt_interval": 5}, tile=(0, 4, 256),
                     what=("gradient",)))
    out.append(_case("store checkpoints", (70, 52), 8, 6, F2, kw={"ckpt_interval": 4}, tile=(64, 64), what=("gradient",)))
    return out


CASES = _cases()


def case_id(c):
    s = "%s-%s-O%d-npml%d-nt%d-%s" % (c.path.replace(" ", "_"), "x".join(map(str, c.shape)), c.order, c.npml, c.nt,
                                      c.dtype[-2:])
    for k, v in sorted(list(c.kw.items()) + list(c.env.items())):
        if k not in ("update_form", "kernel") and k not in c.path:
            s += "-%s=%s" % (k.replace("FWI_", "").lower(), v)
    return s


# ---------------------------------------------------------------------------------------------------------------------
# inputs and references (one per distinct problem, shared by every case and test that runs it)
# ---------------------------------------------------------------------------------------------------------------------
def dense(shape):
    return np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij"), -1).reshape(-1, len(shape))


def lattice(shape, order, nt):
    """Points from which a star of half-width r reaches every cell within H = (nt - 1) // 2 steps, so that the forward
    and the adjoint sweep overlap at every cell: a step moves r cells along ONE axis, the H hops are dealt out to the
    axes (the longest first), and an axis with k hops gets points at most 2 k r cells apart, the outermost on the faces."""
    r, H, nd = order // 2, (nt - 1) // 2, len(shape)
    hops = [H // nd] * nd
    for a in sorted(range(nd), key=lambda a: -shape[a])[:H % nd]:
        hops[a] += 1
    axes = []
    for n, k in zip(shape, hops):
        s = min(2 * k * r, r * nt // 2)
        cnt = -(-(n - 1) // s) + 1 if n > 1 else 1
        axes.append(np.unique(np.round(np.linspace(0, n - 1, cnt)).astype(np.int64)))
    return np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, nd)


def problem_key(c):
    return (c.shape, c.order, c.npml, c.nt, c.dtype, c.abc, c.alpha, int(c.kw.get("image_stride", 1)))


@functools.lru_cache(maxsize=None)
def problem(key):
    """Inputs of a case, every array rounded to the engine's type ONCE (the same rounded arrays go to the engine, the
    oracle and the majorant: input rounding is no part of the error)."""
    shape, order, npml, nt, dtype, abc, alpha, stride = key
    rng = np.random.default_rng([len(shape), order, npml, nt] + list(shape))
    nd = len(shape)
    c = (1500.0 + 1500.0 * rng.random(shape)).astype(dtype)
    h = 7.5
    dt = 0.7 * fo.cfl_dt(float(c.max()), h, nd, order)
    src = lattice(shape, order, nt)
    rec = src[::-1].copy()
    w = rng.standard_normal((nt, len(src))).astype(dtype)
    r = rng.standard_normal((nt, len(rec))).astype(dtype)
    okw = dict(order=order, npml=npml, sigma_max=fo.default_sigma_max(float(c.max()), h, npml), image_stride=stride)
    if abc == "cpml":
        okw.update(abc="cpml", pml_alpha_max=alpha)
    for a in (c, w, r):
        a.setflags(write=False)
    return dict(shape=shape, nd=nd, nt=nt, dtype=dtype, c=c, h=h, dt=dt, src=src, rec=rec, w=w, r=r, okw=okw,
                stride=stride, cells=dense(shape))


def oracle_fields(pb, dtype, cls=fo.Propagator, mutate=None, what=ALL):
    """Forward field (nt, N), adjoint field (nt, N) and slowness gradient (N,) of the oracle ``cls`` in ``dtype``, as
    fp64 arrays, through the same calls as :func:`engine_fields`.  ``mutate(p)`` may alter each propagator first."""
    out = {}

    def make():
        p = cls(pb["c"], pb["h"], pb["dt"], dtype=dtype, **pb["okw"])
        if mutate:
            mutate(p)
        return p
    if "forward" in what:
        out["forward"] = np.asarray(make().forward(pb["src"], pb["w"], pb["cells"], save=False), np.float64)
    if "adjoint" in what:
        p = make()
        # (what forward(all cells, zeros, rec) leaves behind, without injecting N zeros per step)
        p.src_flat, p.rec_flat, p.nt = fo._ravel_idx(pb["cells"], pb["shape"]), fo._ravel_idx(pb["rec"], pb["shape"]), pb["nt"]
        out["adjoint"] = np.asarray(p.adjoint(pb["r"], image=False), np.float64) * pb["h"] ** pb["nd"]
    if "gradient" in what:
        p = make()
        p.forward(pb["src"], pb["w"], pb["rec"], save=True)
        p.adjoint(pb["r"])
        out["gradient"] = np.asarray(p.gradient("slowness2"), np.float64).reshape(-1)
    return out


def majorant_fields(pb):
    m = Majorant(pb["c"], pb["h"], pb["dt"], **pb["okw"])
    M, Mq = m.sweep(fo._ravel_idx(pb["src"], pb["shape"]), pb["w"], 1.0 / pb["h"] ** pb["nd"], False)
    Mmu, _ = m.sweep(fo._ravel_idx(pb["rec"], pb["shape"]), pb["r"], 1.0, True)
    S = pb["stride"]
    G = S * (Mmu[::S] * Mq[::S]).sum(0) / pb["dt"] ** 2
    return {"forward": M, "adjoint": Mmu, "gradient": G}


def ratio(x, ref, M, u, T=0.0):
    """Largest (|x - ref| - floor) / (u M) over the samples with M > 0; with T = 0 there is no floor."""
    err = np.maximum(np.abs(np.asarray(x, np.float64) - ref) - T * TINY[u], 0.0)
    ok = M > 0
    return float(np.max(err[ok] / (u * M[ok]))) if ok.any() else 0.0


@functools.lru_cache(maxsize=6)   # (the cases of one problem follow each other; a problem holds up to 60 MB)
def reference(key):
    """fp64 oracle fields, majorant fields and, for fp32 problems, the fp32 oracle's fields and its own err / (u M) for
    the problem ``key``.  Shared by every test that asks for it: never modified."""
    pb = problem(key)
    order, abc, dtype = key[1], key[5], pb["dtype"]
    ref = oracle_fields(pb, np.float64)
    maj = majorant_fields(pb)
    u = U[dtype]
    o32 = own = None
    if dtype == "float32":
        o32 = oracle_fields(pb, np.float32)
        own = {k: ratio(o32[k], ref[k], maj[k], u) for k in ALL}
    return dict(pb=pb, ref=ref, maj=maj, u=u, o32=o32, own=own, order=order, abc=abc)


def factors(R, form="standard"):
    """{quantity: T} for a case on the reference ``R``: min(T_rig, 4 x the fp32 oracle's own ratio); fp64: T_rig."""
    pb = R["pb"]
    rig = t_rig(pb["nt"], R["order"], pb["nd"], R["abc"], form)
    T = {"forward": rig, "adjoint": rig, "gradient": 2 * rig + pb["nt"], "rig": rig}
    if R["own"] is not None:
        f, a = min(rig, MARGIN * R["own"]["forward"]), min(rig, MARGIN * R["own"]["adjoint"])
        T.update(forward=f, adjoint=a, gradient=f + a + pb["nt"])
    return T


def coverage(R):
    """The coverage condition, on the majorant alone (module docstring)."""
    maj, nt = R["maj"], R["pb"]["nt"]
    n0 = -(-nt // 2)
    assert (maj["forward"][n0:] > 0).all(), "forward majorant: cells the field has not reached by step %d" % n0
    assert (maj["adjoint"][:nt - n0] > 0).all(), "adjoint majorant: cells not reached %d steps into the sweep" % n0
    assert (maj["gradient"] > 0).all(), "gradient majorant: cells where the two sweeps never overlap"


# ---------------------------------------------------------------------------------------------------------------------
# the comparator
# ---------------------------------------------------------------------------------------------------------------------
def rel_l2(x, ref):
    return float(np.linalg.norm(np.asarray(x, np.float64) - ref) / np.linalg.norm(ref))


def check(x_gpu, x_ref64, M, u, T, what, shape=None, tile=None):
    """Assert, at every sample: ``|x_gpu - x_ref64| <= T u M + floor`` (floor = T x the smallest normal number: flushed
    denormals are legitimate); ``x_gpu == 0`` exactly where ``M == 0`` (the wave has not arrived: nothing may have been
    written); ``x_gpu`` finite.  Returns the largest err / (u M).  The failure names the worst sample: its step, cell,
    distance to each face and position in the tile, i.e. which structure of the kernel to read."""
    x = np.asarray(x_gpu, np.float64).reshape(M.shape)
    ref = np.asarray(x_ref64, np.float64).reshape(M.shape)

    def where(flat):
        n, cell = np.unravel_index(flat, M.shape) if M.ndim == 2 else (None, flat)
        s = "%s: " % what + ("step %d, " % n if n is not None else "") + "cell %d" % cell
        if shape is not None:
            idx = np.unravel_index(cell, shape)
            s += " = %s of %s, to the faces %s" % (tuple(int(i) for i in idx), tuple(shape),
                                                   [(int(i), int(m - 1 - i)) for i, m in zip(idx, shape)])
            if tile is not None:
                s += ", in the tile %s at %s" % (tuple(tile), tuple(int(i % t) if t else int(i) for i, t in zip(idx, tile)))
        return s, (n, cell)

    bad = ~np.isfinite(x)
    assert not bad.any(), "%d non-finite samples; first at %s" % (bad.sum(), where(int(np.argmax(bad)))[0])
    bad = (M == 0) & (x != 0)
    assert not bad.any(), "%d samples written where the field has not arrived; first at %s (value %g)" % (
        bad.sum(), where(int(np.argmax(bad)))[0], x.reshape(-1)[int(np.argmax(bad))])
    err = np.abs(x - ref)
    exc = err - (T * u * M + T * TINY[u])
    worst = ratio(x, ref, M, u, T)
    if (exc > 0).any():
        k = int(np.argmax(np.where(M > 0, (err - T * TINY[u]) / np.where(M > 0, u * M, 1.0), 0.0)))
        raise AssertionError("%d samples beyond T u M; worst at %s: got %.9g, oracle %.9g, M %.3g, err / (u M) = %.1f > "
                             "T = %.1f" % ((exc > 0).sum(), where(k)[0], x.reshape(-1)[k], ref.reshape(-1)[k],
                                           M.reshape(-1)[k], worst, T))
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# the engine's side
# ---------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def environment(env):
    """The creation-time hooks of a case, restored afterwards."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@contextlib.contextmanager
def context_report(lines):
    """Collect what a context created inside writes to the C library's stderr under FWI_DEBUG_PML (its own statement of
    the path it takes: "fwi: cpml=1 fused2d=0 pair3d=0 x-in-kernel=1 line-axes=3 (ty 4 zchunk 20)") into ``lines``."""
    import sys
    import tempfile
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            yield
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            tmp.seek(0)
            lines.extend(tmp.read().decode(errors="replace").splitlines())


def context_path(lines):
    """{"cpml": 1, "fused2d": 0, "pair3d": 0, "x-in-kernel": 1, "line-axes": 3, "ty": 4, "zchunk": 20} from the context's
    report."""
    import re
    for ln in lines:
        if ln.startswith("fwi: cpml="):
            return {k: int(v) for k, v in re.findall(r"([a-z0-9-]+)[= ](\d+)", ln[5:])}
    raise AssertionError("the context did not report its path: %r" % (lines,))


def engine_fields(case, pb):
    """The quantities ``case.what`` names from ONE engine context, as fp64 arrays, the kernel's name and the context's
    own report of its path; asserts what the case expects of both."""
    from full_waveform_inversion_amd import Engine
    out = {}
    N, nt = len(pb["cells"]), pb["nt"]
    kw = dict(order=case.order, npml=case.npml, sigma_max=pb["okw"]["sigma_max"], dtype=case.dtype)
    if case.abc == "cpml":
        kw.update(abc="cpml", pml_alpha_max=case.alpha)
    kw.update(case.kw)
    lines = []
    with contextlib.ExitStack() as stack:
        stack.enter_context(environment(dict(case.env, FWI_DEBUG_PML="1")))
        with context_report(lines):
            e = stack.enter_context(Engine(case.shape, pb["h"], pb["dt"], nt, **kw))
        e.set_model(pb["c"])
        out["kernel"] = e.kernel_name
        out["path"] = context_path(lines)
        assert out["kernel"] == case.kernel, (out["kernel"], case.kernel)
        for k, v in case.ctx.items():
            assert out["path"][k] == v, "%s: the context reports %s = %d, the case is meant for %d (%s)" % (
                case_id(case), k, out["path"][k], v, out["path"])
        assert out["path"]["pair3d"] == int(case.path == "pair3d"), out["path"]   # two steps per pass: there and only there
        assert out["path"]["fused2d"] == int(case.kernel == "step2d_fused"), out["path"]
        if "FWI_STREAM_TY" in case.env:
            assert out["path"]["ty"] == int(case.env["FWI_STREAM_TY"]), out["path"]
        if len(case.shape) == 3 and case.kernel == "step3d_stream":
            assert not case.kw.get("zchunk") or out["path"]["zchunk"] == case.kw["zchunk"], out["path"]
        if "forward" in case.what or "forward_nosave" in case.what:
            out["forward"] = np.asarray(e.forward(None, (pb["src"], pb["w"]), pb["cells"],
                                                  save="forward" in case.what), np.float64)
        if "adjoint" in case.what:
            e.forward(None, (pb["cells"], np.zeros((nt, N), case.dtype)), pb["rec"], save=False)
            out["adjoint"] = np.asarray(e.adjoint(pb["r"], image=False), np.float64) * pb["h"] ** pb["nd"]
        if "gradient" in case.what:
            e.reset_gradient()
            e.forward(None, (pb["src"], pb["w"]), pb["rec"], save=True)
            e.adjoint(pb["r"])
            out["gradient"] = np.asarray(e.gradient("slowness2"), np.float64).reshape(-1)
    return out


def judge(case, fields, R):
    """Every quantity of ``fields`` through :func:`check`; returns {quantity: (err / (u M), T)}."""
    T = factors(R, case.kw.get("update_form", "standard"))
    res = {}
    for what in ALL:
        if what in fields:
            res[what] = (check(fields[what], R["ref"][what], R["maj"][what], R["u"], T[what],
                               "%s, %s" % (case_id(case), what), case.shape, case.tile), T[what])
    return res
