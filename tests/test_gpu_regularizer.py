"""First-order Tikhonov and total-variation regularisation on the GPU (include/fwi.h fwi_vec_regularizer, DESIGN.md
s.4g) against the fp64 NumPy restatement of tests/_regularizer.py, cell by cell, and the L-BFGS drivers with the term.

Per-cell bound, derived: every operation before the last is fp64, and about 21 roundings touch a term (the
difference, the square, the sum, the square root, the divide, the six-flux sum, alpha and beta), so
|err_j| <= u_T |ref_j| + 64 * 2^-53 * M_j with M_j the sum of the magnitudes of the terms of cell j
(_regularizer.majorant) and u_T = 2^-24 / 2^-53 the one rounding to the context's format.  Value:
|R - R_ref| <= (N + 16) 2^-53 R_ref, the worst case of any fixed summation order of N non-negative terms.

The kernel's tiles are 16 rows x 64 (fp32) / 32 (fp64) columns, marched over chunks of 16 planes; a 2-D grid is one
plane.  (72, 70, 300) and (300, 2100) span more than two of each and are a multiple of none."""
import ctypes as C
import itertools

import numpy as np
import pytest

import _regularizer as tr
from full_waveform_inversion_amd import Engine, FwiError, _lib, regularizers as rg, shots as sh, workloads
from full_waveform_inversion_amd.lbfgs import lbfgs, lbfgs_device

pytestmark = pytest.mark.gpu

U = {"float32": 2.0 ** -24, "float64": 2.0 ** -53}
U64 = 2.0 ** -53
S2A, S2B, S3A, S3B, S3C = (37, 23), (300, 2100), (19, 21, 23), (72, 70, 300), (9, 6, 1)
LARGE = (S2B, S3B)  # the library twin is the reference there (tests/test_regularizer_host.py pins it to the restatement)
EPS = 0.3
X, X0, V, OUT, OUT2 = 0, 1, 2, 3, 4
WEIGHTS = {2: [1.0, (0.5, 2.0), (0.0, 1.5), (1.25, 0.0)], 3: [1.0, (0.5, 2.0, 1.0), (1.5, 0.0, 0.75), (0.0, 1.0, 0.0)]}
# kind, with x0, with v, beta: all sixteen, the weights taken in turn
CONFIGS = [dict(kind=k, x0=p, v=v, beta=b, alpha=(1.0, -0.75)[i % 2], wsel=i % 4)
           for i, (k, p, v, b) in enumerate(itertools.product(("tikhonov", "tv"), (False, True), (False, True), (0.0, 1.0)))]
_inputs, _refs = {}, {}


def fields(shape):
    """x, x0, v, out_old of a shape: fp32-representable, so that both contexts work on the same numbers; velocities
    near 2000 with contrasts near 1, the case fp32 arithmetic would lose four digits on."""
    if shape not in _inputs:
        rng = np.random.default_rng(sum(shape))
        f = [(2000.0 + rng.standard_normal(shape)).astype(np.float32),
             (2000.0 + 0.5 * rng.standard_normal(shape)).astype(np.float32),
             rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)]
        for a in f:
            a.setflags(write=False)
        _inputs[shape] = f
    return _inputs[shape]


def weight_of(shape, cfg):
    return WEIGHTS[len(shape)][cfg["wsel"]]


def reference(shape, i):
    """(L ref, majorant without the beta term, R ref) of config i."""
    if (shape, i) not in _refs:
        cfg = CONFIGS[i]
        x, x0, v, _ = fields(shape)
        a = dict(kind=cfg["kind"], weight=weight_of(shape, cfg), eps=EPS if cfg["kind"] == "tv" else None,
                 x0=x0 if cfg["x0"] else None)
        vv = v if cfg["v"] else None
        if shape in LARGE:
            L, R = rg.apply(x, vv, **a), rg.value(x, **a)
            k = 1.0 if cfg["kind"] == "tikhonov" else None
            M = _majorant_by_slices(x, vv, k=k, **a)
        else:
            L, R, M = tr.apply(x, vv, **a), tr.value(x, **a), tr.majorant(x, vv, **a)
        _refs[(shape, i)] = (L, M, R)
    return _refs[(shape, i)]


def _majorant_by_slices(x, v, kind, weight, eps, x0, k=None):
    """tr.majorant without the dense matrices (the large shapes)."""
    d = tr.difference(x, x0)
    w = tr.weights(weight, d.ndim)
    v = d if v is None else np.asarray(v, np.float64)
    if k is None:
        k = 1.0 / np.sqrt(rg._s(d, w) + eps * eps)
    M = np.zeros(d.shape)
    for ax, wa in enumerate(w):
        f = k * np.abs(rg._diff(v, ax))
        M += wa * f
        hi = [slice(None)] * d.ndim
        lo = list(hi)
        hi[ax], lo[ax] = slice(1, None), slice(0, -1)
        M[tuple(hi)] += wa * f[tuple(lo)]
    return M


def engine(shape, dtype="float32"):
    return Engine(shape, 10.0, 1e-3, 4, dtype=dtype)


def loaded(shape, dtype):
    e = engine(shape, dtype)
    e.vec_create(5)
    x, x0, v, _ = fields(shape)
    e.vec_upload(X, x)
    e.vec_upload(X0, x0)
    e.vec_upload(V, v)
    return e


def call(e, shape, cfg, out=OUT):
    return e.vec_regularizer(X, out=out, kind=cfg["kind"], x0=X0 if cfg["x0"] else None, v=V if cfg["v"] else None,
                             alpha=cfg["alpha"], beta=cfg["beta"], weight=weight_of(shape, cfg),
                             eps=EPS if cfg["kind"] == "tv" else None)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", [S2A, S3A, S3C, S2B, S3B], ids=str)
def test_every_cell_and_the_value_match_the_restatement(gpu, shape, dtype):
    old = fields(shape)[3]
    worst = 0.0
    with loaded(shape, dtype) as e:
        for i, cfg in enumerate(CONFIGS):
            L, M, R = reference(shape, i)
            # beta = 0: the old contents must not be read -- NaN would spread
            e.vec_upload(OUT, old if cfg["beta"] else np.full(shape, np.nan, np.float32))
            val = call(e, shape, cfg)
            got = e.vec_download(OUT).astype(np.float64)
            ref = cfg["alpha"] * L + (cfg["beta"] * old.astype(np.float64) if cfg["beta"] else 0.0)
            bound = U[dtype] * np.abs(ref) + 64 * U64 * (abs(cfg["alpha"]) * M + abs(cfg["beta"]) * np.abs(old))
            err = np.abs(got - ref)
            assert got.shape == ref.shape and np.isfinite(got).all(), cfg
            ratio = float((err / np.maximum(bound, 1e-300)).max())
            worst = max(worst, ratio)
            print("%s: max |err| = %.3e (bound there %.3e, err / bound <= %.3f); R = %.17g, ref %.17g, bound %.3e"
                  % (cfg, err.max(), bound.flat[err.argmax()], ratio, val, R, (L.size + 16) * U64 * R))
            assert (err <= bound).all(), (cfg, err.max(), ratio)
            assert abs(val - R) <= (L.size + 16) * U64 * R, (cfg, val, R)
    print("largest err / bound:", worst)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", [S2A, S3A, S3B], ids=str)  # (S3B: 125 / 250 blocks in the reduction)
def test_a_repeat_on_a_fresh_copy_gives_the_same_bits(gpu, shape, dtype):
    with loaded(shape, dtype) as e:
        for cfg in (CONFIGS[4], CONFIGS[14], CONFIGS[8]):  # Tikhonov with x0; TV with x0 and v; TV alone
            cfg = dict(cfg, beta=0.0)
            a = call(e, shape, cfg, OUT)
            b = call(e, shape, cfg, OUT2)
            assert a == b and a > 0.0
            o1, o2 = e.vec_download(OUT), e.vec_download(OUT2)
            assert np.array_equal(o1, o2) and o1.any()
            c = e.vec_regularizer(X, out=None, kind=cfg["kind"], x0=X0 if cfg["x0"] else None,
                                  weight=weight_of(shape, cfg), eps=EPS if cfg["kind"] == "tv" else None)
            assert c == a  # the value alone, no out
            assert np.array_equal(e.vec_download(OUT), o1)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", [S2A, S3A, S3C], ids=str)
def test_pad_columns_are_written_as_zeros(gpu, shape, dtype):
    """nx % 4 != 0: the compact rows carry pad columns, which vec_dot sums over and vec_download leaves out.  The
    inputs sit near 2000: a pad cell that took a value, or was read as a neighbour, would weigh in."""
    with loaded(shape, dtype) as e:
        for cfg in (CONFIGS[5], CONFIGS[15], CONFIGS[8]):
            e.vec_upload(OUT, fields(shape)[3])
            call(e, shape, cfg)
            dd = e.vec_dot(OUT, OUT)
            y = e.vec_download(OUT).astype(np.float64)
            ss = float(np.sum(y * y))
            assert ss > 0.0 and abs(dd - ss) <= 1e-13 * ss, (cfg, dd, ss)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", [S2A, S3A, S3B], ids=str)
def test_beta_zero_never_reads_out(gpu, shape, dtype):
    with loaded(shape, dtype) as e:
        for kind in ("tikhonov", "tv"):
            e.vec_upload(OUT, np.full(shape, np.nan, np.float32))
            e.vec_regularizer(X, out=OUT, kind=kind, x0=X0, v=V, alpha=2.0, beta=0.0, weight=1.0, eps=EPS)
            assert np.isfinite(e.vec_download(OUT)).all()
            assert np.isfinite(e.vec_dot(OUT, OUT))  # the pad columns too


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", [S2A, S3A, S3C, S3B], ids=str)
def test_constants_give_zero_exactly(gpu, shape, dtype):
    with engine(shape, dtype) as e:
        e.vec_create(3)
        e.vec_upload(0, np.full(shape, 1234.5, np.float32))
        e.vec_upload(1, np.full(shape, 234.25, np.float32))
        for kind in ("tikhonov", "tv"):
            for x0 in (None, 1):
                e.vec_upload(2, np.full(shape, np.nan, np.float32))
                assert e.vec_regularizer(0, out=2, kind=kind, x0=x0, weight=1.0, eps=EPS) == 0.0
                assert not e.vec_download(2).any() and e.vec_dot(2, 2) == 0.0
        e.vec_upload(2, np.full(shape, np.nan, np.float32))  # x0 = x
        assert e.vec_regularizer(0, out=2, kind="tv", x0=0, weight=1.0, eps=EPS) == 0.0 and not e.vec_download(2).any()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", [S2A, S3A, S3B], ids=str)
def test_the_operator_is_symmetric_on_the_device(gpu, shape, dtype):
    x, x0, v, w = fields(shape)
    wt = WEIGHTS[len(shape)][1]
    with loaded(shape, dtype) as e:
        e.vec_upload(OUT2, w)
        for kind in ("tikhonov", "tv"):
            e.vec_regularizer(X, out=OUT, kind=kind, x0=X0, v=V, weight=wt, eps=EPS)
            Lv = e.vec_download(OUT).astype(np.float64)
            e.vec_regularizer(X, out=OUT, kind=kind, x0=X0, v=OUT2, weight=wt, eps=EPS)
            Lw = e.vec_download(OUT).astype(np.float64)
            v64, w64 = v.astype(np.float64), w.astype(np.float64)
            a, b = float(np.sum(Lv * w64)), float(np.sum(v64 * Lw))
            tol = 4 * U[dtype] * float(np.sum(np.abs(Lv * w64)) + np.sum(np.abs(v64 * Lw)))
            print("%s: |<Lv,w> - <v,Lw>| = %.3e, bound %.3e" % (kind, abs(a - b), tol))
            assert abs(a - b) <= tol, (kind, a, b, tol)
            assert float(np.sum(Lv * v64)) > 0.0 and float(np.sum(Lw * w64)) > 0.0


def test_each_refusal_is_einval_names_its_argument_and_touches_nothing(gpu):
    shape = S3A
    x, x0, v, old = fields(shape)
    nan, inf = float("nan"), float("inf")
    with loaded(shape, "float32") as e:
        e.vec_upload(OUT, old)
        ok = dict(out=OUT, kind="tv", x0=X0, v=V, alpha=1.0, beta=1.0, weight=1.0, eps=EPS)
        cases = [(dict(kind=7), "kind"), (dict(kind=-1), "kind"), (dict(kind="huber"), "kind"),
                 (dict(x=9), "x"), (dict(x0=9), "x0"), (dict(v=9), "v"), (dict(out=9), "out"), (dict(x=-1), "x"),
                 (dict(out=X), "alias x"), (dict(out=X0), "alias x0"), (dict(out=V), "alias v"),
                 (dict(weight=(1.0, -0.5, 1.0)), "weight[1]"), (dict(weight=(nan, 1.0, 1.0)), "weight[0]"),
                 (dict(weight=(1.0, 1.0, inf)), "weight[2]"), (dict(weight=(1.0, 1.0)), "weight"),
                 (dict(weight=(1.0,) * 4), "weight"),
                 (dict(eps=0.0), "eps"), (dict(eps=-1.0), "eps"), (dict(eps=nan), "eps"), (dict(eps=inf), "eps"),
                 (dict(eps=None), "eps"),
                 (dict(alpha=nan), "alpha"), (dict(alpha=inf), "alpha"), (dict(beta=nan), "beta"), (dict(beta=-inf), "beta")]
        for change, word in cases:
            kw = dict(ok, **change)
            xs = kw.pop("x", X)
            with pytest.raises(FwiError) as ei:
                e.vec_regularizer(xs, **kw)
            assert ei.value.code == 1 and all(t in str(ei.value) for t in word.split()), (change, str(ei.value))
        # what the Python method cannot ask for: no output at all, a null weight
        raw, ctx = e._lib.fwi_vec_regularizer, e._c
        w3 = np.ones(3).ctypes.data_as(C.POINTER(C.c_double))
        val = C.c_double(-7.0)
        for args, word in [((ctx, 1, X, X0, V, -1, 1.0, 1.0, w3, EPS, None), "value_out"),
                           ((ctx, 1, X, X0, V, OUT, 1.0, 1.0, None, EPS, C.byref(val)), "weight")]:
            with pytest.raises(FwiError) as ei:
                _lib.check(e._ctx, raw(*args))
            assert ei.value.code == 1 and word in str(ei.value), str(ei.value)
        assert val.value == -7.0
        for slot, a in ((X, x), (X0, x0), (V, v), (OUT, old)):  # nothing was touched
            assert np.array_equal(e.vec_download(slot), a)
        e.vec_regularizer(X, **dict(ok, eps=None, kind="tikhonov"))  # Tikhonov ignores eps; the context still works
        ref = tr.apply(x, v, "tikhonov", 1.0, None, x0) + old
        M = tr.majorant(x, v, "tikhonov", 1.0, None, x0, 1.0, 1.0, old)
        err = np.abs(e.vec_download(OUT).astype(np.float64) - ref)
        assert (err <= U["float32"] * np.abs(ref) + 64 * U64 * M).all()


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / np.linalg.norm(b))


def _small_inversion(nshots):
    w = workloads.cfg5(0.1875, nshots=3)  # 48^3, the problem of test_device_lbfgs_with_smoothing_h0_matches_the_host_one
    wav = w.wavelet()
    shots = [sh.Shot(w.src_idx[i:i + 1], wav, w.rec_idx) for i in range(nshots)]
    return w, shots, w.c_init.astype(np.float32)


def test_regularized_fg_device_adds_the_term_to_the_plain_objective(gpu):
    w, shots, m0 = _small_inversion(3)
    prior = w.c.astype(np.float32)
    seen = {}
    with Engine(w.shape, w.h, w.dt, w.nt, order=w.order, npml=w.npml) as e:
        sh.model_data(e, prior, shots)
        e.vec_create(3)
        e.vec_upload(0, m0)

        def plain(xs, gs):  # the plain objective, keeping what it returned: its float atomics differ from call to call
            seen["f"] = sh.misfit_and_gradient_device(e, xs, gs, shots)
            seen["g"] = e.vec_download(gs)
            return seen["f"]

        assert rg.regularized_fg_device(e, plain, 0.0, "tv", 1.0, 1.0, 2, prior) is plain
        plain(0, 1)
        for kind, eps, x0 in (("tv", 1.0, prior), ("tikhonov", None, None)):
            # a weight that makes the term as large as the gradient it is added to
            lam = float(np.abs(seen["g"]).max() / np.abs(tr.apply(m0, None, kind, (1.0, 0.5, 2.0), eps, x0)).max())
            fg = rg.regularized_fg_device(e, plain, lam, kind, (1.0, 0.5, 2.0), eps, None if x0 is None else 2, x0)
            f = fg(0, 1)
            g = e.vec_download(1).astype(np.float64)
            R, L = tr.value(m0, kind, (1.0, 0.5, 2.0), eps, x0), tr.apply(m0, None, kind, (1.0, 0.5, 2.0), eps, x0)
            M = tr.majorant(m0, None, kind, (1.0, 0.5, 2.0), eps, x0, lam, 1.0, seen["g"])
            ref = seen["g"].astype(np.float64) + lam * L
            err = np.abs(g - ref)
            print("%s: f %.9g = %.9g + lam R %.9g; max |g err| %.3e, |lam L| max %.3e, |g| max %.3e"
                  % (kind, f, seen["f"], lam * R, err.max(), lam * np.abs(L).max(), np.abs(seen["g"]).max()))
            assert R > 0.0 and np.abs(lam * L).max() > 0.1 * np.abs(seen["g"]).max()  # the term is there to be seen
            assert (err <= U["float32"] * np.abs(ref) + 64 * U64 * M).all(), err.max()
            assert abs((f - seen["f"]) - lam * R) <= lam * (m0.size + 16) * U64 * R + 4 * U64 * abs(f)


def test_device_and_host_lbfgs_agree_with_a_tv_term_and_a_prior(gpu):
    w, shots, m0 = _small_inversion(3)
    kw = dict(maxiter=3, history=3, first_step=40.0, bounds=(1000.0, 5000.0))
    eps = 1.0
    with Engine(w.shape, w.h, w.dt, w.nt, order=w.order, npml=w.npml) as e:
        sh.model_data(e, w.c.astype(np.float32), shots)
        fg_h = lambda m: sh.misfit_and_gradient(e, m, shots)  # noqa: E731
        fg_d = lambda xs, gs: sh.misfit_and_gradient_device(e, xs, gs, shots)  # noqa: E731
        # lam R of the order of the misfit after the first step: R of the first trial update, -first_step g / max |g|
        f0, g0 = fg_h(m0)
        step = -kw["first_step"] * np.asarray(g0, np.float64) / float(np.abs(g0).max())
        lam = f0 / rg.value(step, "tv", 1.0, eps)
        print("f0 = %.6g, lam = %.6g" % (f0, lam))
        assert np.isfinite(lam) and lam > 0.0
        xh, fh, logh = lbfgs(rg.regularized_fg(fg_h, lam, "tv", 1.0, eps, m0), m0, dot=e.dot, **kw)
        xs0 = rg.prior_slot(kw["history"])
        xd, fd, logd = lbfgs_device(e, rg.regularized_fg_device(e, fg_d, lam, "tv", 1.0, eps, xs0, m0), m0,
                                    extra_slots=1, **kw)
        xp, fp, logp = lbfgs_device(e, fg_d, m0, **kw)
    print("host", [r["f"] for r in logh], "device", [r["f"] for r in logd], "plain", [r["f"] for r in logp])
    assert [r["evals"] for r in logd] == [r["evals"] for r in logh]
    assert abs(fd - fh) < 1e-3 * fh
    assert rel(xd, xh) < 1e-5
    assert rel(xd, xp) > 1e-4 * rel(xp, m0) and not np.array_equal(xd, xp)  # the term changed the result
    assert rg.value(xd, "tv", 1.0, eps, m0) < rg.value(xp, "tv", 1.0, eps, m0)  # and the way it should
