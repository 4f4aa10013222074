"""The per-cell measurement of tests/_pointwise.py, held to account where there is no GPU: the majorant dominates the
fp64 oracle everywhere; on every problem of tests/test_gpu_pointwise.py the field reaches every cell and the fp32 ORACLE
passes the comparator at the factor the engine will be held to; and seeded errors of the kind a kernel could have -- one
cell's C, one sponge cell's A, one row's outermost stencil weight, one CPML coefficient -- fail it, each while the
relative L2 norm of the very same arrays stays below the 1e-5 of the norm-wise suites."""
import numpy as np
import pytest

import _pointwise as pw

DOMINATION = [(shape, order, npml, abc, alpha)
              for shape, npml in (((33, 47), 6), ((14, 13, 17), 4))
              for order in (2, 4, 8)
              for abc, alpha in (("sponge", 0.0), ("cpml", 0.0), ("cpml", 25.0))]


@pytest.mark.parametrize("shape,order,npml,abc,alpha", DOMINATION)
def test_majorant_dominates_the_fp64_oracle(shape, order, npml, abc, alpha):
    R = pw.reference((shape, order, npml, 12, "float64", abc, alpha, 1))
    for what in pw.ALL:
        x, M = np.abs(R["ref"][what]), R["maj"][what]
        assert np.isfinite(M).all() and (x <= M * (1 + 1e-12)).all(), what
        assert (x[M == 0] == 0).all(), what


def test_majorant_gradient_follows_the_image_stride():
    R1 = pw.reference(((20, 17, 23), 8, 4, 12, "float32", "sponge", 0.0, 1))
    R3 = pw.reference(((20, 17, 23), 8, 4, 12, "float32", "sponge", 0.0, 3))
    assert (np.abs(R3["ref"]["gradient"]) <= R3["maj"]["gradient"] * (1 + 1e-12)).all()
    assert not np.array_equal(R1["maj"]["gradient"], R3["maj"]["gradient"])


KEYS = sorted({pw.problem_key(c) for c in pw.CASES}, key=str)


@pytest.mark.parametrize("key", KEYS, ids=lambda k: "%s-O%d-npml%d-nt%d-%s-%s-a%g-S%d" % (("x".join(map(str, k[0])),) + k[1:]))
def test_reference_alone_covers_and_passes(key):
    """What the GPU cases rely on, checked on the reference side: coverage, and the oracle in the engine's precision
    within the engine's factor (which is 4 x its own need or the rigorous count, whichever is smaller)."""
    R = pw.reference(key)
    pw.coverage(R)
    cases = [c for c in pw.CASES if pw.problem_key(c) == key]
    for form in sorted({c.kw.get("update_form", "standard") for c in cases}):
        T = pw.factors(R, form)
        assert T["forward"] <= T["rig"] and T["adjoint"] <= T["rig"] and T["gradient"] <= 2 * T["rig"] + R["pb"]["nt"]
        if R["o32"] is not None:
            for what in pw.ALL:
                worst = pw.check(R["o32"][what], R["ref"][what], R["maj"][what], R["u"], T[what], what, key[0])
                assert worst <= T[what]
                assert 4 * worst < T["rig"], "the rigorous count would cut the fp32 oracle's margin: recount"


def test_cases_run_the_shapes_they_name():
    ids = [pw.case_id(c) for c in pw.CASES]
    assert len(set(ids)) == len(ids)
    assert all(8 <= c.nt <= 12 for c in pw.CASES)
    assert {c.nt for c in pw.CASES if c.kernel == "step2d_fused" and not c.kw} == {10, 12}
    assert pw.flops(8, 3) == 71 and pw.flops(8, 2) == 56 and pw.flops(2, 3) == 37 and pw.flops(8, 3, "cpml") == 268


def test_cpml_cases_reach_the_lane_paths_they_name():
    """The x border runs in step3d_stream's lanes only where stream_xpml_supported holds (restated in the helper; on the
    GPU every case checks it against the context's own report): full lanes, the masked lane astride the border's inner
    edge, two x tiles, and the slab path are each held by a case of either update form and tile shape."""
    c3 = [c for c in pw.CASES if c.abc == "cpml" and len(c.shape) == 3 and not c.env.keys() & {"FWI_NO_PML_LINES", "FWI_NO_STREAM_XPML"}]
    for c in c3:
        assert c.ctx["x-in-kernel"] == int(pw.xpml_in_lanes(c.shape, c.order, c.npml, c.tile[2])) and c.ctx["line-axes"] == 3
    for form in ("standard", "increment"):
        for ty in (4, 8):
            mine = [c for c in c3 if c.kw["update_form"] == form and c.tile[1] == ty]
            lanes = [c for c in mine if c.ctx["x-in-kernel"]]
            assert any(pw.xpml_masked(c.shape, c.order, c.npml, c.tile[2]) for c in lanes)          # (22, 20, 32) npml 6
            assert any(not pw.xpml_masked(c.shape, c.order, c.npml, c.tile[2]) for c in lanes)      # npml 8
            assert any(c.shape[2] > c.tile[2] for c in lanes)                                        # two x tiles
            assert any(not c.ctx["x-in-kernel"] for c in mine)
    assert pw.xpml_masked((22, 20, 32), 8, 6, 32) and not pw.xpml_in_lanes((22, 20, 30), 8, 6, 32)
    assert not pw.xpml_in_lanes((22, 9, 30), 2, 5, 32) and pw.xpml_in_lanes((20, 18, 300), 8, 8, 152)


def test_comparator_names_the_sample_and_refuses_writes_ahead_of_the_wave():
    M = np.array([[0.0, 1.0, 2.0, 4.0]] * 2)
    ref = np.array([[0.0, 0.5, -1.0, 3.0]] * 2)
    u = pw.U["float32"]
    assert pw.check(ref.astype(np.float32), ref, M, u, 8.0, "x") == 0.0
    x = ref.copy()
    x[1, 2] += 9 * u * 2.0
    with pytest.raises(AssertionError, match=r"step 1, cell 2 = \(1, 0\) of \(2, 2\).*in the tile \(0, 2\) at \(1, 0\)"):
        pw.check(x, ref, M, u, 8.0, "x", shape=(2, 2), tile=(0, 2))
    assert pw.check(x, ref, M, u, 10.0, "x") == pytest.approx(9.0)
    x = ref.copy()
    x[0, 0] = 1e-30
    with pytest.raises(AssertionError, match="has not arrived"):
        pw.check(x, ref, M, u, 8.0, "x")
    x[0, 0] = np.nan
    with pytest.raises(AssertionError, match="non-finite"):
        pw.check(x, ref, M, u, 8.0, "x")
    x = ref.copy()
    x[0, 1] += 7 * float(np.finfo(np.float32).tiny)  # a flushed denormal's worth: inside the floor
    pw.check(x, ref, M, u, 8.0, "x")


# -- sensitivity: seeded errors in a copy of the fp32 oracle -----------------------------------------------------------
SPONGE = ((20, 17, 23), 8, 4, 12, "float32", "sponge", 0.0, 1)
CPML = ((24, 20, 32), 8, 8, 12, "float32", "cpml", 30.0, 1)


def _c_at_a_corner(p):
    p.C[1, 1, 1] *= np.float32(1 + 1e-4)


def _c_at_a_corner_1e2(p):
    p.C[1, 1, 1] *= np.float32(1 + 1e-2)   # (what the gradient's looser bound needs to see that cell)


def _a_of_an_outermost_sponge_cell(p):
    p.A[0, 4, 6] *= np.float32(1 + 1e-3)   # on the face z = 0, between the lattice's points


def _outermost_weight_on_one_row(p):
    plain, r = p.laplacian, p.r

    def laplacian(u):
        out = plain(u)
        coef, p.coef = p.coef, [np.float32(0)] * r + [p.coef[r]]
        shell = plain(u)   # the k = r shell alone
        p.coef = coef
        out[9, 8, :] += np.float32(0.01) * shell[9, 8, :]
        return out
    p.laplacian = laplacian


def _adjoint_cpml_a_of_an_outermost_cell(p):
    """The same 1 %, in the transposed recursion only (the branch an adjoint kernel has to itself)."""
    plain, (a, b) = p._cpml_term, p.cpml[2]
    bad = np.broadcast_to(a, p.shape).copy()
    bad[5, 4, 0] *= np.float32(1.01)

    def term(u, aux, reverse):
        p.cpml[2] = (bad if reverse else a, b)
        return plain(u, aux, reverse)
    p._cpml_term = term


def _cpml_a_of_an_outermost_cell(p):
    a, b = p.cpml[2]
    a = np.broadcast_to(a, p.shape).copy()
    a[5, 4, 0] *= np.float32(1.01)   # ONE cell of the plane x = 0, as a kernel's lane would have it
    p.cpml[2] = (a, b)


@pytest.mark.parametrize("key,mutate,what", [
    (SPONGE, _c_at_a_corner, "forward"), (SPONGE, _a_of_an_outermost_sponge_cell, "forward"),
    (SPONGE, _outermost_weight_on_one_row, "forward"), (CPML, _cpml_a_of_an_outermost_cell, "forward"),
    (SPONGE, _c_at_a_corner, "adjoint"), (SPONGE, _outermost_weight_on_one_row, "adjoint"),
    (CPML, _adjoint_cpml_a_of_an_outermost_cell, "adjoint"),
    (SPONGE, _outermost_weight_on_one_row, "gradient"), (SPONGE, _c_at_a_corner_1e2, "gradient")], ids=lambda v: getattr(v, "__name__", v if isinstance(v, str) else None))
def test_seeded_errors_fail_per_cell_and_pass_the_global_norm(key, mutate, what):
    """(The forward and the adjoint FIELD are what pins a cell.  The gradient's bound, G = sum M_mu M_q, adds magnitudes
    over the steps where the image cancels, so per cell the gradient is held less tightly than the two fields it is made
    of -- measured, err / (u G) against T = 75.1 on the sponge problem: the row's k = r weight off by 1 % 1013 (caught);
    the corner's C off by 1e-2 795 (caught), by 1e-3 80, by 1e-4 8.0 (not seen); the sponge cell's A off by 1e-3 80; on
    the CPML problem either 1 % seed 2.4 against 55.8 (not seen).  The gradient-only cases of the store variants
    therefore see a single-cell error of the stored term from about 1e-3 relative upward, not below.)"""
    R = pw.reference(key)
    T = pw.factors(R)
    x = pw.oracle_fields(R["pb"], np.float32, mutate=mutate, what=(what,))[what]
    assert not np.array_equal(x, R["o32"][what])
    assert pw.rel_l2(x, R["ref"][what]) < pw.GLOBAL_TOL            # what the norm-wise suites would have seen
    with pytest.raises(AssertionError, match="beyond T u M"):
        pw.check(x, R["ref"][what], R["maj"][what], R["u"], T[what], mutate.__name__, key[0])
    pw.check(R["o32"][what], R["ref"][what], R["maj"][what], R["u"], T[what], "unperturbed", key[0])
