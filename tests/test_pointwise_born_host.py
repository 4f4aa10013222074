"""The per-cell measurement of tests/_pointwise_born.py, held to account where there is no GPU: on every problem of
tests/test_gpu_pointwise_born.py the Born majorant dominates the fp64 Born field and ``M_q`` the stored term, the
scattered field reaches every cell, and the fp32 ORACLE needs at most a quarter of the rigorous factor (so the 4 x margin,
not ``T_rig_born``, decides every fp32 case); seeded errors of the kind a Born kernel could have -- one cell's weight,
one stored value, a corner cell's weight under the CPML -- fail the comparator while the relative L2 norm of the very
same arrays stays below the 1e-5 of the norm-wise suites; and a step dropped from the illumination at one border cell
exceeds the illumination's bound while the whole-grid norm moves by less than 1e-5."""
import numpy as np
import pytest

import _pointwise as pw
import _pointwise_born as pb_
from oracle import fwi_oracle as fo

KEYS = sorted({pw.problem_key(b.case) for b in pb_.BORN_CASES + pb_.BF16_CASES} |
              {pw.problem_key(c) for c in pb_.ILLUM_CASES}, key=str)
FORMS = {k: sorted({b.case.kw.get("update_form", "standard") for b in pb_.BORN_CASES if pw.problem_key(b.case) == k} or
                   {"standard"}) for k in KEYS}


def _kid(k):
    return "%s-O%d-npml%d-nt%d-%s-%s-a%g-S%d" % (("x".join(map(str, k[0])),) + k[1:])


@pytest.mark.parametrize("key", KEYS, ids=_kid)
def test_reference_alone_dominates_covers_and_passes(key):
    R = pb_.born_reference(key)
    # dominance: the fp64 Born field under M_B, the fp64 stored term under M_q, at every sample
    assert np.isfinite(R["Mq"]).all() and (np.abs(R["q64"]) <= R["Mq"] * (1 + 1e-12)).all()
    for wrt in pb_.WRTS:
        x, M = np.abs(R["ref"][wrt]), R["maj"][wrt]
        assert np.isfinite(M).all() and (x <= M * (1 + 1e-12)).all(), wrt
        assert (x[M == 0] == 0).all(), wrt
    pb_.born_coverage(R)
    # the fp32 oracle's own ratio: positive, and at most a quarter of the rigorous factor
    for form in FORMS[key]:
        T = pb_.born_factors(R, form)
        if R["own"] is None:
            assert T["velocity"] == T["slowness2"] == T["rig"]
            continue
        for wrt in pb_.WRTS:
            own = R["own"][wrt]
            assert 0.0 < own <= T["rig"] / 4, (wrt, own, T["rig"])
            assert T[wrt] == pw.MARGIN * own
            worst = pw.check(R["o32"][wrt], R["ref"][wrt], R["maj"][wrt], R["u"], T[wrt], wrt, key[0])
            assert worst == pytest.approx(own)
            print("%s %s: fp32 oracle err / (u M_B) = %.2f, T_born = %.1f, T_rig_born = %.0f" % (_kid(key), wrt, own, T[wrt],
                                                                                               T["rig"]))


def test_cases_run_the_shapes_and_paths_they_name():
    ids = [pb_.born_case_id(b) for b in pb_.BORN_CASES]
    assert len(set(ids)) == len(ids) == 34
    assert len({pw.case_id(c) for c in pb_.ILLUM_CASES}) == len(pb_.ILLUM_CASES) == 11
    fused = [b for b in pb_.BORN_CASES if "fused" in b.modes]
    assert all(b.modes == ("scatter", "fused") for b in fused) and len(fused) == 18
    # the variants of the fused kernel (launch_stream_born_mode): rows per tile, damped, full x tile, increment form
    seen = {(c.tile[1], c.npml > 0, c.shape[2] % 256 == 0 and c.shape[1] % c.tile[1] == 0,
             c.kw.get("update_form") == "increment") for c in (b.case for b in fused)}
    want = {(ty, damped, full, inc) for ty in (4, 8) for damped in (True, False) for full in (True, False)
            for inc in (True, False)} - {(8, False, True, False), (8, False, True, True), (4, False, True, True)}
    assert seen == want, seen ^ want
    assert pb_.t_rig_born(12, 8, 3) == pytest.approx(860.52 + 1.01 * 12 * 74)
    # problems shared with tests/_pointwise.py wherever the key exists there
    theirs = {pw.problem_key(c) for c in pw.CASES}
    new = {k for k in KEYS if k not in theirs}
    assert new == {((12, 16, 256), 8, 0, 12, "float32", "sponge", 0.0, 1)}, new


# -- sensitivity: seeded errors in the fp32 restatement ---------------------------------------------------------------
SPONGE = ((20, 17, 23), 8, 4, 12, "float32", "sponge", 0.0, 1)
CPML = ((24, 20, 32), 8, 8, 12, "float32", "cpml", 30.0, 1)


def _weight_off(cell, rel):
    def seed(pert):
        dc = pert["velocity"].copy()
        dc[cell] *= np.float32(1 + rel)   # w = 2 dc / c: the same relative error in w at that cell
        return {"velocity": dc}, None
    return seed


def _stored_q_off(step, cell, rel):
    def seed(pert):
        def mutate_store(p):
            p.q_store[step][cell] *= np.float32(1 + rel)
        return {"velocity": pert["velocity"]}, mutate_store
    return seed


@pytest.mark.parametrize("key,seed", [
    (SPONGE, _weight_off((1, 1, 1), 1e-4)), (SPONGE, _stored_q_off(5, (1, 1, 1), 1e-3)),
    (CPML, _weight_off((0, 0, 0), 1e-4))], ids=["w_1e-4_at_1_1_1", "stored_q_step5_1e-3_at_1_1_1", "cpml_w_1e-4_at_a_corner"])
def test_seeded_errors_fail_per_cell_and_pass_the_global_norm(key, seed):
    R = pb_.born_reference(key)
    T = pb_.born_factors(R)["velocity"]
    assert T == pw.MARGIN * R["own"]["velocity"]
    pert, mutate_store = seed(R["pert"])
    x = pb_.oracle_born(R["pb"], np.float32, pert, mutate_store=mutate_store, wrts=("velocity",))[0]["velocity"]
    ref, M = R["ref"]["velocity"], R["maj"]["velocity"]
    assert not np.array_equal(x, R["o32"]["velocity"])
    print("seeded: err / (u M_B) = %.1f against T = %.1f; global rel L2 %.3g (unseeded %.3g)" % (
        pw.ratio(x, ref, M, R["u"]), T, pw.rel_l2(x, ref), pw.rel_l2(R["o32"]["velocity"], ref)))
    assert pw.rel_l2(x, ref) < pw.GLOBAL_TOL            # what the norm-wise suites would have seen
    with pytest.raises(AssertionError, match="beyond T u M"):
        pw.check(x, ref, M, R["u"], T, "seeded", key[0])
    pw.check(R["o32"]["velocity"], ref, M, R["u"], T, "unperturbed", key[0])


def test_illumination_bound_sees_a_dropped_step_at_a_border_cell():
    R = pb_.born_reference(SPONGE)
    pb = R["pb"]
    T_fwd = pw.factors(pw.reference(SPONGE))["forward"]
    _, p32 = pb_.oracle_born(pb, np.float32, R["pert"], wrts=())
    q = np.asarray(p32.q_store, np.float32).reshape(pb["nt"], -1)

    def H(q):   # the accumulation in the engine's type
        h = np.zeros(q.shape[1], np.float32)
        for n in range(0, pb["nt"], pb["stride"]):
            h += q[n] * q[n]
        return h.astype(np.float64) * (pb["stride"] / pb["dt"] ** 4)
    Hm, E = pb_.illumination_reference(R)
    share, over_uE = pb_.check_illumination(H(q), R, T_fwd, "fp32 oracle", pb["shape"])
    print("fp32 oracle: largest err / bound %.2f, err / (u E) %.2f" % (share, over_uE))
    assert 0.0 < share < 1.0
    cell = int(np.ravel_multi_index((0, 0, 5), pb["shape"]))   # on the edge z = 0, y = 0, between the lattice's points
    assert q[5, cell] != 0 and cell not in fo._ravel_idx(pb["src"], pb["shape"])
    q[5, cell] = 0
    h = H(q)
    assert pw.rel_l2(h, Hm) < 1e-5
    with pytest.raises(AssertionError, match=r"beyond the illumination bound; worst at cell \(0, 0, 5\)"):
        pb_.check_illumination(h, R, T_fwd, "dropped step", pb["shape"])
