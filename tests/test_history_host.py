"""The history tests' own machinery, without a GPU (tests/_history.py): the sequences cover what they promise, the
steps are shaped as the comparison assumes, and the tables say what include/fwi.h says."""
import os

import numpy as np
import pytest

import _history as H

HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fwi.h")).read()
SWEEP_CALLS = {"adjoint", "adjoint_spectral", "born"}


def in_header(words):
    return " ".join(words.split()) in " ".join(HEADER.replace("\n *", " ").split())


@pytest.mark.parametrize("config", list(H.CONFIGS))
def test_every_ordered_pair_of_families_is_adjacent(config):
    fams = H.families_of(config)
    seq = H.sequence(config)
    assert len(seq) == len(fams) ** 2 + 1 <= 700
    pairs = {(a.family, b.family) for (a, _), (b, _) in zip(seq, seq[1:])}
    assert pairs == {(a, b) for a in fams for b in fams}
    assert {s.family for s, _ in seq} == set(fams)


@pytest.mark.parametrize("config", list(H.CONFIGS))
def test_sequences_are_reproducible_from_their_seed(config):
    ids = lambda seq: [(s.family, s.variant, m) for s, m in seq]  # noqa: E731
    assert ids(H.sequence(config, H.SEED)) == ids(H.sequence(config, H.SEED))
    assert ids(H.sequence(config, H.SEED)) != ids(H.sequence(config, H.SEED + 1))
    for other in H.CONFIGS:  # the configuration is part of the seed
        if other != config and H.families_of(other) == H.families_of(config):
            assert ids(H.sequence(config)) != ids(H.sequence(other))


@pytest.mark.parametrize("config", list(H.CONFIGS))
def test_visits_of_a_family_alternate_between_larger_and_smaller(config):
    seq = H.sequence(config)
    model_id = 0
    for fam in H.families_of(config):
        visits = [s for s, _ in seq if s.family == fam]
        assert len(visits) >= len(H.catalogue()[fam])  # every variant is reached
        if fam == "refused":
            assert {s.variant for s in visits} == set(range(len(H.REFUSALS)))
            continue
        sizes = [s.size for s in visits]
        ups = [b > a for a, b in zip(sizes, sizes[1:])]
        assert all(u != v for u, v in zip(ups, ups[1:])), (fam, sizes)
    for step, m in seq:  # the model in force is the one the model steps left
        assert m == model_id
        model_id = 1 - model_id if step.changes_model else model_id
    assert {m for _, m in seq} == {0, 1}


def test_the_sizes_cover_the_edges_of_the_kernels():
    sizes = set(H.SWEEPS) | {s for v in H.SIZES.values() for s in v} | {s[:3] for s in H.FORWARD_AT} | {
        (kw["nt"], kw["nsrc"], kw["nrec"]) for kw in H.MISFIT_VARIANTS}
    assert {5, 31, 33, H.NT_MAX} <= {s[0] for s in sizes}
    assert {0, 1, 3} <= {s[1] for s in sizes}
    assert {0, 1, 7, 65} <= {s[2] for s in sizes}
    v = H.MISFIT_VARIANTS
    assert any(len(H.taps_of(k.get("taps"))) - 1 > k["nt"] - 1 for k in v if k.get("taps"))  # long taps: clipped
    assert any(k.get("taps") and len(H.taps_of(k["taps"])) - 1 < k["nt"] - 1 for k in v) and any(not k.get("taps") for k in v)
    for flag in ("weights", "tw"):
        assert any(k.get(flag) for k in v) and any(not k.get(flag) for k in v)
    assert sum(bool(k.get("off_grid")) for k in v) == 1
    for name in ("A", "B", "C"):  # the frequencies: distinct, inside (0, Nyquist)
        for config in ("3d_f32_fourier", "2d_f32_fused"):
            P = H.Problem(config)
            f = P.freqs[name]
            assert len(set(f)) == f.size and f.min() > 0 and f.max() < 0.5 / P.dt
    assert len(H.Problem("3d_f32_fourier").freqs["A"]) == len(H.Problem("3d_f32_fourier").freqs["B"]) == 4


@pytest.mark.parametrize("config", list(H.CONFIGS))
def test_every_step_is_shaped_as_the_comparison_assumes(config):
    """Through the recording stub: a step starts with reset_gradient, runs its own forward before any other sweep or
    misfit, ends with a context whose settings are the configured ones, and is refused exactly where it says so."""
    P = H.Problem(config)
    cat = H.catalogue()
    for fam in H.families_of(config):
        for step in cat[fam]:
            for model_id in (0, 1):
                e = H.StubEngine(P)
                out = step.run(e, P, model_id)
                calls = e.calls
                assert calls[0] == "reset_gradient", (step, calls)
                sweeps = [c for c in calls if c in SWEEP_CALLS or c.startswith(("misfit_", "forward"))]
                assert sweeps and sweeps[0] in ("forward", "forward_at"), (step, calls)
                assert (e.refusals == 1) == bool(step.refused), (step, e.refusals)
                if step.refused:
                    assert out == {} and fam == "refused"
                    continue
                assert "gradient" in calls or fam in ("fwd_save", "fwd_nosave", "vec"), (step, calls)
                assert all(np.all(np.isfinite(np.asarray(v, np.complex128))) for v in out.values())
                # what the step switched, it switched back
                for setter in ("set_illumination", "set_launch_mode"):
                    assert calls.count(setter) in (0, 2), (step, calls)
                if "set_fourier_store" in calls:
                    assert np.array_equal(e.fourier_freqs, P.freqs["A"])
                assert ("set_model" in calls) == step.changes_model
                # the same outputs whatever the model: the comparison pairs them by name
                assert sorted(out) == sorted(step.run(H.StubEngine(P), P, 1 - model_id))


def test_the_refused_steps_are_those_the_header_lists():
    cat = H.catalogue()
    assert [s.refused for s in cat["refused"]] == [(code, words) for _, code, words in H.REFUSALS]
    for which, code, words in H.REFUSALS:
        assert code in (1, 3) and in_header(words), which
    assert "enum { FWI_SPEC_L2 = 0, FWI_SPEC_PHASE = 1, FWI_SPEC_LOGAMP = 2, FWI_SPEC_LOG = 3 }" in HEADER  # 7 is none
    assert all(s.refused is None for fam, steps in cat.items() if fam != "refused" for s in steps)


def test_the_table_of_families_left_out_is_the_headers():
    assert set(H.LEFT_OUT) == set(H.CONFIGS)
    for config, opts in H.CONFIGS.items():
        fourier = "fourier" in opts
        reduced_store = opts.get("ckpt_interval", 0) > 0 or opts.get("image_stride", 1) > 1 or opts.get("store_dtype") == "bf16"
        want = set()
        if reduced_store:
            want.add("born_exact")  # fwi_born: "Contexts whose store does not hold every q^n in the field's type ..."
        if fourier:
            want |= {"born_exact", "born_imaging", "illum"}
        else:
            want |= set(H.FOURIER_FAMILIES)
        assert set(H.LEFT_OUT[config]) == want, config
        for fam, words in H.LEFT_OUT[config].items():
            assert in_header(words), (config, fam)
        # what fwi_set_fourier_store would refuse is said to be refused, not merely switched off
        refuses_store = opts.get("ckpt_interval", 0) > 0 or opts.get("store_dtype") == "bf16"
        if not fourier:
            assert all((w == H._NO_FOURIER) == refuses_store for w in H.LEFT_OUT[config].values() if w != H._NO_EXACT_BORN)
    # the options fwi_create itself refuses to combine do not occur
    for opts in H.CONFIGS.values():
        assert not (opts.get("image_stride", 1) > 1 and opts.get("ckpt_interval", 0) > 0)
        if opts.get("store_dtype") == "bf16":
            assert len(opts["shape"]) == 3 and opts.get("dtype", "float32") == "float32" and "abc" not in opts
            assert "update_form" not in opts and "ckpt_interval" not in opts and "kernel" not in opts


def test_first_difference_names_the_output():
    a = {"x": np.arange(6.0).reshape(2, 3), "J": 1.5}
    assert H.first_difference(a, {"x": a["x"].copy(), "J": 1.5}) is None
    b = {"x": a["x"].copy(), "J": 1.5}
    b["x"][1, 2] = np.nextafter(5.0, 6.0)
    name, what = H.first_difference(a, b)
    assert name == "x" and "1 of 6" in what and "(1, 2)" in what
    assert H.first_difference(a, {"x": a["x"], "J": np.nan})[0] == "J"
    assert H.first_difference({"x": np.array([np.nan])}, {"x": np.array([np.nan])})[0] == "x"  # a NaN equals nothing
    assert H.first_difference(a, {"x": a["x"]})[0] == "outputs"
    assert H.first_difference(a, {"x": a["x"].astype(np.float32), "J": 1.5})[0] == "x"
