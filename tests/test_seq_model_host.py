"""The sequence tests' host side (tests/seq_util.py) without a GPU: the model against the oracle's own
run, the generator, what the committed seed set covers, the tie guard's cap, and the mutants -- a
pure-numpy driver with one piece of state left stale on purpose must fail at least one committed
sequence of the matching policy, or the seed set has no teeth for that kind of defect."""

import numpy as np
import pytest

from oracle import newton_oracle as O
from tests import seq_util as S


@pytest.fixture(scope="module")
def cases():
    return {a: S.committed(a) for a in S.ADAPTERS}


@pytest.fixture(scope="module")
def host_runs(cases):
    """case id -> (sequence, model after the whole sequence), computed once"""
    out = {}
    for a in S.ADAPTERS:
        for c in cases[a]:
            seq = c.resolved()[0]
            out[c.id] = (seq, c.host_run(seq))
    return out


@pytest.mark.parametrize("kind", S.POLICIES)
def test_steps_only_reproduce_the_oracles_run(kind):
    from pygradflow_amd import problems

    prob = problems.dense_qp(60, 15, seed=3, boxed_frac=0.3, box=0.05)
    x0, y0 = S.op_vectors(prob, 11)
    recs = O.NewtonOracle(prob, kind, x0, y0, 0.5, 10.0, 0.05).run(x0, y0, 5)
    model = S.SequenceModel(prob, kind, 0.05, x0, y0, 0.5, 10.0)
    for k, rec in enumerate(recs):
        exp = model.apply(("S", k % 3 == 2))
        assert exp["diff"] == rec["diff"] and exp["n_neg"] == 15
        assert np.array_equal(model.x, rec["xn"]) and np.array_equal(model.y, rec["yn"])
        assert np.array_equal(model.read("mask")["mask"], rec["mask"])
    assert model.sizes == [int(60 - r["mask"].sum()) for r in recs]


def test_generator_is_deterministic_and_shaped():
    for a, B in (("dense", 0), ("band", 0), ("dense_batch", 5), ("band_batch", 4)):
        steps = 0
        for seed in range(20):
            s1, s2 = S.sequence(seed, adapter=a, B=B), S.sequence(seed, adapter=a, B=B)
            assert s1.key() == s2.key()
            assert len(s1.ops) == 14 and s1.ops[0][0] == "S" and s1.ops[-1][0] == "R"
            assert s1.key() != S.sequence(seed + 1, adapter=a, B=B).key()
            steps += sum(op[0] in "SY" for op in s1.ops)
            n_s = 0
            for op in s1.ops:  # every third S checks the inertia
                if op[0] == "S" and not a.endswith("_batch"):
                    n_s += 1
                    assert op[1] == (n_s % 3 == 0)
        assert 0.4 <= steps / (20 * 14) <= 0.65, (a, steps)
    taus = [S.sequence(s).tau for s in range(200)]
    assert set(taus) == {None, 0.05} and 0.15 <= taus.count(0.05) / 200 <= 0.35
    # dt and rho can each stay, and rho can change alone
    adv = [(op, prev) for s in range(60) for prev, op in _advances(S.sequence(s))]
    assert any(op[1] == pd and op[2] == pr for op, (pd, pr) in adv)
    assert any(op[1] == pd and op[2] != pr for op, (pd, pr) in adv)
    assert any(op[1] != pd and op[2] == pr for op, (pd, pr) in adv)


def _advances(seq):
    cur = (seq.dt, seq.rho)
    for op in seq.ops:
        if op[0] == "A":
            yield cur, op
            cur = (op[1], op[2])
        elif op[0] == "O":
            cur = (op[3], op[4])


def test_committed_shapes_are_the_ones_asked_for(cases):
    dense = cases["dense"][:len(S.DENSE_SHAPES)]
    assert len(dense) == 12 and {c.policy for c in dense} == set(S.POLICIES)
    assert {s[0] for s in S.DENSE_SHAPES} == {100, 257, 300, 513}
    assert all(0 <= m <= n // 3 for n, m, *_ in S.DENSE_SHAPES)
    assert {s[2] for s in S.DENSE_SHAPES} == {0.0, 0.05, 0.3, 0.7} and {s[3] for s in S.DENSE_SHAPES} == {0.01, 0.05, 0.5}
    assert sum(m >= 64 for _, m, *_ in S.DENSE_SHAPES) >= 2
    assert not dense[4].problem(0).var_bounded  # boxed_frac = 0: the unbounded front
    band = cases["band"]
    assert {(c.name, c.policy) for c in band} >= {(p, k) for p in S.BAND_PROBLEMS for k in S.POLICIES}
    from tests.band_util import plan_of

    blocks = {name: plan_of(S._band_problem(name, 40)).block_size for name in S.BAND_PROBLEMS}
    assert blocks["sparse_ocp60"] == 8 and blocks["box_qp300"] == 8
    assert blocks["ms40_split"] == blocks["ms40_nosplit"] == 16
    assert blocks["ms30_split"] == blocks["ms30_nosplit"] == 32
    for name in ("budget300", "ocp_param30"):
        assert plan_of(S._band_problem(name, 40)).k >= 1
    assert len(set(c.seed for c in band)) == len(band)
    for a in ("dense_batch", "band_batch"):
        for pol in S.POLICIES:
            assert sum(c.policy == pol for c in cases[a]) >= 2


def test_committed_sequences_cover_every_operation(cases, host_runs):
    for a in S.ADAPTERS:
        letters, kinds = set(), set()
        for c in cases[a]:
            for op in host_runs[c.id][0].ops:
                letters.add(op[0])
                if op[0] == "H":
                    kinds.add(op[1])
        if a.endswith("_batch"):
            assert letters == set("SAEFR"), (a, letters)
        else:
            assert letters - {"o"} == set("SYAOPRH"), (a, letters)  # ("o": the regression cases' own)
            assert kinds == (set("abcd") if a == "dense" else set("ab")), (a, kinds)


def test_committed_sequences_meet_the_degenerate_steps(cases, host_runs):
    singles = [(c, host_runs[c.id][1]) for a in ("dense", "band") for c in cases[a]]
    sizes = [m.sizes for _, m in singles]
    assert sum(len(set(s)) > 1 for s in sizes) >= len(sizes) // 3  # |I| changes within a sequence
    assert any(0 in s for s in sizes)  # an all-active step
    assert any(m.n in m.sizes for c, m in singles if c.problem(0).var_bounded)  # none active, with bounds
    assert any(m.n in m.sizes for c, m in singles if not c.problem(0).var_bounded)
    # n_I + m above 512: more than two outer blocks of the dense factorisation
    assert any(max(m.sizes) + m.m > 512 for c, m in singles if c.adapter == "dense")
    assert any(m.rho_alone for c, m in singles if c.policy == "Simplified")
    assert any(m.p_between_steps for c, m in singles if c.policy == "ActiveSet")
    for a in ("dense_batch", "band_batch"):
        ms = [host_runs[c.id][1] for c in cases[a]]
        assert any(m.rejected_moved for m in ms) and any(m.frozen_steps for m in ms), a
        assert len({s for m in ms for one in m.models for s in one.sizes}) > 1


def test_the_tie_guard_replaces_at_most_one_sequence_in_ten(cases, host_runs):
    allc = [c for a in S.ADAPTERS for c in cases[a]]
    replaced = [c.id for c in allc if c.resolved()[2]]
    assert 10 * len(replaced) <= len(allc), replaced
    margins = [host_runs[c.id][1].min_margin for c in allc]
    print(f"{len(replaced)} of {len(allc)} replaced; smallest margin {min(margins):.2e}")
    assert min(margins) >= S.MARGIN_BAR


def test_the_numpy_driver_passes_every_committed_sequence(cases):
    for a in S.ADAPTERS:
        for c in cases[a]:
            S.run_sequence(c, S.FakeBackend())


MUTANTS = {  # defect -> (adapters, policies) whose committed sequences must catch it
    1: (("dense", "band"), ("Simplified",)),
    2: (("dense", "band"), ("ActiveSet",)),
    3: (("dense", "band"), S.POLICIES),
    4: (("dense", "band"), S.POLICIES),
    5: (("dense_batch", "band_batch"), S.POLICIES),
}


@pytest.mark.parametrize("defect", sorted(MUTANTS))
def test_each_mutant_fails_a_committed_sequence(cases, defect):
    adapters, policies = MUTANTS[defect]
    caught = []
    for a in adapters:
        for c in cases[a]:
            if c.policy not in policies:
                continue
            try:
                S.run_sequence(c, S.FakeBackend(defect))
            except S.SequenceFailure as e:
                caught.append(c.id)
                msg = str(e)
                assert c.adapter in msg and "first failing op" in msg and f"seed {c.resolved()[1]}" in msg
        if caught and defect in (3, 4):  # one adapter's catch is enough for the policy-free defects
            break
    print(S.DEFECTS[defect], "caught by", caught)
    assert caught, S.DEFECTS[defect]
    if defect in (1, 2):  # on the dense and on the banded handle alike
        assert any(i.startswith("dense-") for i in caught) and any(i.startswith("band-") for i in caught), caught
