"""The plain SQUAREM reference of the solver tests (tests/squarem_reference.py) on its own: against oracle.em.squaremEM on
the expanded reads, on hand-derived exact cases, every condition that tests/test_gpu_squarem_edges.py relies on for its
case table (so that a GPU failure there is the kernel's and not the table's), and a mutant check -- deliberately wrong
variants of the reference must each leave the bound of at least one run of the table, or the table is missing a case.
No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boot_reference as br  # noqa: E402
import squarem_reference as sq  # noqa: E402

from oracle import em as oem  # noqa: E402

STOP_MARGIN = 0.05
LD = np.longdouble


# ------------------------------------------------------------------------------------------------ against the oracle
ORACLE_CASES = [n for n in sq.CASE_NAMES if n.startswith(("rounds-", "alleles-", "weights-zeros", "sets-per-allele", "clamp-tiny",
                                                          "exact-identity", "exact-unnamed", "threshold-"))
                and sq.case(n).n_allele <= 129]


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_float64_reference_is_the_oracle_on_the_expanded_reads(name):
    """Integer weights: set u repeated weight[u] times is what the oracle (and the reference project) sees.  The oracle is a
    float64 evaluation of the reference's formulas that differs from its float64 run in the order of the sums only (w equal
    rows against w times one row): it has to meet the longdouble run within the very bound the kernel has to."""
    c = sq.case(name)
    alleles = [f"A*{a:03d}" for a in range(c.n_allele)]
    reads = br.replicateReads(c.packed, c.weight.astype(np.int64), alleles)
    for k in c.iter_maxes:
        if k == 0:
            continue
        want, want_iters = oem.squaremEM(reads, iter_max=k, diff_threshold=c.threshold)
        got = sq.reference(name, k, np.float64)
        full = np.array([want.get(a, 0.0) for a in alleles])
        _, limit = sq.bound(name, k)
        assert np.abs(full.astype(LD) - sq.reference(name, k).prob).max() <= limit, k
        assert not got.prob[[a not in want for a in alleles]].any()
        if got.iterations < k:
            assert want_iters == got.iterations, k
        else:
            # The oracle's count is its Python loop variable: a run that uses up iter_max leaves it at iter_max - 1, the
            # value it also has after a stop in the last pass.  The kernel and the reference say iter_max: "did not stop".
            assert want_iters == k - 1 and got.iterations == k, k


def test_the_oracle_counts_one_less_when_iter_max_is_used_up():
    c = sq.case("threshold-0")
    alleles = [f"A*{a:03d}" for a in range(c.n_allele)]
    _, want_iters = oem.squaremEM(br.replicateReads(c.packed, c.weight.astype(np.int64), alleles), iter_max=5, diff_threshold=0.0)
    assert want_iters == 4
    assert sq.reference("threshold-0", 5).iterations == 5 and sq.reference("threshold-0", 5, np.float64).iterations == 5


# ------------------------------------------------------------------------------------------------ hand-derived cases
@pytest.mark.parametrize("name", [n for n in sq.CASE_NAMES if sq.case(n).exact is not None])
def test_hand_derived_cases_are_exact(name):
    """Every intermediate is a dyadic fraction: both precisions give the bits derived by hand, skip the extrapolation
    (vs == 0) and stop in pass 0."""
    c = sq.case(name)
    for dtype in (LD, np.float64):
        for k in c.iter_maxes:
            run = sq.reference(name, k, dtype)
            assert np.array_equal(run.prob, c.exact.astype(dtype)), (dtype, k)
            assert run.iterations == 0 and run.clamped == 0 and run.zero_sum == 0
            assert run.vs_zero == (1 if k else 0)


def test_first_step_by_hand():
    """iter_max = 0 is the first step from ones alone: sets {0, 1} (weight 3) and {1} (weight 1) give (3/2, 3/2 + 1) / 4."""
    run = sq.squarem([[True, True], [False, True]], [3, 1], iter_max=0)
    assert np.array_equal(run.prob, np.array([0.375, 0.625], dtype=LD)) and run.iterations == 0


# ------------------------------------------------------------------------------------------------ the case table
def test_the_table_names_the_shapes():
    names = set(sq.CASE_NAMES)
    assert {f"rounds-{n}" for n in (1, 31, 32, 33, 63, 64, 65, 129)} <= names
    assert {f"alleles-{n}" for n in (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 511, 512)} <= names
    assert {f"scale-row-{n}" for n in (8191, 8192, 8193)} <= names
    for n in (1, 31, 32, 33, 63, 64, 65, 129):
        c = sq.case(f"rounds-{n}")
        assert c.packed.shape == (n, 2) and c.n_allele == 33
    for n in (8191, 8192, 8193):
        c = sq.case(f"scale-row-{n}")
        assert c.packed.shape == (n, 1) and c.n_allele == 24
    members = sq.case("members-per-set")
    assert members.n_allele == 512 and {1, 15, 16, 17, 31, 32, 33, 48, 511, 512} == set(members.sets.sum(axis=1).tolist())
    per = sq.case("sets-per-allele")
    assert len(per.packed) == 200 and all(per.sets[:, a].sum() == k for a, k in sq.SETS_PER_ALLELE.items())
    assert set(sq.SETS_PER_ALLELE.values()) == {1, 15, 16, 17, 33, 200}
    for c in sq.cases():      # as gk_em_run takes them: ascending, distinct, non-empty
        assert c.packed.dtype == np.uint32 and c.packed.any(axis=1).all()
        assert np.array_equal(sq.ascending(c.packed), np.arange(len(c.packed))), c.name
        assert len(np.unique(c.packed, axis=0)) == len(c.packed), c.name
        assert c.weight.dtype == np.float64 and (c.weight >= 0).all() and c.weight.sum() > 0


@pytest.mark.parametrize("n_allele", [n for n in sq.ALLELE_COUNTS if n % 32])
def test_bits_past_the_last_allele(n_allele):
    """Where n_allele is no multiple of 32, some sets carry bits past it, and one set of positive weight carries only
    such bits: its member list is empty, its weight names nobody."""
    c = sq.case(f"alleles-{n_allele}")
    ghost = np.unpackbits(c.packed.view(np.uint8), axis=1, bitorder="little")[:, n_allele:].any(axis=1)
    named = c.sets.any(axis=1)
    assert (ghost & named).any() and ((~named) & (c.weight > 0)).sum() == 1
    assert sq.reference(c.name, 300).zero_sum > 0


def test_the_weights_named():
    w = sq.case("weights-zeros").weight
    assert (w == 0).any() and (w > 0).any()
    assert set(sq.case("weights-fractions").weight.tolist()) == {0.25, 1.0 / 3.0}
    assert set(sq.case("weights-mixed").weight.tolist()) == {1.0, 100000.0}
    assert (sq.case("weights-two31").weight == 2.0 ** 31).sum() == 1


@pytest.mark.parametrize("name,iter_max", sq.RUNS)
def test_conditions_of_every_run(name, iter_max):
    """What the GPU tests take for granted of a run of the table."""
    c = sq.case(name)
    want, f64 = sq.reference(name, iter_max), sq.reference(name, iter_max, np.float64)
    dev64, limit = sq.bound(name, iter_max)
    assert np.isfinite(want.prob).all() and np.isfinite(f64.prob).all()
    assert abs(float(want.prob.sum()) - 1.0) < 1e-15
    assert limit <= sq.BOUND_CEILING, (dev64, limit)
    assert f64.iterations == want.iterations      # the float64 restatement takes the same number of passes
    assert 0 <= want.iterations <= iter_max
    if want.iterations < iter_max:      # a stop: not a matter of rounding
        assert want.margin >= STOP_MARGIN, want.margin
    if c.threshold > 0 and iter_max:
        assert want.margin >= STOP_MARGIN      # nor is any "go on"
    if iter_max == 300 and c.threshold == sq.THRESHOLD:
        assert want.iterations < 300
    if want.zero_sum and c.sets.any(axis=1).all():
        # a set loses every member to the clamp.  A member that one evaluation clamps and another leaves at 1e-20 would
        # bring the set's whole weight back: every clamped entry must be below 0 by far more than rounding
        assert want.clamped > 0 and want.clamp_gap >= 1e-9 and f64.zero_sum == want.zero_sum
    assert not want.prob[~c.sets.any(axis=0)].any()      # alleles that no set names: exactly 0
    # the premise of the bound, tried on the reference itself: float64 runs in other summation orders stay within it
    for prob in sq.other_orders(c, iter_max):
        assert np.abs(prob.astype(LD) - want.prob).max() <= limit


def test_cases_reach_the_edges_they_name():
    r = sq.reference("clamp-random", 300)
    assert r.clamped > 0 and r.zero_sum > 0
    assert sq.reference("clamp-tiny", 1).clamped == 2      # alleles 0 and 1, in the first pass
    assert sq.reference("clamp-tiny", 1).clamp_gap > 1e-3
    assert np.array_equal(sq.reference("clamp-tiny", 1).prob[:2], np.zeros(2, dtype=LD))
    assert sq.reference("exact-identity", 300).vs_zero > 0
    for name, k in sq.RUNS:      # the first pass of every lane, round and allele-count case clamps or at least extrapolates
        if name.startswith(("rounds-", "alleles-", "members-", "sets-per-")) and k == 300 and name not in ("rounds-1", "alleles-1"):
            assert sq.reference(name, k).iterations >= 1, name
    one = sq.reference("threshold-1", 300)      # stops in pass 0 and returns the first step's p
    assert one.iterations == 0 and np.array_equal(one.prob, sq.reference("threshold-1", 0).prob) and one.margin >= STOP_MARGIN
    zero = sq.reference("threshold-0", 5)       # used up, without a clamp, never at an exact fixed point
    assert zero.iterations == 5 and zero.clamped == 0 and sq.reference("threshold-0", 5, np.float64).clamped == 0


# ------------------------------------------------------------------------------------------------ mutants
def _drop_member_16(c):
    S = c.sets.copy()
    for row in S:
        at = np.nonzero(row)[0]
        if len(at) > 16:
            row[at[16]] = False
    return S, c.weight


def _drop_set(u):
    def mutate(c):
        keep = np.arange(len(c.packed)) != u
        return c.sets[keep], c.weight[keep]
    return mutate


INPUT_MUTANTS = {"member 16 of every set dropped": _drop_member_16, "set 64 dropped": _drop_set(64), "set 32 dropped": _drop_set(32)}
MUTANTS = list(INPUT_MUTANTS) + list(sq.FAULTS)


@pytest.mark.parametrize("mutant", MUTANTS)
def test_every_mutant_leaves_the_bound_somewhere(mutant):
    """A wrong solver must not pass the GPU tests: each variant deviates from the true reference by more than the GPU
    bound of at least one run of the table (NaN counts as a deviation)."""
    caught = None
    for name, k in sorted(sq.RUNS, key=lambda run: run[1]):      # the short runs first: they are cheap
        c = sq.case(name)
        if mutant in INPUT_MUTANTS:
            S, w = INPUT_MUTANTS[mutant](c)
            if S.shape == c.sets.shape and np.array_equal(S, c.sets):
                continue
            if not len(S) or not w.sum():
                continue
            got = sq.squarem(S, w, k, c.threshold)
        else:
            got = sq.squarem(c.sets, c.weight, k, c.threshold, fault=mutant)
        want = sq.reference(name, k)
        _, limit = sq.bound(name, k)
        if not (np.abs(got.prob - want.prob) <= limit).all() or got.iterations != want.iterations:
            caught = (name, k)
            break
    assert caught is not None, f"no run of the table tells '{mutant}' from the reference"
    print(f"mutant '{mutant}' caught by {caught[0]} at iter_max {caught[1]}")
