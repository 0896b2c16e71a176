"""Plain weighted SQUAREM solver in numpy ``longdouble`` (helper of the solver tests, not a test), and the case table
that tests/test_squarem_reference_host.py and tests/test_gpu_squarem_edges.py share.

``squarem`` restates the reference project's ``hisatEMnp`` (typing_em.py 107-188) line for line, on DISTINCT sets with
weights instead of on reads: ``w`` equal reads are ``w`` equal rows of the reference's matrix, so their sum over the rows
is ``w`` times one row.  It is dense, knows nothing of lanes, rounds or workgroups, and is never handed to the GPU.  Called
with ``dtype=np.float64`` the same code is the float64 restatement whose distance from the longdouble run sets the
tolerance of the GPU tests.

``iterations`` is defined as the kernel defines it (csrc/gk_squarem.h): the number, from 0, of the pass whose difference met
the threshold, or ``iter_max`` when no pass did.  (A Python ``for`` variable would be left at ``iter_max - 1`` then.)
"""
from __future__ import annotations

from functools import lru_cache
from typing import NamedTuple

import numpy as np

assert np.finfo(np.longdouble).eps < 1e-18, "the reference needs a long double wider than float64"

ITER_MAXES = (0, 1, 2, 3, 300)
THRESHOLD = 1e-4
BOUND_CEILING = 1e-9      # no case's bound may exceed this


class Run(NamedTuple):
    prob: np.ndarray          # [n_allele], in the dtype of the run
    iterations: int
    clamped: int              # entries of the extrapolated point that were below 0 and set to 0
    zero_sum: int             # (pass, set) pairs: a set of positive weight whose members summed to 0 in a step of the pass
    vs_zero: int              # passes that skipped the extrapolation because vs == 0
    margin: float             # smallest |d - threshold| / threshold over the passes (inf without a pass or a threshold)
    clamp_gap: float          # smallest |x| / (|p| + |2 r g| + |v g^2|) of an extrapolated entry x = p - 2 r g + v g^2 before
                              # the clamp: how far the sign of every x is from a matter of rounding (inf without one)


# The deliberately wrong variants of the mutant check.  Nothing else may pass ``fault``.
FAULTS = ("total_without_allele_64", "no_clamp", "zero_sum_shared", "zero_sum_unguarded", "extrapolate_always", "return_p1")


def squarem(sets, weight, iter_max: int = 300, diff_threshold: float = THRESHOLD, dtype=np.longdouble,
            fault: str | None = None) -> Run:
    """``sets``: bool [n_sets][n_allele]; ``weight`` [n_sets]."""
    assert fault is None or fault in FAULTS
    S = np.asarray(sets, dtype=bool).astype(dtype)
    w = np.asarray(weight).astype(dtype)
    n_sets, n_allele = S.shape
    zero_seen = np.zeros(n_sets, dtype=bool)

    def getNextProb(p):
        a = p * S
        b = a.sum(axis=1)[:, None]
        zero_seen[:] |= (b[:, 0] == 0) & (w > 0)
        if fault == "zero_sum_unguarded":
            with np.errstate(invalid="ignore", divide="ignore"):
                a = a / b
        else:
            a = np.divide(a, b, out=np.zeros(a.shape, dtype=dtype), where=b != 0)
        if fault == "zero_sum_shared":      # what equal tiny abundances would give: a share of 1 / members each
            n = S.sum(axis=1)[:, None]
            a = np.where((b == 0) & (n > 0), S / np.maximum(n, 1), a)
        a = a * w[:, None]
        a = a.sum(axis=0)
        total = a.sum() - a[64] if fault == "total_without_allele_64" and n_allele > 64 else a.sum()
        return a / total

    clamped = vs_zero = zero_sum = 0
    margin = clamp_gap = float("inf")
    prob = getNextProb(np.ones(n_allele, dtype=dtype))
    iterations = iter_max
    for iters in range(iter_max):
        zero_seen[:] = False
        prob_next = getNextProb(prob)
        prob_next2 = getNextProb(prob_next)
        r = prob_next - prob
        v = prob_next2 - prob_next - r
        r_sum = (r ** 2).sum()
        v_sum = (v ** 2).sum()
        if v_sum > 0.0 or fault == "extrapolate_always":
            with np.errstate(invalid="ignore", divide="ignore"):
                g = -np.sqrt(r_sum / v_sum)
                prob_next3 = prob - r * g * 2 + v * g ** 2
                size = np.abs(prob) + np.abs(r * g * 2) + np.abs(v * g ** 2)
            clamped += int((prob_next3 < 0).sum())
            if (size > 0).any():
                clamp_gap = min(clamp_gap, float((np.abs(prob_next3[size > 0]) / size[size > 0]).min()))
            if fault != "no_clamp":
                prob_next3 = np.maximum(prob_next3, 0)
            prob_next = getNextProb(prob_next3)
        else:
            vs_zero += 1
        zero_sum += int(zero_seen.sum())
        diff = np.abs(prob - prob_next).sum()
        if diff_threshold > 0:
            margin = min(margin, float(abs(diff - diff_threshold) / diff_threshold))
        if diff <= diff_threshold:
            iterations = iters
            if fault == "return_p1":
                prob = prob_next
            break
        prob = prob_next
    return Run(prob, iterations, clamped, zero_sum, vs_zero, margin, clamp_gap)


# ------------------------------------------------------------------------------------------------ packing
def pack(bits: np.ndarray) -> np.ndarray:
    """bool [n_sets][words * 32] -> uint32 [n_sets][words], bit ``a % 32`` of word ``a // 32`` = allele ``a``."""
    assert bits.shape[1] % 32 == 0
    return np.ascontiguousarray(np.packbits(bits.astype(np.uint8), axis=1, bitorder="little").view(np.uint32))


def unpack(packed: np.ndarray, n_allele: int) -> np.ndarray:
    """uint32 [n_sets][words] -> bool [n_sets][n_allele]: the bits past ``n_allele`` name nobody."""
    return np.unpackbits(np.ascontiguousarray(packed).view(np.uint8), axis=1, bitorder="little")[:, :n_allele].astype(bool)


def ascending(packed: np.ndarray) -> np.ndarray:
    """The order that makes the rows ascending, word 0 first (``np.unique(axis=0)``'s)."""
    return np.lexsort(packed.T[::-1])


class Case(NamedTuple):
    name: str
    group: str
    packed: np.ndarray        # uint32 [n_sets][words]: ascending, distinct, non-empty -- as gk_em_run takes them
    weight: np.ndarray        # float64 [n_sets]
    n_allele: int
    iter_maxes: tuple
    threshold: float
    exact: np.ndarray | None = None      # hand-derived abundances, met bit for bit at iterations == 0

    @property
    def sets(self) -> np.ndarray:
        return unpack(self.packed, self.n_allele)


def _case(name, group, bits, weight, n_allele, iter_maxes=ITER_MAXES, threshold=THRESHOLD, exact=None) -> Case:
    """``bits``: bool [n_sets][words * 32], ghost bits (columns past ``n_allele``) included."""
    packed = pack(np.asarray(bits, dtype=bool))
    order = ascending(packed)
    packed, weight = np.ascontiguousarray(packed[order]), np.ascontiguousarray(np.asarray(weight, dtype=np.float64)[order])
    assert packed.any(axis=1).all(), name
    assert len(np.unique(packed, axis=0)) == len(packed), name
    assert 1 <= n_allele <= packed.shape[1] * 32 and len(weight) == len(packed)
    return Case(name, group, packed, weight, n_allele, tuple(iter_maxes), threshold,
                None if exact is None else np.asarray(exact, dtype=np.float64))


def _random_bits(rng, n_sets: int, n_allele: int, density: float, words: int | None = None) -> np.ndarray:
    """``n_sets`` distinct non-empty random rows over ``n_allele`` alleles."""
    words = words or (n_allele + 31) // 32
    rows = np.zeros((0, words * 32), dtype=bool)
    while len(rows) < n_sets:
        new = np.zeros((2 * n_sets + 8, words * 32), dtype=bool)
        new[:, :n_allele] = rng.random((len(new), n_allele)) < density
        rows = np.concatenate([rows, new[new.any(axis=1)]])
        _, first = np.unique(pack(rows), axis=0, return_index=True)
        rows = rows[np.sort(first)]
    return rows[:n_sets]


def _sized_row(rng, n_allele: int, size: int, width: int) -> np.ndarray:
    row = np.zeros(width, dtype=bool)
    row[rng.choice(n_allele, size=size, replace=False)] = True
    return row


# ------------------------------------------------------------------------------------------------ the case table
# The seeds are chosen so that the reference ALONE meets the conditions of the runs (stop margin >= 0.05, the float64
# restatement stops in the same pass, its runs in other summation orders and the oracle on the expanded reads stay within
# the bound) and reaches the edge a case names; tests/test_squarem_reference_host.py asserts every one of them.  No seed
# was chosen by what a kernel gives.
def _rounds(n_sets: int, seed: int) -> Case:
    rng = np.random.default_rng(seed)
    bits = _random_bits(rng, n_sets, 33, 0.3, words=2)
    return _case(f"rounds-{n_sets}", "rounds of sets", bits, rng.integers(1, 20, n_sets), 33)


def _members(seed: int) -> Case:
    rng = np.random.default_rng(seed)
    sizes = [1, 1, 15, 15, 16, 16, 17, 17, 31, 31, 32, 32, 33, 33, 48, 48, 511, 511, 512]
    bits = np.array([_sized_row(rng, 512, k, 512) for k in sizes])
    return _case("members-per-set", "members per set", bits, rng.integers(1, 10, len(sizes)), 512)


SETS_PER_ALLELE = {0: 200, 1: 1, 2: 15, 3: 16, 4: 17, 5: 33}


def _sets_per_allele(seed: int) -> Case:
    rng = np.random.default_rng(seed)
    bits = np.zeros((200, 64), dtype=bool)
    bits[:, 6:40] = rng.random((200, 34)) < 0.2
    for a, k in SETS_PER_ALLELE.items():
        bits[rng.choice(200, size=k, replace=False), a] = True
    return _case("sets-per-allele", "sets per allele", bits, rng.integers(1, 10, 200), 40)


def _alleles(n_allele: int, seed: int) -> Case:
    """Up to 40 sets over ``n_allele`` alleles; where the last word has room, every third set also carries bits past
    ``n_allele`` and one set of positive weight carries nothing else (its member list is empty)."""
    rng = np.random.default_rng(seed)
    words = (n_allele + 31) // 32
    width = words * 32
    n_sets = 40
    bits = np.zeros((n_sets, width), dtype=bool)
    bits[:, :n_allele] = rng.random((n_sets, n_allele)) < max(0.1, min(0.6, 4.0 / n_allele))
    for u in np.nonzero(~bits.any(axis=1))[0]:
        bits[u, rng.integers(0, n_allele)] = True
    if width > n_allele:
        ghost = rng.random((n_sets, width - n_allele)) < 0.5
        ghost[:, 0] |= ~ghost.any(axis=1)
        bits[::3, n_allele:] = ghost[::3]
        bits[1, :n_allele] = False      # positive weight, ghost bits only
        bits[1, n_allele:] = ghost[1]
    _, first = np.unique(pack(bits), axis=0, return_index=True)
    bits = bits[np.sort(first)]
    return _case(f"alleles-{n_allele}", "allele counts", bits, rng.integers(1, 20, len(bits)), n_allele)


def _scale_row(n_sets: int, seed: int) -> Case:
    """Thousands of sets stay narrow (24 alleles); the reads favour two alleles, so the abundances are well determined."""
    rng = np.random.default_rng(seed)
    bits = np.zeros((0, 32), dtype=bool)
    while len(bits) < n_sets:
        new = np.zeros((3 * n_sets, 32), dtype=bool)
        new[:, :24] = rng.random((len(new), 24)) < 0.15
        truth = rng.random(len(new)) < 0.6
        new[truth, 3] = True
        new[~truth, 7] = True
        bits = np.concatenate([bits, new])
        _, first = np.unique(pack(bits), axis=0, return_index=True)
        bits = bits[np.sort(first)]
    return _case(f"scale-row-{n_sets}", "scale row in LDS or HBM", bits[:n_sets], rng.integers(1, 3, n_sets), 24)


def _weights(kind: str, seed: int) -> Case:
    rng = np.random.default_rng(seed)
    bits = _random_bits(rng, 65, 33, 0.3, words=2)
    if kind == "zeros":
        w = rng.integers(1, 20, 65).astype(np.float64)
        w[rng.choice(65, size=20, replace=False)] = 0.0
    elif kind == "fractions":
        w = np.where(rng.random(65) < 0.5, 0.25, 1.0 / 3.0)
    elif kind == "mixed":
        w = np.where(rng.random(65) < 0.25, 100000.0, 1.0)
    else:
        w = rng.integers(1, 20, 65).astype(np.float64)
        w[rng.integers(0, 65)] = 2.0 ** 31
    return _case(f"weights-{kind}", "weights", bits, w, 33)


def _clamp_random(seed: int) -> Case:
    """Sparse sets and a quarter of them a thousand times as heavy as the rest: the alleles that only light sets name are
    carried below 0 by the extrapolation, and light sets lose every member."""
    rng = np.random.default_rng(seed)
    bits = _random_bits(rng, 200, 129, 0.05)
    return _case("clamp-random", "clamp and zero-sum sets", bits, np.where(rng.random(200) < 0.25, 1000.0, 1.0), 129)


def _clamp_tiny() -> Case:
    """Alleles 0 and 1 are seen only together with allele 2, which has reads of its own and shares others with allele 3:
    the first extrapolation carries alleles 0 and 1 below 0 (by 4e-3 of the terms' size, no matter of rounding)."""
    bits = np.zeros((3, 32), dtype=bool)
    bits[0, :3] = True
    bits[1, 2] = True
    bits[2, 2:4] = True
    return _case("clamp-tiny", "clamp and zero-sum sets", bits, [2.0, 1.0, 1.0], 4)


def _threshold(kind: str, seed: int) -> Case:
    rng = np.random.default_rng(seed)
    if kind == "one":      # stops in pass 0 and returns the first step's p
        bits = _random_bits(rng, 65, 33, 0.3, words=2)
        return _case("threshold-1", "thresholds", bits, rng.integers(1, 20, 65), 33, iter_maxes=(300,), threshold=1.0)
    # never stops: iter_max is used up.  Every allele has reads of its own, so nothing is clamped on the way.
    bits = np.zeros((65, 64), dtype=bool)
    bits[np.arange(33), np.arange(33)] = True
    bits[33:] = _random_bits(rng, 32, 33, 0.3, words=2)
    _, first = np.unique(pack(bits), axis=0, return_index=True)
    bits = bits[np.sort(first)]
    return _case("threshold-0", "thresholds", bits, rng.integers(1, 20, len(bits)), 33, iter_maxes=(5,), threshold=0.0)


def _exact_cases() -> list[Case]:
    eye = np.zeros((4, 32), dtype=bool)
    eye[np.arange(4), np.arange(4)] = True
    all512 = np.ones((1, 512), dtype=bool)
    one64 = np.ones((1, 64), dtype=bool)
    one = np.zeros((1, 32), dtype=bool)
    one[0, 0] = True
    return [
        _case("exact-identity", "exact", eye, [1, 1, 2, 4], 4, exact=[.125, .125, .25, .5]),
        _case("exact-512", "exact", all512, [3], 512, exact=np.full(512, 1 / 512)),
        _case("exact-64", "exact", one64, [1], 64, exact=np.full(64, 1 / 64)),
        _case("exact-1", "exact", one, [1], 1, exact=[1.0]),
        # alleles inside n_allele that no set names: exactly 0
        _case("exact-unnamed", "exact", eye, [1, 1, 2, 4], 30, exact=np.concatenate([[.125, .125, .25, .5], np.zeros(26)])),
    ]


ROUND_SETS = (1, 31, 32, 33, 63, 64, 65, 129)
ALLELE_COUNTS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 511, 512)
SCALE_SETS = (8191, 8192, 8193)
# case name -> seed, where the default (below) did not meet the conditions
SEEDS: dict[str, int] = {"rounds-32": 136, "rounds-63": 164, "rounds-64": 168, "rounds-65": 168, "alleles-33": 435,
                         "alleles-64": 465, "weights-zeros": 602, "weights-fractions": 602, "weights-mixed": 606,
                         "clamp-random": 702, "threshold-1": 808}


def _seed(name: str, default: int) -> int:
    return SEEDS.get(name, default)


@lru_cache(maxsize=None)
def cases() -> tuple[Case, ...]:
    out = _exact_cases()
    out += [_rounds(n, _seed(f"rounds-{n}", 100 + n)) for n in ROUND_SETS]
    out += [_members(_seed("members-per-set", 200)), _sets_per_allele(_seed("sets-per-allele", 300))]
    out += [_alleles(n, _seed(f"alleles-{n}", 400 + n)) for n in ALLELE_COUNTS]
    out += [_scale_row(n, _seed(f"scale-row-{n}", 500 + n % 10)) for n in SCALE_SETS]
    out += [_weights(k, _seed(f"weights-{k}", 600 + i)) for i, k in enumerate(("zeros", "fractions", "mixed", "two31"))]
    out += [_clamp_random(_seed("clamp-random", 700)), _clamp_tiny()]
    out += [_threshold("one", _seed("threshold-1", 800)), _threshold("zero", _seed("threshold-0", 801))]
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def case(name: str) -> Case:
    return next(c for c in cases() if c.name == name)


CASE_NAMES = tuple(c.name for c in cases())
RUNS = tuple((c.name, k) for c in cases() for k in c.iter_maxes)      # every (case, iter_max) of the table


@lru_cache(maxsize=None)
def reference(name: str, iter_max: int, dtype=np.longdouble) -> Run:
    """The run of a case of the table, computed once per process and shared; callers leave it unchanged."""
    c = case(name)
    run = squarem(c.sets, c.weight, iter_max, c.threshold, dtype)
    run.prob.setflags(write=False)
    return run


def bound(name: str, iter_max: int) -> tuple[float, float]:
    """(dev64, bound) of a run: ``dev64`` is the largest absolute deviation of the float64 run of the reference code from
    its longdouble run; a float64 evaluation of the same formulas in another summation order (the kernel's: a tree over 16
    lanes, against numpy's row-sequential sums, over up to 8193 terms) must lie within ``32 * max(dev64, 2^-52)``."""
    want, f64 = reference(name, iter_max), reference(name, iter_max, np.float64)
    dev64 = float(np.abs(f64.prob.astype(np.longdouble) - want.prob).max())
    return dev64, 32.0 * max(dev64, 2.0 ** -52)


def other_orders(c: Case, iter_max: int) -> list[np.ndarray]:
    """The float64 run of the reference code on the same sets and alleles in three other orders (both reversed; two seeded
    shuffles), brought back to the case's allele order: float64 evaluations of the same formulas that differ from the
    plain one in the order of their sums only -- what the bound says of the kernel, tried on the reference itself."""
    out = []
    for which in range(3):
        if which == 0:
            rows, cols = np.arange(len(c.packed))[::-1], np.arange(c.n_allele)[::-1]
        else:
            rng = np.random.default_rng(which)
            rows, cols = rng.permutation(len(c.packed)), rng.permutation(c.n_allele)
        run = squarem(c.sets[rows][:, cols], c.weight[rows], iter_max, c.threshold, np.float64)
        prob = np.empty(c.n_allele, dtype=np.float64)
        prob[cols] = run.prob
        out.append(prob)
    return out
