"""No GPU: the host side of --call-dosage (kir_graph_amd/call_dosage.py) against the brute force of tests/dosage_reference.py
(math.fsum loops and np.longdouble), hand-derived exact cases, the rounding and tie rules, the text, the parser flag and the
refusals.

The bound of a table-driven case is the SQUAREM tests' (tests/test_gpu_squarem_edges.py): ``32 * max(dev64, 2^-52)`` around
the longdouble run at the solver's own pass count, dev64 = the distance of the reference's float64 (fsum) run from its
longdouble run.  The largest bound over CASES is 7.11e-15 (dev64 <= 1.4e-16 everywhere, so 2^-52 decides); none comes near the ceiling of 1e-9
(``dosage_reference.BOUND_CEILING``), which is asserted."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import dosage_reference as dr  # noqa: E402

from kir_graph_amd import call_dosage as cd  # noqa: E402
from kir_graph_amd import main as cli  # noqa: E402


def randomCase(seed, k, n_rows, copies, absent=0.0, share=None, elsewhere=0.3):
    """Rows drawn from K alleles with shares ``share``: zero on the drawn column; on another column 1 .. 3 with probability
    ``elsewhere``, else 0.  Sizes are kept small: the reference is Python loops."""
    rng = np.random.default_rng(seed)
    share = np.full(k, 1.0 / k) if share is None else np.asarray(share, dtype=np.float64)
    src = rng.choice(k, n_rows, p=share / share.sum())
    t = (rng.random((k, n_rows)) < elsewhere) * rng.integers(1, 4, (k, n_rows))
    t[src, np.arange(n_rows)] = 0
    t = t + rng.integers(0, 3, n_rows)                     # m1 > 0 on many rows
    t[rng.random((k, n_rows)) < absent] = 255
    return t.astype(np.uint8), list(copies)


CASES = {
    "two alleles": randomCase(1, 2, 3000, (1, 1)),
    "two alleles, 3 : 1": randomCase(2, 2, 4000, (1, 1), share=(3, 1)),
    "three alleles from (2, 1, 1)": randomCase(3, 3, 2000, (2, 1, 1), share=(1, 2, 1)),
    "four alleles with absent bytes": randomCase(4, 4, 600, (1, 1, 1, 1), absent=0.1, elsewhere=0.6),
    "eight alleles": randomCase(5, 8, 400, (1,) * 8, elsewhere=0.7),
    "sixteen alleles": randomCase(6, 16, 300, (1,) * 16, absent=0.05, elsewhere=0.8),
    "few rows": randomCase(7, 3, 40, (1, 1, 1)),
    "one allele nearly unsupported": randomCase(8, 3, 2000, (1, 1, 1), share=(10, 10, 0.05)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_solver_equals_the_reference(name):
    table, copies = CASES[name]
    k = len(copies)
    pats, counts, oor = dr.patterns(table, np.arange(k))
    assert len(counts) >= 2 and int(counts.sum()) + oor == table.shape[1]
    got = cd.solveDosage(pats, counts, copies)
    ref = dr.em(pats, counts, copies)
    assert ref.converged and ref.iterations < 5000                   # the reference alone converges
    assert got.converged and got.kkt <= 1e-10 and abs(got.iterations - ref.iterations) <= 1
    dev64, limit, want = dr.bound(pats, counts, copies, got.iterations)
    assert limit <= dr.BOUND_CEILING
    worst = max(float(abs(dr.LD(a) - b)) for a, b in zip(got.theta, want.theta))
    print(f"{name}: {len(counts)} patterns, {got.iterations} passes, dev64 {dev64:.3g}, bound {limit:.3g}, off by {worst:.3g}")
    assert worst <= limit
    assert abs(float(np.sum(got.theta)) - 1) <= 1e-12 and (got.theta >= 0).all()
    # the likelihoods: a sum of len(counts) terms of size |n log10 s|, each with a relative error of a few ulp
    scale = 16 * 2.0 ** -52 * float(np.sum(counts * np.abs(np.log10(cd.mixture(cd.patternWeights(pats), got.theta))))) + 1e-300
    assert abs(got.loglik_free - float(dr.loglik(pats, counts, got.theta, dtype=dr.LD))) <= scale
    assert abs(got.loglik_called - float(want.loglik_called)) <= 16 * 2.0 ** -52 * abs(float(want.loglik_called)) * len(counts)
    assert got.loglik_free >= got.loglik_called
    # the compositions: each is a candidate the brute force scores the same, and none of its neighbours scores higher
    cn = sum(copies)
    for total, (c, delta) in got.compositions.items():
        assert sum(c) == total and min(c) >= 0 and total in (cn - 1, cn, cn + 1)
        value = dr.loglik(pats, counts, [x / total for x in c])
        if value == -math.inf:                                       # a pattern with rows has no share at all
            assert delta == -math.inf
            continue
        assert abs((value - got.loglik_called) - delta) <= 1e-9 * max(1.0, abs(value))
        start = cd.largestRemainder(got.theta * total, total)
        for moves, other in cd.compositionCandidates(start, tuple(copies) if total == cn else None):
            assert dr.loglik(pats, counts, [x / total for x in other]) <= value + 1e-9 * max(1.0, abs(value))
    assert got.compositions[cn][1] >= 0
    assert set(got.compositions) == {t for t in (cn - 1, cn, cn + 1) if t >= 1}


def test_one_allele_is_share_one_without_a_pass():
    got = cd.solveDosage(np.zeros((1, 1), dtype=np.uint8), np.array([1234]), [2])
    assert got.theta.tolist() == [1.0] and got.iterations == 0 and got.converged and got.kkt == 0.0
    assert got.loglik_called == 0.0 and got.loglik_free == 0.0
    assert got.compositions == {1: ((1,), 0.0), 2: ((2,), 0.0), 3: ((3,), 0.0)}


@pytest.mark.parametrize("n1,n2", [(2000, 1000), (7, 3), (1, 999), (123457, 3)])
def test_private_reads_alone_give_their_ratio_after_one_pass(n1, n2):
    """(0, 255) x n1 and (255, 0) x n2 from (1/2, 1/2): s = 1/2 on every row, g_0 = (n1 / (1/2)) / N = 2 n1 / N rounded once,
    theta_0 = (1/2) g_0 = n1 / N, bit for bit."""
    pats = np.array([[0, 255], [255, 0]], dtype=np.uint8)
    got = cd.solveDosage(pats, np.array([n1, n2]), [1, 1])
    assert got.iterations == 1 and got.converged
    assert got.theta[0] == n1 / (n1 + n2) and got.theta[1] == n2 / (n1 + n2)
    assert got.kkt <= 2.0 ** -50


def test_shared_reads_do_not_move_the_optimum():
    pats = np.array([[0, 0], [0, 255], [255, 0]], dtype=np.uint8)
    got = cd.solveDosage(pats, np.array([5000, 2000, 1000]), [1, 1])
    assert got.converged and got.kkt <= 1e-10 and 1 < got.iterations < 5000
    # a rate of 5/8 per pass: the distance left at kkt <= 1e-10 is below 1e-10 / (1 - 5/8) x a small factor
    assert abs(got.theta[0] - 2 / 3) <= 1e-9 and abs(got.theta[1] - 1 / 3) <= 1e-9
    ref = dr.em(pats, [5000, 2000, 1000], [1, 1])
    assert ref.converged and abs(ref.iterations - got.iterations) <= 1


def test_called_two_to_one_is_its_own_best_composition():
    pats = np.array([[0, 255], [255, 0]], dtype=np.uint8)
    got = cd.solveDosage(pats, np.array([2000, 1000]), [2, 1])
    assert got.iterations == 0 and got.converged                    # the start is the optimum
    assert got.compositions[3] == ((2, 1), 0.0)
    assert got.compositions[2][1] < 0 and got.compositions[4][1] < 0
    assert got.loglik_free == got.loglik_called


def test_called_one_to_one_on_two_to_one_reads_points_at_one_more_copy():
    pats = np.array([[0, 255], [255, 0]], dtype=np.uint8)
    got = cd.solveDosage(pats, np.array([2000, 1000]), [1, 1])
    same, plus = got.compositions[2], got.compositions[3]
    assert same == ((1, 1), 0.0)
    assert plus[0] == (2, 1) and plus[1] > same[1]
    # l(2/3, 1/3) - l(1/2, 1/2) = 2000 log10(4/3) + 1000 log10(2/3)
    assert abs(plus[1] - (2000 * math.log10(4 / 3) + 1000 * math.log10(2 / 3))) <= 1e-9
    assert got.compositions[1][1] == -math.inf                      # one copy cannot explain the other allele's reads
    assert got.loglik_free - got.loglik_called == pytest.approx(plus[1], abs=1e-9)


def test_largest_remainder_and_ties():
    assert cd.largestRemainder(np.array([1.5, 1.5]), 3) == (2, 1)          # equal remainders: the lower column first
    assert cd.largestRemainder(np.array([0.5, 0.5, 1.0]), 2) == (1, 0, 1)
    assert cd.largestRemainder(np.array([0.2, 2.8]), 3) == (0, 3)
    assert cd.largestRemainder(np.array([2.0, 1.0]), 3) == (2, 1)
    assert cd.largestRemainder(np.array([0.4, 0.3, 0.3]), 1) == (1, 0, 0)
    cands = dict((c, m) for m, c in cd.compositionCandidates((2, 0, 1), (1, 1, 1)))
    assert cands == {(2, 0, 1): 0, (1, 1, 1): 1, (1, 0, 2): 1, (3, 0, 0): 1, (2, 1, 0): 1}
    assert dict((c, m) for m, c in cd.compositionCandidates((3, 0), (1, 2)))[(1, 2)] == 2
    # every composition scores the same (all rows shared): the rounding itself wins, zero moves
    pats, counts = np.zeros((1, 2), dtype=np.uint8), np.array([10])
    w = cd.patternWeights(pats)
    assert cd.bestComposition(w, counts, np.array([0.5, 0.5]), 3, None) == ((2, 1), 0.0)
    # two candidates one move away tie exactly above the rounding: the lexicographically smaller one
    pats = np.array([[0, 0, 255], [255, 255, 0]], dtype=np.uint8)
    w = cd.patternWeights(pats)
    c, _ = cd.bestComposition(w, np.array([9, 1]), np.array([0.0, 0.0, 1.0]), 2, None)
    assert c == (0, 1, 1)


def test_tied_alleles_keep_their_starting_ratio():
    """Columns 0 and 2 are equal on every row: only theta_0 + theta_2 is identified."""
    rng = np.random.default_rng(3)
    table, _ = randomCase(11, 2, 3000, (1, 1), share=(3, 1))
    table = np.stack([table[0], table[1], table[0]])
    pats, counts, _ = dr.patterns(table, np.arange(3))
    assert cd.tiedColumns(pats, 3) == [[2], [], [0]]
    got = cd.solveDosage(pats, counts, [2, 1, 1])
    assert got.converged and abs(got.theta[0] / got.theta[2] - 2) <= 1e-12
    pair = cd.solveDosage(*dr.patterns(table[:2], np.arange(2))[:2], [3, 1])
    assert abs(got.theta[0] + got.theta[2] - pair.theta[0]) <= 1e-9 and abs(got.theta[1] - pair.theta[1]) <= 1e-9
    del rng


def entryOf(pats, counts, copies, names, oor=0, scope="all"):
    sol = cd.solveDosage(pats, counts, copies)
    cn, tied = sum(copies), cd.tiedColumns(pats, len(copies))
    alleles = [cd.DosageAllele(names[j], copies[j], float(sol.theta[j]), float(sol.theta[j]) * cn, [names[i] for i in tied[j]])
               for j in range(len(copies))]
    sets = [([(names[j], c[j]) for j in range(len(copies))], d) if t in sol.compositions else None
            for t in (cn - 1, cn, cn + 1) for c, d in [sol.compositions.get(t, ((), 0.0))]]
    return cd.CallDosage(cn=cn, reads=int(np.sum(counts)) + oor, out_of_range=oor, patterns=pats, counts=np.asarray(counts),
                         iterations=sol.iterations, converged=sol.converged, kkt=sol.kkt, loglik_called=sol.loglik_called,
                         loglik_free=sol.loglik_free, alleles=alleles, minus=sets[0], same=sets[1], plus=sets[2], scope=scope)


def test_text():
    pats = np.array([[0, 255], [255, 0]], dtype=np.uint8)
    a = entryOf(pats, np.array([2000, 1000]), [1, 1], ["G*001", "G*002"], oor=5)
    b = entryOf(np.zeros((1, 1), dtype=np.uint8), np.array([40]), [1], ["H*001"], scope="candidates")
    empty = cd.CallDosage(cn=2, reads=7, out_of_range=7, patterns=np.zeros((0, 1), dtype=np.uint8), counts=np.zeros(0, dtype=np.int64),
                          iterations=None, converged=None, kkt=None, loglik_called=None, loglik_free=None,
                          alleles=[cd.DosageAllele("J*001", 2, None, None)])
    tied = entryOf(np.array([[0, 0], [1, 1]], dtype=np.uint8), np.array([5, 5]), [1, 1], ["K*001", "K*002"])
    text = cd.callDosageText({"G": a, "H": b, "J": empty, "K": tied})
    lines = text.split("\n")
    assert text.endswith("\n") and lines[0].split("\t") == cd.CALL_DOSAGE_COLUMNS and len(lines) == 1 + 2 + 1 + 1 + 2 + 1
    rows = [line.split("\t") for line in lines[1:-1]]
    assert all(len(r) == len(cd.CALL_DOSAGE_COLUMNS) == 22 for r in rows)
    g0, g1, h, j, k0, k1 = rows
    assert g0[:7] == ["G", "2", "3005", "5", "2", "1", "1"] and g0[:10] == g1[:10] and g0[15:] == g1[15:]
    assert [float(g0[8]), float(g0[9])] == [a.loglik_called, a.loglik_free] and float(g0[7]) == a.kkt
    assert g0[10:12] == ["G*001", "1"] and float(g0[12]) == 2000 / 3000 and float(g0[13]) == 2 * (2000 / 3000) and g0[14] == ""
    assert g1[10:12] == ["G*002", "1"] and float(g1[12]) == 1000 / 3000
    assert g0[15] == "G*001:1,G*002:0" and g0[16] == "-inf"
    assert g0[17] == "G*001:1,G*002:1" and g0[18] == "0.0"
    assert g0[19] == "G*001:2,G*002:1" and float(g0[20]) == a.plus[1] and g0[21] == "all"
    assert h[:7] == ["H", "1", "40", "0", "1", "0", "1"] and h[12:15] == ["1.0", "1.0", ""]
    assert h[15:17] == ["", ""] and h[17:] == ["H*001:1", "0.0", "H*001:2", "0.0", "candidates"]
    assert j == ["J", "2", "7", "7", "0", "", "", "", "", "", "J*001", "2", "", "", "", "", "", "", "", "", "", "all"]
    assert k0[14] == "K*002" and k1[14] == "K*001" and float(k0[12]) == 0.5
    assert cd.callDosageText({}) == "\t".join(cd.CALL_DOSAGE_COLUMNS) + "\n"


def test_sorted_patterns_have_one_order():
    pats = np.array([[1, 0, 9] + [0] * 13, [0, 255, 9] + [0] * 13, [0, 3, 9] + [0] * 13, [0, 3, 1] + [0] * 13], dtype=np.uint8)
    got_p, got_n = cd.sortedPatterns(pats, np.array([1, 2, 3, 4]), 3)
    assert got_p.tolist() == [[0, 3, 1], [0, 3, 9], [0, 255, 9], [1, 0, 9]] and got_n.tolist() == [4, 3, 2, 1]
    got_p, got_n = cd.sortedPatterns(np.zeros((0, 16), dtype=np.uint8), np.zeros(0, dtype=np.int64), 2)
    assert got_p.shape == (0, 2) and len(got_n) == 0


def test_parser_takes_the_call_dosage_flag():
    base = ["--step-skip-extraction", "--alignment", "s.sam"]
    args = cli.createParser().parse_args(base)
    assert args.call_dosage is False and cli.callReportArgs(args, report="call_dosage") == {}
    args = cli.createParser().parse_args(base + ["--allele-strategy", "exonfirst", "--call-dosage"])
    assert cli.callReportArgs(args, report="call_dosage") == {"call_dosage": True}
    # it combines with the fit report and the copy-number bootstrap's sibling flags
    args = cli.createParser().parse_args(base + ["--call-dosage", "--call-fit", "--call-alternatives"])
    assert cli.callReportArgs(args, report="call_dosage") == {"call_dosage": True}
    assert cli.callReportArgs(args, report="call_fit") == {"call_fit": True, "call_fit_extra": 3}


@pytest.mark.parametrize("strategy", ["em", "report"])
def test_command_line_refuses_the_em_strategy(strategy, monkeypatch):
    for name in ("GK_WAIT_POLICY", "GK_SAMPLE_LANES", "GK_SEARCH_SLOTS"):      # main() sets its defaults: put them back
        monkeypatch.setenv(name, os.environ.get(name, "1"))
    args = cli.createParser().parse_args(["--step-skip-extraction", "--alignment", "s.sam", "--allele-strategy", strategy,
                                          "--call-dosage"])
    with pytest.raises(ValueError, match="--call-dosage"):
        cli.main(args)


def test_factory_refusals():
    from kir_graph_amd.kir_typing import TypingWithReport, selectKirTypingModel
    for method in ("em", "report"):
        with pytest.raises(ValueError, match="call_dosage"):
            selectKirTypingModel(method, "nothing.json", call_dosage=True)
    with pytest.raises(TypeError):
        TypingWithReport("nothing.json", call_dosage=True)


def test_write_call_dosage(tmp_path):
    pats = np.array([[0, 255], [255, 0]], dtype=np.uint8)
    entry = entryOf(pats, np.array([20, 10]), [1, 1], ["G*001", "G*002"])
    [path] = cli.writeCallReport("call_dosage", str(tmp_path / "s"), {"G": entry})
    assert path == str(tmp_path / "s") + ".dosage.tsv"
    assert open(path).read() == cd.callDosageText({"G": entry})
