"""Alternatives of each called allele, host side (no GPU): the restatement of tests/callswap_reference.py on a table worked
out by hand and its identities with the fit report's restatement, the class rule, the listing order, the ``resolved`` rule,
the ``.alternatives.tsv`` text, command-line flags and factory refusals."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import callfit_reference as fr  # noqa: E402
import callswap_reference as sr  # noqa: E402

from kir_graph_amd import main as cli  # noqa: E402
from kir_graph_amd.call_alternatives import (CALL_ALTERNATIVES_COLUMNS, CALL_ALTERNATIVES_HEADER, Alternative,  # noqa: E402
                                             CallAlternatives, CalledAlternatives, alternativesFromSums, callAlternativesText,
                                             classOf, nameFields, rankAlternatives, resolvedName)

# [column][row]: columns 2 and 0 are called (in that order), 1 and 3 are not (the table of tests/test_call_fit_host.py)
TABLE = np.array([[0, 1, 2, 0, 255, 30],
                  [0, 0, 0, 0, 0, 0],
                  [0, 0, 5, 1, 255, 40],
                  [9, 9, 9, 9, 9, 9]])


def test_restatement_on_a_hand_built_table():
    got = sr.swaps(TABLE, [2, 0])
    # m1 = (0, 0, 2, 0, 255, 30), M = 287, one row out of range.
    # k = 0 (column 2), rest = column 0 = (0, 1, 2, 0, 255, 30):
    #   a = 0: new = rest,            new - m1 = (0, 1, 0, 0, 0, 0)          loss 1 on 1 row
    #   a = 1: new = 0,               new - m1 = (0, 0, -2, 0, -255, -30)    gain 287 on 3 rows
    #   a = 2: the allele itself: new = m1
    #   a = 3: new = (0, 1, 2, 0, 9, 9),  new - m1 = (0, 1, 0, 0, -246, -21)   loss 1 on 1 row, gain 267 on 2 rows
    # k = 1 (column 0), rest = column 2 = (0, 0, 5, 1, 255, 40):
    #   a = 2: new = rest,            new - m1 = (0, 0, 3, 1, 0, 10)         loss 14 on 3 rows
    #   a = 3: new = (0, 0, 5, 1, 9, 9),  new - m1 = (0, 0, 3, 1, -246, -21)   loss 4 on 2 rows, gain 267 on 2 rows
    assert got["m"] == 287 and got["out_of_range"] == 1
    assert got["loss"].tolist() == [[1, 0, 0, 1], [0, 0, 14, 4]]
    assert got["rows_for"].tolist() == [[1, 0, 0, 1], [0, 0, 3, 2]]
    assert got["gain"].tolist() == [0, 287, 0, 267]
    assert got["rows_against"].tolist() == [0, 3, 0, 2]
    assert got["delta"].tolist() == [[1, -287, 0, -266], [0, -287, 14, -263]]
    # the literal form of one swap gives the same
    for k in range(2):
        for a in range(4):
            assert sr.swapOne(TABLE, [2, 0], k, a) == (got["loss"][k, a], got["rows_for"][k, a], got["gain"][a],
                                                       got["rows_against"][a], got["delta"][k, a])
    # the order of the listed columns moves the rows of k and nothing else
    other = sr.swaps(TABLE, [0, 2])
    assert other["loss"].tolist() == got["loss"][::-1].tolist() and other["gain"].tolist() == got["gain"].tolist()
    # one called column: the rest is 255
    one = sr.swaps(TABLE, [3])
    assert one["m"] == 54 and one["loss"].tolist() == [[246 + 21, 0, 246 + 31, 0]] and one["rows_for"].tolist() == [[2, 0, 2, 0]]
    assert one["gain"].tolist() == [9 + 8 + 7 + 9, 54, 9 + 9 + 4 + 8, 0]


def test_identities_with_the_fit_report():
    rng = np.random.default_rng(5)
    for k_n in (1, 2, 3, 5):
        table = rng.integers(0, 4, (9, 200))
        table[:, :7] = rng.choice([0, 100, 254, 255], (9, 7))
        cols = rng.permutation(9)[:k_n]
        got = sr.swaps(table, cols)
        _, m, per_col, m1 = fr.profile(table, cols)
        assert got["m"] == m
        for k, c in enumerate(cols):
            # a == k gives zeros
            assert got["loss"][k, c] == got["rows_for"][k, c] == got["gain"][c] == got["rows_against"][c] == 0
            for j, other in enumerate(cols):
                if j != k:      # a swap to another called column: nothing gained, the loss is the fit report's `only`
                    assert got["gain"][other] == 0 and got["loss"][k, other] == per_col[k, 2]
        assert np.array_equal(got["gain"], m - fr.extra(table, m1))
        state = sr.rowState(table, cols)
        assert np.array_equal(state[0], m1) and ((state[2] == 255) | (state[1] > state[0]) | (k_n == 1)).all()


def test_class_rule():
    assert classOf(0, 3, 1) == "better" and classOf(5, 6, 0) == "better"
    assert classOf(0, 0, 0) == "identical"
    assert classOf(4, 4, 0) == "balanced"
    assert classOf(1, 0, 1) == "near" and classOf(7, 5, 2) == "near"
    assert classOf(1, 0, 0) is None and classOf(7, 4, 2) is None


def test_listing_order_and_truncation():
    #               0   1   2   3   4   5   6   7   8   9
    loss = np.array([0, 5, 0, 2, 0, 9, 1, 2, 0, 3])
    gain = np.array([0, 9, 0, 2, 3, 2, 0, 0, 0, 7])
    # delta          0  -4   0   0  -3   7   1   2   0  -4 ; column 2 is the called one
    counts, listed = rankAlternatives(loss, gain, 2, 2, 20)
    assert counts == {"better": 3, "identical": 2, "balanced": 1, "near": 2}
    assert listed == [(1, "better"), (9, "better"), (4, "better"), (0, "identical"), (8, "identical"), (3, "balanced"),
                      (6, "near"), (7, "near")]
    counts, listed = rankAlternatives(loss, gain, 2, 1, 20)
    assert counts["near"] == 1 and listed[-1] == (6, "near") and len(listed) == 7
    counts, listed = rankAlternatives(loss, gain, 2, 0, 20)
    assert counts["near"] == 0 and len(listed) == 6
    # truncation keeps the order and the full counts
    counts, listed = rankAlternatives(loss, gain, 2, 2, 4)
    assert counts == {"better": 3, "identical": 2, "balanced": 1, "near": 2}
    assert listed == [(1, "better"), (9, "better"), (4, "better"), (0, "identical")]
    # the called column itself is never its own alternative
    assert rankAlternatives(np.zeros(3), np.zeros(3), 1, 0, 20) == ({"better": 0, "identical": 2, "balanced": 0, "near": 0},
                                                                   [(0, "identical"), (2, "identical")])


def test_resolved_rule():
    assert nameFields("KIR2DL1*0030201") == ("KIR2DL1*", "0030201") and nameFields("KIR2DL1*003") == ("KIR2DL1*", "003")
    for odd in ("KIR2DL1*00", "KIR2DL1*00302011", "KIR2DL1*0030201N", "KIR2DL1", "*003", "KIR2DL1*003e"):
        assert nameFields(odd) is None, odd
    r = resolvedName
    assert r("KIR2DL1*0030201", []) == "KIR2DL1*0030201"                                    # no alternative: the full name
    assert r("KIR2DL1*0030201", ["KIR2DL1*0030202"]) == "KIR2DL1*00302"                     # the 7-digit field differs
    assert r("KIR2DL1*0030201", ["KIR2DL1*0030202", "KIR2DL1*00303"]) == "KIR2DL1*003"
    assert r("KIR2DL1*0030201", ["KIR2DL1*0030202", "KIR2DL1*0040101"]) == "KIR2DL1*"       # not even three digits
    assert r("KIR2DL1*0030201", ["KIR2DS1*0030201"]) == "KIR2DL1*"                          # another gene of the group
    assert r("KIR2DL1*00302", ["KIR2DL1*0030201"]) == "KIR2DL1*00302"                       # a short name keeps its fields
    assert r("KIR2DL1*0030201", ["KIR2DL1*00302"]) == "KIR2DL1*00302"
    assert r("KIR2DL1*0030201", ["KIR2DL1*003"]) == "KIR2DL1*003"
    assert r("KIR2DL1*003", ["KIR2DL1*00301"]) == "KIR2DL1*003" and r("KIR2DL1*003", ["KIR2DL1*004"]) == "KIR2DL1*"
    assert r("KIR2DL1*0030", ["KIR2DL1*0031"]) == "KIR2DL1*003"                             # four digits: the 3-digit field
    # a name that is not GENE* plus 3 to 7 digits is compared as a whole
    assert r("KIR2DL1*0030201", ["KIR2DL1*0030202e"]) == "KIR2DL1*"
    assert r("KIR2DL1*0030201N", ["KIR2DL1*0030202"]) == "KIR2DL1*" and r("KIR2DL1*0030201N", []) == "KIR2DL1*0030201N"
    assert r("backbone", ["other"]) == ""


def calls():
    swap = [Alternative("KIR2DL1*0030202", "identical", 0, 0, 0, 0, 0), Alternative("KIR2DL1*00401", "near", 1, 3, 2, 2, 1)]
    return {
        "KIR2DL1S1": CallAlternatives(cn=3, reads=1195, mismatches=1330, out_of_range=5, scope="all", alleles=[
            CalledAlternatives("KIR2DL1*0030201", 2, "KIR2DL1*00302", 0, 1, 0, 7, swap),
            CalledAlternatives("KIR2DS1*002", 1, "KIR2DS1*002", 0, 0, 0, 0, [])]),
        "KIR2DL2": CallAlternatives(cn=2, reads=566, mismatches=0, out_of_range=0, scope="candidates", alleles=[
            CalledAlternatives("KIR2DL2*003", 2, "KIR2DL2*", 1, 0, 0, 0, [Alternative("KIR2DL2*001", "better", -4, 1, 5, 1, 3)])]),
    }


def test_alternatives_file_bytes(tmp_path):
    [path] = cli.writeCallReport("call_alternatives", str(tmp_path / "s.pv"), calls())
    assert path.endswith("s.pv.alternatives.tsv")
    want = (CALL_ALTERNATIVES_HEADER +
            "gene\tcn\treads\tmismatches\tout_of_range\tscope\tallele\tcopies\tresolved\tn_better\tn_identical\tn_balanced\tn_near\t"
            "alternative\tclass\tdelta\tloss\tgain\trows_for\trows_against\n"
            "KIR2DL1S1\t3\t1195\t1330\t5\tall\tKIR2DL1*0030201\t2\tKIR2DL1*00302\t0\t1\t0\t7\tKIR2DL1*0030202\tidentical\t0\t0\t0\t0\t0\n"
            "KIR2DL1S1\t3\t1195\t1330\t5\tall\tKIR2DL1*0030201\t2\tKIR2DL1*00302\t0\t1\t0\t7\tKIR2DL1*00401\tnear\t1\t3\t2\t2\t1\n"
            "KIR2DL1S1\t3\t1195\t1330\t5\tall\tKIR2DS1*002\t1\tKIR2DS1*002\t0\t0\t0\t0\t\t\t\t\t\t\t\n"
            "KIR2DL2\t2\t566\t0\t0\tcandidates\tKIR2DL2*003\t2\tKIR2DL2*\t1\t0\t0\t0\tKIR2DL2*001\tbetter\t-4\t1\t5\t1\t3\n")
    assert open(path).read() == want == callAlternativesText(calls())
    head = CALL_ALTERNATIVES_HEADER.split("\n")
    assert len(head) == 3 and head[2] == "" and all(line.startswith("# ") for line in head[:2])
    assert "candidates" in head[0] and "out_of_range > 0" in head[1] and "bound" in head[1]
    assert CALL_ALTERNATIVES_COLUMNS == ["gene", "cn", "reads", "mismatches", "out_of_range", "scope", "allele", "copies",
                                         "resolved", "n_better", "n_identical", "n_balanced", "n_near", "alternative", "class",
                                         "delta", "loss", "gain", "rows_for", "rows_against"]
    assert callAlternativesText({}) == CALL_ALTERNATIVES_HEADER + "\t".join(CALL_ALTERNATIVES_COLUMNS) + "\n"


def test_report_from_the_sums_of_the_hand_built_table():
    got = sr.swaps(TABLE, [2, 0])
    names = ["KIR2DL1*0030201", "KIR2DL1*0030202", "KIR2DL1*00401", "KIR2DL1*0050101"]
    rep = alternativesFromSums(got["loss"], got["rows_for"], got["gain"], got["rows_against"], [2, 0], [names[2], names[0]],
                               [1, 2], lambda a: names[a], cn=3, reads=6, m=got["m"], out_of_range=got["out_of_range"],
                               scope="all", within=1, max_listed=1)
    assert (rep.cn, rep.reads, rep.mismatches, rep.out_of_range, rep.scope) == (3, 6, 287, 1, "all")
    first, second = rep.alleles
    # column 2: deltas 1 (near), -287, -266 (better)
    assert (first.allele, first.copies, first.n_better, first.n_identical, first.n_balanced, first.n_near) == (names[2], 1, 2, 0, 0, 1)
    assert first.listed == [Alternative(names[1], "better", -287, 0, 287, 0, 3)]            # one listed, all counted
    assert first.resolved == "KIR2DL1*"                            # every better alternative counts, listed or not
    # column 0: deltas -287, 14 (beyond), -263
    assert (second.n_better, second.n_identical, second.n_balanced, second.n_near) == (2, 0, 0, 0)
    assert second.listed == [Alternative(names[1], "better", -287, 0, 287, 0, 3)] and second.resolved == "KIR2DL1*"


def test_parser_takes_the_call_alternatives_flags():
    base = ["--step-skip-extraction", "--alignment", "s.sam"]
    args = cli.createParser().parse_args(base)
    assert args.call_alternatives is False and args.call_alternatives_within == 1 and args.call_alternatives_max == 20
    assert cli.callReportArgs(args, report="call_alternatives") == {}
    args = cli.createParser().parse_args(base + ["--allele-strategy", "exonfirst", "--call-alternatives",
                                                 "--call-alternatives-within", "0", "--call-alternatives-max", "256"])
    assert cli.callReportArgs(args, report="call_alternatives") == {"call_alternatives": True, "call_alternatives_within": 0,
                                               "call_alternatives_max": 256}
    # it combines with the fit report
    args = cli.createParser().parse_args(base + ["--call-alternatives", "--call-fit"])
    assert cli.callReportArgs(args, report="call_alternatives") == {"call_alternatives": True, "call_alternatives_within": 1, "call_alternatives_max": 20}
    assert cli.callReportArgs(args, report="call_fit") == {"call_fit": True, "call_fit_extra": 3}
    # without the flag the ranges alone ask for nothing
    args = cli.createParser().parse_args(base + ["--call-alternatives-within", "65", "--call-alternatives-max", "0"])
    assert cli.callReportArgs(args, report="call_alternatives") == {}


@pytest.mark.parametrize("extra", [["--allele-strategy", "em", "--call-alternatives"],
                                   ["--allele-strategy", "report", "--call-alternatives"],
                                   ["--allele-strategy", "full", "--call-alternatives", "--call-alternatives-within", "65"],
                                   ["--allele-strategy", "full", "--call-alternatives", "--call-alternatives-within", "-1"],
                                   ["--allele-strategy", "exonfirst", "--call-alternatives", "--call-alternatives-max", "0"],
                                   ["--allele-strategy", "exonfirst", "--call-alternatives", "--call-alternatives-max", "257"]])
def test_command_line_refuses_what_cannot_work(extra, monkeypatch):
    for name in ("GK_WAIT_POLICY", "GK_SAMPLE_LANES", "GK_SEARCH_SLOTS"):      # main() sets its defaults: put them back
        monkeypatch.setenv(name, os.environ.get(name, "1"))
    args = cli.createParser().parse_args(["--step-skip-extraction", "--alignment", "s.sam"] + extra)
    with pytest.raises(ValueError, match="--call-alternatives"):
        cli.main(args)


def test_factory_refusals():
    from kir_graph_amd.kir_typing import TypingWithPosNegAllele, TypingWithReport, selectKirTypingModel
    for method in ("em", "report"):
        with pytest.raises(ValueError, match="call_alternatives"):
            selectKirTypingModel(method, "nothing.json", call_alternatives=True, call_alternatives_within=1,
                                 call_alternatives_max=20)
    with pytest.raises(TypeError):
        TypingWithReport("nothing.json", call_alternatives=True)
    # checked before the sample is touched
    for bad in (-1, 65):
        with pytest.raises(ValueError, match="call_alternatives_within"):
            TypingWithPosNegAllele("nothing.json", call_alternatives=True, call_alternatives_within=bad)
    for bad in (0, 257):
        with pytest.raises(ValueError, match="call_alternatives_max"):
            TypingWithPosNegAllele("nothing.json", call_alternatives=True, call_alternatives_max=bad)
