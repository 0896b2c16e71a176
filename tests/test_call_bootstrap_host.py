"""Call bootstrap of the likelihood strategies, host side (no GPU): the summary of a score matrix, the confidence file,
command-line flags and factory refusals, ``TypingResult.bestRank`` and the restatement of tests/callboot_reference.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import boot_reference as br  # noqa: E402
import callboot_reference as cr  # noqa: E402

from kir_graph_amd import main as cli  # noqa: E402
from kir_graph_amd.call_bootstrap import (CALL_CONFIDENCE_COLUMNS, CallBootstrap, callConfidenceText, candidateRows,  # noqa: E402
                                          homoFactor, summariseCall)
from kir_graph_amd.typing_mulit_allele import AlleleTyping, TypingResult  # noqa: E402


def test_summary_of_hand_made_scores():
    s = np.array([[-10.0, -10.0, -12.0],       # a tie: the lowest row wins
                  [-11.0, -9.0, -12.0],
                  [-8.0, -9.0, -8.5],
                  [-10.0, -9.5, -9.5]])        # a tie between rows 1 and 2
    support, mean, lo, hi = summariseCall(s, 0)
    assert support.tolist() == [0.5, 0.5, 0.0] and support.sum() == 1.0
    d = s - s[:, [0]]
    assert np.array_equal(mean, d.mean(axis=0)) and mean[0] == 0.0
    want_lo, want_hi = np.percentile(d, [2.5, 97.5], axis=0)
    assert np.array_equal(lo, want_lo) and np.array_equal(hi, want_hi)
    assert lo[0] == hi[0] == 0.0
    # the called row is not row 0: distances are taken to it
    support1, mean1, lo1, hi1 = summariseCall(s, 1)
    assert np.array_equal(support1, support)
    d1 = s - s[:, [1]]
    assert np.array_equal(mean1, d1.mean(axis=0)) and mean1[1] == lo1[1] == hi1[1] == 0.0
    assert np.array_equal(lo1, np.percentile(d1, 2.5, axis=0)) and np.array_equal(hi1, np.percentile(d1, 97.5, axis=0))


def test_summary_of_one_replicate():
    support, mean, lo, hi = summariseCall(np.array([[-3.0, -1.0, -2.0]]), 2)
    assert support.tolist() == [0.0, 1.0, 0.0]
    assert mean.tolist() == lo.tolist() == hi.tolist() == [-1.0, 1.0, 0.0]


def test_supports_sum_to_one():
    rng = np.random.default_rng(3)
    for n_boot, n_sets in ((1, 1), (7, 5), (100, 33)):
        s = -rng.integers(0, 4, (n_boot, n_sets)).astype(np.float64)       # many ties
        support = summariseCall(s, n_sets - 1)[0]
        assert support.sum() == pytest.approx(1.0, abs=1e-12) and (support >= 0).all()
        assert np.array_equal(support, np.bincount(s.argmax(axis=1), minlength=n_sets) / n_boot)


def test_call_confidence_file_bytes(tmp_path):
    boot = {
        "KIR2DL1": CallBootstrap(rows=np.array([0, 2]), called=0, value=np.array([-120.5, -121.0]), scores=np.zeros((2, 2)),
                                 support=np.array([0.75, 0.25]), delta_mean=np.array([0.0, -0.5]),
                                 delta_lo=np.array([0.0, -1.25]), delta_hi=np.array([0.0, 1 / 3]), cn=1,
                                 alleles=[["KIR2DL1*001"], ["KIR2DL1*002"]]),
        "KIR3DL3": CallBootstrap(rows=np.array([0, 1, 40]), called=2, value=np.array([-300.0, -300.0, -301.5]),
                                 scores=np.zeros((2, 3)), support=np.array([0.5, 0.0, 0.5]),
                                 delta_mean=np.array([1.5, 1e-300, 0.0]), delta_lo=np.array([-2.0, -3.0, 0.0]),
                                 delta_hi=np.array([4.0, np.float64(0.4), 0.0]), cn=3,
                                 alleles=[["KIR3DL3*001", "KIR3DL3*001", "KIR3DL3*002"], ["KIR3DL3*001", "KIR3DL3*002", "KIR3DL3*003"],
                                          ["KIR3DL3*004", "KIR3DL3*004", "KIR3DL3*004"]]),
    }
    [path] = cli.writeCallReport("call_bootstrap", str(tmp_path / "s.pv"), boot)
    assert path.endswith("s.pv.call_confidence.tsv")
    want = ("gene\tcn\trank\tcalled\tvalue\tsupport\tdelta_mean\tdelta_q025\tdelta_q975\t1\t2\t3\n"
            "KIR2DL1\t1\t0\t1\t-120.5\t0.75\t0.0\t0.0\t0.0\tKIR2DL1*001\t\t\n"
            "KIR2DL1\t1\t2\t0\t-121.0\t0.25\t-0.5\t-1.25\t0.3333333333333333\tKIR2DL1*002\t\t\n"
            "KIR3DL3\t3\t0\t0\t-300.0\t0.5\t1.5\t-2.0\t4.0\tKIR3DL3*001\tKIR3DL3*001\tKIR3DL3*002\n"
            "KIR3DL3\t3\t1\t0\t-300.0\t0.0\t1e-300\t-3.0\t0.4\tKIR3DL3*001\tKIR3DL3*002\tKIR3DL3*003\n"
            "KIR3DL3\t3\t40\t1\t-301.5\t0.5\t0.0\t0.0\t0.0\tKIR3DL3*004\tKIR3DL3*004\tKIR3DL3*004\n")
    assert open(path).read() == want == callConfidenceText(boot)
    assert want.split("\n")[0].split("\t")[:9] == CALL_CONFIDENCE_COLUMNS
    assert boot["KIR3DL3"].call_support == 0.5
    assert callConfidenceText({}) == "\t".join(CALL_CONFIDENCE_COLUMNS) + "\n"


def test_parser_takes_the_call_bootstrap_flags():
    base = ["--step-skip-extraction", "--alignment", "s.sam"]
    args = cli.createParser().parse_args(base)
    assert not args.call_bootstrap and args.call_bootstrap_seed == 2022 and args.call_bootstrap_top == 32
    assert cli.callReportArgs(args, report="call_bootstrap") == {}
    args = cli.createParser().parse_args(base + ["--allele-strategy", "exonfirst", "--call-bootstrap", "100",
                                                 "--call-bootstrap-seed", "5", "--call-bootstrap-top", "8"])
    assert (args.call_bootstrap, args.call_bootstrap_seed, args.call_bootstrap_top) == (100, 5, 8)
    assert cli.callReportArgs(args, report="call_bootstrap") == {"call_bootstrap": 100, "call_bootstrap_seed": 5, "call_bootstrap_top": 8}


@pytest.mark.parametrize("extra", [["--allele-strategy", "em", "--call-bootstrap", "8"],
                                   ["--allele-strategy", "report", "--call-bootstrap", "8"],
                                   ["--allele-strategy", "full", "--call-bootstrap", "0"],
                                   ["--allele-strategy", "exonfirst", "--call-bootstrap", "-3"],
                                   ["--allele-strategy", "pv", "--call-bootstrap", "8", "--call-bootstrap-top", "0"],
                                   ["--allele-strategy", "pv", "--call-bootstrap", "8", "--call-bootstrap-top", "257"]])
def test_command_line_refuses_what_cannot_work(extra, monkeypatch):
    for name in ("GK_WAIT_POLICY", "GK_SAMPLE_LANES", "GK_SEARCH_SLOTS"):      # main() sets its defaults: put them back
        monkeypatch.setenv(name, os.environ.get(name, "1"))
    args = cli.createParser().parse_args(["--step-skip-extraction", "--alignment", "s.sam"] + extra)
    with pytest.raises(ValueError, match="--call-bootstrap"):
        cli.main(args)


def test_factory_refusals():
    from kir_graph_amd.kir_typing import TypingWithPosNegAllele, TypingWithReport, selectKirTypingModel
    for method in ("em", "report"):
        with pytest.raises(ValueError, match="call_bootstrap"):
            selectKirTypingModel(method, "nothing.json", call_bootstrap=8, call_bootstrap_seed=1, call_bootstrap_top=4)
    with pytest.raises(TypeError):
        TypingWithReport("nothing.json", call_bootstrap=8)
    # the EM's keywords stay refused for the likelihood strategies, with or without the new ones
    for method in ("full", "pv", "exonfirst_1", "pv_exonfirst_0.9"):
        with pytest.raises(ValueError, match="bootstrap"):
            selectKirTypingModel(method, "nothing.json", bootstrap=8, bootstrap_seed=1, call_bootstrap=8)
    # checked before the sample is touched
    for bad in ({"call_bootstrap": -1}, {"call_bootstrap": 10001}, {"call_bootstrap": 8, "call_bootstrap_top": 0},
                {"call_bootstrap": 8, "call_bootstrap_top": 257}):
        with pytest.raises(ValueError, match="call_bootstrap"):
            TypingWithPosNegAllele("nothing.json", **bad)


def result(ids, fraction, value=None):
    ids = np.asarray(ids)
    k, n = ids.shape
    value = -np.arange(k, dtype=np.float64) if value is None else np.asarray(value, dtype=np.float64)
    return TypingResult(n=n, value=value, value_sum_indv=np.ones((k, n)), allele_id=ids,
                        allele_name=[[f"A*{i:03d}" for i in row] for row in ids.tolist()], allele_prob=np.zeros((0, k)),
                        fraction=np.asarray(fraction, dtype=np.float64), fraction_uniq=np.ones((k, n)))


def test_best_rank_is_the_row_select_best_names():
    every = result([[0, 1], [0, 2], [1, 2]], [[0.5, 0.5], [0.6, 0.4], [0.3, 0.7]])
    assert every.bestRank() == 0 and every.selectBest() == every.allele_name[0]
    # rows 0 and 1 fail the fraction filter (a share below 1 / (2 n)): the call is row 2
    some = result([[0, 1], [0, 2], [1, 2]], [[0.9, 0.1], [0.2, 0.8], [0.3, 0.7]])
    assert some.bestRank() == 2 and some.selectBest() == ["A*001", "A*002"]
    assert some.bestRank(filter_fraction=False) == 0 and some.selectBest(filter_fraction=False) == ["A*000", "A*001"]
    # no row passes: row 0
    none = result([[0, 1], [0, 2]], [[0.9, 0.1], [0.2, 0.8]])
    assert none.bestRank() == 0 and none.selectBest() == ["A*000", "A*001"]
    e = np.array([])
    fail = TypingResult(2, e, e, e, [], e, e, e)
    assert fail.bestRank() == 0 and fail.selectBest() == ["fail", "fail"]
    homo = AlleleTyping.createHomoResult(result([[4], [7]], [[1.0], [1.0]]), 3)
    assert homo.bestRank() == 0 and homo.selectBest() == ["A*004"] * 3


def test_candidate_rows():
    # rows 1 and 3 repeat the multisets of rows 0 and 2 (exon-first merges the searches of several exon sets)
    r = result([[0, 1], [1, 0], [0, 2], [2, 0], [1, 2], [3, 4]], [[0.5, 0.5]] * 6)
    rows, called = candidateRows(r, 32)
    assert rows.tolist() == [0, 2, 4, 5] and called == 0
    rows, called = candidateRows(r, 2)
    assert rows.tolist() == [0, 2] and called == 0
    # the called row lies beyond the kept ones: appended
    far = result([[0, 1], [1, 0], [0, 2], [2, 0], [1, 2], [3, 4]], [[0.9, 0.1]] * 5 + [[0.5, 0.5]])
    assert far.bestRank() == 5
    rows, called = candidateRows(far, 2)
    assert rows.tolist() == [0, 2, 5] and called == 2
    rows, called = candidateRows(far, 4)
    assert rows.tolist() == [0, 2, 4, 5] and called == 3
    one = result([[3]], [[1.0]])
    assert candidateRows(one, 1)[0].tolist() == [0] and candidateRows(one, 1)[1] == 0


def test_homo_factor():
    class Parts:
        def __init__(self, parts):
            self.parts = parts
    step1 = result([[4], [7]], [[1.0], [1.0]])
    step1.allele_prob = Parts([(None, step1.allele_id)])
    assert homoFactor(step1) == 1
    assert homoFactor(AlleleTyping.createHomoResult(step1, 3)) == 3
    step2 = result([[4, 7], [7, 7]], [[0.5, 0.5]] * 2)
    step2.allele_prob = Parts([(None, step2.allele_id)])
    assert homoFactor(step2) == 1


def test_restatement_of_the_weights():
    for n in (1, 2, 1000, 16385):
        for b in (0, 4):
            w = cr.rowCounts(2022, 3, b, n)
            assert w.shape == (n,) and w.sum() == n and w.min() >= 0
            assert np.array_equal(w, np.bincount(br.draws(2022, 3, b, n).astype(np.int64), minlength=n))
    # replicate b is replicate b, however many there are
    three, seventeen = cr.weights(2022, 1, range(3), 500), cr.weights(2022, 1, range(17), 500)
    assert np.array_equal(three, seventeen[:3]) and not np.array_equal(seventeen[3], seventeen[4])
    assert not np.array_equal(cr.rowCounts(2022, 1, 0, 500), cr.rowCounts(2022, 2, 0, 500))
    assert not np.array_equal(cr.rowCounts(2022, 1, 0, 500), cr.rowCounts(2023, 1, 0, 500))
    V = -np.arange(1, 1001, dtype=np.float64).reshape(2, 500) / 8
    assert np.array_equal(cr.scores(three, V), np.array([[float((w * v).sum()) for v in V] for w in three]))
