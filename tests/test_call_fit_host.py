"""Fit report of a likelihood call, host side (no GPU): the restatement of tests/callfit_reference.py on a table worked out
by hand, the choice of the extra alleles, the ``.fit.tsv`` text, command-line flags and factory refusals."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import callfit_reference as fr  # noqa: E402

from kir_graph_amd import main as cli  # noqa: E402
from kir_graph_amd.call_fit import CALL_FIT_COLUMNS, CalledAllele, CallFit, callFitText, largestGains  # noqa: E402

# [column][row]: columns 2 and 0 are called (in that order), 1 and 3 are not
TABLE = np.array([[0, 1, 2, 0, 255, 30],
                  [0, 0, 0, 0, 0, 0],
                  [0, 0, 5, 1, 255, 40],
                  [9, 9, 9, 9, 9, 9]])


def test_restatement_on_a_hand_built_table():
    hist, m, per_col, d_min = fr.profile(TABLE, [2, 0])
    # row:          0       1        2        3        4            5
    # (b_0, b_1): (0, 0)  (0, 1)   (5, 2)   (1, 0)   (255, 255)   (40, 30)
    # m1:           0       0        2        0        255          30
    # A:          both     {0}      {1}      {1}      both         {1}
    # second - m1:  -       1        3        1        -            10
    assert d_min.tolist() == [0, 0, 2, 0, 255, 30]
    want_hist = [0] * 18
    want_hist[0], want_hist[2], want_hist[16], want_hist[17] = 3, 1, 1, 1
    assert hist.tolist() == want_hist and hist.sum() == 6
    assert m == 287
    assert per_col.tolist() == [[3, 1, 1], [5, 3, 14]]
    # only = M without the column minus M
    assert int(TABLE[0].sum()) - m == 1 and int(TABLE[2].sum()) - m == 14
    with_a = fr.extra(TABLE, d_min)
    assert with_a.tolist() == [287, 0, 287, 20]
    # the order of the listed columns moves the per-column rows and nothing else
    hist2, m2, per_col2, d_min2 = fr.profile(TABLE, [0, 2])
    assert hist2.tolist() == want_hist and m2 == m and per_col2.tolist() == [[5, 3, 14], [3, 1, 1]]
    assert d_min2.tolist() == d_min.tolist()


def test_restatement_of_one_column_and_of_equal_columns():
    hist, m, per_col, d_min = fr.profile(TABLE, [3])
    assert hist[9] == 6 and hist.sum() == 6 and m == 54 and per_col.tolist() == [[6, 6, 0]]
    assert d_min.tolist() == [9] * 6
    hist, m, per_col, _ = fr.profile(np.stack([TABLE[0]] * 3), [0, 1, 2])
    assert per_col.tolist() == [[6, 0, 0]] * 3 and m == int(TABLE[0].sum())


def test_largest_gains():
    gain = np.array([0, 287, 0, 267, 267, 5, 0])
    assert largestGains(gain, [2, 0], 3) == [(1, 287), (3, 267), (4, 267)]      # the lower column first among equals
    assert largestGains(gain, [2, 0], 64) == [(1, 287), (3, 267), (4, 267), (5, 5)]      # gains of 0 are dropped
    assert largestGains(gain, [1, 3], 2) == [(4, 267), (5, 5)]                   # a called column is never an extra
    assert largestGains(gain, [2, 0], 0) == [] and largestGains(np.zeros(4, dtype=np.int64), [0], 3) == []


def fits():
    hist = np.zeros(18, dtype=np.int64)
    hist[[0, 1, 2, 3, 7, 16, 17]] = [1179, 3, 2, 1, 1, 4, 5]
    homo = np.zeros(18, dtype=np.int64)
    homo[0] = 566
    return {
        "KIR2DL1S1": CallFit(cn=3, reads=1195, hist=hist, mismatches=1330, out_of_range=5,
                             alleles=[CalledAllele("KIR2DL1*001", 2, 865, 605, 1438), CalledAllele("KIR2DS1*002", 1, 577, 317, 667)],
                             extra=[("KIR2DL1*007", 12), ("KIR2DS1*005", 1)], extra_scope="all"),
        "KIR2DL2": CallFit(cn=2, reads=566, hist=homo, mismatches=0, out_of_range=0,
                           alleles=[CalledAllele("KIR2DL2*003", 2, 566, 566, None)], extra=[], extra_scope="candidates"),
    }


def test_fit_file_bytes(tmp_path):
    [path] = cli.writeCallReport("call_fit", str(tmp_path / "s.pv"), fits())
    assert path.endswith("s.pv.fit.tsv")
    want = ("gene\tcn\treads\texplained\tmiss1\tmiss2\tmiss3plus\tout_of_range\tmismatches\tallele\tcopies\tbest\tunique\t"
            "only_explains\textra_scope\textra_1\tgain_1\textra_2\tgain_2\n"
            "KIR2DL1S1\t3\t1195\t1179\t3\t2\t6\t5\t1330\tKIR2DL1*001\t2\t865\t605\t1438\tall\tKIR2DL1*007\t12\tKIR2DS1*005\t1\n"
            "KIR2DL1S1\t3\t1195\t1179\t3\t2\t6\t5\t1330\tKIR2DS1*002\t1\t577\t317\t667\tall\tKIR2DL1*007\t12\tKIR2DS1*005\t1\n"
            "KIR2DL2\t2\t566\t566\t0\t0\t0\t0\t0\tKIR2DL2*003\t2\t566\t566\t\tcandidates\t\t\t\t\n")
    assert open(path).read() == want == callFitText(fits())
    assert want.split("\n")[0].split("\t")[:15] == CALL_FIT_COLUMNS
    assert CALL_FIT_COLUMNS == ["gene", "cn", "reads", "explained", "miss1", "miss2", "miss3plus", "out_of_range", "mismatches",
                                "allele", "copies", "best", "unique", "only_explains", "extra_scope"]


def test_fit_file_of_one_allele_and_without_extras():
    only = {"KIR2DL2": fits()["KIR2DL2"]}
    text = callFitText(only).split("\n")
    assert text[0].split("\t") == CALL_FIT_COLUMNS and text[2] == "" and len(text) == 3      # no extra columns at all
    cells = text[1].split("\t")
    assert len(cells) == 15 and cells[13] == "" and cells[14] == "candidates"                # only_explains is undefined
    assert callFitText({}) == "\t".join(CALL_FIT_COLUMNS) + "\n"


def test_parser_takes_the_call_fit_flags():
    base = ["--step-skip-extraction", "--alignment", "s.sam"]
    args = cli.createParser().parse_args(base)
    assert args.call_fit is False and args.call_fit_extra == 3 and cli.callReportArgs(args, report="call_fit") == {}
    args = cli.createParser().parse_args(base + ["--allele-strategy", "exonfirst", "--call-fit", "--call-fit-extra", "0"])
    assert cli.callReportArgs(args, report="call_fit") == {"call_fit": True, "call_fit_extra": 0}
    # it combines with the call bootstrap
    args = cli.createParser().parse_args(base + ["--call-fit", "--call-bootstrap", "8"])
    assert cli.callReportArgs(args, report="call_fit") == {"call_fit": True, "call_fit_extra": 3}
    assert cli.callReportArgs(args, report="call_bootstrap")["call_bootstrap"] == 8
    # without the flag the count alone asks for nothing
    args = cli.createParser().parse_args(base + ["--call-fit-extra", "65"])
    assert cli.callReportArgs(args, report="call_fit") == {}


@pytest.mark.parametrize("extra", [["--allele-strategy", "em", "--call-fit"],
                                   ["--allele-strategy", "report", "--call-fit"],
                                   ["--allele-strategy", "full", "--call-fit", "--call-fit-extra", "65"],
                                   ["--allele-strategy", "exonfirst", "--call-fit", "--call-fit-extra", "-1"]])
def test_command_line_refuses_what_cannot_work(extra, monkeypatch):
    for name in ("GK_WAIT_POLICY", "GK_SAMPLE_LANES", "GK_SEARCH_SLOTS"):      # main() sets its defaults: put them back
        monkeypatch.setenv(name, os.environ.get(name, "1"))
    args = cli.createParser().parse_args(["--step-skip-extraction", "--alignment", "s.sam"] + extra)
    with pytest.raises(ValueError, match="--call-fit"):
        cli.main(args)


def test_factory_refusals():
    from kir_graph_amd.kir_typing import TypingWithPosNegAllele, TypingWithReport, selectKirTypingModel
    for method in ("em", "report"):
        with pytest.raises(ValueError, match="call_fit"):
            selectKirTypingModel(method, "nothing.json", call_fit=True, call_fit_extra=3)
    with pytest.raises(TypeError):
        TypingWithReport("nothing.json", call_fit=True)
    # checked before the sample is touched
    for bad in (-1, 65):
        with pytest.raises(ValueError, match="call_fit_extra"):
            TypingWithPosNegAllele("nothing.json", call_fit=True, call_fit_extra=bad)
