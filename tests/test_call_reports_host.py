"""Host: the table of per-call reports (``call_report.CALL_REPORTS``) against the parser, the command line's refusals and
the typer -- one case per entry, so a new report is held to the same."""
import re

import pytest

from kir_graph_amd import kir_typing
from kir_graph_amd import main as cli
from kir_graph_amd.call_report import CALL_REPORTS, callReport

BASE = ["--step-skip-extraction", "--alignment", "s.sam"]
KEYS = [r.key for r in CALL_REPORTS]


def test_the_table_is_in_launch_order():
    assert KEYS == ["call_bootstrap", "call_fit", "call_alternatives", "call_dosage", "call_coverage"]
    assert all(callReport(k) is r and r.options[0].name == k for k, r in zip(KEYS, CALL_REPORTS))
    suffixes = [s for r in CALL_REPORTS for s, _, _ in r.files]
    assert suffixes == [".call_confidence.tsv", ".fit.tsv", ".alternatives.tsv", ".dosage.tsv", ".coverage.tsv",
                        ".coverage.depth.tsv"]


@pytest.mark.parametrize("report", CALL_REPORTS, ids=KEYS)
def test_flags_exist_with_the_entry_s_defaults(report):
    parser = cli.createParser()
    args = parser.parse_args(BASE)
    flags = {s for a in parser._actions for s in a.option_strings}
    for o in report.options:
        if o.from_index is None:
            assert o.flag in flags and getattr(args, o.name) == o.default and type(getattr(args, o.name)) is type(o.default), o.name
    assert report.flag == "--" + report.key.replace("_", "-")
    assert cli.callReportArgs(args, report=report.key) == {} == cli.callReportArgs(args)


@pytest.mark.parametrize("strategy", ["em", "report"])
@pytest.mark.parametrize("report", CALL_REPORTS, ids=KEYS)
def test_refused_for_the_em_strategy_naming_the_flag(report, strategy):
    asked = [report.flag] + (["8"] if report.count else [])
    args = cli.createParser().parse_args(BASE + ["--allele-strategy", strategy] + asked)
    with pytest.raises(ValueError, match=re.escape(report.flag) + " needs .*a likelihood strategy"):
        cli.callReportArgs(args)
    with pytest.raises(ValueError, match=re.escape(report.flag)):
        cli.callReportArgs(args, report=report.key)
    # the same flags with a likelihood strategy: the report alone is asked for
    args = cli.createParser().parse_args(BASE + asked)
    assert list(cli.callReportArgs(args))[0] == report.key and cli.callReportArgs(args) == cli.callReportArgs(args, report=report.key)
    with pytest.raises(ValueError, match=f"{report.key}: only the likelihood strategies {report.does}, not '{strategy}'"):
        kir_typing.selectKirTypingModel(strategy, "nothing.json", **{report.key: 8 if report.count else True})


@pytest.mark.parametrize("report", CALL_REPORTS, ids=KEYS)
def test_a_typer_without_report_keywords_reports_nothing(report, monkeypatch):
    monkeypatch.setattr(kir_typing, "_sample", lambda source, device: source)
    typer = kir_typing.TypingWithPosNegAllele("nothing.json")
    assert getattr(typer, report.key) == {} and isinstance(getattr(typer, report.key), dict)
    assert not report.switchedOn(typer._call_options[report.key])
    assert all(getattr(typer, other.key) is not getattr(typer, report.key) for other in CALL_REPORTS if other is not report)
    with pytest.raises(TypeError, match="call_no_such_report"):
        kir_typing.TypingWithPosNegAllele("nothing.json", call_no_such_report=True)
    with pytest.raises(TypeError, match="call_no_such_report"):
        cli.sampleTyper("full", call_no_such_report=True)
