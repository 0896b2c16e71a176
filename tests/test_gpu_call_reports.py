"""GPU: a per-call report does not depend on the reports that run with it (``call_report.CALL_REPORTS``).

The typer makes every switched-on report of a gene's adopted result in one loop over the table.  A sample typed with all
five reports on must give, byte for byte, the text each report gives when it alone is on, and the same calls -- for the
plain and the exon-first strategy, through the whole-sample drivers and through ``typingPerGene``.
"""
import pytest

from kir_graph_amd import packed
from kir_graph_amd.call_report import CALL_REPORTS
from kir_graph_amd.engine import DeviceIndex, Tabulation
from kir_graph_amd.hisat2 import SampleData
from kir_graph_amd.kir_typing import TypingWithPosNegAllele

pytestmark = pytest.mark.gpu

STRATEGIES = {"full": {}, "exonfirst": {"exon_first": True}}


@pytest.fixture(scope="module")
def tabulated(device, small_case):
    """The sample of tests/test_gpu_call_dosage.py, its records kept in HBM for the coverage report."""
    sidx, gidx, sample = small_case
    rec, table = packed.packSample(sample, gidx)
    tab = Tabulation(DeviceIndex(device, gidx), rec)
    gene_len = {g: len(sidx.backbone[g]) for g in sidx.genes}
    yield SampleData(tab, gidx, tab.novelVariants(table.strings)), sample, gene_len
    tab.mates.free()
    tab.close()


def switches(gene_len) -> dict[str, dict]:
    """The typer keywords that switch each report on, the options at their defaults."""
    on = {"call_bootstrap": {"call_bootstrap": 16}, "call_fit": {"call_fit": True}, "call_alternatives": {"call_alternatives": True},
          "call_dosage": {"call_dosage": True}, "call_coverage": {"call_coverage": True, "call_coverage_len": gene_len}}
    assert list(on) == [r.key for r in CALL_REPORTS]      # a new report joins this test
    return on


def typeSample(data, sample, per_gene: bool, **kw):
    typer = TypingWithPosNegAllele(data, variant_correction=True, **kw)
    if per_gene:
        calls = [typer.typingPerGene(gene, int(cn)) for gene, cn in sample.gene_cn.items() if cn]
    else:
        calls = typer.typing(sample.gene_cn)
    return typer, calls


def texts(typer, report) -> list[str]:
    entries = {gene: e for gene, e in getattr(typer, report.key).items() if e is not None}
    return [text(entries) for _, text, _ in report.files]


@pytest.mark.parametrize("per_gene", [False, True], ids=["whole sample", "per gene"])
@pytest.mark.parametrize("strategy", list(STRATEGIES))
def test_all_reports_together_equal_each_alone(tabulated, strategy, per_gene):
    data, sample, gene_len = tabulated
    on = switches(gene_len)
    both, both_calls = typeSample(data, sample, per_gene, **STRATEGIES[strategy],
                                  **{k: v for options in on.values() for k, v in options.items()})
    assert both._wholeSample() == (strategy == "full") and both._wholeSampleExonFirst() == (strategy == "exonfirst")
    typed = {g for g, cn in sample.gene_cn.items() if cn and both._result.get(g) and not both._result[g][-1].isFail()}
    assert len(typed) >= 2
    for report in CALL_REPORTS:
        alone, alone_calls = typeSample(data, sample, per_gene, **STRATEGIES[strategy], **on[report.key])
        assert alone_calls == both_calls, (strategy, report.key)
        got, want = getattr(both, report.key), getattr(alone, report.key)
        assert set(got) == set(want) == typed and all(e is not None for e in got.values()), (strategy, report.key)
        assert texts(both, report) == texts(alone, report), (strategy, report.key)
        assert all(t.count("\n") > 1 for t in texts(both, report)), (strategy, report.key)      # more than a header
        for other in CALL_REPORTS:      # what is switched off stays empty
            assert other is report or getattr(alone, other.key) == {}, (report.key, other.key)
