"""Host side of the tabulation from compact words: what the roofline prices for ``tab_count`` and what a sample's records
count for in the admission of samples to the typing lanes."""
from types import SimpleNamespace

from kir_graph_amd import cohort, roofmodel


def test_tab_count_is_priced_from_the_bytes_it_reads():
    """A call-log entry of ``tab_count`` carries the bytes of the compact words when the sample was tabulated from them;
    without that figure the records are 2 x 128 bytes per pair."""
    n_pairs, n_valid, n_ids = 1000, 900, 50_000
    lists = 4.0 * n_ids + 22.0 * n_valid
    assert roofmodel.tabLaunch(n_pairs, n_valid, n_ids) == (256.0 * n_pairs + lists, 0.0)
    assert roofmodel.tabLaunch(n_pairs, n_valid, n_ids, 61_000) == (61_000.0 + lists, 0.0)
    records = roofmodel.stepRoofline([("tab_count", n_pairs, n_valid, n_ids)], 1, 2.0)["kernels"]["tab_count"]["bytes_per_step"]
    compact = roofmodel.stepRoofline([("tab_count", n_pairs, n_valid, n_ids, 61_000)], 1, 2.0)["kernels"]["tab_count"]["bytes_per_step"]
    assert records - compact == 256.0 * n_pairs - 61_000.0


def test_a_sample_counts_for_the_record_bytes_it_holds():
    def sample(mates):
        tab = SimpleNamespace(n_valid=1000, n_ids=60_000, n_pairs=1200, mates=mates, dev=None)
        return SimpleNamespace(tab=tab, index=SimpleNamespace(tables=[SimpleNamespace(n_allele=100)] * 2))

    none = cohort.sampleFootprint(sample(None), "full")
    assert cohort.sampleFootprint(sample(SimpleNamespace(nbytes=70_000)), "full") == none + 70_000
    assert cohort.sampleFootprint(sample(object()), "full") == none + 256 * 1200      # a buffer that does not say: records
