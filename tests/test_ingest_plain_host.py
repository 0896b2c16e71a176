"""``packed.packBamPlainHost`` -- the split route of the device ingest with the kernel's decoder run on the host
(``gk_bam_pack_plain_host``) -- against ``packed.packBam``: equal outcomes, exceptions included, and a shared decoder
that takes most pairs of a synthetic sample (a route that flags every pair HOST would be "equal" too)."""
from ingest_cases import awkwardFiles, headerOf, outcome
from kir_graph_amd import packed, synth


def test_plain_host_route_equals_the_host_route_on_a_sample(small_case, tmp_path):
    sidx, gidx, sample = small_case
    path = str(tmp_path / "small.bam")
    packed.writeBam(path, "\n".join(headerOf(sidx, "unsorted") + synth.toSamLines(sample)) + "\n")
    want, _, _ = outcome(lambda: packed.packBam(path, gidx))
    got, decode, _ = outcome(lambda: packed.packBamPlainHost(path, gidx))
    assert want[0] == "ok" and got == want
    assert decode["route"] == "plain_host"
    assert decode["plain_pairs"] + decode["host_pairs"] == want[4]["pairs"] == 4000
    print("plain pairs", decode["plain_pairs"], "of", want[4]["pairs"])
    # measured with gk_pair_decode over the paired records of this sample: 3734 of 4000
    assert decode["plain_pairs"] >= 3600


def test_plain_host_route_equals_the_host_route_on_awkward_records(tmp_path):
    files, gidx = awkwardFiles(tmp_path)
    kinds = {}
    for tag, path, kind in files:
        want, _, _ = outcome(lambda: packed.packBam(path, gidx))
        got, decode, _ = outcome(lambda: packed.packBamPlainHost(path, gidx))
        assert got == want, tag
        kinds[tag] = want[0]
        if kind is not None:
            assert want[0] == kind, tag
        if want[0] == "ok":
            assert decode["plain_pairs"] >= 300 and decode["host_pairs"] >= 1, (tag, decode)
    assert len(kinds) == 17 and sum(k != "ok" for k in kinds.values()) >= 8
