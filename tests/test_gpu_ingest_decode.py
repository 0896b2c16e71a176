"""``packed.packBamDevice`` (``gk_bam_pack_device``, csrc/gk_ingest_decode.hip: the plain pairs of a BAM file decoded by
``ingest_decode_pairs``, the rest by the host decoder) against ``packed.packBam`` on small files: equal records, strings,
pair_lines, counts and spill, or the same exception kind, line and reason; the records kept on the device equal the host
array; the kernel takes exactly the pairs the same decoder takes on the host (``packBamPlainHost``).  Shapes: the wave
and block edges of a launch with two lanes per pair, record starts on every residue mod 4, every stream length mod 4,
the capacity edges of ``gk_mate``, header-only pairs, a reference that is no backbone, the awkward records of
test_host.py.  One command-line run with and without ``--ingest-decode device``: the same bytes in every file."""
import logging

import pytest

from ingest_cases import awkwardFiles, headerOf, outcome, smallIndex
from kir_graph_amd import packed, synth

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ hand-made pairs
def alignment(ops, mism=()):
    """(CIGAR, SEQ, MD) of M / D / I ops with mismatches at the given read offsets."""
    seq, md, run, ri = [], "", 0, 0
    mism = set(mism)
    for op, n in ops:
        if op == "M":
            for _ in range(n):
                base = "ACGT"[(ri * 7 + 3) % 4]
                seq.append(base)
                if ri in mism:
                    md += str(run) + ("C" if base == "A" else "A")
                    run = 0
                else:
                    run += 1
                ri += 1
        elif op == "D":
            md += str(run) + "^" + "ACGT"[:min(n, 3)]
            run = 0
        else:
            for _ in range(n):
                seq.append("ACGT"[(ri * 7 + 3) % 4])
                ri += 1
    return "".join(f"{n}{op}" for op, n in ops), "".join(seq), md + str(run)


def alternating(n_ops, m_len=5, d_len=1):
    return [("M", m_len) if i % 2 == 0 else ("D", d_len) for i in range(n_ops)]


CLEAN = alignment([("M", 50)])
KINDS = {
    "clean": (CLEAN, 0),
    "busy": (alignment([("M", 10), ("D", 2), ("M", 30)], [3, 17]), 4),
    "insertion": (alignment([("M", 10), ("I", 2), ("M", 10)]), 2),
    "ops14": (alignment(alternating(14)), 4),
    "ops15": (alignment(alternating(15)), 4),
    "mm16": (alignment([("M", 40)], range(16)), 4),
    "mm17": (alignment([("M", 40)], range(17)), 4),
    "events22": (alignment(alternating(13), range(16)), 4),
    "events23": (alignment(alternating(14), range(16)), 4),
    "nm5": (alignment([("M", 10), ("D", 2), ("M", 30)], [3]), 5),
}


def pairOf(name, kind, ref, flag_mask=0xFFFF, extra=""):
    """The two SAM lines of a pair: the first mate of the given kind, the second clean."""
    (cigar, seq, md), nm = KINDS[kind]
    lines = []
    for (cg, sq, m), n, flag in (((cigar, seq, md), nm, 131 & flag_mask), (CLEAN, 0, 67)):
        lines.append(f"{name}\t{flag}\t{ref}\t101\t60\t{cg}\t=\t101\t0\t{sq}\t{'I' * len(sq)}\tNM:i:{n}\tMD:Z:{m}\tNH:i:1{extra}")
    return lines


def mixedPairs(n, ref):
    cycle = ["clean", "busy", "clean", "nm5", "clean", "busy", "insertion"]
    lines = []
    for i in range(n):
        lines += pairOf(f"p{i:04d}", cycle[i % len(cycle)], ref)
    return lines


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """The index of the hand-made files, their header (with one reference the index does not have) and a writer."""
    from bamwriter import samToBam
    sidx, gidx = smallIndex()
    header = headerOf(sidx) + ["@SQ\tSN:OTHER\tLN:5000"]
    folder = tmp_path_factory.mktemp("ingest")
    count = [0]

    def write(lines):
        count[0] += 1
        path = str(folder / f"f{count[0]}.bam")
        samToBam(header + lines, path, block=20000)
        return path

    def layout(lines):
        """(length of the inflated stream, offset of every record in it): the stream an open file holds is the file's,
        header included, and a record starts behind its length word."""
        import struct
        from bamwriter import bamBytes
        raw = bamBytes(header + lines)
        starts, at = [], len(bamBytes(header))
        while at < len(raw):
            starts.append(at + 4)
            at += 4 + struct.unpack_from("<I", raw, at)[0]
        assert at == len(raw) and len(starts) == len(lines)
        return len(raw), starts

    write.layout = layout
    return gidx, sidx.genes[0], write


def check(path, gidx, device, expect_ok=None, forced_host=False):
    """packBam, packBamPlainHost and packBamDevice (with the records kept) on one file; returns the device's report.
    ``forced_host``: the hook that keeps every file off the device is set."""
    want, _, _ = outcome(lambda: packed.packBam(path, gidx))
    rehearsal, plain, _ = outcome(lambda: packed.packBamPlainHost(path, gidx))
    got, decode, mates = outcome(lambda: packed.packBamDevice(path, gidx, device, keep_device=True))
    assert rehearsal == want
    assert got == want
    if expect_ok is not None:
        assert (want[0] == "ok") == expect_ok, want[:3]
    if want[0] != "ok":
        return None
    n_pairs = want[4]["pairs"]
    assert decode["device_pairs"] + decode["host_pairs"] == n_pairs
    assert decode["device_pairs"] == (0 if forced_host else plain["plain_pairs"]), (decode, plain)
    assert decode["route"] == ("device" if decode["device_pairs"] or not n_pairs else "host")
    assert mates.shape == (2 * n_pairs,) and mates.download().tobytes() == want[1]
    mates.free()
    plain_too, decode_too, none = outcome(lambda: packed.packBamDevice(path, gidx, device))
    assert plain_too == want and decode_too == decode and none is None
    return decode


@pytest.mark.parametrize("n_pairs", [0, 1, 31, 32, 33, 127, 128, 129])
def test_wave_and_block_edges(world, device, n_pairs):
    gidx, ref, write = world
    decode = check(write(mixedPairs(n_pairs, ref)), gidx, device, expect_ok=True)
    n_host = sum(1 for i in range(n_pairs) if i % 7 == 6)
    assert decode["host_pairs"] == n_host and decode["device_pairs"] == n_pairs - n_host


def test_records_that_pair_into_nothing(world, device):
    gidx, ref, write = world
    lines = [pairOf(f"q{i}", "clean", ref)[0] for i in range(5)]
    decode = check(write(lines), gidx, device, expect_ok=True)
    assert decode == {"route": "device", "device_pairs": 0, "host_pairs": 0}


@pytest.mark.parametrize("last", ["insertion", "clean"])
def test_last_pair_of_the_file(world, device, last):
    gidx, ref, write = world
    lines = mixedPairs(5, ref) + pairOf("z", last, ref)
    decode = check(write(lines), gidx, device, expect_ok=True)
    assert decode["host_pairs"] == (1 if last == "insertion" else 0)


def test_record_starts_on_every_residue(world, device):
    """Names of 1 .. 4 characters and a tag whose length differs from mate to mate: the records of busy mates (mismatches,
    a deletion, every field of the walk) and of clean ones start on every residue mod 4, which the test checks."""
    gidx, ref, write = world
    lines = []
    for i, name in enumerate(("a", "bb", "ccc", "dddd", "e", "ff", "ggg", "hhhh")):
        left, right = pairOf(name, "busy", ref)
        lines += [left + "\tXX:Z:" + "a" * (i % 3), right + "\tXX:Z:" + "a" * ((3 * i + 1) % 4)]
    _, starts = write.layout(lines)
    for mate in (0, 1):              # the busy mates and the clean ones, each on all four residues
        assert {s % 4 for s in starts[mate::2]} == {0, 1, 2, 3}, [s % 4 for s in starts]
    decode = check(write(lines), gidx, device, expect_ok=True)
    assert decode["device_pairs"] == 8


@pytest.mark.parametrize("residue", [0, 1, 2, 3])
def test_stream_lengths_mod_4(world, device, residue):
    """The last record of the stream, a plain one, padded by a tag of 0 .. 3 characters until the inflated stream's
    length is `residue` mod 4 (checked): every shape of the uploaded stream's last word."""
    gidx, ref, write = world
    head = mixedPairs(3, ref)
    left, right = pairOf("z", "busy", ref)
    files = {}
    for pad in range(4):
        lines = head + [left, right + "\tXX:Z:" + "a" * pad]
        files[write.layout(lines)[0] % 4] = lines
    assert sorted(files) == [0, 1, 2, 3]
    lines = files[residue]
    length, starts = write.layout(lines)
    assert length % 4 == residue and starts[-1] == max(starts)
    decode = check(write(lines), gidx, device, expect_ok=True)
    assert decode["device_pairs"] == 4


@pytest.mark.parametrize("kind,flag_mask,done", [("nm5", 0xFFFF, True), ("busy", 0xFFFF & ~2, True),
                                                 ("ops14", 0xFFFF, True), ("ops15", 0xFFFF, False),
                                                 ("mm16", 0xFFFF, True), ("mm17", 0xFFFF, False),
                                                 ("events22", 0xFFFF, True), ("events23", 0xFFFF, False)])
def test_capacity_edges_and_header_only_pairs(world, device, kind, flag_mask, done):
    gidx, ref, write = world
    lines = pairOf("a", "clean", ref) + pairOf("b", kind, ref, flag_mask) + pairOf("c", "clean", ref)
    decode = check(write(lines), gidx, device, expect_ok=True)
    assert decode["device_pairs"] == (3 if done else 2)
    if kind == "nm5" or flag_mask != 0xFFFF:          # both records are header-only
        rec = packed.packBam(write(lines), gidx)[0]
        assert rec["n_cig"][2] == 0 and rec["n_cig"][3] == 0 and rec["n_mm"][2] == 0 and rec["n_cig"][0] == 1


def test_a_reference_that_is_no_backbone(world, device):
    gidx, ref, write = world
    lines = pairOf("a", "clean", ref) + pairOf("b", "clean", "OTHER") + pairOf("c", "clean", ref)
    assert check(write(lines), gidx, device, expect_ok=False) is None


def test_awkward_records(device, tmp_path):
    files, gidx = awkwardFiles(tmp_path)
    kinds = {}
    for tag, path, kind in files:
        want, _, _ = outcome(lambda: packed.packBam(path, gidx))
        got, decode, _ = outcome(lambda: packed.packBamDevice(path, gidx, device))
        assert got == want, tag
        kinds[tag] = want[0]
        if kind is not None:
            assert want[0] == kind, tag
        if want[0] == "ok":
            assert decode["route"] == "device" and decode["device_pairs"] >= 300 and decode["host_pairs"] >= 1, (tag, decode)
    assert len(kinds) == 17 and sum(k != "ok" for k in kinds.values()) >= 8


def test_sample_and_the_forced_host_route(small_case, device, tmp_path, monkeypatch):
    sidx, gidx, sample = small_case
    path = str(tmp_path / "small.bam")
    packed.writeBam(path, "\n".join(headerOf(sidx, "unsorted") + synth.toSamLines(sample)) + "\n")
    decode = check(path, gidx, device, expect_ok=True)
    print("device pairs", decode["device_pairs"], "of 4000")
    assert decode["route"] == "device" and decode["device_pairs"] >= 3600
    # a file the route may not take goes wholly through the host decode: the same bytes, on the device too when asked
    monkeypatch.setenv("GK_TEST_HOOKS", "ingest_device_max_bytes=1000")
    forced = check(path, gidx, device, expect_ok=True, forced_host=True)
    assert forced == {"route": "host", "device_pairs": 0, "host_pairs": 4000}


# ------------------------------------------------------------------------------------------------ the command line
def test_command_line_same_bytes(device, tmp_path, monkeypatch):
    """graphkir on two BAM samples with --no-variant-json, and again with --ingest-decode device: every output file holds
    the same bytes, and the log of the second run names the device route."""
    from kir_graph_amd import main as cli
    from kir_graph_amd.msa2hisat import Variant
    from kir_graph_amd.utils import logger
    novel_start = Variant.novel_id

    def runCli(name, sams, extra):
        Variant.novel_id = novel_start       # the numbering of novel variants is process-wide: both runs start alike
        run = tmp_path / name
        run.mkdir()
        monkeypatch.chdir(run)
        argv = ["--step-skip-extraction", "--index-folder", "../index", "--output-folder", "out", "--allele-strategy", "pv",
                "--cn-3dl3-not-diploid"] + [x for s in sams for x in ("--alignment", s)] + extra
        cli.main(cli.createParser().parse_args(argv))
        return {p.name: p for p in (run / "out").iterdir()}

    sidx = synth.makeIndex(seed=11, n_genes=3, var_range=(200, 300), allele_range=(12, 20))
    folder = tmp_path / "index"
    folder.mkdir()
    sidx.write(str(folder / "kir_2100_withexon_ab_2dl1s1.leftalign.mut01"))
    bams = []
    for k in range(2):
        s = synth.makeSample(sidx, seed=50 + k, n_pairs=2500)
        packed.writeBam(str(tmp_path / f"s{k}.bam"), "\n".join(headerOf(sidx, "unsorted") + synth.toSamLines(s)) + "\n")
        bams.append(f"../s{k}.bam")
    seen = []
    handler = logging.Handler()
    handler.emit = lambda record: seen.append(record.getMessage())
    logger.addHandler(handler)
    try:
        host = runCli("host", bams, ["--no-variant-json"])
        assert not any("Ingest decode" in m for m in seen)
        dev = runCli("device", bams, ["--no-variant-json", "--ingest-decode", "device"])
    finally:
        logger.removeHandler(handler)
    routes = [m for m in seen if "Ingest decode on the device route" in m]
    assert len(routes) == 2, seen
    assert set(host) == set(dev) and len(host) >= 8, sorted(host)
    assert sum(n.endswith(".npz") for n in host) == 2
    for n in host:                   # the hand-off files too: numpy stamps no time on an archive's members
        assert host[n].read_bytes() == dev[n].read_bytes(), n
