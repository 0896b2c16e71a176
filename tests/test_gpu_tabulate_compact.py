"""``gk_tabulate_compact`` / ``gk_depth_compact``: a sample tabulated from its compact words (``gk_mates_compact_host``:
word offsets + the words the mates use) must give what the same sample gives as 128-byte records -- every count, flag,
offset, id, pair source, gene, NH and novel key, bit for bit -- and ``packed.CompactMates.toDevice`` hands out an object
that the tabulation, the depth and a parked sample read as it is and that still serves records to whoever asks.

Pass 1 stages the run of words of a workgroup's 256 mates in LDS up to ``_lib.COMPACT_STAGE_WORDS`` words and reads the
rest from global memory, so the hand-built cases put that cap on a mate boundary, inside a mate's mismatch words and far
inside the run (every mate full), and keep every mate at its minimum of three words."""
import gzip
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")
FIELDS = ("counts", "off", "ids", "pair_src", "pair_gene", "pair_nh", "novel_key")


def exposed(tab) -> dict:
    """Everything a tabulation exposes."""
    return {"counts": np.array([tab.n_pairs, tab.n_valid, tab.n_ids, tab.n_novel, int(tab.info.err_flags)]),
            "off": tab.offsets().copy(), "ids": tab.ids().copy(), "pair_src": tab.pairSrc().copy(),
            "pair_gene": tab.pairGene().copy(), "pair_nh": tab.pairNH().copy(), "novel_key": tab.novelKeys().copy()}


def both(device, dindex, rec, spill=None, correction=None, keep=False):
    """(from records, from compact words): ``exposed`` of the two tabulations of the same sample."""
    from kir_graph_amd.engine import Tabulation
    from kir_graph_amd.packed import CompactMates, DeviceCompactMates
    rec = np.ascontiguousarray(rec)
    a = Tabulation(dindex, rec, dev=device, spill=spill, correction=correction)
    b = Tabulation(dindex, CompactMates(rec, threads=2), dev=device, spill=spill, correction=correction)
    assert isinstance(b.mates, DeviceCompactMates) and b.mates._records is None      # nothing was expanded on the way
    out = exposed(a), exposed(b)
    if keep:
        return out + (a, b)
    for t in (a, b):
        t.mates.free()
        t.close()
    return out


def assert_equal(got_a: dict, got_b: dict, what=""):
    for f in FIELDS:
        assert np.array_equal(got_a[f], got_b[f]), (what, f)


@pytest.fixture(scope="module")
def synthetic(device):
    """bench.build_inputs(7, 3000): (index, device index, records, string table, copy numbers), made once."""
    sys.path.insert(0, ROOT)
    import bench
    from kir_graph_amd.engine import DeviceIndex
    sidx, gidx, sample, rec, table = bench.build_inputs(7, 3000)
    rec.setflags(write=False)
    dindex = DeviceIndex(device, gidx)
    yield gidx, dindex, rec, table, sample.gene_cn
    dindex.close()


# ---------------------------------------------------------------------------------------------- golden inputs
def _golden(name, device, tmp_path):
    from kir_graph_amd.hisat2 import extractVariant, pairLines
    from kir_graph_amd.index import GkIndex
    from kir_graph_amd.msa2hisat import Variant
    with gzip.open(os.path.join(GOLD, name), "rt") as f:
        case = json.load(f)
    for ext, body in case["index"].items():
        (tmp_path / f"ix.{ext}").write_text(body)
    gidx = GkIndex.load(str(tmp_path / "ix"))
    Variant.novel_id = 0
    data = extractVariant(pairLines(case["lines"]), gidx, dev=device)
    return case, data


@pytest.mark.parametrize("name", ["t1_tabulation.json.gz", "t12_wide.json.gz"])
def test_golden_records_tabulate_the_same_from_compact_words(device, tmp_path, name):
    """The records behind T1 and T12 (wide pairs, n_spill > 0, novel ids in first-appearance order)."""
    case, data = _golden(name, device, tmp_path)
    tab = data.tab
    rec = tab.mates.download()
    spill = getattr(tab, "_spill", None)
    if name.startswith("t12"):
        assert spill is not None and len(spill[1]) >= 8 and tab.n_novel > 1
    want = exposed(tab)
    got_rec, got_compact = both(device, tab.dindex, rec, spill=spill, correction=getattr(tab, "_correction", None))
    assert_equal(want, got_rec, "records again")
    assert_equal(want, got_compact, "compact")
    tab.close()


# ---------------------------------------------------------------------------------------------- hand-built runs
def _full(rec, at, rng):
    """Mates ``at`` become full: GK_MAX_CIG operations, GK_MAX_MM mismatches, GK_MAX_INS strings (32 words, 22 events)."""
    from kir_graph_amd._lib import CIG_I, CIG_M, MAX_CIG, MAX_INS, MAX_MM
    ops = []
    for k in range(MAX_INS):
        ops += [(10 << 4) | CIG_M, (1 << 4) | CIG_I]
    ops += [(10 << 4) | CIG_M] * (MAX_CIG - len(ops))           # 8 M runs: reference offsets [0, 80)
    rec["cig"][at] = np.array(ops, dtype=np.uint16)
    rec["n_cig"][at], rec["n_mm"][at], rec["n_ins"][at] = MAX_CIG, MAX_MM, MAX_INS
    rec["mm"]["ref_off"][at] = 5 * np.arange(MAX_MM) + 2
    rec["mm"]["base"][at] = rng.choice(np.frombuffer(b"ACGTN", np.uint8), size=(len(at), MAX_MM))
    rec["mm"]["rsv"][at] = 0
    rec["ins"][at] = rng.integers(0, 50, size=(len(at), MAX_INS))
    rec["flag"][at] |= 3
    rec["nm"][at] = 4


def _short(rec, at, n_mm=4):
    """Mates ``at`` become one M run with ``n_mm`` mismatches: 4 + n_mm words, index and novel substitutions, lists."""
    from kir_graph_amd._lib import CIG_M
    rec["cig"][at] = 0
    rec["cig"][at, 0] = (100 << 4) | CIG_M
    rec["n_cig"][at], rec["n_mm"][at], rec["n_ins"][at] = 1, n_mm, 0
    rec["mm"][at] = np.zeros((), rec["mm"].dtype)
    rec["mm"]["ref_off"][at, :n_mm] = 10 * np.arange(1, n_mm + 1)
    rec["mm"]["base"][at, :n_mm] = np.frombuffer(b"ACGTACGTACGTACGT", np.uint8)[:n_mm]
    rec["ins"][at] = 0
    rec["flag"][at] |= 3
    rec["nm"][at] = 2


def _words(rec) -> np.ndarray:
    """Words per mate of the compact form (the host packer's own offsets)."""
    from kir_graph_amd.packed import CompactMates
    c = CompactMates(np.ascontiguousarray(rec), threads=1)
    return np.diff(np.asarray(c.words[:c.n_mates + 1]).astype(np.int64))


@pytest.mark.parametrize("n_pairs", [0, 1, 127, 128, 129, 255, 256, 257])
def test_pair_counts_around_a_workgroup(device, synthetic, n_pairs):
    """A workgroup takes 256 mates = 128 pairs: none, one, one short of / exactly / one beyond one and two workgroups."""
    gidx, dindex, rec, _, _ = synthetic
    a, b = both(device, dindex, rec[:2 * n_pairs])
    assert a["counts"][0] == n_pairs and (n_pairs < 100 or a["counts"][2] > 0)
    assert_equal(a, b, n_pairs)


@pytest.mark.parametrize("case", ["min", "full", "cap on a mate boundary", "cap inside the mismatches",
                                  "an insertion without a string"])
def test_mates_at_the_extremes_of_the_staged_run(device, synthetic, case):
    from kir_graph_amd._lib import COMPACT_STAGE_WORDS as CAP
    gidx, dindex, src, _, _ = synthetic
    rng = np.random.default_rng(5)
    rec = src[:2 * 700].copy()
    if case == "min":            # header only: no CIGAR, no mismatch, no string
        rec["n_cig"] = rec["n_mm"] = rec["n_ins"] = 0
        rec["flag"] |= 3
        rec["nm"] = 0
        assert (_words(rec) == 3).all()
    elif case == "an insertion without a string":      # the CIGAR names an insertion, n_ins is 0: string id 0 in either form,
        from kir_graph_amd._lib import CIG_I, CIG_M      # not the word that follows the mate (the next mate's position)
        _short(rec, np.arange(len(rec)), n_mm=2)
        rec["cig"][:, :3] = np.array([(50 << 4) | CIG_M, (2 << 4) | CIG_I, (50 << 4) | CIG_M], dtype=np.uint16)
        rec["n_cig"] = 3
        assert (_words(rec) == 3 + 2 + 2).all() and (rec["pos0"] > 0).any()
    elif case == "full":         # 256 x 32 words per workgroup: most of every run lies beyond the cap
        _full(rec, np.arange(len(rec)), rng)
        assert (_words(rec) == 32).all() and 256 * 32 > CAP
    elif case == "cap on a mate boundary":
        assert CAP % 32 == 0
        _full(rec, np.arange(CAP // 32), rng)             # then the sample's own mates, the first of them at word CAP
        _short(rec, np.arange(CAP // 32, CAP // 32 + 8))
        assert int(_words(rec)[:CAP // 32].sum()) == CAP
    else:
        n = CAP // 32 - 1
        _full(rec, np.arange(n), rng)
        _short(rec, np.array([n]), n_mm=4)                # 8 words, then a full mate: header 3, CIGAR 7, mismatches 16
        _full(rec, np.array([n + 1]), rng)
        _short(rec, np.arange(n + 2, n + 10))
        start = int(_words(rec)[:n + 1].sum())
        assert start + 10 < CAP < start + 26              # the cap falls inside mate n + 1's mismatch words
    a, b = both(device, dindex, rec)
    assert a["counts"][1] > 0
    if case != "min":
        assert a["counts"][3] > 0                         # novel variants out of the hand-built words
    if case.startswith("cap"):
        assert a["counts"][2] > 0
    assert_equal(a, b, case)


def test_invalid_pairs(device, synthetic):
    """Flag without bit 2, NM absent, NM > 4, a clipped mate -- in one mate of a pair whose other mate is fine."""
    from kir_graph_amd._lib import CIG_M, CIG_S, NM_ABSENT
    gidx, dindex, src, _, _ = synthetic
    rec = src[:2 * 600].copy()
    fine = np.flatnonzero(((rec["flag"] & 2) != 0) & (rec["nm"] <= 4) & (rec["n_cig"] > 0) & (rec["n_cig"] < 14))
    fine = fine[np.isin(fine ^ 1, fine)]                  # both mates pass
    pairs = np.unique(fine >> 1)[:80]
    assert len(pairs) == 80
    for k, p in enumerate(pairs):
        m = 2 * p + (k >> 2 & 1)                          # left mate or right mate
        if k % 4 == 0:
            rec["flag"][m] &= ~np.uint16(2)
        elif k % 4 == 1:
            rec["nm"][m] = NM_ABSENT
        elif k % 4 == 2:
            rec["nm"][m] = 5
        else:                                             # a soft clip in front: the pair stays, the mate yields nothing
            n = int(rec["n_cig"][m])
            rec["cig"][m, 1:n + 1] = rec["cig"][m, :n].copy()
            rec["cig"][m, 0] = (5 << 4) | CIG_S
            rec["n_cig"][m] = n + 1
    a, b = both(device, dindex, rec)
    before, _ = both(device, dindex, src[:2 * 600])
    assert a["counts"][1] == before["counts"][1] - 60     # three of the four kinds take the pair away
    assert_equal(a, b)


def test_pileup_correction_table(device, synthetic):
    """The d_corr path: a table that rewrites a fifth of the (position, base) entries."""
    gidx, dindex, rec, _, _ = synthetic
    rng = np.random.default_rng(11)
    last = np.zeros(len(gidx.genes), dtype=np.int64)
    np.maximum.at(last, rec["ref"], rec["pos0"].astype(np.int64) + 400)
    pos0 = np.concatenate([[0], np.cumsum(last)]).astype(np.int64)
    table = np.where(rng.random((int(pos0[-1]), 5)) < 0.2, rng.choice(np.frombuffer(b"ACGT", np.uint8), (int(pos0[-1]), 5)),
                     0).astype(np.uint8)
    plain, _ = both(device, dindex, rec)
    a, b = both(device, dindex, rec, correction=(table, pos0))
    assert not np.array_equal(plain["ids"], a["ids"])     # the table did something
    assert_equal(a, b)


def _two_walks_child(out_path: str) -> None:
    """Child process under GK_TEST_HOOKS=two_walks: a small synthetic sample both ways -> .npz."""
    sys.path.insert(0, ROOT)
    from kir_graph_amd import _lib, packed, synth
    from kir_graph_amd.engine import DeviceIndex
    from kir_graph_amd.index import GkIndex
    assert os.environ.get("GK_TEST_HOOKS") == "two_walks"
    sidx = synth.makeIndex(seed=2022, n_genes=4, var_range=(300, 600), allele_range=(20, 40))
    gidx = GkIndex.fromVariants(sidx.variants, genes=sidx.genes, exons=sidx.exons)
    rec, _ = packed.packSample(synth.makeSample(sidx, seed=1031, n_pairs=700), gidx)
    dev = _lib.Device(0)
    dev.profEnable(True)
    a, b = both(dev, DeviceIndex(dev, gidx), rec)
    prof = dev.profCollect()
    arrays = {f"a_{f}": a[f] for f in FIELDS}
    arrays.update({f"b_{f}": b[f] for f in FIELDS})
    np.savez(out_path, tab_emit=np.array(prof.get("tab_emit", (0, 0.0))[0]), tab_expand=np.array(prof.get("tab_expand", (0, 0.0))[0]),
             **arrays)


def test_two_walk_fallback_in_a_fresh_process(tmp_path):
    """GK_TEST_HOOKS=two_walks: pass 2 walks the records again (tab_emit) -- from compact words they are expanded into a
    temporary buffer inside the call."""
    out = str(tmp_path / "two_walks.npz")
    env = dict(os.environ, GK_TEST_HOOKS="two_walks")
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "two_walks", out], env=env, capture_output=True, text=True,
                         timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    z = np.load(out)
    assert int(z["tab_emit"]) == 2 and int(z["tab_expand"]) == 0
    assert z["a_counts"][2] > 0
    for f in FIELDS:
        assert np.array_equal(z[f"a_{f}"], z[f"b_{f}"]), f


# ---------------------------------------------------------------------------------------------- a synthetic sample
def test_synthetic_sample_and_its_depth(device, synthetic):
    from kir_graph_amd._lib import check, lib
    gidx, dindex, rec, _, _ = synthetic
    a, b, tab_a, tab_b = both(device, dindex, rec, keep=True)
    assert a["counts"][1] > 2000 and a["counts"][3] > 0
    assert_equal(a, b)
    lens = np.zeros(len(gidx.genes), dtype=np.int64)
    np.maximum.at(lens, rec["ref"], rec["pos0"].astype(np.int64) + 100)      # some reads run past the end: clamped
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    for multiple in (0, 1):
        d_rec, d_compact, d_cross = (np.zeros(int(off[-1]), dtype=np.uint32) for _ in range(3))
        check(lib().gk_depth(device.ctx, tab_a.handle, tab_a.mates.ptr, multiple, off.ctypes.data, len(lens), d_rec.ctypes.data))
        check(lib().gk_depth_compact(device.ctx, tab_b.handle, tab_b.mates.words.ptr, multiple, off.ctypes.data, len(lens),
                                     d_compact.ctypes.data))
        # ... and the records' tabulation read with the compact words of the same sample
        check(lib().gk_depth_compact(device.ctx, tab_a.handle, tab_b.mates.words.ptr, multiple, off.ctypes.data, len(lens),
                                     d_cross.ctypes.data))
        assert d_rec.sum() > 0 and np.array_equal(d_rec, d_compact) and np.array_equal(d_rec, d_cross)
    assert tab_b.mates._records is None
    for t in (tab_a, tab_b):
        t.mates.free()
        t.close()


def test_depth_of_wide_pairs_from_compact_words(device, tmp_path):
    """T12: a mate whose pair is in the wide array carries that pair's place in word 3 of its compact form."""
    from kir_graph_amd.hisat2 import SampleData
    from kir_graph_amd.samtools_utils import depthOfSample
    case, data = _golden("t12_wide.json.gz", device, tmp_path)
    tab = data.tab
    rec = tab.mates.download()
    _, _, tab_a, tab_b = both(device, tab.dindex, rec, spill=tab._spill, keep=True)
    gene_len = {g: int(rec["pos0"].max()) + 6000 for g in data.index.genes}
    frames = [depthOfSample(SampleData(t, data.index, None), gene_len) for t in (tab_a, tab_b)]
    assert frames[0]["depth"].sum() > 0 and frames[0].equals(frames[1])
    assert tab_b.mates._records is None
    for t in (tab_a, tab_b, tab):
        t.mates.free()
        t.close()


@pytest.mark.parametrize("method", ["exonfirst", "em"])
def test_typing_through_compact_words_and_through_records(device, synthetic, method):
    """The 3000-pair sample typed from ``compact.toDevice(...)`` and from the plain records: calls and every array of
    ``bench.step_outputs`` are equal."""
    import bench
    from kir_graph_amd import cohort
    from kir_graph_amd.engine import Tabulation
    from kir_graph_amd.hisat2 import SampleData
    from kir_graph_amd.packed import CompactMates
    gidx, dindex, rec, table, gene_cn = synthetic
    got = []

    def finish(typer, calls, warn, item):
        got.append((list(calls), list(warn), bench.step_outputs(typer, calls, gidx)))
        typer._data.tab.close()

    for mates in (np.ascontiguousarray(rec), CompactMates(np.ascontiguousarray(rec), threads=2).toDevice(device, wait=True)):
        tab = Tabulation(dindex, mates, dev=device)
        sample = [(SampleData(tab, gidx, None, ins_strings=table.strings), gene_cn, 0)]
        for _ in cohort.typeSamples(sample, method, lanes=1, finish=finish):
            pass
        tab.mates.free()
    (calls_a, warn_a, out_a), (calls_b, warn_b, out_b) = got
    assert calls_a == calls_b and warn_a == warn_b and any(c for c in calls_a)
    assert sorted(out_a) == sorted(out_b)
    for k in out_a:
        assert np.array_equal(out_a[k], out_b[k]), k


# ---------------------------------------------------------------------------------------------- the device-side object
def test_lazy_expansion_and_parking(device, synthetic):
    """``.ptr`` / ``.download()`` expand once, under a lock; the records equal gk_mates_expand's byte for byte; a parked
    sample keeps the words as they are and comes back with the same lists."""
    from kir_graph_amd import _lib
    from kir_graph_amd._lib import check, lib
    from kir_graph_amd.engine import Tabulation
    from kir_graph_amd.hisat2 import ParkedRecords, SampleData
    from kir_graph_amd.packed import CompactMates
    gidx, dindex, rec, table, _ = synthetic
    host = CompactMates(np.ascontiguousarray(rec), threads=2)
    mates = host.toDevice(device, wait=True)
    assert mates.size == len(rec) and mates._records is None and mates.nbytes == host.nbytes
    want = device.alloc(len(rec), _lib.MATE_DTYPE)
    check(lib().gk_mates_expand(device.ctx, mates.words.ptr, len(rec), want.ptr))
    device.sync()
    ptrs = []
    threads = [threading.Thread(target=lambda: ptrs.append(mates.ptr)) for _ in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert len(ptrs) == 2 and ptrs[0] == ptrs[1] == mates._records.ptr and ptrs[0] != 0
    assert mates.download().tobytes() == want.download().tobytes()
    assert mates.nbytes == host.nbytes + rec.nbytes
    want.free()
    # parked: the same device words, no compaction kernel, and the same tabulation afterwards
    tab = Tabulation(dindex, mates, dev=device)
    first = exposed(tab)
    words_ptr = mates.words.ptr
    parked = ParkedRecords(SampleData(tab, gidx, None, ins_strings=table.strings))
    assert parked.ptr == words_ptr and parked.nbytes == host.nbytes and tab.mates is None and tab.handle is None
    assert np.array_equal(device.view(parked.ptr, len(host.words), np.uint32), host.words)
    back = parked.restore()
    assert parked.ptr == 0 and back.tab.mates.words.ptr == words_ptr and back.tab.mates._records is None
    assert_equal(first, exposed(back.tab))
    back.tab.mates.free()
    assert back.tab.mates.words is None
    back.tab.close()


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "two_walks":
    _two_walks_child(sys.argv[2])
