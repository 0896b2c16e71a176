"""GPU: the read bootstrap of the copy-number stage (gk_depth_weighted: depthw_mark, one scan, depthw_finish, depthw_select)
against the depth of the sample, against the restatement of tests/depthboot_reference.py, through
cn_bootstrap.bootstrapGeneDepths and through the command line.  Everything is an integer or a float made of integers in one
rounding: every comparison is an equality.

Pair counts follow the marking kernel (csrc/gk_depthboot.hip): one thread per mate, 256 threads per workgroup -- a
workgroup holds 128 pairs -- and kBootPerThread = 8 replicates per thread.  Depth values follow the digits of the radix
select (11 / 11 / 10 bits): boundaries at 2^21 and 2^10."""
import logging
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import depthboot_reference as dr  # noqa: E402

from kir_graph_amd import _lib, packed, synth  # noqa: E402
from kir_graph_amd import cn_bootstrap as cb  # noqa: E402
from kir_graph_amd.engine import DeviceIndex, Tabulation  # noqa: E402
from kir_graph_amd.hisat2 import SampleData, pairLines  # noqa: E402
from kir_graph_amd.kir_cn import aggrDepths, filterDepth, readSamtoolsDepth  # noqa: E402
from kir_graph_amd.samtools_utils import depthOfSample  # noqa: E402
from kir_graph_amd.utils import logger  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5A5A5A5
SENTINEL64 = 0xA5A5A5A5A5A5A5A5
POISON = 0xFFFFFFFF
TAIL = 16
FORMS = ("mates", "compact")
SEED = 2022


class Sample:
    """One sample tabulated from its 128-byte records and from its compact words: the same valid pairs either way."""

    def __init__(self, device, gidx, rec, spill=None):
        self.dev, self.gidx = device, gidx
        self.rec = np.ascontiguousarray(rec)
        self.wide = None if spill is None else spill[0]
        dindex = DeviceIndex(device, gidx)
        self.tabs = {"mates": Tabulation(dindex, self.rec, dev=device, spill=spill),
                     "compact": Tabulation(dindex, packed.CompactMates(self.rec, threads=2), dev=device, spill=spill)}
        assert isinstance(self.tabs["compact"].mates, packed.DeviceCompactMates)
        self.n_valid = self.tabs["mates"].n_valid
        assert self.n_valid == self.tabs["compact"].n_valid
        self.pair_src = self.tabs["mates"].pairSrc().copy()
        self.pair_nh = self.tabs["mates"].pairNH().copy()
        assert np.array_equal(self.pair_src, self.tabs["compact"].pairSrc())
        self._marks = {}

    def records(self, form):
        """(d_mates, d_compact) of one form; the compact tabulation never writes its 128-byte records."""
        mates = self.tabs[form].mates
        return (mates.ptr, 0) if form == "mates" else (0, mates.words.ptr)

    def depth(self, form, gene_off, multiple=0):
        """gk_depth / gk_depth_compact."""
        out = np.zeros(int(gene_off[-1]), dtype=np.uint32)
        tab = self.tabs[form]
        if form == "mates":
            _lib.check(_lib.lib().gk_depth(self.dev.ctx, tab.handle, tab.mates.ptr, multiple, gene_off.ctypes.data,
                                           len(gene_off) - 1, out.ctypes.data))
        else:
            _lib.check(_lib.lib().gk_depth_compact(self.dev.ctx, tab.handle, tab.mates.words.ptr, multiple, gene_off.ctypes.data,
                                                   len(gene_off) - 1, out.ctypes.data))
        return out.astype(np.int64)

    def weighted(self, form, W, gene_off, multiple=0, sel=None, rank=None, pad=5):
        """gk_depth_weighted with every host output pre-filled and a tail that must survive, the weights in a table of
        ``n_valid + pad`` columns whose entries beyond ``n_valid`` are 0xFFFFFFFF: (stat, sum, depth) as int64 / uint64."""
        W = np.asarray(W, dtype=np.int64).reshape(len(W), self.n_valid)
        n_boot, n_gene, total = len(W), len(gene_off) - 1, int(gene_off[-1])
        ldw = self.n_valid + pad
        table = np.full((n_boot, ldw), POISON, dtype=np.uint32)
        table[:, :self.n_valid] = W.astype(np.uint32)
        gene_off = np.ascontiguousarray(gene_off, dtype=np.int64)
        rank = np.ascontiguousarray(np.zeros((n_gene, 2)) if rank is None else rank, dtype=np.int64)
        sel = None if sel is None else np.ascontiguousarray(sel, dtype=np.uint8)
        stat = np.full(2 * n_boot * n_gene + TAIL, SENTINEL, dtype=np.uint32)
        total_out = np.full(n_boot * n_gene + TAIL, SENTINEL64, dtype=np.uint64)
        depth = np.full(n_boot * total + TAIL, SENTINEL, dtype=np.uint32)
        d_W = self.dev.put(table)
        d_mates, d_compact = self.records(form)
        try:
            _lib.check(_lib.lib().gk_depth_weighted(self.dev.ctx, self.tabs[form].handle, d_mates, d_compact, multiple,
                                                    gene_off.ctypes.data, n_gene, d_W.ptr, ldw, n_boot,
                                                    None if sel is None else sel.ctypes.data, rank.ctypes.data, stat.ctypes.data,
                                                    total_out.ctypes.data, depth.ctypes.data))
        finally:
            d_W.free()
        assert (stat[2 * n_boot * n_gene:] == SENTINEL).all() and (total_out[n_boot * n_gene:] == SENTINEL64).all()
        assert (depth[n_boot * total:] == SENTINEL).all()                  # nothing beyond the end is written
        return (stat[:2 * n_boot * n_gene].reshape(n_boot, n_gene, 2).astype(np.int64),
                total_out[:n_boot * n_gene].reshape(n_boot, n_gene), depth[:n_boot * total].reshape(n_boot, total).astype(np.int64))

    def marks(self, gene_off, multiple):
        key = (tuple(int(x) for x in gene_off), int(multiple))
        if key not in self._marks:
            self._marks[key] = dr.pairMarks(self.rec, self.pair_src, self.pair_nh, multiple, gene_off, wide=self.wide)
        return self._marks[key]

    def reference(self, W, gene_off, multiple=0):
        return dr.weightedDepth(self.marks(gene_off, multiple), W, int(gene_off[-1]))

    def close(self):
        for t in self.tabs.values():
            t.mates.free()
            t.close()


def offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def p75Ranks(gene_off, sel=None, q=0.75):
    n = np.diff(gene_off) if sel is None else np.add.reduceat((np.asarray(sel) != 0).astype(np.int64), gene_off[:-1])
    return np.array([cb.quantileRanks(q, int(x)) for x in n], dtype=np.int64)


@pytest.fixture(scope="module")
def records(small_case):
    sidx, gidx, s = small_case
    rec, table = packed.packSample(s, gidx)
    return np.ascontiguousarray(rec), table


@pytest.fixture(scope="module")
def real_off(small_case):
    sidx, gidx, _ = small_case
    return offsets([len(sidx.backbone[g]) for g in gidx.genes])


@pytest.fixture(scope="module")
def sample(device, small_case, records):
    out = Sample(device, small_case[1], records[0])
    yield out
    out.close()


@pytest.fixture(scope="module")
def wide_sample(device, small_case):
    sidx, gidx, s = small_case
    rng = np.random.default_rng(3)
    lines = synth.toSamLines(s)
    lines = synth.withManyMismatches(lines, sidx, rng.choice(s.n_pairs, size=40, replace=False).tolist(), rng)
    spill = []
    rec, _ = packed.packPairs(list(pairLines(lines)), gidx, spill=spill)
    wide = packed.spillArrays(spill)
    assert wide is not None and len(wide[1]) >= 3
    out = Sample(device, gidx, rec, spill=wide)
    yield out
    out.close()


@pytest.fixture(scope="module")
def subsamples(device, small_case, records, sample):
    """Samples of exactly n valid pairs: records of n valid pairs of the shared sample (NH == 1 and NH > 1 among them) mixed
    with pairs that fail the filter (the same records without the proper-pair flag), so a valid pair's index is not its
    source's."""
    made = {}

    def get(n_valid):
        if n_valid not in made:
            rng = np.random.default_rng(100 + n_valid)
            rec = records[0]
            keep = rng.permutation(sample.pair_src)[:n_valid]
            bad = rng.permutation(sample.pair_src)[:3 + n_valid // 10]
            order = [(int(p), True) for p in keep] + [(int(p), False) for p in bad]
            order = [order[i] for i in rng.permutation(len(order))]
            sub = np.zeros(2 * len(order), dtype=rec.dtype)
            for j, (p, good) in enumerate(order):
                sub[2 * j:2 * j + 2] = rec[2 * p:2 * p + 2]
                if not good:
                    sub["flag"][2 * j:2 * j + 2] &= np.uint16(0xFFFF ^ 2)
            made[n_valid] = Sample(device, small_case[1], sub)
            assert made[n_valid].n_valid == n_valid
        return made[n_valid]

    yield get
    for s in made.values():
        s.close()


# ------------------------------------------------------------------------------------------------ unit weights
@pytest.mark.parametrize("multiple", [0, 1])
def test_unit_weights_give_the_depth_of_the_sample(sample, wide_sample, real_off, multiple):
    for name, smp in (("plain", sample), ("wide", wide_sample)):
        ones = np.ones((1, smp.n_valid), dtype=np.int64)
        want = {form: smp.depth(form, real_off, multiple) for form in FORMS}
        assert np.array_equal(want["mates"], want["compact"]) and want["mates"].sum() > 100 * smp.n_valid
        for form in FORMS:
            stat, total, depth = smp.weighted(form, ones, real_off, multiple, rank=p75Ranks(real_off))
            assert np.array_equal(depth[0], want[form]), (name, form)
            assert [int(x) for x in total[0]] == [int(want[form][a:b].sum()) for a, b in zip(real_off[:-1], real_off[1:])]
    # the inputs are what the test means them to be: pairs with NH > 1 change the depth, wide pairs carry depth of their own
    assert (sample.pair_nh != 1).any()
    if multiple:
        assert not np.array_equal(sample.depth("mates", real_off, 1), sample.depth("mates", real_off, 0))
    is_wide = wide_sample.rec["n_cig"][2 * wide_sample.pair_src] == 0xFF
    assert is_wide.any()
    narrow = dr.weightedDepth(dr.pairMarks(wide_sample.rec, wide_sample.pair_src, wide_sample.pair_nh, 1, real_off, wide=None),
                              np.ones((1, wide_sample.n_valid)), int(real_off[-1]))
    if multiple:
        assert narrow.sum() < wide_sample.depth("mates", real_off, 1).sum()


# ------------------------------------------------------------------------------------------------ the restatement
def weightKinds(rng, n_boot, n_valid):
    if n_valid == 0:
        return {"none": np.zeros((n_boot, 0), dtype=np.int64)}
    one = np.zeros((n_boot, n_valid), dtype=np.int64)
    one[np.arange(n_boot), rng.integers(0, n_valid, n_boot)] = 1 << 24
    return {"zeros": np.zeros((n_boot, n_valid), dtype=np.int64), "mixed": rng.integers(0, 2, (n_boot, n_valid)),
            "65535": np.full((n_boot, n_valid), 65535, dtype=np.int64), "one_2^24": one}


@pytest.mark.parametrize("n_boot", [1, 2, 5])
@pytest.mark.parametrize("n_valid", [0, 1, 2, 127, 128, 129, 257])
def test_kernel_equals_the_restatement(subsamples, real_off, n_valid, n_boot):
    smp = subsamples(n_valid)
    rng = np.random.default_rng(1000 * n_valid + n_boot)
    n_gene = len(real_off) - 1
    case = 0
    for lens in ([1] * n_gene, [37] * n_gene, np.diff(real_off)):       # the short ones clip most runs at both ends
        gene_off = offsets(lens)
        rank = p75Ranks(gene_off)
        for kind, W in weightKinds(rng, n_boot, n_valid).items():
            multiple = case % 2
            case += 1
            want = smp.reference(W, gene_off, multiple)
            want_stat, want_sum = dr.select(want, gene_off, None, rank)
            for form in FORMS:
                stat, total, depth = smp.weighted(form, W, gene_off, multiple, rank=rank, pad=1 + case % 7)
                where = (form, kind, multiple, tuple(lens)[:1])
                assert np.array_equal(depth, want), where
                assert np.array_equal(stat, want_stat), where
                assert [int(x) for x in total.ravel()] == [int(x) for x in want_sum.ravel()], where
            if kind == "65535" and lens[0] > 37 and n_valid >= 257:
                assert want.max() > 65535                                # several pairs over one position
            if kind == "zeros":
                assert not want.any()
    assert case == (3 if n_valid == 0 else 12)


def test_eight_replicates_per_thread_and_a_ninth(subsamples, real_off):
    """9 replicates: the second group of a thread's replicates (kBootPerThread = 8) holds one."""
    smp = subsamples(129)
    W = np.random.default_rng(9).integers(0, 4, (9, 129))
    want = smp.reference(W, real_off)
    for form in FORMS:
        assert np.array_equal(smp.weighted(form, W, real_off)[2], want), form
    assert len({tuple(row) for row in want}) == 9


# ------------------------------------------------------------------------------------------------ selection
def selVariants(small_case, real_off):
    sidx, gidx, _ = small_case
    exon = cb.regionMask(list(gidx.genes), real_off, sidx.exons)
    one_empty = np.ones(int(real_off[-1]), dtype=np.uint8)
    one_empty[real_off[1]:real_off[2]] = 0
    one_position = np.zeros(int(real_off[-1]), dtype=np.uint8)
    one_position[(real_off[:-1] + np.diff(real_off) // 2)] = 7                  # any non-zero byte selects
    assert 0 < exon.sum() < len(exon)
    return {"all": None, "exon": exon, "one_gene_empty": one_empty, "one_position": one_position}


def rankPairs(gene_off, sel):
    n = (np.diff(gene_off) if sel is None else np.add.reduceat((np.asarray(sel) != 0).astype(np.int64), gene_off[:-1])).astype(np.int64)
    last = np.maximum(n - 1, 0)
    return {"first": np.stack([0 * n, 0 * n], axis=1), "last": np.stack([last, last], axis=1),
            "p75": p75Ranks(gene_off, sel), "median": p75Ranks(gene_off, sel, 0.5)}


@pytest.mark.parametrize("regime", ["all_equal", "below_2^10", "across_2^10_2^11", "across_2^21_2^22"])
def test_selection_is_exact(sample, small_case, real_off, regime):
    rng = np.random.default_rng(5)
    n = sample.n_valid
    unit = sample.reference(np.ones((1, n)), real_off)[0]
    top = int(unit.max())
    assert 8 <= top < 1 << 10
    scale = {"all_equal": 0, "below_2^10": 1, "across_2^10_2^11": (3 << 10) // top, "across_2^21_2^22": (3 << 21) // top}[regime]
    # three replicates: every pair the same weight, weights 0 .. 2 scale, and a third with many distinct depths
    W = np.stack([np.full(n, scale), rng.integers(0, 2 * scale + 1, n), rng.integers(0, scale + 1, n)]).astype(np.int64)
    want = sample.reference(W, real_off)
    if regime == "all_equal":
        assert not want.any()
    elif regime == "below_2^10":
        assert want.max() < 1 << 10
    elif regime == "across_2^10_2^11":
        assert want.max() > 1 << 11 and ((want > 0) & (want < 1 << 10)).any() and ((want > 1 << 10) & (want < 1 << 11)).any()
    else:
        assert want.max() > 1 << 22 and ((want > 0) & (want < 1 << 21)).any() and ((want > 1 << 21) & (want < 1 << 22)).any()
    for sel_name, sel in selVariants(small_case, real_off).items():
        for rank_name, rank in rankPairs(real_off, sel).items():
            want_stat, want_sum = dr.select(want, real_off, sel, rank)
            for form in FORMS:
                stat, total, depth = sample.weighted(form, W, real_off, sel=sel, rank=rank)
                where = (regime, sel_name, rank_name, form)
                assert np.array_equal(depth, want), where
                assert np.array_equal(stat, want_stat), where
                assert total.dtype == np.uint64 and [int(x) for x in total.ravel()] == [int(x) for x in want_sum.ravel()], where
            if sel_name == "one_gene_empty":
                assert not want_stat[:, 1].any() and not any(want_sum[:, 1])
    if regime == "across_2^21_2^22":
        assert max(int(x) for x in dr.select(want, real_off, None, rankPairs(real_off, None)["first"])[1].ravel()) > 1 << 32


def test_ranks_inside_runs_of_equal_values(sample, real_off):
    """The depth of the sample holds a few dozen distinct values, each many times: ranks from the first position to the last
    of the shortest gene, two neighbours at a time."""
    ones = np.ones((1, sample.n_valid), dtype=np.int64)
    want = sample.reference(ones, real_off)
    shortest = int(np.diff(real_off).min())
    assert len(np.unique(want)) < 100 < shortest
    for r in list(range(0, shortest - 1, shortest // 25)) + [shortest - 2]:
        rank = np.array([[r, r + 1]] * (len(real_off) - 1), dtype=np.int64)
        want_stat, _ = dr.select(want, real_off, None, rank)
        stat, _, _ = sample.weighted("compact", ones, real_off, rank=rank)
        assert np.array_equal(stat, want_stat), r


# ------------------------------------------------------------------------------------------------ composition
@pytest.fixture(scope="module")
def tabulated(device, small_case, records):
    sidx, gidx, s = small_case
    rec, table = records
    tab = Tabulation(DeviceIndex(device, gidx), packed.CompactMates(rec, threads=2), dev=device)
    gene_len = {g: len(sidx.backbone[g]) for g in sidx.genes}
    yield SampleData(tab, gidx, tab.novelVariants(table.strings)), gene_len
    tab.mates.free()
    tab.close()


@pytest.fixture(scope="module")
def replicate_depths(sample, real_off):
    """The restatement's tracks of the first 3 replicates of the documented generator, and of unit weights."""
    W = dr.weights(SEED, range(3), sample.n_valid)
    assert W.shape == (3, sample.n_valid) and (W.sum(axis=1) == sample.n_valid).all()
    return sample.reference(W, real_off), sample.reference(np.ones((1, sample.n_valid)), real_off)


@pytest.mark.parametrize("with_regions", [False, True])
@pytest.mark.parametrize("mode", ["p75", "mean", "median"])
def test_bootstrap_equals_the_restatement(small_case, tabulated, sample, real_off, replicate_depths, mode, with_regions):
    sidx, gidx, _ = small_case
    data, gene_len = tabulated
    assert data.tab.n_valid == sample.n_valid
    regions = sidx.exons if with_regions else None
    sel = cb.regionMask(list(gidx.genes), real_off, regions) if with_regions else None
    boot = cb.bootstrapGeneDepths(data, gene_len, 3, seed=SEED, select_mode=mode, regions=regions)
    assert boot.genes == list(gidx.genes) and boot.seed == SEED and boot.select_mode == mode
    assert boot.replicates.dtype == np.float64 and boot.replicates.shape == (3, len(gidx.genes))
    reps, unit = replicate_depths
    assert np.array_equal(boot.replicates, dr.statistic(reps, real_off, sel, mode))
    assert np.array_equal(boot.point, dr.statistic(unit, real_off, sel, mode)[0])
    assert (boot.point > 0).all()
    if mode == "mean":
        assert len({tuple(r) for r in boot.replicates}) == 3


def test_a_replicate_depends_on_seed_and_number_alone(tabulated, real_off):
    data, gene_len = tabulated
    three = cb.bootstrapGeneDepths(data, gene_len, 3, seed=SEED)
    seven = cb.bootstrapGeneDepths(data, gene_len, 7, seed=SEED)
    assert np.array_equal(seven.replicates[:3], three.replicates) and np.array_equal(seven.point, three.point)
    for k in (1, 2):
        assert np.array_equal(cb.bootstrapGeneDepths(data, gene_len, 7, seed=SEED, slice=k).replicates, seven.replicates), k
    other = cb.bootstrapGeneDepths(data, gene_len, 3, seed=SEED + 1)
    assert not np.array_equal(other.replicates, three.replicates) and np.array_equal(other.point, three.point)
    # the library's own slices: a budget that holds the arrays of two replicates
    before = os.environ.get("GK_TEST_HOOKS")
    os.environ["GK_TEST_HOOKS"] = f"depthw_budget={2 * 2 * 4 * (int(real_off[-1]) + 1)}"
    try:
        dev = data.tab.dev
        dev.profEnable(True)
        dev.profCollect()
        sliced = cb.bootstrapGeneDepths(data, gene_len, 7, seed=SEED)
        ran = dev.profCollect()
        dev.profEnable(False)
    finally:
        if before is None:
            del os.environ["GK_TEST_HOOKS"]
        else:
            os.environ["GK_TEST_HOOKS"] = before
    assert np.array_equal(sliced.replicates, seven.replicates)
    assert ran["depthw_mark"][0] == 1 + 4 and ran["depthw_select"][0] == 1 + 4          # the point, then 2 + 2 + 2 + 1


@pytest.mark.parametrize("with_regions", [False, True])
def test_point_equals_pandas_on_the_depth_file(small_case, tabulated, tmp_path, with_regions):
    sidx = small_case[0]
    data, gene_len = tabulated
    path = str(tmp_path / "s.depth.tsv")
    depthOfSample(data, gene_len, path, want_frame=False)
    if with_regions:
        filterDepth(path, str(tmp_path / "s.depth.exon.tsv"), sidx.exons)
        path = str(tmp_path / "s.depth.exon.tsv")
    for mode in ("p75", "mean", "median"):
        want = aggrDepths(readSamtoolsDepth(path), select_mode=mode)
        want = dict(zip(want["gene"], want["depth"]))
        boot = cb.bootstrapGeneDepths(data, gene_len, 1, select_mode=mode, regions=sidx.exons if with_regions else None)
        assert list(want) == sorted(boot.genes)
        for g, gene in enumerate(boot.genes):
            assert float(boot.point[g]).hex() == float(want[gene]).hex(), (mode, gene)


def test_overlapping_regions_are_refused(small_case, tabulated):
    sidx = small_case[0]
    data, gene_len = tabulated
    gene = data.index.genes[1]
    regions = {g: list(r) for g, r in sidx.exons.items()}
    s, e = regions[gene][0]
    regions[gene] = regions[gene] + [(e, e + 5)]                       # shares position e with the first exon
    with pytest.raises(ValueError):
        cb.bootstrapGeneDepths(data, gene_len, 2, regions=regions)
    with pytest.raises(ValueError):
        cb.bootstrapGeneDepths(data, gene_len, 0)
    with pytest.raises(ValueError):
        cb.bootstrapGeneDepths(data, gene_len, 10001)


def test_arguments_are_checked(sample, real_off):
    dev, tab = sample.dev, sample.tabs["mates"]
    n, n_gene, total = sample.n_valid, len(real_off) - 1, int(real_off[-1])
    ldw = n + 3
    d_W = dev.put(np.ones((2, ldw), dtype=np.uint32))
    stat = np.full(4 * n_gene + TAIL, SENTINEL, dtype=np.uint32)
    total_out = np.full(2 * n_gene + TAIL, SENTINEL64, dtype=np.uint64)
    depth = np.full(2 * total + TAIL, SENTINEL, dtype=np.uint32)
    lib, ctx, h = _lib.lib(), dev.ctx, tab.handle
    m, c = tab.mates.ptr, sample.tabs["compact"].mates.words.ptr
    off, w, s, t, d = real_off.ctypes.data, d_W.ptr, stat.ctypes.data, total_out.ctypes.data, depth.ctypes.data
    good = np.zeros((n_gene, 2), dtype=np.int64)
    negative, beyond = good.copy(), good.copy()
    negative[2, 0] = -1
    beyond[1, 1] = real_off[2] - real_off[1]
    sel = np.ones(total, dtype=np.uint8)
    sel[real_off[1] + 10:real_off[2]] = 0                               # 10 positions of gene 1 are selected
    beyond_sel = good.copy()
    beyond_sel[1, 0] = 10
    r = good.ctypes.data
    call = lib.gk_depth_weighted
    bad = [
        lambda: call(ctx, h, m, c, 0, off, n_gene, w, ldw, 2, None, r, s, t, d),              # both forms
        lambda: call(ctx, h, 0, 0, 0, off, n_gene, w, ldw, 2, None, r, s, t, d),              # neither
        lambda: call(ctx, h, m, 0, 0, off, n_gene, w, ldw, 0, None, r, s, t, d),
        lambda: call(ctx, h, m, 0, 0, off, n_gene, w, ldw, -1, None, r, s, t, d),
        lambda: call(ctx, h, m, 0, 0, off, n_gene, w, ldw, 10001, None, r, s, t, d),
        lambda: call(ctx, h, m, 0, 0, off, n_gene, w, n - 1, 2, None, r, s, t, d),            # ldw < n_valid
        lambda: call(ctx, h, m, 0, 0, off, n_gene, w, ldw, 2, None, negative.ctypes.data, s, t, d),
        lambda: call(ctx, h, m, 0, 0, off, n_gene, w, ldw, 2, None, beyond.ctypes.data, s, t, d),
        lambda: call(ctx, h, m, 0, 0, off, n_gene, w, ldw, 2, sel.ctypes.data, beyond_sel.ctypes.data, s, t, d),
        lambda: call(ctx, h, m, 0, 0, off, n_gene, w, ldw, 2, None, r, None, t, d),           # null outputs
        lambda: call(ctx, h, m, 0, 0, off, n_gene, w, ldw, 2, None, r, s, None, d),
        lambda: call(ctx, h, m, 0, 0, off, n_gene, w, ldw, 2, None, None, s, t, d),
        lambda: call(ctx, h, m, 0, 0, None, n_gene, w, ldw, 2, None, r, s, t, d),
        lambda: call(ctx, h, m, 0, 0, off, n_gene, 0, ldw, 2, None, r, s, t, d),              # null weights
        lambda: call(ctx, h, m, 0, 0, off, 0, w, ldw, 2, None, r, s, t, d),
        lambda: call(ctx, None, m, 0, 0, off, n_gene, w, ldw, 2, None, r, s, t, d),
    ]
    dev.profEnable(True)
    dev.profCollect()
    for k, f in enumerate(bad):
        assert f() == -3, k                                          # GK_ERR_ARG
        assert lib.gk_last_error(), k
    launched = dev.profCollect()
    dev.profEnable(False)
    assert not any(name.startswith("depthw_") for name in launched), launched      # nothing was launched
    assert (stat == SENTINEL).all() and (total_out == SENTINEL64).all() and (depth == SENTINEL).all()
    # the context still works; a rank inside the selected positions is taken, a null depth_out is allowed
    beyond_sel[1, 0] = 9
    _lib.check(call(ctx, h, m, 0, 0, off, n_gene, w, ldw, 2, sel.ctypes.data, beyond_sel.ctypes.data, s, t, None))
    want = sample.reference(np.ones((2, n)), real_off)
    want_stat, want_sum = dr.select(want, real_off, sel, beyond_sel)
    assert np.array_equal(stat[:4 * n_gene].reshape(2, n_gene, 2), want_stat) and (stat[4 * n_gene:] == SENTINEL).all()
    assert [int(x) for x in total_out[:2 * n_gene]] == [int(x) for x in want_sum.ravel()] and (depth == SENTINEL).all()
    d_W.free()


def test_a_tabulation_without_pair_sources_is_refused(device, tabulated, real_off, tmp_path):
    """A hand-off file gives a tabulation that has lists but no pair sources: GK_ERR_ARG, and the module says why."""
    from kir_graph_amd.hisat2 import loadCompact, writeCompact
    data, gene_len = tabulated
    path = str(tmp_path / "s.variant.npz")
    writeCompact(data, path)
    back = loadCompact(path, device, index=data.index)
    try:
        assert not cb.hasRecords(back)
        with pytest.raises(ValueError):
            cb.bootstrapGeneDepths(back, gene_len, 2)
        n_gene = len(real_off) - 1
        d_W = device.put(np.ones((1, max(back.tab.n_valid, 1)), dtype=np.uint32))
        rank = np.zeros((n_gene, 2), dtype=np.int64)
        stat, total = np.zeros(2 * n_gene, dtype=np.uint32), np.zeros(n_gene, dtype=np.uint64)
        rc = _lib.lib().gk_depth_weighted(device.ctx, back.tab.handle, data.tab.mates.words.ptr, 0, 0, real_off.ctypes.data, n_gene,
                                          d_W.ptr, max(back.tab.n_valid, 1), 1, None, rank.ctypes.data, stat.ctypes.data,
                                          total.ctypes.data, None)
        d_W.free()
        assert rc == -3
    finally:
        back.tab.close()


# ------------------------------------------------------------------------------------------------ the drivers
def makeCohort(tmp_path):
    """Two small samples as name-collated SAM text beside an index folder; the command lines below name both relative to the
    working directory (see tests/test_gpu_cn_cli.py)."""
    import gzip
    sidx = synth.makeIndex(seed=11, n_genes=3, var_range=(200, 300), allele_range=(12, 20))
    folder = tmp_path / "index"
    folder.mkdir()
    sidx.write(str(folder / "kir_2100_withexon_ab_2dl1s1.leftalign.mut01"))
    sams = []
    for k in range(2):
        s = synth.makeSample(sidx, seed=50 + k, n_pairs=2500)
        with gzip.open(tmp_path / f"s{k}.sam.gz", "wt") as f:
            f.write("@HD\tVN:1.0\tSO:queryname\n" + "".join(f"@SQ\tSN:{g}\tLN:{len(sidx.backbone[g])}\n" for g in sidx.genes) +
                    "\n".join(synth.toSamLines(s)) + "\n")
        sams.append(f"../s{k}.sam.gz")
    return sidx, sams


NOVEL_START: dict = {}


def runCli(cli, monkeypatch, tmp_path, name, sams, extra):
    from kir_graph_amd.msa2hisat import Variant
    # the numbering of novel variants is process-wide: every run starts where the first one started, as a fresh process would
    NOVEL_START.setdefault("id", Variant.novel_id)
    Variant.novel_id = NOVEL_START["id"]
    run = tmp_path / name
    run.mkdir()
    monkeypatch.chdir(run)
    argv = ["--step-skip-extraction", "--index-folder", "../index", "--output-folder", "out", "--allele-strategy", "pv",
            "--cn-3dl3-not-diploid"] + [x for s in sams for x in ("--alignment", s)] + extra
    cli.main(cli.createParser().parse_args(argv))
    return {p.name: p for p in (run / "out").iterdir()}


def readTable(path):
    lines = path.read_text().split("\n")
    assert lines[0].startswith("# conditional on the copy-number model") and lines[-1] == ""
    return lines[1].split("\t"), [line.split("\t") for line in lines[2:-1]]


def checkConfidence(files, sidx, n_boot, cn_suffix):
    boots = sorted(n for n in files if n.endswith(".boot.tsv"))
    confs = sorted(n for n in files if n.endswith(cn_suffix + ".confidence.tsv"))
    assert len(boots) == 2 and len(confs) == 2, sorted(files)
    for boot_name, conf_name in zip(boots, confs):
        boot = cb.readDepthBootstrap(str(files[boot_name]))
        assert boot.genes == list(sidx.genes) and boot.replicates.shape == (n_boot, len(sidx.genes)) and boot.seed == SEED
        cn_name = conf_name[:-len(".confidence.tsv")] + ".tsv"
        cn_lines = [line.split("\t") for line in files[cn_name].read_text().split("\n") if line]
        assert cn_lines[0] == ["gene", "cn", "depth"]
        header, rows = readTable(files[conf_name])
        assert header == cb.CN_CONFIDENCE_COLUMNS and [r[0] for r in rows] == list(sidx.genes)
        by_gene = {g: (int(c), float(d)) for g, c, d in cn_lines[1:]}
        for r, point in zip(rows, boot.point):
            row = dict(zip(header, r))
            assert (int(row["cn"]), float(row["depth"])) == by_gene[row["gene"]] and float(row["depth"]) == point
            assert 0.0 <= float(row["support"]) <= 1.0 and int(row["cn_lo"]) <= int(row["cn_hi"])
            assert float(row["depth_lo"]) <= float(row["depth_hi"]) and float(row["depth_sd"]) >= 0.0
            if row["alt_cn"] == "":
                assert row["alt_share"] == "" and float(row["support"]) == 1.0 and row["cn_lo"] == row["cn_hi"] == row["cn"]
            else:
                assert int(row["alt_cn"]) != int(row["cn"]) and 0.0 < float(row["alt_share"]) <= 1.0 - float(row["support"])
    header, rows = readTable(files["cohort.cn.confidence.tsv"])
    assert header == ["name"] + cb.CN_CONFIDENCE_COLUMNS and len(rows) == 2 * len(sidx.genes)
    want = []
    for conf_name in confs:                                          # cohort order = the order of the command line
        cn_file = conf_name[:-len(".confidence.tsv")] + ".tsv"
        want += [[next(r for r in rows if r[0].endswith(cn_file))[0]] + r for r in readTable(files[conf_name])[1]]
    assert rows == want
    return boots, confs


def test_command_line_per_sample(device, tmp_path, monkeypatch):
    """graphkir on two samples with --cn-bootstrap 8, without the flag, and with it again under --step-skip-typing: the new
    files appear only when asked for, hold the CN file's numbers and are the same bytes on every run; nothing else moves."""
    from kir_graph_amd import main as cli
    sidx, sams = makeCohort(tmp_path)
    flagged = runCli(cli, monkeypatch, tmp_path, "flagged", sams, ["--cn-bootstrap", "8"])
    plain = runCli(cli, monkeypatch, tmp_path, "plain", sams, [])
    again = runCli(cli, monkeypatch, tmp_path, "again", sams, ["--cn-bootstrap", "8", "--cn-bootstrap-seed", "2022",
                                                             "--step-skip-typing"])
    boots, confs = checkConfidence(flagged, sidx, 8, ".p75.LCND")
    new = set(boots) | set(confs) | {"cohort.cn.confidence.tsv"}
    assert set(plain) == set(flagged) - new and not any(".boot." in n or ".confidence." in n for n in plain)
    for n in plain:                                                  # every other file: the same bytes
        assert plain[n].read_bytes() == flagged[n].read_bytes(), n
    kinds = (".depth.tsv", ".LCND.tsv", ".LCND.json", ".full.tsv", ".possible.tsv", ".variant.json", "cohort.cn.tsv", "cohort.allele.tsv")
    assert all(sum(n.endswith(k) for n in plain) >= 1 for k in kinds), sorted(plain)
    assert new <= set(again) and not any(n.endswith(".possible.tsv") for n in again)
    for n in new:
        assert again[n].read_bytes() == flagged[n].read_bytes(), n
    other = runCli(cli, monkeypatch, tmp_path, "other", sams[:1], ["--cn-bootstrap", "8", "--cn-bootstrap-seed", "7",
                                                                  "--step-skip-typing"])
    assert other[boots[0]].read_bytes() != flagged[boots[0]].read_bytes()


def test_command_line_cohort_exon_median_kde(device, tmp_path, monkeypatch):
    """--cn-cohort --cn-exon --cn-select median --cn-algorithm KDE: the pooled model assigns the replicates, the bootstrap
    follows the exon depths."""
    from kir_graph_amd import main as cli
    sidx, sams = makeCohort(tmp_path)
    files = runCli(cli, monkeypatch, tmp_path, "cohort", sams, ["--cn-bootstrap", "5", "--cn-cohort", "--cn-exon", "--cn-select",
                                                               "median", "--cn-algorithm", "KDE", "--step-skip-typing"])
    boots, confs = checkConfidence(files, sidx, 5, ".median.cohort.KDE")
    assert all(n.endswith(".depth.exon.boot.tsv") for n in boots)
    assert cb.readDepthBootstrap(str(files[boots[0]])).select_mode == "median"


def test_provided_copy_numbers_and_text_pairs(device, tmp_path, monkeypatch):
    """A sample whose copy numbers are provided gets one line of information and no file; a sample that arrives as text
    pairs (the samtools reader) gets one warning and no file."""
    from bamwriter import samToBam
    from kir_graph_amd import main as cli
    sidx, sams = makeCohort(tmp_path)
    s = synth.makeSample(sidx, seed=50, n_pairs=2500)
    (tmp_path / "s.cn.tsv").write_text("gene\tcn\n" + "".join(f"{g}\t{c}\n" for g, c in s.gene_cn.items()))
    seen = []
    handler = logging.Handler()
    handler.emit = lambda record: seen.append(record.getMessage())
    logger.addHandler(handler)
    try:
        files = runCli(cli, monkeypatch, tmp_path, "provided", sams[:1], ["--cn-bootstrap", "4", "--cn-provided", "../s.cn.tsv",
                                                                         "--step-skip-typing"])
        assert not any(".boot." in n or n.endswith(".confidence.tsv") and n != "cohort.cn.confidence.tsv" for n in files)
        assert len([m for m in seen if "cn bootstrap" in m and "provided" in m]) == 1
        assert readTable(files["cohort.cn.confidence.tsv"])[1] == []
        # the same sample as a BAM that the samtools reader would collate: pairs of SAM lines, no packed records
        lines = synth.toSamLines(s)
        header = ["@HD\tVN:1.0\tSO:coordinate"] + [f"@SQ\tSN:{g}\tLN:{len(sidx.backbone[g])}" for g in sidx.genes]
        for name in ("a.bam", "b.bam"):
            samToBam(header + sorted(lines, key=lambda l: (l.split("\t")[2], int(l.split("\t")[3]))), str(tmp_path / name))
        monkeypatch.setenv("GK_TEST_HOOKS", "bam_reader=samtools")
        monkeypatch.setattr(cli, "readPair", lambda source: pairLines(lines))
        del seen[:]
        files = runCli(cli, monkeypatch, tmp_path, "pairs", ["../a.bam", "../b.bam"], ["--cn-bootstrap", "4", "--step-skip-typing",
                                                                                      "--no-variant-json"])
    finally:
        logger.removeHandler(handler)
    assert any(n.endswith(".depth.tsv") for n in files) and any(n.endswith(".LCND.tsv") for n in files)
    assert not any(".boot." in n or n.endswith(".confidence.tsv") and n != "cohort.cn.confidence.tsv" for n in files)
    assert len([m for m in seen if "cn bootstrap" in m and "without packed records" in m]) == 1, seen
