"""GPU: the per-allele coverage of a likelihood call (gk_call_coverage: callcov_mark, one scan, callcov_finish) against the
restatement of tests/callcov_reference.py, against the depth of the sample, and through TypingWithPosNegAllele and the
command line.  Everything is an integer: every comparison is an equality.

Row counts follow the marking kernels (csrc/gk_callcov.hip): one thread per mate, 256 threads per workgroup -- a wave holds
32 rows, a workgroup 128 (a workgroup of the LDS form takes 128 rows per turn).  The LDS form marks a gene whose track fits
a workgroup's LDS (gene_len <= LDS_MAX_LEN), the direct form the others and every gene under GK_CALLCOV=direct: both are
checked on every case."""
import logging
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import callcov_reference as cr  # noqa: E402
from test_gpu_call_fit import KINDS, makeTable  # noqa: E402

from kir_graph_amd import _lib, packed, synth  # noqa: E402
from kir_graph_amd.call_report import modelOf  # noqa: E402
from kir_graph_amd.call_coverage import (CALL_COVERAGE_COLUMNS, CALL_COVERAGE_DEPTH_COLUMNS, callCoverageDepthText,  # noqa: E402
                                         callCoverageText, coverCall, regionsOf)
from kir_graph_amd.engine import DeviceIndex, Tabulation  # noqa: E402
from kir_graph_amd.hisat2 import SampleData, pairLines  # noqa: E402
from kir_graph_amd.kir_typing import TypingWithPosNegAllele  # noqa: E402
from kir_graph_amd.utils import logger  # noqa: E402
from oracle import depth as odepth, tabulate as ot, typing as oty  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5A5A5A5
TAIL = 16
FORMS = ("mates", "compact")
MARKS = ("lds", "direct")                 # the LDS form where it fits (the default), the direct form forced
LDS_MAX_LEN = 144 * 1024 // 4 - 1         # kCovLdsBytes: gene_len + 1 words


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
        self.pair_src = self.tabs["mates"].pairSrc().copy()
        assert np.array_equal(self.pair_src, self.tabs["compact"].pairSrc())
        self.valid = {}
        for g in range(len(gidx.genes)):
            rows, n = self.tabs["mates"].selectGene(g)
            self.valid[g] = rows.download()[:n].copy()
            rows.free()

    def records(self, form):
        """(d_mates, d_compact) of one form; the compact tabulation never writes its 128-byte records."""
        mates = self.tabs[form].mates
        return (mates.ptr, 0) if form == "mates" else (0, mates.words.ptr)

    def coverage(self, form, rows, table, cols, gene, gene_len, mark="lds"):
        """gk_call_coverage with the host output pre-filled: uint32 [2 + 2K][gene_len]."""
        before = os.environ.pop("GK_CALLCOV", None)
        if mark == "direct":
            os.environ["GK_CALLCOV"] = "direct"
        try:
            return self._coverage(form, rows, table, cols, gene, gene_len)
        finally:
            os.environ.pop("GK_CALLCOV", None)
            if before is not None:
                os.environ["GK_CALLCOV"] = before

    def _coverage(self, form, rows, table, cols, gene, gene_len):
        n_table_cols, ldm = table.shape
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        n = (2 + 2 * len(cols)) * gene_len
        out = np.full(n + TAIL, SENTINEL, dtype=np.uint32)
        d_rows, d_table = self.dev.put(rows), self.dev.put(table)
        d_mates, d_compact = self.records(form)
        try:
            _lib.check(_lib.lib().gk_call_coverage(self.dev.ctx, self.tabs[form].handle, d_mates, d_compact, d_rows.ptr, len(rows),
                                                   d_table.ptr, ldm, n_table_cols, cols.ctypes.data, len(cols), gene, gene_len,
                                                   out.ctypes.data))
        finally:
            d_rows.free()
            d_table.free()
        assert (out[n:] == SENTINEL).all()                          # nothing beyond the end is written
        return out[:n].reshape(2 + 2 * len(cols), gene_len).astype(np.int64)

    def reference(self, rows, table, cols, gene, gene_len):
        return cr.tracks(self.rec, self.pair_src, rows, table, cols, gene, gene_len, wide=self.wide)

    def close(self):
        for t in self.tabs.values():
            t.mates.free()
            t.close()
        assert self.tabs["compact"].mates._records is None


@pytest.fixture(scope="module")
def sample(device, small_case):
    sidx, gidx, s = small_case
    rec, _ = packed.packSample(s, gidx)
    out = Sample(device, gidx, rec)
    yield out
    out.close()


def checkInvariants(got, k, tie_depth, where):
    info, mism, best, uniq = got[0], got[1], got[2:2 + k], got[2 + k:]
    assert (uniq <= best).all() and (best <= info[None, :]).all() and (mism <= info).all(), where
    # every row is in exactly one unique track or ties: unique_0 + ... + unique_K-1 + the rows with |A| > 1 = informative
    assert np.array_equal(uniq.sum(axis=0) + tie_depth, info), where
    assert int(uniq.sum()) + int(tie_depth.sum()) == int(info.sum()), where
    if k == 1:
        assert np.array_equal(best[0], info) and np.array_equal(uniq[0], info) and not tie_depth.any(), where


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("k", [1, 2, 3, 16])
@pytest.mark.parametrize("n_rows", [1, 2, 31, 32, 33, 127, 128, 129, 261])
def test_kernel_equals_the_restatement(sample, small_case, n_rows, k):
    sidx = small_case[0]
    rng = np.random.default_rng(1000 * n_rows + k)
    g = 1 + (n_rows + k) % 3
    real_len = len(sidx.backbone[sample.gidx.genes[g]])
    everyone = np.concatenate(list(sample.valid.values()))
    assert len(sample.valid[g]) >= 261
    kinds = KINDS + ("zeros",)
    case = 0
    for n_table_cols in (k, k + 3, 40):
        cols = rng.permutation(n_table_cols)[:k]                          # scattered and unordered
        for gene_len in (1, 37, real_len):                                # the short ones clip most runs at both ends
            # a scattered, unordered subset of the gene's valid pairs; at 37 of every gene's: other backbones mark nothing
            rows = rng.permutation(everyone if gene_len == 37 else sample.valid[g])[:n_rows]
            kind = kinds[(case + n_rows + k) % len(kinds)]          # every kind meets every length over the parameters
            pad = (7, 255)[case % 2]
            ldm = (n_rows + 63) // 64 * 64 + 64 * (case % 3 == 0)
            case += 1
            where = (n_table_cols, gene_len, kind, pad, ldm)
            if kind == "zeros":
                table = np.full((n_table_cols, ldm), pad, dtype=np.uint8)
                table[:, :n_rows] = 0
            else:
                table = makeTable(rng, kind, n_rows, n_table_cols, cols, ldm, pad)
            want = sample.reference(rows, table[:, :n_rows], cols, g, gene_len)
            m1, tie = cr.tieSets(table[:, :n_rows], cols)
            tied = np.flatnonzero(tie.sum(axis=1) > 1)
            tie_depth = sample.reference(rows[tied], np.zeros((1, len(tied)), dtype=np.uint8), [0], g, gene_len)[0]
            for form in FORMS:
                for mark in MARKS:
                    got = sample.coverage(form, rows, table, cols, g, gene_len, mark)
                    assert np.array_equal(got, want), (form, mark) + where
                    checkInvariants(got, k, tie_depth, (form, mark) + where)
                    if kind == "zeros":
                        assert not got[1].any(), where
            # the test's own data is what it is meant to be
            if kind == "out_of_range":
                assert (m1 == 255).any()                                  # all-255 rows: in `mismatch`, tied everywhere
                if gene_len == real_len:
                    assert want[1].any() and (k == 1 or tie_depth.any()), where
            if gene_len == real_len:
                assert want[0].sum() > 100 * n_rows, where                # both mates of every row, ~100 bases each
    assert case == 9


def test_runs_are_clipped_at_both_ends(sample, small_case):
    """A short gene_len cuts runs that straddle the end and drops runs that lie wholly beyond it."""
    g = 2
    rows = sample.valid[g][:200]
    pos0 = sample.rec["pos0"][2 * sample.pair_src[rows]].astype(np.int64)
    cut = int(np.sort(pos0)[100]) + 20                                   # inside the first run of one of the mates
    assert (pos0 >= cut).any() and ((pos0 < cut) & (pos0 + 60 > cut)).any()      # wholly beyond, and straddling
    table = np.zeros((1, 256), dtype=np.uint8)
    want = sample.reference(rows, table[:, :200], [0], g, cut)
    for form in FORMS:
        for mark in MARKS:
            assert np.array_equal(sample.coverage(form, rows, table, [0], g, cut, mark), want), (form, mark)
    assert want[0][-1] > 0


@pytest.mark.parametrize("gene_len", [LDS_MAX_LEN, LDS_MAX_LEN + 1])
def test_forms_meet_at_the_lds_capacity(sample, gene_len):
    """The longest gene the LDS form takes and the shortest it leaves to the direct form."""
    g, n = 3, 300
    rng = np.random.default_rng(gene_len)
    rows = rng.permutation(sample.valid[g])[:n]
    cols = np.array([4, 0, 2])
    table = makeTable(rng, "ties", n, 5, cols, 320, 255)
    want = sample.reference(rows, table[:, :n], cols, g, gene_len)
    assert want[0].sum() > 100 * n and want[5:].any(axis=1).all()
    dev = sample.dev
    dev.profEnable(True)
    try:
        for form in FORMS:
            for mark in MARKS:
                dev.profCollect()
                assert np.array_equal(sample.coverage(form, rows, table, cols, g, gene_len, mark), want), (form, mark)
                ran = {name for name in dev.profCollect() if name.startswith("callcov_mark")}
                assert ran == {"callcov_mark_lds" if mark == "lds" and gene_len <= LDS_MAX_LEN else "callcov_mark"}, (form, mark)
    finally:
        dev.profEnable(False)


# ------------------------------------------------------------------------------------------------ wide pairs
def test_wide_pairs(device, small_case):
    sidx, gidx, s = small_case
    rng = np.random.default_rng(3)
    lines = synth.toSamLines(s)
    lines = synth.withManyMismatches(lines, sidx, rng.choice(s.n_pairs, size=40, replace=False).tolist(), rng)
    spill = []
    rec, _ = packed.packPairs(list(pairLines(lines)), gidx, spill=spill)
    wide = packed.spillArrays(spill)
    assert wide is not None and len(wide[1]) >= 3
    smp = Sample(device, gidx, rec, spill=wide)
    try:
        n_wide = 0
        for g, valid in smp.valid.items():
            if not len(valid):
                continue
            is_wide = smp.rec["n_cig"][2 * smp.pair_src[valid]] == 0xFF
            rows = np.concatenate([valid[is_wide], valid[~is_wide][:50]])
            rows = rows[rng.permutation(len(rows))]
            n_wide += int(is_wide.sum())
            n = len(rows)
            ldm = (n + 63) // 64 * 64
            table = makeTable(rng, "ties", n, 5, np.array([3, 1]), ldm, 255)
            gene_len = len(sidx.backbone[gidx.genes[g]])
            want = smp.reference(rows, table[:, :n], [3, 1], g, gene_len)
            if is_wide.any():      # the wide mates' runs are in the expected value
                narrow = cr.tracks(smp.rec, smp.pair_src, rows, table[:, :n], [3, 1], g, gene_len, wide=None)
                assert want[0].sum() > narrow[0].sum()
            for form in FORMS:
                for mark in MARKS:
                    assert np.array_equal(smp.coverage(form, rows, table, [3, 1], g, gene_len, mark), want), (g, form, mark)
        assert n_wide >= 1                                              # at least one listed row is a wide pair
    finally:
        smp.close()


# ------------------------------------------------------------------------------------------------ the existing primitive
def test_all_rows_and_zeros_give_the_depth_of_the_gene(sample, small_case):
    sidx = small_case[0]
    genes = sample.gidx.genes
    lens = np.array([len(sidx.backbone[g]) for g in genes], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    depth = np.zeros(int(off[-1]), dtype=np.uint32)
    tab = sample.tabs["compact"]
    _lib.check(_lib.lib().gk_depth_compact(sample.dev.ctx, tab.handle, tab.mates.words.ptr, 0, off.ctypes.data, len(genes),
                                           depth.ctypes.data))
    assert depth.sum() > 0
    for g in range(len(genes)):
        rows = sample.valid[g]                                          # selectGene(g): the NH == 1 pairs of the gene
        n = len(rows)
        table = np.zeros((1, (n + 63) // 64 * 64), dtype=np.uint8)
        want = depth[off[g]:off[g + 1]].astype(np.int64)
        for form in FORMS:
            for mark in MARKS:
                got = sample.coverage(form, rows, table, [0], g, int(lens[g]), mark)
                assert np.array_equal(got[0], want) and np.array_equal(got[2], want) and np.array_equal(got[3], want), (g, form, mark)
                assert not got[1].any(), (g, form, mark)


# ------------------------------------------------------------------------------------------------ arguments
def test_arguments_are_checked(sample):
    dev, tab = sample.dev, sample.tabs["mates"]
    n, ldm, a, gene_len, g = 100, 128, 5, 50, 1
    d_table = dev.put(np.zeros((a, ldm), dtype=np.uint8))
    d_rows = dev.put(np.ascontiguousarray(sample.valid[g][:n], dtype=np.int32))
    out = np.full(34 * gene_len + TAIL, SENTINEL, dtype=np.uint32)
    lib, ctx, h = _lib.lib(), dev.ctx, tab.handle
    m, c = tab.mates.ptr, sample.tabs["compact"].mates.words.ptr
    t, r, o = d_table.ptr, d_rows.ptr, out.ctypes.data

    def cols(*x):
        arr = np.array(x, dtype=np.int32)
        return arr, arr.ctypes.data

    good, good_p = cols(0, 3)
    seventeen, seventeen_p = cols(*range(17))
    twice, twice_p = cols(1, 2, 1)
    outside, outside_p = cols(0, 5)
    negative, negative_p = cols(-1)
    call = lib.gk_call_coverage
    bad = [
        # gk_call_fit's list
        lambda: call(ctx, h, m, 0, r, 0, t, ldm, a, good_p, 2, g, gene_len, o),
        lambda: call(ctx, h, m, 0, r, 1 << 31, t, 1 << 31, a, good_p, 2, g, gene_len, o),
        lambda: call(ctx, h, m, 0, r, n, t, 64, a, good_p, 2, g, gene_len, o),              # ldm < n_rows
        lambda: call(ctx, h, m, 0, r, n, t, 120, a, good_p, 2, g, gene_len, o),             # ldm % 64 != 0
        lambda: call(ctx, h, m, 0, r, n, t, ldm, 0, good_p, 2, g, gene_len, o),
        lambda: call(ctx, h, m, 0, r, n, t, ldm, a, good_p, 0, g, gene_len, o),
        lambda: call(ctx, h, m, 0, r, n, t, ldm, 20, seventeen_p, 17, g, gene_len, o),
        lambda: call(ctx, h, m, 0, r, n, t, ldm, a, twice_p, 3, g, gene_len, o),
        lambda: call(ctx, h, m, 0, r, n, t, ldm, a, outside_p, 2, g, gene_len, o),
        lambda: call(ctx, h, m, 0, r, n, t, ldm, a, negative_p, 1, g, gene_len, o),
        lambda: call(ctx, h, m, 0, r, n, 0, ldm, a, good_p, 2, g, gene_len, o),
        lambda: call(ctx, h, m, 0, r, n, t + 8, ldm, a, good_p, 2, g, gene_len, o),         # not 16-byte aligned
        lambda: call(ctx, h, m, 0, r, n, t, ldm, a, None, 2, g, gene_len, o),
        lambda: call(ctx, h, m, 0, r, n, t, ldm, a, good_p, 2, g, gene_len, None),
        # its own
        lambda: call(ctx, h, m, c, r, n, t, ldm, a, good_p, 2, g, gene_len, o),             # both forms
        lambda: call(ctx, h, 0, 0, r, n, t, ldm, a, good_p, 2, g, gene_len, o),             # neither
        lambda: call(ctx, h, m, 0, r, n, t, ldm, a, good_p, 2, g, 0, o),
        lambda: call(ctx, h, m, 0, r, n, t, ldm, a, good_p, 2, g, -5, o),
        lambda: call(ctx, h, m, 0, r, n, t, ldm, a, good_p, 2, -1, gene_len, o),
        lambda: call(ctx, h, m, 0, r, n, t, ldm, a, good_p, 2, len(sample.gidx.genes), gene_len, o),
        lambda: call(ctx, h, m, 0, r, n, t, ldm, a, good_p, 2, 256, gene_len, o),
        lambda: call(ctx, h, m, 0, 0, n, t, ldm, a, good_p, 2, g, gene_len, o),             # null d_rows
        lambda: call(ctx, None, m, 0, r, n, t, ldm, a, good_p, 2, g, gene_len, o),
    ]
    dev.profEnable(True)
    dev.profCollect()
    for k, f in enumerate(bad):
        assert f() == -3, k                                          # GK_ERR_ARG
        assert lib.gk_last_error(), k
    launched = dev.profCollect()
    dev.profEnable(False)
    assert not any(name.startswith("callcov_") for name in launched), launched      # nothing was launched
    assert (out == SENTINEL).all()                                   # the output is untouched
    # the context still works: a table of zeros
    _lib.check(call(ctx, h, m, 0, r, n, t, ldm, a, good_p, 2, g, gene_len, o))
    got = out[:6 * gene_len].reshape(6, gene_len)
    assert (out[6 * gene_len:] == SENTINEL).all()
    want = sample.reference(sample.valid[g][:n], np.zeros((a, n), dtype=np.uint8), [0, 3], g, gene_len)
    assert np.array_equal(got, want) and not got[1].any() and not got[4:].any() and np.array_equal(got[2], got[3])
    d_table.free()
    d_rows.free()


# ------------------------------------------------------------------------------------------------ the drivers
STRATEGIES = {"full": {}, "exonfirst": {"exon_first": True}}


@pytest.fixture(scope="module")
def tabulated(device, small_case):
    sidx, gidx, s = small_case
    rec, table = packed.packSample(s, gidx)
    tab = Tabulation(DeviceIndex(device, gidx), rec)
    gene_len = {g: len(sidx.backbone[g]) for g in sidx.genes}
    yield SampleData(tab, gidx, tab.novelVariants(table.strings)), s, gene_len, np.ascontiguousarray(rec)
    tab.mates.free()
    tab.close()


@pytest.fixture(scope="module")
def typed(tabulated):
    """Per strategy: the sample typed without and with the coverage report (the whole-sample paths)."""
    data, s, gene_len, _ = tabulated
    out = {}
    for name, kw in STRATEGIES.items():
        plain = TypingWithPosNegAllele(data, variant_correction=True, **kw)
        plain_calls = plain.typing(s.gene_cn)
        cov = TypingWithPosNegAllele(data, variant_correction=True, call_coverage=True, call_coverage_len=gene_len, **kw)
        cov_calls = cov.typing(s.gene_cn)
        out[name] = (plain, plain_calls, cov, cov_calls)
    return out


def test_point_result_does_not_change(typed):
    for name, (plain, plain_calls, cov, cov_calls) in typed.items():
        assert cov_calls == plain_calls, name                   # calls and warnings
        assert plain.call_coverage == {}
        assert list(plain._result) == list(cov._result)
        for gene in plain._result:
            a, b = list(plain._result[gene]), list(cov._result[gene])
            assert len(a) == len(b), (name, gene)
            for x, y in zip(a, b):
                assert x.n == y.n and list(x.allele_name) == list(y.allele_name)
                for f in ("value", "value_sum_indv", "allele_id", "fraction", "fraction_uniq"):
                    assert np.array_equal(getattr(x, f), getattr(y, f)), (name, gene, f)


def test_every_typed_gene_has_an_entry(tabulated, typed):
    data, s, gene_len, _ = tabulated
    for name, (_, _, cov, _) in typed.items():
        want = {g for g, cn in s.gene_cn.items() if cn and cov._result.get(g) and not cov._result[g][-1].isFail()}
        assert set(cov.call_coverage) == want and len(want) >= 2, name
        assert all(c is not None for c in cov.call_coverage.values()), name
        # the sample's genes are called with 1, 2 and 3 distinct alleles (the literals of test_gpu_call_fit.py)
        assert {len(c.alleles) for c in cov.call_coverage.values()} >= {1, 2, 3}, name
        for gene, c in cov.call_coverage.items():
            k = len(c.alleles)
            result = cov._result[gene][-1]
            assert c.length == gene_len[gene] and c.depth.shape == (2 + 2 * k, c.length) and c.depth.dtype == np.uint32
            assert c.cn == result.n == sum(n for _, n in c.alleles) and c.reads == modelOf(result).n_rows
            assert sorted(a for a, n in c.alleles for _ in range(n)) == sorted(result.selectBest()), (name, gene)
            assert c.regions == regionsOf(data.index.exons[gene], c.length) and len(c.regions) > 3
            assert c.depth[2 + k:].any(axis=1).all(), (name, gene)          # every called allele has reads of its own


def checkHostSide(c, table, ids, pos, where):
    """regions, sums and private sites of one entry against the restatement, from its own depth."""
    sites = [[min(int(pos[v]), c.length - 1) for v in mine] for mine in cr.privateSites(table.mask, list(ids))]
    want = cr.summary(c.depth, c.regions, sites)
    for r in range(len(c.regions)):
        got = (c.bases[r].tolist(), c.covered[r].tolist(), c.private_sites[r].tolist(), c.private_unsupported[r].tolist())
        assert got == tuple(want[r]), (where, c.regions[r])
    if len(ids) > 1:
        assert c.private_sites[0].sum() > 0, where
    else:
        assert not c.private_sites.any(), where


def test_full_entries_equal_the_oracle(small_case, tabulated, typed):
    """Every track is the depth (oracle.depth.depthFromPairs, M runs from the reads' own SAM lines) of the oracle model's
    reads of that class, the classes from the oracle's mismatch table."""
    sidx, gidx, s = small_case
    gene_len = tabulated[2]
    cov = typed["full"][2]
    ref = ot.tabulateLines(synth.toSamLines(s), gidx.variants)
    for gene, c in cov.call_coverage.items():
        reads = [dict(r) for r in ref["reads"] if r["backbone"] == gene and r["multiple"] == 1]
        variants = [v for v in ref["variants"] if v.ref == gene]
        om = oty.GeneModel(reads, variants, top_n=300, variant_correction=True)
        miss, _ = oty.missTable(om.reads, om.variants, om.allele_to_id)
        assert c.reads == om.readsNum() == len(miss) and miss.max() < 100
        cols = [om.allele_to_id[a] for a, _ in c.alleles]
        assert cols == sorted(cols), gene
        k = len(cols)
        m1, tie = cr.tieSets(miss.T, cols)
        classes = [np.ones(len(miss), dtype=bool), m1 > 0] + [tie[:, j] for j in range(k)] + \
                  [tie[:, j] & (tie.sum(axis=1) == 1) for j in range(k)]
        for t, member in enumerate(classes):
            pairs = [(om.reads[i]["l_sam"], om.reads[i]["r_sam"], 1) for i in np.flatnonzero(member)]
            want = odepth.depthFromPairs(pairs, gene_len)[gene]
            assert np.array_equal(c.depth[t], want), (gene, t)
        g = gidx.gene_id[gene]
        table = gidx.tables[g]
        ids = [table.alleles.index(a) for a, _ in c.alleles]
        pos = [v.pos for v in gidx.variants[table.vbeg:table.vend]]
        checkHostSide(c, table, ids, pos, gene)


def test_exonfirst_entries_equal_the_table_in_hbm(small_case, tabulated, typed):
    sidx, gidx, s = small_case
    data, _, gene_len, rec = tabulated
    cov = typed["exonfirst"][2]
    pair_src = data.tab.pairSrc().copy()
    for gene, c in cov.call_coverage.items():
        result = cov._result[gene][-1]
        model = modelOf(result)
        g = gidx.gene_id[gene]
        before = model.tableColumns
        row = np.asarray(result.allele_id, dtype=np.int64)[result.bestRank()]
        ids = np.unique(row)
        miss8, ldm, n_table_cols, cols = model.missFor(ids)
        table = miss8.download().reshape(n_table_cols, ldm)[:, :model.n_rows].astype(np.int64)
        rows = model.rows.download()[:model.n_rows]
        want = cr.tracks(rec, pair_src, rows, table, cols.tolist(), g, gene_len[gene])
        assert np.array_equal(c.depth, want), gene
        assert [a for a, _ in c.alleles] == [gidx.tables[g].alleles[i] for i in ids], gene
        # the report (made while the sample was typed) and this look wrote no all-allele table
        after = model.tableColumns
        assert (after is None) == (before is None), gene
        assert n_table_cols == (len(gidx.tables[g].alleles) if after is None else len(after)), gene
        info = getattr(cov, "exon_info", {}).get(gene)
        if info is not None and "table_columns" in info:
            assert info["table_columns"] == n_table_cols, gene
        checkHostSide(c, gidx.tables[g], ids.tolist(), [v.pos for v in gidx.variants[gidx.tables[g].vbeg:gidx.tables[g].vend]], gene)


def sameEntry(a, b):
    return ((a.cn, a.reads, a.length, a.alleles, a.regions) == (b.cn, b.reads, b.length, b.alleles, b.regions)
            and all(np.array_equal(getattr(a, f), getattr(b, f))
                    for f in ("depth", "bases", "covered", "private_sites", "private_unsupported")))


def test_per_gene_path_gives_the_same_entries(tabulated, typed):
    data, s, gene_len, _ = tabulated
    for name, kw in STRATEGIES.items():
        whole = typed[name][2]
        per_gene = TypingWithPosNegAllele(data, variant_correction=True, call_coverage=True, call_coverage_len=gene_len, **kw)
        for gene, cn in s.gene_cn.items():
            if cn:
                per_gene.typingPerGene(gene, int(cn))
        assert per_gene.call_coverage.keys() == whole.call_coverage.keys(), name
        for gene, a in whole.call_coverage.items():
            assert sameEntry(a, per_gene.call_coverage[gene]), (name, gene)
        # a gene typed again replaces its entry
        gene = next(iter(whole.call_coverage))
        per_gene.typingPerGene(gene, int(s.gene_cn[gene]))
        assert sameEntry(whole.call_coverage[gene], per_gene.call_coverage[gene]) and len(per_gene.call_coverage) == len(whole.call_coverage)
    # the report of an adopted result, asked for directly
    cov = typed["full"][2]
    for gene, a in cov.call_coverage.items():
        g = data.index.gene_id[gene]
        assert sameEntry(a, coverCall(cov._result[gene][-1], gene_len[gene], data.index.exons[gene], data.index.tables[g]))


def launches():
    out = {}
    for dev in _lib.Device.instances:
        if dev.ctx:
            for name, (n, _) in dev.profCollect().items():
                out[name] = out.get(name, 0) + n
    return out


def test_without_the_flag_nothing_is_launched(tabulated, typed):
    """The contexts of the typing lanes exist (``typed`` made them): their per-kernel spans see every launch."""
    data, s, gene_len, _ = tabulated
    live = [dev for dev in _lib.Device.instances if dev.ctx]
    for dev in live:
        dev.profEnable(True)
    try:
        launches()
        for name, kw in STRATEGIES.items():
            plain = TypingWithPosNegAllele(data, variant_correction=True, **kw)
            plain.typing(s.gene_cn)
            seen = launches()
            assert plain.call_coverage == {} and seen and not any(k.startswith("callcov_") for k in seen), (name, seen)
            cov = TypingWithPosNegAllele(data, variant_correction=True, call_coverage=True, call_coverage_len=gene_len, **kw)
            cov.typing(s.gene_cn)
            seen = launches()
            marks = seen.get("callcov_mark", 0) + seen.get("callcov_mark_lds", 0)
            assert marks == seen.get("callcov_finish") == len(cov.call_coverage) >= 2, (name, seen)
    finally:
        for dev in live:
            dev.profEnable(False)


def test_a_sample_without_records_gets_none_and_one_warning(device, small_case):
    sidx, gidx, s = small_case
    rec, table = packed.packSample(s, gidx)
    tab = Tabulation(DeviceIndex(device, gidx), rec)
    data = SampleData(tab, gidx, tab.novelVariants(table.strings))
    tab.mates.free()                                                   # what main.releaseInputs does without the flag
    tab.mates = None
    gene_len = {g: len(sidx.backbone[g]) for g in sidx.genes}
    seen = []
    handler = logging.Handler()
    handler.emit = lambda record: seen.append(record.getMessage())
    logger.addHandler(handler)
    try:
        cov = TypingWithPosNegAllele(data, variant_correction=True, call_coverage=True, call_coverage_len=gene_len)
        calls = cov.typing(s.gene_cn)
    finally:
        logger.removeHandler(handler)
        tab.close()
    assert calls[0] and len(cov.call_coverage) >= 2 and all(c is None for c in cov.call_coverage.values())
    assert len([m for m in seen if "call coverage" in m]) == 1, seen
    assert callCoverageText({g: c for g, c in cov.call_coverage.items() if c is not None}) == "\t".join(CALL_COVERAGE_COLUMNS) + "\n"


# ------------------------------------------------------------------------------------------------ the command line
def test_command_line_writes_the_coverage_files(device, tmp_path, monkeypatch):
    """graphkir --allele-strategy exonfirst on a small BAM without the flag, with --call-coverage and with
    --call-coverage-depth (in-process, like tests/test_gpu_cn_cli.py): the typing files do not change, the new files appear
    only when asked for and hold the typer's numbers."""
    from bamwriter import samToBam
    from kir_graph_amd import main as cli
    sidx = synth.makeIndex(seed=11, n_genes=3, var_range=(200, 300), allele_range=(12, 20))
    folder = tmp_path / "index"
    folder.mkdir()
    sidx.write(str(folder / "kir_2100_withexon_ab_2dl1s1.leftalign.mut01"))
    s = synth.makeSample(sidx, seed=50, n_pairs=2500)
    lines = synth.toSamLines(s)
    header = ["@HD\tVN:1.0\tSO:coordinate"] + [f"@SQ\tSN:{g}\tLN:{len(sidx.backbone[g])}" for g in sidx.genes]
    samToBam(header + sorted(lines, key=lambda l: (l.split("\t")[2], int(l.split("\t")[3]))), str(tmp_path / "s.bam"))
    (tmp_path / "s.cn.tsv").write_text("gene\tcn\n" + "".join(f"{g}\t{c}\n" for g, c in s.gene_cn.items()))
    files, typers = [], []
    write = cli.writeTyping
    monkeypatch.setattr(cli, "writeTyping", lambda name, typer, *rest: (typers.append(typer), write(name, typer, *rest))[1])
    for k, extra in enumerate(([], ["--call-coverage"], ["--call-coverage-depth"])):
        run = tmp_path / f"run{k}"       # paths relative to the run's folder: the files name the sample's output
        run.mkdir()
        monkeypatch.chdir(run)
        cli.main(cli.createParser().parse_args(
            ["--step-skip-extraction", "--index-folder", "../index", "--output-folder", "out", "--allele-strategy", "exonfirst",
             "--cn-provided", "../s.cn.tsv", "--alignment", "../s.bam"] + extra))
        files.append({p.name: p for p in (run / "out").iterdir()})
    cov_files = [n for n in files[2] if n.endswith(".coverage.tsv")]
    depth_files = [n for n in files[2] if n.endswith(".coverage.depth.tsv")]
    assert len(cov_files) == 1 and len(depth_files) == 1
    assert files[0].keys() | set(cov_files) == files[1].keys() and files[1].keys() | set(depth_files) == files[2].keys()
    assert not any(".coverage." in n for n in files[0]) and not any(n.endswith(".coverage.depth.tsv") for n in files[1])
    stem = cov_files[0][:-len(".coverage.tsv")]
    for n in (stem + ".tsv", stem + ".possible.tsv"):
        assert files[0][n].read_bytes() == files[1][n].read_bytes() == files[2][n].read_bytes(), n
    assert files[1][cov_files[0]].read_bytes() == files[2][cov_files[0]].read_bytes()
    assert len(typers) == 3 and typers[0].call_coverage == {}
    typer = typers[2]
    typed_genes = [g for g, cn in s.gene_cn.items() if cn and typer._result.get(g) and not typer._result[g][-1].isFail()]
    assert list(typer.call_coverage) == typed_genes and len(typed_genes) >= 2
    assert all(c is not None for c in typer.call_coverage.values())
    text = files[2][cov_files[0]].read_text()
    assert text == callCoverageText(typer.call_coverage)
    lines_ = text.split("\n")
    assert lines_[0].split("\t") == CALL_COVERAGE_COLUMNS and lines_[-1] == ""
    rows = [line.split("\t") for line in lines_[1:-1]]
    assert all(len(r) == 18 for r in rows)
    at = 0
    for gene in typed_genes:
        c = typer.call_coverage[gene]
        k = len(c.alleles)
        assert k == len(set(typer._result[gene][-1].selectBest()))
        for r, (name, a, b) in enumerate(c.regions):
            for j, (allele, copies) in enumerate(c.alleles):
                d = c.depth.astype(np.int64)
                want = [gene, c.cn, c.reads, name, a, b, b - a, d[0, a:b].sum(), d[1, a:b].sum(), (d[1, a:b] > 0).sum(), allele,
                        copies, d[2 + j, a:b].sum(), d[2 + k + j, a:b].sum(), (d[2 + j, a:b] > 0).sum(),
                        (d[2 + k + j, a:b] > 0).sum(), c.private_sites[r, j], c.private_unsupported[r, j]]
                assert rows[at] == [str(x) for x in want], (gene, name, allele)
                at += 1
    assert at == len(rows)
    # the depth file's runs expand to the typer's tracks
    text = files[2][depth_files[0]].read_text()
    assert text == callCoverageDepthText(typer.call_coverage) and text.split("\n")[0].split("\t") == CALL_COVERAGE_DEPTH_COLUMNS
    back = cr.expandDepthText(text)
    n_tracks = 0
    for gene in typed_genes:
        c = typer.call_coverage[gene]
        keys = [(gene, "informative", ""), (gene, "mismatch", "")] + [(gene, "best", a) for a, _ in c.alleles] + \
               [(gene, "unique", a) for a, _ in c.alleles]
        for t, key in enumerate(keys):
            assert np.array_equal(back[key], c.depth[t]), key
        n_tracks += len(keys)
    assert len(back) == n_tracks
    # the records went with the sample to the lane that typed it, and that lane freed them
    assert all(t._data.tab.mates is None for t in typers)
