"""The candidate sets of the EM strategy (csrc/gk_em.hip) driven directly, against the plain reference of
tests/emsets_reference.py -- packed words with ``np.array_equal``, counts exactly:

* ``gk_em_sets`` (em_sets_groups) on hand-built genes of every group width (2, 4, 8 lanes per pair, both ends of each and
  odd widths between), lists of every length around the 4 G ids handed round at a time, ids that are not the gene's, the
  ballot that decides "named by both mates", bit rows staged in LDS and read from global memory, the sizes either side of
  that switch and the sizes whose padded rows do not fit a CU's LDS although their plain size would, row counts around a
  round of a workgroup, a workgroup's share and the grid's cap;
* ``gk_em_distinct`` (em_sets_hash, em_sets_verify, em_sets_emit) on synthetic sets: one set, all sets distinct with a
  workgroup's local table overrun, sets one bit apart, heavy sets among singletons, the output capacity;
* ``gk_sample_em`` with genes of different widths in one call (narrow genes in wide groups), its capacity of 2^18 distinct
  sets per gene, and the driver's way out of it.

The second hashing seed (two different sets under one 64-bit hash) is not reached here: no two sets with equal hashes can
be constructed from outside, so that retry stays covered by reading alone."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emsets_reference as er  # noqa: E402

from kir_graph_amd import _lib  # noqa: E402
from kir_graph_amd._lib import check, lib  # noqa: E402
from oracle import em as oem  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0x5EA71E55          # what nobody wrote
GK_ERR_CAPACITY = -5
WIDTHS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16]
MASK_LDS_MAX = 100 * 1024      # bit rows beyond this many bytes are read from global memory


# ------------------------------------------------------------------------------------------------------------ cases
class Case:
    """A gene, the CSR of its row families (unlisted rows between them) and the reference of every family -- computed
    once, never changed."""

    def __init__(self, words, n_allele, n_span=None):
        self.g = g = er.Gene(words, n_allele, n_span)
        fams = er.rowFamilies(g)
        self.names = [f[0] for f in fams]
        csr, at = [], []
        for k, (_, four, _) in enumerate(fams):
            if k % 7 == 0:
                csr.append([[g.at["all"]], [], [int(g.novel[1])], [5, 6]])      # a row nobody lists
            at.append(len(csr))
            csr.append(four)
        self.off, self.ids = er.packLists(csr)
        self.at = np.array(at, dtype=np.int32)                                  # the last listed row ends the CSR
        self.n_csr = len(csr)
        self.ref = er.pack(er.candidateSets(self.off, self.ids, self.at, g.vbeg, g.vend, g.bits), words)
        self.ref.setflags(write=False)


@functools.lru_cache(maxsize=None)
def caseOf(words, n_allele, n_span=None):
    return Case(words, n_allele, n_span)


def globalSpan(words):
    """The smallest span whose bit rows are read from global memory."""
    return MASK_LDS_MAX // (4 * words) + 1


class OnDevice:
    """A tabulation from CSR lists (``gk_tab_from_csr``) and a gene's bit rows on the device."""

    def __init__(self, device, off, ids, n_var_total, mask):
        self.dev = device
        n = (len(off) - 1) // 4
        h = C.c_void_p()
        gene, nh = np.zeros(max(n, 1), np.uint8), np.ones(max(n, 1), np.uint8)
        off, ids = np.ascontiguousarray(off, np.uint32), np.ascontiguousarray(ids, np.uint32)
        check(lib().gk_tab_from_csr(device.ctx, int(n_var_total), n, off.ctypes.data, ids.ctypes.data if len(ids) else None,
                                    gene.ctypes.data, nh.ctypes.data, C.byref(h)))
        self.tab = h
        self.mask = device.put(mask) if mask is not None else None

    @classmethod
    def of(cls, device, case: Case):
        return cls(device, case.off, case.ids, case.g.n_total, case.g.mask)

    def sets(self, rows, vbeg, vend, words, tail=5, mask=None):
        """``gk_em_sets`` of ``rows`` into a buffer full of sentinels, ``tail`` rows longer than needed: the sets, after the
        tail was seen untouched."""
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        n = len(rows)
        d_rows = self.dev.put(rows if n else np.zeros(1, np.int32))
        out = self.dev.put(np.full((n + tail, words), SENTINEL, dtype=np.uint32))
        check(lib().gk_em_sets(self.dev.ctx, self.tab, d_rows.ptr, n, vbeg, vend, (mask or self.mask).ptr, words, out.ptr))
        self.dev.sync()
        got = out.download()
        d_rows.free()
        out.free()
        assert (got[n:] == SENTINEL).all(), "written past the last row"
        return got[:n]

    def close(self):
        if self.mask is not None:
            self.mask.free()
        lib().gk_tab_destroy(self.tab)


def assert_sets(got, want, names=None):
    if np.array_equal(got, want):
        return
    bad = np.nonzero((got != want).any(axis=1))[0]
    i = int(bad[0])
    what = names[i] if names is not None else ""
    raise AssertionError(f"{len(bad)} of {len(want)} rows differ; row {i} ({what}): got {got[i].tolist()}, want {want[i].tolist()}")


def run_families(device, case: Case):
    g = case.g
    gpu = OnDevice.of(device, case)
    try:
        got = gpu.sets(case.at, g.vbeg, g.vend, g.words)
        assert_sets(got, case.ref, case.names)
        back = gpu.sets(case.at[::-1], g.vbeg, g.vend, g.words)      # the same pairs in another order
        assert_sets(back, case.ref[::-1], case.names[::-1])
    finally:
        gpu.close()


# ------------------------------------------------------------------------------------------------------------ gk_em_sets
def test_the_cases_say_something():
    """The reference of a case is not all alike: empty and full sets, sets of one and of two alleles, and rows whose
    mates agree in one word only -- a kernel that always took the union would differ there."""
    for words in WIDTHS:
        case = caseOf(words, 32 * words)
        size = np.unpackbits(case.ref.view(np.uint8), axis=1).sum(axis=1)
        assert (size == 0).any() and (size == 32 * words).any() and (size == 1).sum() > 4 and (size == 2).any()
        assert len({r.tobytes() for r in case.ref}) > 50


@pytest.mark.parametrize("multiple", [True, False], ids=["multiple of 32", "11 short of it"])
@pytest.mark.parametrize("words", WIDTHS)
def test_row_families_with_bit_rows_in_lds(device, words, multiple):
    case = caseOf(words, 32 * words - (0 if multiple else 11))
    assert case.g.n_span * words * 4 <= MASK_LDS_MAX
    run_families(device, case)


@pytest.mark.parametrize("words", WIDTHS)
def test_row_families_with_bit_rows_in_global_memory(device, words):
    case = caseOf(words, 32 * words - (11 if words % 2 else 0), globalSpan(words) + 17)
    assert case.g.n_span * words * 4 > MASK_LDS_MAX
    run_families(device, case)


# (words, n_span): either side of the switch between LDS and global memory; spans whose rows, padded to an even number of
# words for LDS, do not fit a CU next to the local table although their plain size is below the switch (first and last of
# each such range), and the last span before each range (a request of exactly 160 KiB)
SWITCH = [(16, 1600), (16, 1601), (5, 5120), (5, 5121)]
PADDED = [(1, 16366), (1, 16400), (1, 25600), (3, 8182), (3, 8200), (3, 8533)]


@pytest.mark.parametrize("words,n_span", SWITCH + PADDED)
def test_row_families_at_the_sizes_where_the_bit_rows_leave_lds(device, words, n_span):
    run_families(device, caseOf(words, 32 * words - 11, n_span))


@pytest.mark.parametrize("words", WIDTHS)
def test_row_counts_around_a_round_and_a_workgroups_share(device, words):
    """Pairs drawn from the families with repetition, in no order: 1 pair, a round of one workgroup (1024 / G pairs) and one
    either side, one pair more than the share of one workgroup, no pair at all."""
    case = caseOf(words, 32 * words)
    g = case.g
    rng = np.random.default_rng(300 + words)
    share = 4096 if words <= 4 else 2048 if words <= 8 else 1024
    gpu = OnDevice.of(device, case)
    try:
        for n_rows in (1, 1024 // g.G - 1, 1024 // g.G, 1024 // g.G + 1, share + 1):
            pick = rng.integers(0, len(case.at), n_rows)
            got = gpu.sets(case.at[pick], g.vbeg, g.vend, words)
            assert_sets(got, case.ref[pick], [case.names[k] for k in pick])
        assert gpu.sets(np.zeros(0, np.int32), g.vbeg, g.vend, words).shape == (0, words)      # the sentinels stand
    finally:
        gpu.close()


@pytest.mark.parametrize("in_lds", [True, False], ids=["lds", "global"])
def test_more_rows_than_the_grid_takes_in_one_pass(device, in_lds):
    """256 workgroups of 128 pairs a round, 16 rounds: 262 144 pairs; 300 more make the strided loop go round again."""
    words = 9
    case = caseOf(words, 32 * words) if in_lds else caseOf(words, 32 * words - 11, globalSpan(words) + 17)
    g = case.g
    pick = np.random.default_rng(9).integers(0, len(case.at), 262144 + 300)
    gpu = OnDevice.of(device, case)
    try:
        got = gpu.sets(case.at[pick], g.vbeg, g.vend, words)
        assert np.array_equal(got, case.ref[pick])
    finally:
        gpu.close()


@pytest.mark.parametrize("words", [1, 5, 16])
def test_a_gene_without_variants(device, words):
    """``vend == vbeg``: every id is somebody else's, every set is empty."""
    rng = np.random.default_rng(words)
    n_total, vbeg = 100, 50
    lists = [[rng.integers(0, n_total, int(m)).tolist() for m in rng.integers(0, 40, 4)] for _ in range(300)]
    off, ids = er.packLists(lists)
    bits = np.zeros((0, 32 * words - 3), dtype=bool)
    want = er.pack(er.candidateSets(off, ids, np.arange(300), vbeg, vbeg, bits), words)
    assert not want.any()
    gpu = OnDevice(device, off, ids, n_total, np.full((1, words), 0xFFFFFFFF, dtype=np.uint32))   # a row nobody may read
    try:
        assert np.array_equal(gpu.sets(np.arange(300), vbeg, vbeg, words), want)
    finally:
        gpu.close()


# ------------------------------------------------------------------------------------------------------------ gk_em_distinct
def distinct_on_device(device, sets, max_out, extra=8):
    """``gk_em_distinct`` into host arrays full of sentinels, ``extra`` entries longer than ``max_out``: (rc, n_out, sets,
    counts), after the entries from ``max_out`` on were seen untouched."""
    sets = np.ascontiguousarray(sets, dtype=np.uint32)
    n_rows, words = sets.shape
    buf = device.put(sets if n_rows else np.zeros((1, words), np.uint32))
    out_sets = np.full((max_out + extra, words), SENTINEL, dtype=np.uint32)
    out_count = np.full(max_out + extra, SENTINEL, dtype=np.uint32)
    n = C.c_int32(-7)
    rc = lib().gk_em_distinct(device.ctx, buf.ptr, n_rows, words, max_out, out_sets.ctypes.data, out_count.ctypes.data, C.byref(n))
    buf.free()
    assert (out_sets[max_out:] == SENTINEL).all() and (out_count[max_out:] == SENTINEL).all()
    return rc, n.value, out_sets, out_count


def assert_distinct(device, sets, want_sets, want_count, key_word=None):
    """The device's distinct sets of ``sets``, put in order, are ``want_sets`` (ascending) with ``want_count``."""
    n = len(want_sets)
    rc, n_out, got_sets, got_count = distinct_on_device(device, sets, max(n, 1))
    check(rc)
    assert n_out == n
    got_sets, got_count = got_sets[:n], got_count[:n]
    order = er.sortedRows(got_sets) if key_word is None else np.argsort(got_sets[:, key_word], kind="stable")
    assert np.array_equal(got_sets[order], want_sets)
    assert np.array_equal(got_count[order].astype(np.int64), want_count)


DISTINCT_WIDTHS = [1, 4, 5, 8, 9, 16]


@pytest.mark.parametrize("words", DISTINCT_WIDTHS)
def test_distinct_of_equal_rows(device, words):
    row = (np.arange(1, words + 1, dtype=np.uint32) * np.uint32(0x9E3779B1)) | np.uint32(0x80000000)
    sets = np.tile(row, (100000, 1))
    assert_distinct(device, sets, row[None, :], np.array([100000]))
    assert_distinct(device, np.zeros((1000, words), np.uint32), np.zeros((1, words), np.uint32), np.array([1000]))   # the empty set alone


@pytest.mark.parametrize("words,key_word", [(1, 0), (4, 0), (4, 3)])
def test_distinct_rows_overrun_the_local_table(device, words, key_word):
    """3 workgroups, each with 4096 different hashes for its 2048 local slots: the rest goes straight to the gene's table."""
    n = 4096 * 3
    sets = np.tile(np.arange(1, words + 1, dtype=np.uint32) << 8, (n, 1))
    sets[:, key_word] = np.random.default_rng(words + key_word).permutation(n).astype(np.uint32)
    want = sets[np.argsort(sets[:, key_word])]
    assert_distinct(device, sets, want, np.ones(n, np.int64), key_word)


@pytest.mark.parametrize("key_word", [0, 15])
def test_distinct_rows_past_the_grid_cap(device, key_word):
    """600 000 different sets of 16 words: 256 workgroups go round 37 times, every local table is crowded."""
    n, words = 600000, 16
    sets = np.tile(np.arange(words, dtype=np.uint32) * np.uint32(0x01010101), (n, 1))
    sets[:, key_word] = np.random.default_rng(key_word).permutation(n).astype(np.uint32)
    want = sets[np.argsort(sets[:, key_word])]
    assert_distinct(device, sets, want, np.ones(n, np.int64), key_word)


@pytest.mark.parametrize("words", DISTINCT_WIDTHS)
def test_distinct_of_sets_one_bit_apart(device, words):
    """Sets that differ in the last word only, in bit 31 of a middle word only, in the word of the group's last lane only
    (words 4, 8, 16 fill their group), in bit 0 of word 0 only; the empty set among them; each a different number of times."""
    base = np.arange(1, words + 1, dtype=np.uint32) * np.uint32(0x00010001)
    variants = [np.zeros(words, np.uint32), base.copy()]
    for w, bit in ((words - 1, 0), (words - 1, 31), (words // 2, 31), (0, 0), (0, 31)):
        v = base.copy()
        v[w] ^= np.uint32(1 << bit)
        variants.append(v)
    only_last = np.zeros(words, np.uint32)
    only_last[words - 1] = 0x80000000
    variants.append(only_last)
    variants = np.unique(np.array(variants), axis=0)
    times = 1 + 37 * np.arange(len(variants))
    sets = np.repeat(variants, times, axis=0)
    sets = sets[np.random.default_rng(words).permutation(len(sets))]
    want_sets, want_count = er.distinct(sets)
    assert len(want_sets) == len(variants) and sorted(want_count.tolist()) == times.tolist()
    assert_distinct(device, sets, want_sets, want_count)


@pytest.mark.parametrize("words", [1, 5, 16])
def test_distinct_of_heavy_sets_among_singletons(device, words):
    rng = np.random.default_rng(40 + words)
    heavy = rng.integers(0, 1 << 32, (3, words), dtype=np.uint64).astype(np.uint32) | np.uint32(0x40000000)
    single = rng.integers(0, 1 << 30, (5000, words), dtype=np.uint64).astype(np.uint32)
    single[:, words - 1] = np.arange(5000, dtype=np.uint32)                       # different from one another and from the heavy
    sets = np.concatenate([np.repeat(heavy, [50000, 49999, 50001], axis=0), single, np.zeros((7, words), np.uint32)])
    sets = sets[rng.permutation(len(sets))]
    want_sets, want_count = er.distinct(sets)
    assert len(want_sets) == 5000 + 3 + (0 if words == 1 else 1)      # one word: the singleton 0 is the empty set
    assert_distinct(device, sets, want_sets, want_count)


def test_distinct_output_capacity(device):
    words, n = 5, 3000
    sets = np.zeros((2 * n, words), np.uint32)
    sets[:, 2] = np.arange(2 * n) % n
    want_sets, want_count = er.distinct(sets)
    assert len(want_sets) == n and (want_count == 2).all()
    rc, n_out, got_sets, got_count = distinct_on_device(device, sets, n)            # exactly enough
    assert rc == 0 and n_out == n
    order = er.sortedRows(got_sets[:n])
    assert np.array_equal(got_sets[:n][order], want_sets) and (got_count[:n] == 2).all()
    rc, n_out, got_sets, got_count = distinct_on_device(device, sets, n - 1)        # one short: nothing handed over
    assert rc == GK_ERR_CAPACITY and n_out == n
    assert b"exceed the output capacity" in lib().gk_last_error()
    rc, n_out, _, _ = distinct_on_device(device, np.zeros((0, words), np.uint32), 4)
    assert rc == 0 and n_out == 0


# ------------------------------------------------------------------------------------------------------------ gk_sample_em
class Sample:
    """Genes of different widths side by side in one universe of ordinals, one CSR of their pairs.  Per gene: its row
    families and ``n_fav`` pairs that favour two alleles."""

    def __init__(self, shapes, n_fav=1500):
        self.genes, at = [], 37
        for words, n_allele, n_span in shapes:
            g = er.Gene(words, n_allele, n_span, vbeg=at, n_var=1 << 30, n_total=1 << 30, seed=len(self.genes))
            self.genes.append(g)
            at = g.vend
        for g in self.genes:
            g.n_var, g.n_total = at + 63, at + 63 + 40
        self.n_total = at + 63 + 40
        csr, self.rows = [], []
        for g in self.genes:
            mine = [f[1] for f in er.rowFamilies(g)] + er.favouringRows(g, n_fav)
            self.rows.append(np.arange(len(csr), len(csr) + len(mine), dtype=np.int32))
            csr += mine
        self.off, self.ids = er.packLists(csr)

    def reference(self, k, rows=None):
        g = self.genes[k]
        return er.candidateSets(self.off, self.ids, self.rows[k] if rows is None else rows, g.vbeg, g.vend, g.bits)


def em_run(device, uniq, weight, words, n_allele, iter_max=300):
    prob, iters = np.zeros(n_allele, dtype=np.float64), C.c_int32(-1)
    uniq, weight = np.ascontiguousarray(uniq, np.uint32), np.ascontiguousarray(weight, np.float64)
    check(lib().gk_em_run(device.ctx, uniq.ctypes.data, weight.ctypes.data, len(uniq), words, n_allele, iter_max, 1e-4,
                          prob.ctypes.data, C.byref(iters)))
    return prob, iters.value


def test_genes_of_different_widths_in_one_call(device):
    """Jobs of 1, 5 and 16 words (the narrow ones then run in groups of 8 lanes), bit rows in LDS next to bit rows in global
    memory, a job without rows, a job whose pairs all give the empty set."""
    shapes = [(1, 21, None), (5, 149, None), (16, 512, None), (16, 501, 1601), (3, 96, None)]
    s = Sample(shapes)
    empty_job = len(shapes) - 1
    g_e = s.genes[empty_job]
    all_sets = s.reference(empty_job)
    s.rows[empty_job] = s.rows[empty_job][~all_sets.any(axis=1)]         # of the last gene only the pairs that name nobody
    assert len(s.rows[empty_job]) > 10
    gpu = OnDevice(device, s.off, s.ids, s.n_total, None)
    bufs = []
    try:
        order = [0, 1, 2, 3, None, empty_job]                           # None: the job without rows (gene 0's tables)
        jobs = (_lib.EmJob * len(order))()
        for q, k in enumerate(order):
            g = s.genes[0 if k is None else k]
            rows = s.rows[k] if k is not None else np.zeros(1, np.int32)
            d_rows, d_mask = device.put(rows), device.put(g.mask)
            bufs += [d_rows, d_mask]
            jobs[q] = _lib.EmJob(d_rows=d_rows.ptr, n_rows=0 if k is None else len(rows), d_mask=d_mask.ptr, vbeg=g.vbeg,
                                 vend=g.vend, words=g.words, n_allele=g.n_allele, n_distinct=-1, iterations=-1)
        total = sum(s.genes[0 if k is None else k].n_allele for k in order)
        prob = np.full(total, np.nan, dtype=np.float64)
        count = np.full(total, -1, dtype=np.int64)
        check(lib().gk_sample_em(device.ctx, gpu.tab, jobs, len(order), 300, 1e-4, prob.ctypes.data, count.ctypes.data))
        at = 0
        for q, k in enumerate(order):
            g = s.genes[0 if k is None else k]
            p, c = prob[at:at + g.n_allele], count[at:at + g.n_allele]
            at += g.n_allele
            if k is None:
                assert jobs[q].n_distinct == 0 and jobs[q].iterations == 0 and not p.any() and not c.any()
                continue
            sets = s.reference(k)
            uniq, mult = er.distinct(er.pack(sets, g.words))
            assert jobs[q].n_distinct == len(uniq), k
            assert np.array_equal(c, sets.sum(axis=0)), k
            if k == empty_job:
                assert len(uniq) == 1 and not uniq.any() and not p.any() and jobs[q].iterations == 0
                continue
            assert not uniq[0].any() and uniq[1:].any(axis=1).all()     # the empty set is among them, and comes first
            want_p, want_iters = em_run(device, uniq[1:], mult[1:].astype(np.float64), g.words, g.n_allele)
            assert np.array_equal(p, want_p) and jobs[q].iterations == want_iters and want_iters > 0, k
            names = [f"A*{a:04d}" for a in range(g.n_allele)]
            oracle, _ = oem.squaremEM([[names[a] for a in np.nonzero(row)[0]] for row in sets])
            for a, name in enumerate(names):
                if name in oracle:
                    assert p[a] == pytest.approx(oracle[name], rel=1e-5, abs=1e-9), (k, name)   # BASELINE.json north_star
                else:
                    assert p[a] == 0.0, (k, name)
            assert sorted(sorted(oracle, key=oracle.get)[-2:]) == [names[3], names[7]], k      # the reads do favour two alleles
    finally:
        for b in bufs:
            b.free()
        gpu.close()


def test_capacity_of_the_one_call_form(device):
    """A gene of 32 alleles, variant k < 19 carried by allele k alone, variant 19 by everybody; pair i names variant 19 and,
    as negatives, the set bits of i: its set is ``~i``, different for every i.  2^18 pairs fill the capacity of the one-call
    form exactly; 64 more are refused with GK_ERR_CAPACITY."""
    n_most, n_allele = (1 << 18) + 64, 32
    bits = np.zeros((20, n_allele), dtype=bool)
    bits[np.arange(19), np.arange(19)] = True
    bits[19] = True
    i = np.arange(n_most, dtype=np.uint32)
    has = ((i[:, None] >> np.arange(19, dtype=np.uint32)) & 1).astype(bool)            # [pair][k]
    lens = np.zeros((n_most, 4), dtype=np.int64)
    lens[:, 0], lens[:, 2] = 1, has.sum(axis=1)
    off = np.zeros(4 * n_most + 1, dtype=np.uint32)
    np.cumsum(lens.ravel(), out=off[1:])
    ids = np.zeros(int(off[-1]), dtype=np.uint32)
    ids[off[0:-1:4]] = 19
    neg = np.ones(len(ids), dtype=bool)
    neg[off[0:-1:4]] = False
    ids[neg] = np.nonzero(has)[1]                                                      # row-major: pair by pair, k ascending
    few = np.array([0, 1, 2, 5, 255, 256, 0x3FFFF, 0x40000, n_most - 1])
    assert np.array_equal(er.pack(er.candidateSets(off, ids, few, 0, 20, bits), 1)[:, 0], ~few.astype(np.uint32))
    gpu = OnDevice(device, off, ids, 20, er.pack(bits, 1))
    d_rows = device.put(np.arange(n_most, dtype=np.int32))
    try:
        def call(n_rows):
            job = (_lib.EmJob * 1)(_lib.EmJob(d_rows=d_rows.ptr, n_rows=n_rows, d_mask=gpu.mask.ptr, vbeg=0, vend=20, words=1,
                                              n_allele=n_allele, n_distinct=-1, iterations=-1))
            prob, count = np.zeros(n_allele), np.zeros(n_allele, dtype=np.int64)
            rc = lib().gk_sample_em(device.ctx, gpu.tab, job, 1, 2, 1e-4, prob.ctypes.data, count.ctypes.data)
            return rc, job[0], prob, count
        rc, job, prob, count = call(1 << 18)
        check(rc)
        assert job.n_distinct == 1 << 18
        want = np.where(np.arange(n_allele) < 18, 1 << 17, 1 << 18)      # pairs i < 2^18 whose bit a is clear
        assert np.array_equal(count, want)
        assert prob.sum() == pytest.approx(1.0, rel=1e-9)
        rc, job, _, _ = call(n_most)
        assert rc == GK_ERR_CAPACITY
        assert b"exceed the capacity" in lib().gk_last_error()
    finally:
        d_rows.free()
        gpu.close()


def test_driver_takes_the_per_gene_calls_when_the_one_call_form_is_full(device, small_case, monkeypatch):
    """``gk_sample_em`` answering GK_ERR_CAPACITY sends ``TypingWithReport.typing`` to the per-gene calls: same calls, same
    reports, same ``em_info``."""
    from kir_graph_amd import packed
    from kir_graph_amd.engine import DeviceIndex, Tabulation
    from kir_graph_amd.hisat2 import SampleData
    from kir_graph_amd.kir_typing import TypingWithReport
    sidx, gidx, sample = small_case
    rec, table = packed.packSample(sample, gidx)
    dindex = DeviceIndex(device, gidx)
    tab = Tabulation(dindex, rec)
    data = SampleData(tab, gidx, tab.novelVariants(table.strings))

    def typed():
        typer = TypingWithReport(data)
        calls = typer.typing(sample.gene_cn)
        return calls, {g: [(r.allele, r.count, r.prob, r.cn) for r in rep] for g, rep in typer._result.items()}, dict(typer.em_info)

    try:
        want = typed()
        asked = []
        monkeypatch.setattr(lib(), "gk_sample_em", lambda *a: asked.append(len(a)) or GK_ERR_CAPACITY)
        got = typed()
        monkeypatch.undo()
        assert asked == [8]
        assert got[0] == want[0] and list(got[1]) == list(want[1]) and got[1] == want[1] and got[2] == want[2]
        assert any(rep for rep in want[1].values()) and any(v["iterations"] > 0 for v in want[2].values())
    finally:
        tab.close()
        dindex.close()
