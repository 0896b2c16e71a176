"""GPU: the pattern histogram of a likelihood call (gk_call_patterns: calldosage_patterns) against np.unique over the rows of
the expanded table (tests/dosage_reference.py), and the dosage report through TypingWithPosNegAllele and the command line.
Patterns, counts and out_of_range are integers: every comparison of them is an equality.

Shapes follow the kernel of csrc/gk_calldosage.hip: a lane takes 16 rows (kPatLaneRows), a wave 64 x 16 = 1024, a workgroup
C = 4096 rows per turn (kPatChunk), at most G = 1024 workgroups stride over the chunks (kPatMaxGroups); a workgroup holds up
to 1024 patterns in LDS (kPatLdsSlots), each within 16 slots of its start (kPatLdsProbes), and sends the runs beyond them to
the table in HBM directly; K <= 8 keys are the pattern
itself, K > 8 keys are pairs of interned halves."""
import ctypes as C_
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import dosage_reference as dr  # noqa: E402

from kir_graph_amd import _lib, packed, synth  # noqa: E402
from kir_graph_amd.call_report import modelOf  # noqa: E402
from kir_graph_amd.call_dosage import (CALL_DOSAGE_COLUMNS, callDosageText, dosageOfCall, patternsOfColumns,  # noqa: E402
                                       sortedPatterns)
from kir_graph_amd.engine import DeviceIndex, Tabulation  # noqa: E402
from kir_graph_amd.hisat2 import SampleData  # noqa: E402
from kir_graph_amd.index import GkIndex  # noqa: E402
from kir_graph_amd.kir_typing import TypingWithPosNegAllele  # noqa: E402

pytestmark = pytest.mark.gpu

C = 4096                  # kPatChunk
WAVE = 1024               # 64 lanes x 16 rows
G = 1024                  # kPatMaxGroups
SENTINEL = 0xA5A5A5A5A5A5A5A5
KINDS = ("few", "m1_positive", "some_255", "equal", "spread")


def makeTable(rng, kind, n_rows, n_table_cols, cols, ldm, pad):
    """uint8 [n_table_cols][ldm]: the rows beyond n_rows of every column hold ``pad``."""
    k = len(cols)
    t = rng.integers(0, 256, (n_table_cols, n_rows))                        # the columns not listed hold anything
    sub = (rng.random((k, n_rows)) < 0.15) * rng.integers(1, 4, (k, n_rows))    # mostly zero, 1 .. 3 here and there
    if kind == "m1_positive":                                               # the smallest byte of every row is 1 .. 200
        sub = sub + rng.integers(1, 201, n_rows)
    elif kind == "some_255":                                                # 255 in every listed column / in some of them
        every = rng.random(n_rows) < 0.2
        every[0] = True
        sub[rng.random((k, n_rows)) < 0.2] = 255
        sub[:, every] = 255
    elif kind == "equal":                                                   # one class holds all rows
        sub = np.repeat(rng.integers(0, 5, (k, 1)), n_rows, axis=1)
    elif kind == "spread":                                                  # many patterns
        sub = rng.integers(0, 7, (k, n_rows))
    t[cols] = sub
    full = np.full((n_table_cols, ldm), pad, dtype=np.uint8)
    full[:, :n_rows] = t
    return full


def rawPatterns(dev, d_table, ldm, n_rows, n_table_cols, cols, n_slots):
    """gk_call_patterns with every host output pre-filled and checked beyond its end: (rc, patterns [n, 16], counts [n],
    out_of_range, unplaced)."""
    cols = np.ascontiguousarray(cols, dtype=np.int32)
    patterns = np.full((n_slots + 2, 16), 0xA5, dtype=np.uint8)
    counts = np.full(n_slots + 2, SENTINEL, dtype=np.uint64)
    n = np.full(3, -7, dtype=np.int64)
    oor, unplaced = np.full(3, SENTINEL, dtype=np.uint64), np.full(3, SENTINEL, dtype=np.uint64)
    rc = _lib.lib().gk_call_patterns(dev.ctx, d_table.ptr, ldm, n_rows, n_table_cols, cols.ctypes.data, len(cols), n_slots,
                                     patterns.ctypes.data, counts.ctypes.data, n.ctypes.data, oor.ctypes.data,
                                     unplaced.ctypes.data)
    if rc != 0:
        return rc, None, None, None, None
    found = int(n[0])
    assert 0 <= found <= n_slots and (n[1:] == -7).all() and (oor[1:] == SENTINEL).all() and (unplaced[1:] == SENTINEL).all()
    assert (patterns[found:] == 0xA5).all() and (counts[found:] == SENTINEL).all()      # nothing beyond the list is written
    return rc, patterns[:found], counts[:found].astype(np.int64), int(oor[0]), int(unplaced[0])


def check(dev, table, n_rows, cols, where, n_slots=1 << 14):
    """One call against np.unique: the sorted patterns, their counts and out_of_range are equal.  ``n_slots`` holds every
    row of the shapes used here as a pattern of its own."""
    n_table_cols, ldm = table.shape
    d_table = dev.put(table)
    try:
        rc, patterns, counts, oor, unplaced = rawPatterns(dev, d_table, ldm, n_rows, n_table_cols, cols, n_slots)
    finally:
        d_table.free()
    assert rc == 0, (_lib.lib().gk_last_error(), where)
    want_p, want_n, want_oor = dr.patterns(table[:, :n_rows], cols)
    assert unplaced == 0 and oor == want_oor, where
    assert int(counts.sum()) + oor == n_rows, where
    assert (patterns[:, len(cols):] == 0).all(), where                       # zero-extended to 16 bytes
    got_p, got_n = sortedPatterns(patterns, counts, len(cols))
    assert np.array_equal(got_p, want_p) and np.array_equal(got_n, want_n), where
    assert (counts > 0).all() and len({bytes(p) for p in patterns}) == len(patterns), where      # no pattern twice
    assert len(got_p) == 0 or (got_p.min(axis=1) == 0).all(), where
    return want_p, want_n, want_oor


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("k", [1, 2, 3, 8, 9, 16])
@pytest.mark.parametrize("n_rows", [1, 15, 16, 17, WAVE - 1, WAVE, WAVE + 1, C - 1, C, C + 1, 2 * C + 5])
def test_patterns_equal_np_unique(device, n_rows, k):
    rng = np.random.default_rng(1000 * n_rows + k)
    for n_table_cols, more, pad in ((k, 0, 7), (k + 3, 64, 255)):
        cols = rng.permutation(n_table_cols)[:k]                          # scattered and unordered
        ldm = (n_rows + 63) // 64 * 64 + more
        for kind in KINDS:
            where = (n_table_cols, ldm, pad, kind)
            table = makeTable(rng, kind, n_rows, n_table_cols, cols, ldm, pad)
            pats, counts, oor = check(device, table, n_rows, cols, where)
            # the test's own data is what it is meant to be
            if kind == "equal":
                assert len(counts) == 1 and counts[0] == n_rows, where
            if kind == "m1_positive":
                assert table[cols][:, :n_rows].min(axis=0).min() >= 1 and oor == 0, where
            if kind == "some_255":
                assert oor >= 1 and (k == 1 or n_rows < 64 or ((pats == 255).any() and oor < n_rows)), where
            if k == 1:
                assert len(counts) <= 1 and not pats.any(), where


@pytest.mark.parametrize("k", range(1, 17))
def test_every_number_of_called_columns(device, k):
    rng = np.random.default_rng(50 + k)
    n_rows, n_table_cols = C + 33, 20
    cols = rng.permutation(n_table_cols)[:k]
    for kind in ("few", "some_255", "spread"):
        table = makeTable(rng, kind, n_rows, n_table_cols, cols, (n_rows + 63) // 64 * 64, 255)
        check(device, table, n_rows, cols, (k, kind))


@pytest.mark.parametrize("n_table_cols", [1, 16, 17, 577])
def test_table_widths_and_places_of_the_called_columns(device, n_table_cols):
    rng = np.random.default_rng(n_table_cols)
    n_rows = C + 1
    k = min(3, n_table_cols)
    places = {"first": np.arange(k), "last": np.arange(n_table_cols - k, n_table_cols)[::-1],
              "scattered": rng.permutation(n_table_cols)[:k]}
    for name, cols in places.items():
        table = makeTable(rng, "few", n_rows, n_table_cols, cols, (n_rows + 63) // 64 * 64 + 64, 7)
        check(device, table, n_rows, cols, (n_table_cols, name))


def test_more_chunks_than_workgroups(device):
    """G * C + C + 1 rows of two columns: the first workgroups take a second turn, the last lane with rows takes one.  The
    patterns here are two bytes, so the reference counts them in 65536 bins."""
    rng = np.random.default_rng(8)
    n_rows = G * C + C + 1
    ldm = (n_rows + 63) // 64 * 64
    table = np.full((2, ldm), 255, dtype=np.uint8)
    table[:, :n_rows] = rng.integers(0, 3, (2, n_rows)) * (rng.random((2, n_rows)) < 0.2)
    table[:, n_rows - 1] = (9, 255)                                       # the last row alone has this pattern
    d_table = device.put(table)
    try:
        rc, patterns, counts, oor, unplaced = rawPatterns(device, d_table, ldm, n_rows, 2, [1, 0], 4096)
    finally:
        d_table.free()
    assert rc == 0 and unplaced == 0 and oor == 0
    b = table[::-1, :n_rows].astype(np.int64)                             # the listed order: column 1, column 0
    d = np.where(b == 255, 255, b - b.min(axis=0))
    bins = np.bincount(d[0] * 256 + d[1], minlength=65536)
    want = {(int(i) // 256, int(i) % 256): int(bins[i]) for i in np.flatnonzero(bins)}
    got = {(int(p[0]), int(p[1])): int(c) for p, c in zip(patterns, counts)}
    assert got == want and got[(255, 0)] == 1 and sum(got.values()) == n_rows      # column 1 first: (255, 9 - 9)


def distinctRows(n_rows, k, a, b):
    """[k][n_rows]: every row another pattern (column 0 is zero, columns a and b count the row)."""
    t = np.zeros((k, n_rows), dtype=np.uint8)
    t[a] = np.arange(n_rows) % 250
    t[b] = np.arange(n_rows) // 250
    return t


@pytest.mark.parametrize("k,a,b", [(3, 1, 2), (16, 9, 12), (12, 3, 11)])
def test_every_row_distinct_grows_the_slots(device, k, a, b):
    """5000 rows, 5000 patterns: more than a workgroup's LDS table and more than the wrapper's first 4096 slots.  Directly
    with 64 slots rows stay unplaced and the conservation sum holds."""
    n_rows = 5000
    ldm = (n_rows + 63) // 64 * 64
    table = np.full((k, ldm), 255, dtype=np.uint8)
    table[:, :n_rows] = distinctRows(n_rows, k, a, b)
    cols = np.arange(k, dtype=np.int32)
    want_p, want_n, _ = dr.patterns(table[:, :n_rows], cols)
    assert len(want_n) == n_rows
    d_table = device.put(table)
    try:
        found = patternsOfColumns(device, d_table, ldm, n_rows, k, cols)
        assert found is not None
        got_p, got_n, oor = found
        assert oor == 0 and np.array_equal(got_p, want_p) and np.array_equal(got_n, want_n)
        assert patternsOfColumns(device, d_table, ldm, n_rows, k, cols, first_slots=64, max_slots=512) is None
        rc, patterns, counts, oor, unplaced = rawPatterns(device, d_table, ldm, n_rows, k, cols, 64)
        assert rc == 0 and unplaced > 0 and len(counts) <= 64
        assert int(counts.sum()) + unplaced + oor == n_rows
        assert len({bytes(p) for p in patterns}) == len(patterns)
        held = {bytes(p[:k]) for p in want_p}
        assert all(bytes(p[:k]) in held for p in patterns) and (counts == 1).all()
    finally:
        d_table.free()


def test_halves_of_eight_bytes_255(device):
    """K > 8: a pattern whose low or high eight bytes are all 255 (the empty word of the tables), next to patterns that
    share a half with it."""
    rows = [[255] * 8 + [0] * 8, [0] * 8 + [255] * 8, [255] * 8 + [3] + [255] * 7, [4] + [255] * 15, [255] * 16,
            [0] * 16, [255] * 8 + [0] * 8, [1] * 8 + [255] * 8, [255] * 15 + [200], [2] * 16, [255] * 8 + [0, 1] * 4]
    n_rows = len(rows)
    for k in (16, 9):
        table = np.full((k, 64), 255, dtype=np.uint8)
        table[:, :n_rows] = np.array(rows, dtype=np.uint8).T[:k]
        pats, counts, oor = check(device, table, n_rows, np.arange(k), k)
        assert oor >= 1 and (pats[:, :8] == 255).all(axis=1).any()


@pytest.mark.parametrize("k", [2, 8, 16])
def test_hash_of_four_bits_changes_nothing(device, monkeypatch, k):
    """GK_TEST_HOOKS=calldosage_hashbits=4 (and 0): every key starts its probe in one of 16 slots (in one slot); identity
    is decided on the keys, so the list is the same."""
    rng = np.random.default_rng(k)
    n_rows = C + 77
    cols = rng.permutation(k + 2)[:k]
    table = makeTable(rng, "few", n_rows, k + 2, cols, (n_rows + 63) // 64 * 64, 255)
    if k == 2:                                                            # two columns of 0 .. 3 are 7 patterns: 0 .. 29 give 59
        table[cols, :n_rows] = rng.integers(0, 30, (2, n_rows))
    plain = check(device, table, n_rows, cols, (k, "plain"))
    assert len(plain[1]) >= 16
    for bits in (4, 0):
        monkeypatch.setenv("GK_TEST_HOOKS", f"calldosage_hashbits={bits}")
        narrow = check(device, table, n_rows, cols, (k, bits))
        assert all(np.array_equal(x, y) for x, y in zip(plain, narrow))
    monkeypatch.delenv("GK_TEST_HOOKS")


def test_arguments_are_checked(device):
    n, ldm, a, slots = 100, 128, 5, 64
    d_table = device.put(np.zeros((a, ldm), dtype=np.uint8))
    patterns, counts = np.zeros((slots, 16), dtype=np.uint8), np.zeros(slots, dtype=np.uint64)
    n_out, oor, unplaced = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    lib, ctx = _lib.lib(), device.ctx
    p, c, no, o, u = (x.ctypes.data for x in (patterns, counts, n_out, oor, unplaced))

    def cols(*v):
        arr = np.array(v, dtype=np.int32)
        return arr, arr.ctypes.data

    good, good_p = cols(0, 3)
    seventeen, seventeen_p = cols(*range(17))
    twice, twice_p = cols(1, 2, 1)
    outside, outside_p = cols(0, 5)
    negative, negative_p = cols(-1)
    t, f = d_table.ptr, lib.gk_call_patterns
    bad = [
        lambda: f(ctx, t, ldm, 0, a, good_p, 2, slots, p, c, no, o, u),
        lambda: f(ctx, t, 1 << 31, 1 << 31, a, good_p, 2, slots, p, c, no, o, u),
        lambda: f(ctx, t, 64, n, a, good_p, 2, slots, p, c, no, o, u),               # ldm < n_rows
        lambda: f(ctx, t, 120, n, a, good_p, 2, slots, p, c, no, o, u),              # ldm % 64 != 0
        lambda: f(ctx, t, ldm, n, 0, good_p, 2, slots, p, c, no, o, u),
        lambda: f(ctx, t, ldm, n, a, good_p, 0, slots, p, c, no, o, u),
        lambda: f(ctx, t, ldm, n, 20, seventeen_p, 17, slots, p, c, no, o, u),
        lambda: f(ctx, t, ldm, n, a, twice_p, 3, slots, p, c, no, o, u),
        lambda: f(ctx, t, ldm, n, a, outside_p, 2, slots, p, c, no, o, u),
        lambda: f(ctx, t, ldm, n, a, negative_p, 1, slots, p, c, no, o, u),
        lambda: f(ctx, 0, ldm, n, a, good_p, 2, slots, p, c, no, o, u),
        lambda: f(ctx, t + 8, ldm, n, a, good_p, 2, slots, p, c, no, o, u),          # not 16-byte aligned
        lambda: f(ctx, t, ldm, n, a, None, 2, slots, p, c, no, o, u),
        lambda: f(ctx, t, ldm, n, a, good_p, 2, 8, p, c, no, o, u),                  # too few slots
        lambda: f(ctx, t, ldm, n, a, good_p, 2, 96, p, c, no, o, u),                 # no power of two
        lambda: f(ctx, t, ldm, n, a, good_p, 2, 1 << 25, p, c, no, o, u),
        lambda: f(ctx, t, ldm, n, a, good_p, 2, slots, None, c, no, o, u),
        lambda: f(ctx, t, ldm, n, a, good_p, 2, slots, p, None, no, o, u),
        lambda: f(ctx, t, ldm, n, a, good_p, 2, slots, p, c, None, o, u),
        lambda: f(ctx, t, ldm, n, a, good_p, 2, slots, p, c, no, None, u),
        lambda: f(ctx, t, ldm, n, a, good_p, 2, slots, p, c, no, o, None),
    ]
    for k, call in enumerate(bad):
        assert call() == -3, k                                  # GK_ERR_ARG, and nothing was launched
        assert lib.gk_last_error(), k
    assert not patterns.any() and not counts.any() and not n_out.any() and not oor.any() and not unplaced.any()
    # the context still works: a table of zeros is one pattern
    _lib.check(f(ctx, t, ldm, n, a, good_p, 2, slots, p, c, no, o, u))
    assert n_out[0] == 1 and counts[0] == n and not patterns[0].any() and oor[0] == 0 and unplaced[0] == 0
    d_table.free()


def poolHook(ctx, nth):
    """Arm the test-only failure of the n-th pool allocation (0: disarm): (blocks of the context that are out,
    allocations counted since the call before), as tests/test_gpu_pool_ownership.py uses it."""
    live, count = C_.c_int64(), C_.c_int64()
    _lib.check(_lib.lib().gk_test_pool_fail(ctx, nth, C_.byref(live), C_.byref(count)))
    return live.value, count.value


def test_a_failed_allocation_leaves_no_block_out(device):
    """gk_call_patterns takes two pool blocks (the keys; the counts and counters): with either failing, the call returns
    an error, no block of the context stays out and the same call with nothing armed gives the clean run's list."""
    rng = np.random.default_rng(20261020)
    n, ldm, a = 300, 320, 12
    cols = np.array([4, 1, 6, 0, 2, 3, 5, 7, 9, 11], dtype=np.int32)      # K > 8: the three key tables are one block
    table = makeTable(rng, "few", n, a, cols, ldm, 255)
    d_table = device.put(table)

    def run(nth):
        before, _ = poolHook(device.ctx, nth)
        try:
            out = rawPatterns(device, d_table, ldm, n, a, cols, 256)
        finally:
            after, taken = poolHook(device.ctx, 0)
        return out, before, after, taken

    try:
        poolHook(device.ctx, 0)
        for _ in range(2):
            out, before, after, taken = run(1 << 40)
            assert out[0] == 0 and after == before, _lib.lib().gk_last_error()
        assert taken == 2
        want_p, want_n, want_oor = dr.patterns(table[:, :n], cols)
        clean = sortedPatterns(out[1], out[2], len(cols))
        assert np.array_equal(clean[0], want_p) and np.array_equal(clean[1], want_n) and out[3] == want_oor
        for nth in (1, 2):
            out, before, after, taken = run(nth)
            assert out[0] != 0 and taken == nth and _lib.lib().gk_last_error()
            assert after == before, f"{after - before} blocks of the context left out"
            out, before, after, _ = run(1 << 40)
            assert out[0] == 0 and after == before
            again = sortedPatterns(out[1], out[2], len(cols))
            assert np.array_equal(again[0], want_p) and np.array_equal(again[1], want_n) and out[3:] == (want_oor, 0)
    finally:
        poolHook(device.ctx, 0)
        d_table.free()


# ------------------------------------------------------------------------------------------------ the drivers
STRATEGIES = {"full": {}, "exonfirst": {"exon_first": True}}


@pytest.fixture(scope="module")
def tabulated(device, small_case):
    sidx, gidx, sample = small_case
    rec, table = packed.packSample(sample, gidx)
    tab = Tabulation(DeviceIndex(device, gidx), rec)
    return SampleData(tab, gidx, tab.novelVariants(table.strings)), sample


@pytest.fixture(scope="module")
def typed(tabulated):
    """Per strategy: the sample typed without and with the dosage report (the whole-sample paths)."""
    data, sample = tabulated
    out = {}
    for name, kw in STRATEGIES.items():
        plain = TypingWithPosNegAllele(data, variant_correction=True, **kw)
        plain_calls = plain.typing(sample.gene_cn)
        dosage = TypingWithPosNegAllele(data, variant_correction=True, call_dosage=True, **kw)
        dosage_calls = dosage.typing(sample.gene_cn)
        out[name] = (plain, plain_calls, dosage, dosage_calls)
    return out


def checkEntry(entry, result, where):
    """One CallDosage against the brute force on the table downloaded from HBM."""
    model = modelOf(result)
    row = np.asarray(result.allele_id, dtype=np.int64)[result.bestRank()]
    ids, copies = np.unique(row, return_counts=True)
    miss8, ldm, n_table_cols, cols = model.missFor(ids)
    table = miss8.download().reshape(n_table_cols, ldm)[:, :model.n_rows]
    pats, counts, oor = dr.patterns(table, cols)
    assert np.array_equal(entry.patterns, pats) and np.array_equal(entry.counts, counts), where
    assert (entry.out_of_range, entry.reads, entry.cn) == (oor, model.n_rows, result.n), where
    assert int(counts.sum()) + oor == model.n_rows and len(counts) >= 1, where
    called = list(result.selectBest())
    assert sorted(a.allele for a in entry.alleles for _ in range(a.copies)) == sorted(called), where
    assert [a.copies for a in entry.alleles] == copies.tolist(), where
    ref = dr.em(pats, counts, copies.tolist())
    assert ref.converged, where                                     # the reference alone converges
    assert entry.converged and abs(entry.iterations - ref.iterations) <= 1, where
    dev64, limit, want = dr.bound(pats, counts, copies.tolist(), entry.iterations)
    assert limit <= dr.BOUND_CEILING, where
    worst = max(float(abs(dr.LD(a.share) - t)) for a, t in zip(entry.alleles, want.theta))
    print(f"{where}: K {len(ids)}, {len(counts)} patterns, {entry.iterations} passes, dev64 {dev64:.3g}, bound {limit:.3g}, "
          f"share off by {worst:.3g}, kkt {entry.kkt:.3g}")
    assert worst <= limit, where
    assert abs(sum(a.share for a in entry.alleles) - 1) <= 1e-12 and entry.kkt <= 1e-10, where
    assert [a.dosage for a in entry.alleles] == [a.share * entry.cn for a in entry.alleles], where
    assert entry.loglik_free >= entry.loglik_called, where
    scale = 1e-12 * max(1.0, abs(float(want.loglik_called)))
    assert abs(entry.loglik_called - float(want.loglik_called)) <= scale, where
    assert entry.same is not None and entry.same[1] >= 0 and entry.plus is not None, where
    assert (entry.minus is None) == (entry.cn == 1), where
    for which, total in ((entry.minus, entry.cn - 1), (entry.same, entry.cn), (entry.plus, entry.cn + 1)):
        if which is not None:
            pairs, delta = which
            assert [a for a, _ in pairs] == [a.allele for a in entry.alleles] and sum(c for _, c in pairs) == total, where
            value = dr.loglik(pats, counts, [c / total for _, c in pairs])
            assert abs((value - entry.loglik_called) - delta) <= 1e-9 * max(1.0, abs(value)) or value == delta == -math.inf, where
    return len(ids)


def test_point_result_does_not_change(typed):
    for name, (plain, plain_calls, dosage, dosage_calls) in typed.items():
        assert dosage_calls == plain_calls, name                 # calls and warnings
        assert plain.call_dosage == {}
        assert list(plain._result) == list(dosage._result)
        for gene in plain._result:
            a, b = list(plain._result[gene]), list(dosage._result[gene])
            assert len(a) == len(b), (name, gene)
            for x, y in zip(a, b):
                assert x.n == y.n and list(x.allele_name) == list(y.allele_name)
                for f in ("value", "value_sum_indv", "allele_id", "fraction", "fraction_uniq"):
                    assert np.array_equal(getattr(x, f), getattr(y, f)), (name, gene, f)


def test_whole_sample_entries_equal_the_brute_force(tabulated, typed):
    data, sample = tabulated
    for name, (_, _, dosage, _) in typed.items():
        want = {g for g, cn in sample.gene_cn.items() if cn and dosage._result.get(g) and not dosage._result[g][-1].isFail()}
        assert set(dosage.call_dosage) == want and len(want) >= 2, name
        widths = [checkEntry(entry, dosage._result[gene][-1], (name, gene)) for gene, entry in dosage.call_dosage.items()]
        assert max(widths) >= 2, name
        scopes = {e.scope for e in dosage.call_dosage.values()}
        assert scopes <= {"all", "candidates"} and (name != "full" or scopes == {"all"})


def test_per_gene_path_gives_the_same_entries(tabulated, typed):
    data, sample = tabulated
    for name, kw in STRATEGIES.items():
        whole = typed[name][2]
        per_gene = TypingWithPosNegAllele(data, variant_correction=True, call_dosage=True, **kw)
        for gene, cn in sample.gene_cn.items():
            if cn:
                per_gene.typingPerGene(gene, int(cn))
        assert per_gene.call_dosage.keys() == whole.call_dosage.keys(), name
        for gene, a in whole.call_dosage.items():
            b = per_gene.call_dosage[gene]
            checkEntry(b, per_gene._result[gene][-1], (name, gene, "per gene"))
            assert np.array_equal(a.patterns, b.patterns) and np.array_equal(a.counts, b.counts), (name, gene)
            assert a.alleles == b.alleles and (a.minus, a.same, a.plus) == (b.minus, b.same, b.plus), (name, gene)
            assert (a.iterations, a.kkt, a.loglik_called, a.loglik_free) == (b.iterations, b.kkt, b.loglik_called, b.loglik_free)


def test_command_line_writes_the_dosage_file(device, tmp_path, monkeypatch):
    """graphkir --allele-strategy exonfirst on a small BAM, without and with --call-dosage (in-process, like
    tests/test_gpu_cn_cli.py): the typing files do not change, the new file is the typer's report."""
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
    for k, extra in enumerate(([], ["--call-dosage"])):
        run = tmp_path / f"run{k}"       # paths relative to the run's folder: the files name the sample's output
        run.mkdir()
        monkeypatch.chdir(run)
        cli.main(cli.createParser().parse_args(
            ["--step-skip-extraction", "--index-folder", "../index", "--output-folder", "out", "--allele-strategy", "exonfirst",
             "--cn-provided", "../s.cn.tsv", "--alignment", "../s.bam"] + extra))
        files.append({p.name: p for p in (run / "out").iterdir()})
    new = [n for n in files[1] if n.endswith(".dosage.tsv")]
    assert len(new) == 1 and files[0].keys() | set(new) == files[1].keys()
    assert not any(n.endswith(".dosage.tsv") for n in files[0])
    def content(path):
        # The novel variants of the .variant.json hand-off are numbered by a counter of the process ("nv0" in the first
        # run of a process, "nv707" in the second, with or without the flag): numbered here by first appearance instead.
        data = path.read_bytes()
        if path.name.endswith(".variant.json"):
            seen: dict = {}
            data = re.sub(rb'"nv\d+"', lambda m: seen.setdefault(m.group(0), b'"nv#%d"' % len(seen)), data)
        return data

    for n in files[0]:                                           # every other output, byte for byte
        if files[0][n].is_file():
            assert content(files[0][n]) == content(files[1][n]), n
    assert len(typers) == 2 and typers[0].call_dosage == {}
    typer = typers[1]
    typed_genes = [g for g, cn in s.gene_cn.items() if cn and typer._result.get(g) and not typer._result[g][-1].isFail()]
    assert list(typer.call_dosage) == typed_genes and len(typed_genes) >= 2
    text = files[1][new[0]].read_text()
    assert text == callDosageText(typer.call_dosage)
    rows = [line.split("\t") for line in text.split("\n")[1:-1]]
    assert text.split("\n")[0].split("\t") == CALL_DOSAGE_COLUMNS and all(len(r) == len(CALL_DOSAGE_COLUMNS) for r in rows)
    assert [r[0] for r in rows] == [g for g in typed_genes for _ in typer.call_dosage[g].alleles]
    for gene in typed_genes:
        checkEntry(typer.call_dosage[gene], typer._result[gene][-1], ("cli", gene))


# ------------------------------------------------------------------------------------------------ one planted case
def test_planted_two_to_one(device):
    """One gene whose three drawn copies are (A, B, A) -- the first sample seed of the generator with two distinct alleles
    among three copies -- so its error-free reads come 2 : 1 from A and B, typed at copy number 2.  The search calls
    (A, B); the dosage of A lies within three binomial sigmas of the planted 2 / 3 x 2, sigma from the reads private to one
    of the two, and the best composition at three copies doubles A."""
    sidx = synth.makeIndex(seed=41, n_genes=1, len_range=(4200, 4600), var_range=(60, 60), allele_range=(6, 6), frac_del=0,
                           frac_ins=0)
    gene = sidx.genes[0]
    sample = synth.makeSample(sidx, seed=1, n_pairs=3000, err_rate=0.0, gene_cn={gene: 3}, frac_multi=0, frac_improper=0,
                              frac_clip=0)
    truth = sample.truth[gene]
    doubled = max(set(truth), key=truth.count)
    single = min(set(truth), key=truth.count)
    assert sorted(truth.count(a) for a in set(truth)) == [1, 2]
    gidx = GkIndex.fromVariants(sidx.variants, genes=sidx.genes, exons=sidx.exons)
    rec, table = packed.packSample(sample, gidx)
    tab = Tabulation(DeviceIndex(device, gidx), rec)
    data = SampleData(tab, gidx, tab.novelVariants(table.strings))
    typer = TypingWithPosNegAllele(data, variant_correction=True, call_dosage=True)
    calls, _ = typer.typing({gene: 2})
    assert sorted(calls) == sorted([doubled, single])
    entry = typer.call_dosage[gene]
    checkEntry(entry, typer._result[gene][-1], "planted")
    by_name = {a.allele: (j, a) for j, a in enumerate(entry.alleles)}
    jd, a_doubled = by_name[doubled]
    js, a_single = by_name[single]
    # reads private to one of the two: zero on its column, more on the other
    private_d = int(entry.counts[(entry.patterns[:, jd] == 0) & (entry.patterns[:, js] > 0)].sum())
    private_s = int(entry.counts[(entry.patterns[:, js] == 0) & (entry.patterns[:, jd] > 0)].sum())
    n_private = private_d + private_s
    share = 2.0 / 3.0
    sigma = math.sqrt(share * (1 - share) / n_private)
    print(f"planted: private reads {private_d} : {private_s}, share {a_doubled.share!r}, three sigma {3 * sigma:.4f}, "
          f"dosage {a_doubled.dosage!r}, deltas {entry.minus[1]!r} {entry.same[1]!r} {entry.plus[1]!r}")
    assert n_private >= 200 and entry.cn == 2 and (a_doubled.copies, a_single.copies) == (1, 1)
    assert abs(a_doubled.share - share) <= 3 * sigma
    assert abs(a_doubled.dosage - 2 * share) <= 2 * 3 * sigma
    assert dict(entry.plus[0]) == {doubled: 2, single: 1} and entry.plus[1] > entry.same[1]
    assert a_doubled.tied_with == [] and a_single.tied_with == []
    tab.close()
