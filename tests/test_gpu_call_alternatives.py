"""GPU: the alternatives of each called allele (gk_call_swap: callswap_rows, callswap_sums) against the brute-force numpy
restatement of tests/callswap_reference.py, and through TypingWithPosNegAllele and the command line.  Everything is an
integer: every comparison is an equality.

Shapes follow the kernels of csrc/gk_callswap.hip: a lane takes 16 rows, a wave 1024, a workgroup C = 4096 rows per turn;
callswap_sums takes 32 / KT columns per workgroup (at most 16), KT = the called columns rounded up to 1, 2, 4, 8 or 16."""
import ctypes as C_
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import callswap_reference as sr  # noqa: E402

from kir_graph_amd import _lib, packed, synth  # noqa: E402
from kir_graph_amd.call_alternatives import CALL_ALTERNATIVES_COLUMNS, CLASSES, alternativesOfCall  # noqa: E402
from kir_graph_amd.call_report import modelOf  # noqa: E402
from kir_graph_amd.engine import DeviceIndex, Tabulation  # noqa: E402
from kir_graph_amd.hisat2 import SampleData  # noqa: E402
from kir_graph_amd.index import GkIndex  # noqa: E402
from kir_graph_amd.kir_typing import TypingWithPosNegAllele  # noqa: E402
from kir_graph_amd.msa2hisat import Variant  # noqa: E402
from oracle import tabulate as ot, typing as oty  # noqa: E402

pytestmark = pytest.mark.gpu

C = 4096                  # kSwapChunk
SENTINEL = 0xA5A5A5A5A5A5A5A5
STATE_SENTINEL = 0xA5
KINDS = ("ties", "equal", "smallest", "out_of_range", "large")


def tile(k):
    """swapTile(KT): the columns of a workgroup of callswap_sums for k called columns."""
    kt = next(t for t in (1, 2, 4, 8, 16) if k <= t)
    return min(16, 32 // kt)


def makeTable(rng, kind, n_rows, n_table_cols, cols, ldm, pad):
    """uint8 [n_table_cols][ldm]: the rows beyond n_rows of every column hold ``pad`` (the kinds of
    tests/test_gpu_call_fit.py, restated)."""
    k = len(cols)
    t = rng.integers(0, 4, (n_table_cols, n_rows))                           # 0 .. 3: many ties
    if kind == "equal":                                                     # the listed columns are one column
        t[cols] = t[cols[0]]
    elif kind == "smallest":                                                # one listed column strictly smallest everywhere
        t[cols] = rng.integers(3, 9, (k, n_rows))
        t[cols[k // 2]] = rng.integers(0, 3, n_rows)
    elif kind == "out_of_range":                                            # 255 in every listed column / in some of them
        every = rng.random(n_rows) < 0.3
        every[0] = True
        t[np.ix_(cols, np.flatnonzero(every))] = 255
        some = rng.random((k, n_rows)) < 0.3
        sub = t[cols]
        sub[some] = 255
        t[cols] = sub
    elif kind == "large":                                                   # the levels 0 .. 255: the listed columns of a
        levels = np.array([0, 1, 14, 15, 16, 17, 99, 100, 254, 255])       # row start at the row's own level
        t = rng.choice(levels, (n_table_cols, n_rows))
        t[cols] = np.maximum(t[cols], rng.choice(levels, n_rows))
    full = np.full((n_table_cols, ldm), pad, dtype=np.uint8)
    full[:, :n_rows] = t
    return full


def callSwap(dev, table, n_rows, cols, want_state=True):
    """gk_call_swap with every host output pre-filled: (dict like callswap_reference.swaps, row state [3][n_rows] or
    None)."""
    n_table_cols, ldm = table.shape
    cols = np.ascontiguousarray(cols, dtype=np.int32)
    k, a = len(cols), n_table_cols
    d_table = dev.put(table)
    loss, rows_for = np.full(k * a + 2, SENTINEL, dtype=np.uint64), np.full(k * a + 2, SENTINEL, dtype=np.uint64)
    gain, against = np.full(a + 2, SENTINEL, dtype=np.uint64), np.full(a + 2, SENTINEL, dtype=np.uint64)
    m, beyond = np.full(3, SENTINEL, dtype=np.uint64), np.full(3, SENTINEL, dtype=np.uint64)
    d_state = dev.put(np.full(3 * ldm + 16, STATE_SENTINEL, dtype=np.uint8)) if want_state else None
    try:
        _lib.check(_lib.lib().gk_call_swap(dev.ctx, d_table.ptr, ldm, n_rows, a, cols.ctypes.data, k, loss.ctypes.data,
                                           rows_for.ctypes.data, gain.ctypes.data, against.ctypes.data, m.ctypes.data,
                                           beyond.ctypes.data, d_state.ptr if want_state else 0))
        state = d_state.download() if want_state else None
    finally:
        d_table.free()
        if d_state is not None:
            d_state.free()
    for arr, n in ((loss, k * a), (rows_for, k * a), (gain, a), (against, a), (m, 1), (beyond, 1)):
        assert (arr[n:] == SENTINEL).all()                           # nothing beyond the end of an output
    if want_state:
        assert (state[3 * ldm:] == STATE_SENTINEL).all()
        planes = state[:3 * ldm].reshape(3, ldm)
        assert (planes[:, n_rows:] == STATE_SENTINEL).all()          # nothing at or beyond n_rows is written
        state = planes[:, :n_rows].astype(np.int64)
    got = {"loss": loss[:k * a].reshape(k, a).astype(np.int64), "rows_for": rows_for[:k * a].reshape(k, a).astype(np.int64),
           "gain": gain[:a].astype(np.int64), "rows_against": against[:a].astype(np.int64), "m": int(m[0]),
           "out_of_range": int(beyond[0])}
    got["delta"] = got["loss"] - got["gain"][None, :]
    return got, state


def assertSame(got, want, where):
    for key in ("m", "out_of_range"):
        assert got[key] == want[key], (key, where)
    for key in ("gain", "rows_against", "loss", "rows_for", "delta"):
        assert np.array_equal(got[key], want[key]), (key, where)


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("k", [1, 2, 3, 4, 8, 16])
@pytest.mark.parametrize("n_rows", [1, 15, 16, 17, 63, 64, 65, C - 1, C, C + 1, 2 * C + 5])
def test_swaps_equal_the_restatement(device, n_rows, k):
    rng = np.random.default_rng(1000 * n_rows + k)
    t = tile(k)
    at = (k + t) // t * t                                             # the first tile edge above k
    # the table's width: the called columns alone, one below, at and above a tile edge
    widths = sorted({k, max(k, at - 1), at, at + 1})
    case = 0
    for n_table_cols in widths:
        cols = rng.permutation(n_table_cols)[:k]                      # scattered and unordered
        for more, pad in ((0, 7), (64, 255)) if (case + k) % 2 else ((0, 255), (64, 7)):
            ldm = (n_rows + 63) // 64 * 64 + more
            kind = KINDS[(case + n_rows + k) % len(KINDS)]
            where = (n_table_cols, ldm, pad, kind)
            table = makeTable(rng, kind, n_rows, n_table_cols, cols, ldm, pad)
            case += 1
            got, state = callSwap(device, table, n_rows, cols, want_state=case % 4 != 0)
            want = sr.swaps(table[:, :n_rows], cols)
            assertSame(got, want, where)
            if state is not None:
                m1, m2, own = sr.rowState(table[:, :n_rows], cols)
                assert np.array_equal(state[0], m1) and np.array_equal(state[1], m2) and np.array_equal(state[2], own), where
            # the test's own data is what it is meant to be
            for j, c in enumerate(cols):
                assert not got["loss"][j, c] and not got["rows_for"][j, c] and not got["gain"][c], where
            if kind == "equal" and k > 1:                              # nobody owns a row: no called allele is missed
                assert not got["loss"][:, cols].any(), where
            if kind == "out_of_range":
                assert got["out_of_range"] >= 1, where
    assert case == 2 * len(widths)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", [1, 4, 16])
def test_swaps_on_a_wide_table(device, k, kind):
    """577 columns (37 tiles of 16 and one column, 289 of 2 and one), 65 and C + 1 rows."""
    rng = np.random.default_rng(577 * k + len(kind))
    for n_rows in (65, C + 1):
        cols = rng.permutation(577)[:k]
        ldm = (n_rows + 63) // 64 * 64 + 64
        table = makeTable(rng, kind, n_rows, 577, cols, ldm, 255)
        got, _ = callSwap(device, table, n_rows, cols, want_state=False)
        assertSame(got, sr.swaps(table[:, :n_rows], cols), (n_rows, k, kind))


def test_arguments_are_checked(device):
    n, ldm, a = 100, 128, 5
    d_table = device.put(np.zeros((a, ldm), dtype=np.uint8))
    d_state = device.put(np.zeros(3 * ldm + 16, dtype=np.uint8))
    loss, rows_for = np.zeros(16 * 20, dtype=np.uint64), np.zeros(16 * 20, dtype=np.uint64)
    gain, against = np.zeros(20, dtype=np.uint64), np.zeros(20, dtype=np.uint64)
    m, beyond = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    lib, ctx = _lib.lib(), device.ctx
    lo, fo, ga, ag, mm, be = (x.ctypes.data for x in (loss, rows_for, gain, against, m, beyond))

    def cols(*c):
        arr = np.array(c, dtype=np.int32)
        return arr, arr.ctypes.data

    good, good_p = cols(0, 3)
    seventeen, seventeen_p = cols(*range(17))
    twice, twice_p = cols(1, 2, 1)
    outside, outside_p = cols(0, 5)
    negative, negative_p = cols(-1)
    t, st = d_table.ptr, d_state.ptr
    call = lib.gk_call_swap
    bad = [
        lambda: call(ctx, t, ldm, 0, a, good_p, 2, lo, fo, ga, ag, mm, be, st),
        lambda: call(ctx, t, 1 << 31, 1 << 31, a, good_p, 2, lo, fo, ga, ag, mm, be, st),
        lambda: call(ctx, t, 64, n, a, good_p, 2, lo, fo, ga, ag, mm, be, st),              # ldm < n_rows
        lambda: call(ctx, t, 120, n, a, good_p, 2, lo, fo, ga, ag, mm, be, st),             # ldm % 64 != 0
        lambda: call(ctx, t, ldm, n, 0, good_p, 2, lo, fo, ga, ag, mm, be, st),
        lambda: call(ctx, t, ldm, n, a, good_p, 0, lo, fo, ga, ag, mm, be, st),
        lambda: call(ctx, t, ldm, n, 20, seventeen_p, 17, lo, fo, ga, ag, mm, be, st),
        lambda: call(ctx, t, ldm, n, a, twice_p, 3, lo, fo, ga, ag, mm, be, st),
        lambda: call(ctx, t, ldm, n, a, outside_p, 2, lo, fo, ga, ag, mm, be, st),
        lambda: call(ctx, t, ldm, n, a, negative_p, 1, lo, fo, ga, ag, mm, be, st),
        lambda: call(ctx, 0, ldm, n, a, good_p, 2, lo, fo, ga, ag, mm, be, st),
        lambda: call(ctx, t + 8, ldm, n, a, good_p, 2, lo, fo, ga, ag, mm, be, st),         # a table that is not aligned
        lambda: call(ctx, t, ldm, n, a, good_p, 2, lo, fo, ga, ag, mm, be, st + 8),         # a state that is not aligned
        lambda: call(ctx, t, ldm, n, a, None, 2, lo, fo, ga, ag, mm, be, st),
        lambda: call(ctx, t, ldm, n, a, good_p, 2, None, fo, ga, ag, mm, be, st),
        lambda: call(ctx, t, ldm, n, a, good_p, 2, lo, None, ga, ag, mm, be, st),
        lambda: call(ctx, t, ldm, n, a, good_p, 2, lo, fo, None, ag, mm, be, st),
        lambda: call(ctx, t, ldm, n, a, good_p, 2, lo, fo, ga, None, mm, be, st),
        lambda: call(ctx, t, ldm, n, a, good_p, 2, lo, fo, ga, ag, None, be, st),
        lambda: call(ctx, t, ldm, n, a, good_p, 2, lo, fo, ga, ag, mm, None, st),
    ]
    for k, one in enumerate(bad):
        assert one() == -3, k                                   # GK_ERR_ARG, and nothing was launched
        assert lib.gk_last_error(), k
    assert not any(x.any() for x in (loss, rows_for, gain, against, m, beyond)) and not d_state.download().any()
    # the context still works: a table of zeros has no owner anywhere
    _lib.check(call(ctx, t, ldm, n, a, good_p, 2, lo, fo, ga, ag, mm, be, st))
    assert not any(x.any() for x in (loss, rows_for, gain, against, m, beyond))
    state = d_state.download()
    assert not state[:2 * ldm].any() and (state[2 * ldm:2 * ldm + n] == 255).all() and not state[2 * ldm + n:].any()
    d_table.free()
    d_state.free()


def poolHook(ctx, nth):
    """Arm the test-only failure of the n-th pool allocation (0: disarm): (blocks of the context that are out,
    allocations counted since the call before), as tests/test_gpu_pool_ownership.py uses it."""
    live, count = C_.c_int64(), C_.c_int64()
    _lib.check(_lib.lib().gk_test_pool_fail(ctx, nth, C_.byref(live), C_.byref(count)))
    return live.value, count.value


def test_a_failed_allocation_leaves_no_block_out(device):
    """gk_call_swap takes two pool blocks (the counters, the row state): with either failing, the call returns an error,
    no block of the context stays out and the same call with nothing armed gives the clean run's numbers."""
    rng = np.random.default_rng(20261020)
    n, ldm, a = 300, 320, 7
    table = makeTable(rng, "ties", n, a, [4, 1, 6], ldm, 255)
    d_table = device.put(table)
    cols = np.array([4, 1, 6], dtype=np.int32)
    outs = [np.zeros(3 * a, np.uint64), np.zeros(3 * a, np.uint64), np.zeros(a, np.uint64), np.zeros(a, np.uint64),
            np.zeros(1, np.uint64), np.zeros(1, np.uint64)]

    def run(nth):
        before, _ = poolHook(device.ctx, nth)
        try:
            rc = _lib.lib().gk_call_swap(device.ctx, d_table.ptr, ldm, n, a, cols.ctypes.data, 3, *(o.ctypes.data for o in outs), 0)
        finally:
            after, taken = poolHook(device.ctx, 0)
        return rc, before, after, taken

    try:
        poolHook(device.ctx, 0)
        for _ in range(2):
            rc, before, after, taken = run(1 << 40)
            assert rc == 0 and after == before, _lib.lib().gk_last_error()
        assert taken == 2
        clean = [o.copy() for o in outs]
        want = sr.swaps(table[:, :n], cols)
        assert np.array_equal(clean[0].reshape(3, a), want["loss"]) and np.array_equal(clean[2], want["gain"])
        for nth in (1, 2):
            rc, before, after, taken = run(nth)
            assert rc != 0 and taken == nth and _lib.lib().gk_last_error()
            assert after == before, f"{after - before} blocks of the context left out"
            rc, before, after, _ = run(1 << 40)
            assert rc == 0 and after == before
            assert all(np.array_equal(x, y) for x, y in zip(outs, clean))
    finally:
        poolHook(device.ctx, 0)
        d_table.free()


# ------------------------------------------------------------------------------------------------ the drivers
STRATEGIES = {"full": {}, "exonfirst": {"exon_first": True}}
WITHIN, LISTED = 1, 20


@pytest.fixture(scope="module")
def tabulated(device, small_case):
    sidx, gidx, sample = small_case
    rec, table = packed.packSample(sample, gidx)
    tab = Tabulation(DeviceIndex(device, gidx), rec)
    return SampleData(tab, gidx, tab.novelVariants(table.strings)), sample


@pytest.fixture(scope="module")
def typed(tabulated):
    """Per strategy: the sample typed without and with the alternatives (the whole-sample paths)."""
    data, sample = tabulated
    out = {}
    for name, kw in STRATEGIES.items():
        plain = TypingWithPosNegAllele(data, variant_correction=True, **kw)
        plain_calls = plain.typing(sample.gene_cn)
        alt = TypingWithPosNegAllele(data, variant_correction=True, call_alternatives=True, **kw)
        alt_calls = alt.typing(sample.gene_cn)
        out[name] = (plain, plain_calls, alt, alt_calls)
    return out


@pytest.fixture(scope="module")
def oracle_models(small_case):
    """gene -> (oracle model, mismatch table [reads, alleles]): computed once on the CPU."""
    sidx, gidx, sample = small_case
    ref = ot.tabulateLines(synth.toSamLines(sample), gidx.variants)
    out = {}
    for gname in gidx.genes:
        reads = [dict(r) for r in ref["reads"] if r["backbone"] == gname and r["multiple"] == 1]
        variants = [v for v in ref["variants"] if v.ref == gname]
        om = oty.GeneModel(reads, variants, top_n=300, variant_correction=True)
        miss, _ = oty.missTable(om.reads, om.variants, om.allele_to_id)
        out[gname] = (om, miss)
    return out


def expectedAlleles(table, cols, name_of, within, listed):
    """Per called column what the report must say, from the restatement on ``table`` [columns][reads]: (counts per class,
    the listed rows as (name, class, delta, loss, gain, rows_for, rows_against), every free alternative's name)."""
    want = sr.swaps(table, cols)
    out = []
    for k, col in enumerate(cols):
        found, free = [], []
        for a in range(table.shape[0]):
            if a == col:
                continue
            loss, gain = int(want["loss"][k, a]), int(want["gain"][a])
            delta = loss - gain
            cls = "better" if delta < 0 else ("identical" if loss == 0 else "balanced") if delta == 0 else \
                "near" if delta <= within else None
            if cls is None:
                continue
            if cls != "near":
                free.append(name_of(a))
            found.append((CLASSES.index(cls), delta if cls in ("better", "near") else 0, a,
                          (name_of(a), cls, delta, loss, gain, int(want["rows_for"][k, a]), int(want["rows_against"][a]))))
        found.sort(key=lambda f: f[:3])
        counts = [sum(1 for f in found if f[0] == i) for i in range(4)]
        out.append((counts, [f[3] for f in found[:listed]], free))
    return want, out


def checkEntry(entry, result, table, cols, name_of, scope, where):
    """One CallAlternatives against the restatement on ``table`` [columns][reads], ``cols`` the called columns in
    ascending allele ordinal."""
    want, alleles = expectedAlleles(table, cols, name_of, WITHIN, LISTED)
    assert (entry.cn, entry.reads, entry.mismatches, entry.out_of_range, entry.scope) == \
        (result.n, table.shape[1], want["m"], want["out_of_range"], scope), where
    called = list(result.selectBest())
    assert sorted(a.allele for a in entry.alleles for _ in range(a.copies)) == sorted(called), where
    assert [a.allele for a in entry.alleles] == [name_of(c) for c in cols], where
    for a, (counts, rows, free) in zip(entry.alleles, alleles):
        assert [a.n_better, a.n_identical, a.n_balanced, a.n_near] == counts, (where, a.allele)
        assert [(x.allele, x.cls, x.delta, x.loss, x.gain, x.rows_for, x.rows_against) for x in a.listed] == rows, (where, a.allele)
        assert a.resolved == expectedResolved(a.allele, free), (where, a.allele)
    return want


def expectedResolved(name, free):
    """The rule for names that are all GENE* plus seven digits (synth.makeIndex makes no others)."""
    gene, digits = name.split("*")
    assert len(digits) == 7 and digits.isdigit() and all(len(f.split("*")[1]) == 7 for f in free)
    if not free:
        return name
    for width in (5, 3):
        if all(f.startswith(f"{gene}*{digits[:width]}") for f in free):
            return f"{gene}*{digits[:width]}"
    return gene + "*"


def test_point_result_does_not_change(typed):
    for name, (plain, plain_calls, alt, alt_calls) in typed.items():
        assert alt_calls == plain_calls, name                   # calls and warnings
        assert plain.call_alternatives == {}
        assert list(plain._result) == list(alt._result)
        for gene in plain._result:
            a, b = list(plain._result[gene]), list(alt._result[gene])
            assert len(a) == len(b), (name, gene)
            for x, y in zip(a, b):
                assert x.n == y.n and list(x.allele_name) == list(y.allele_name)
                for f in ("value", "value_sum_indv", "allele_id", "fraction", "fraction_uniq"):
                    assert np.array_equal(getattr(x, f), getattr(y, f)), (name, gene, f)
        assert plain.getAllPossibleTyping() == alt.getAllPossibleTyping(), name      # the rows of .possible.tsv


def test_every_typed_gene_has_an_entry(tabulated, typed):
    data, sample = tabulated
    for name, (_, _, alt, _) in typed.items():
        want = {g for g, cn in sample.gene_cn.items() if cn and alt._result.get(g) and not alt._result[g][-1].isFail()}
        assert set(alt.call_alternatives) == want and len(want) >= 2, name


def test_full_entries_equal_the_oracle(small_case, typed, oracle_models):
    alt = typed["full"][2]
    for gene, entry in alt.call_alternatives.items():
        om, miss = oracle_models[gene]
        result = alt._result[gene][-1]
        assert entry.reads == om.readsNum(), gene
        assert miss.max() < 100                                     # the byte table holds these counts as they are
        cols = [om.allele_to_id[a.allele] for a in entry.alleles]
        assert cols == sorted(cols), gene
        want = checkEntry(entry, result, miss.T, cols, lambda a: om.id_to_allele[a], "all", gene)
        # a swap to another called allele gains nothing
        assert not want["gain"][cols].any(), gene
        print(f"{gene}: M {entry.mismatches}, " + ", ".join(
            f"{a.allele} -> {a.resolved} ({a.n_better} / {a.n_identical} / {a.n_balanced} / {a.n_near})" for a in entry.alleles))


def test_exonfirst_entries_equal_the_table_in_hbm(small_case, typed):
    sidx, gidx, sample = small_case
    alt = typed["exonfirst"][2]
    n_restricted = 0
    for gene, entry in alt.call_alternatives.items():
        result = alt._result[gene][-1]
        model = modelOf(result)
        alleles = gidx.tables[gidx.gene_id[gene]].alleles
        before = model.tableColumns
        row = np.asarray(result.allele_id, dtype=np.int64)[result.bestRank()]
        miss8, ldm, n_table_cols, cols = model.missFor(np.unique(row))
        table = miss8.download().reshape(n_table_cols, ldm)[:, :model.n_rows].astype(np.int64)
        ordinal = (lambda c: int(c)) if before is None else (lambda c: int(before[c]))
        checkEntry(entry, result, table, cols.tolist(), lambda c: alleles[ordinal(c)], "all" if before is None else "candidates",
                   gene)
        # the report (made while the sample was typed) and this look wrote no all-allele table
        after = model.tableColumns
        assert (after is None) == (before is None) and n_table_cols == (len(alleles) if after is None else len(after)), gene
        n_restricted += before is not None
    assert n_restricted >= 1                                        # scope == candidates is met
    print(f"exon-first: {n_restricted} of {len(alt.call_alternatives)} genes typed on a table of their candidates alone")


def test_per_gene_path_gives_the_same_entries(tabulated, typed):
    data, sample = tabulated
    for name, kw in STRATEGIES.items():
        whole = typed[name][2]
        per_gene = TypingWithPosNegAllele(data, variant_correction=True, call_alternatives=True, **kw)
        for gene, cn in sample.gene_cn.items():
            if cn:
                per_gene.typingPerGene(gene, int(cn))
        assert per_gene.call_alternatives.keys() == whole.call_alternatives.keys(), name
        for gene, a in whole.call_alternatives.items():
            b = per_gene.call_alternatives[gene]
            assert (a.cn, a.reads, a.mismatches, a.out_of_range) == (b.cn, b.reads, b.mismatches, b.out_of_range), (name, gene)
            if a.scope == b.scope:
                assert a == b, (name, gene)
                continue
            # the per-gene path of exon-first holds every allele's column, the whole-sample path the candidates: a subset
            assert (name, a.scope, b.scope) == ("exonfirst", "candidates", "all"), gene
            for x, y in zip(a.alleles, b.alleles):
                assert (x.allele, x.copies) == (y.allele, y.copies), (name, gene)
                assert x.n_better <= y.n_better and x.n_identical <= y.n_identical and x.n_balanced <= y.n_balanced and \
                    x.n_near <= y.n_near, (name, gene)
                assert len(y.resolved) <= len(x.resolved), (name, gene)
                if len(y.listed) < LISTED:                          # nothing cut off: every candidate's row is there as it is
                    assert all(row in y.listed for row in x.listed), (name, gene)
    # other settings: the counts follow `within`, the list follows `max_listed`
    alt = typed["full"][2]
    for gene, a in alt.call_alternatives.items():
        b = alternativesOfCall(alt._result[gene][-1], within=0, max_listed=1)
        for x, y in zip(a.alleles, b.alleles):
            assert (y.n_better, y.n_identical, y.n_balanced, y.n_near) == (x.n_better, x.n_identical, x.n_balanced, 0)
            assert y.listed == [r for r in x.listed if r.cls != "near"][:1] and y.resolved == x.resolved


def test_command_line_writes_the_alternatives_file(device, tmp_path, monkeypatch):
    """graphkir --allele-strategy exonfirst on a small BAM, without and with --call-alternatives (in-process, like
    tests/test_gpu_cn_cli.py): the typing files do not change, the new file holds the typer's numbers."""
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
    flags = ["--call-alternatives", "--call-alternatives-within", "2", "--call-alternatives-max", "3"]
    for k, extra in enumerate(([], flags)):
        run = tmp_path / f"run{k}"       # paths relative to the run's folder: the files name the sample's output
        run.mkdir()
        monkeypatch.chdir(run)
        cli.main(cli.createParser().parse_args(
            ["--step-skip-extraction", "--index-folder", "../index", "--output-folder", "out", "--allele-strategy", "exonfirst",
             "--cn-provided", "../s.cn.tsv", "--alignment", "../s.bam"] + extra))
        files.append({p.name: p for p in (run / "out").iterdir()})
    new = [n for n in files[1] if n.endswith(".alternatives.tsv")]
    assert len(new) == 1 and files[0].keys() | set(new) == files[1].keys()
    assert not any(n.endswith(".alternatives.tsv") for n in files[0])
    stem = new[0][:-len(".alternatives.tsv")]
    for n in (stem + ".tsv", stem + ".possible.tsv"):
        assert files[0][n].read_bytes() == files[1][n].read_bytes(), n
    assert len(typers) == 2 and typers[0].call_alternatives == {}
    typer = typers[1]
    typed_genes = [g for g, cn in s.gene_cn.items() if cn and typer._result.get(g) and not typer._result[g][-1].isFail()]
    assert list(typer.call_alternatives) == typed_genes and len(typed_genes) >= 2
    text = files[1][new[0]].read_text().split("\n")
    assert text[0].startswith("# scope candidates") and text[1].startswith("# delta") and text[-1] == ""
    assert text[2].split("\t") == CALL_ALTERNATIVES_COLUMNS
    rows = [line.split("\t") for line in text[3:-1]]
    assert all(len(r) == 20 for r in rows)
    want = []
    for gene in typed_genes:
        c = typer.call_alternatives[gene]
        assert len(c.alleles) == len(set(typer._result[gene][-1].selectBest()))
        for a in c.alleles:
            assert len(a.listed) <= 3 and all(x.delta <= 2 for x in a.listed)
            head = [gene, c.cn, c.reads, c.mismatches, c.out_of_range, c.scope, a.allele, a.copies, a.resolved, a.n_better,
                    a.n_identical, a.n_balanced, a.n_near]
            tails = [[x.allele, x.cls, x.delta, x.loss, x.gain, x.rows_for, x.rows_against] for x in a.listed] or [[""] * 7]
            want += [[str(v) for v in head + t] for t in tails]
    assert rows == want


# ------------------------------------------------------------------------------------------------ one planted case
def plantedCase():
    """One gene, four alleles, 60 error-free pairs of ONE of them (the truth), and two alleles added to the index after
    the reads were drawn: a TWIN that carries the truth's variants and one more at a position no mate covers, and a
    NEIGHBOUR that carries the truth's variants and one more at a position exactly one mate covers, well inside it.  The
    reads hold the backbone's base at both, so they do not change."""
    sidx = synth.makeIndex(seed=31, n_genes=1, len_range=(4200, 4600), var_range=(60, 60), allele_range=(4, 4), frac_del=0,
                           frac_ins=0)
    gene = sidx.genes[0]
    sample = synth.makeSample(sidx, seed=7, n_pairs=60, err_rate=0.0, gene_cn={gene: 1}, frac_multi=0, frac_improper=0,
                              frac_clip=0)
    truth = sample.truth[gene][0]
    length = len(sidx.backbone[gene])
    depth = np.zeros(length + 1, dtype=np.int64)
    for p, s in zip(sample.pos0, sample.span):
        depth[p:p + s] += 1
    taken = np.array(sorted({v.pos for v in sidx.variants}))

    def clear(p):
        return np.abs(taken - p).min() >= 3

    def inside_one_mate(p):
        over = [i for i, (q, s) in enumerate(zip(sample.pos0, sample.span)) if q <= p < q + s]
        return len(over) == 1 and p - sample.pos0[over[0]] >= 20 and sample.pos0[over[0]] + sample.span[over[0]] - p >= 20

    free = next(p for p in range(60, length - 60) if not depth[p - 5:p + 6].any() and clear(p))
    once = next(p for p in range(60, length - 60) if depth[p] == 1 and clear(p) and inside_one_mate(p) and abs(p - free) > 3)
    names = sidx.alleles[gene]
    twin = next(truth[:-2] + f"{d:02d}" for d in range(100) if truth[:-2] + f"{d:02d}" not in names)
    neighbour = gene.split("*")[0] + "*9990101"
    for v in sidx.variants:
        if truth in v.allele:
            v.allele = sorted(v.allele + [twin, neighbour])

    def other_base(p):
        return next(b for b in "ACGT" if ord(b) != int(sidx.backbone[gene][p]))

    sidx.variants.append(Variant(pos=int(free), typ="single", ref=gene, val=other_base(free), allele=[twin]))
    sidx.variants.append(Variant(pos=int(once), typ="single", ref=gene, val=other_base(once), allele=[neighbour]))
    sidx.variants.sort()
    for i, v in enumerate(sidx.variants):
        v.id = f"hv{i}"
        v.in_exon = any(s <= v.pos < e for s, e in sidx.exons[gene])
    sidx.alleles[gene] = sorted(names + [twin, neighbour])
    return sidx, sample, gene, truth, twin, neighbour


def test_planted_twin_and_neighbour(device):
    """Without variant correction (a variant with fewer than three observations would be dropped by it).  The search
    calls the truth or its twin -- they tie exactly -- and the report says so either way."""
    sidx, sample, gene, truth, twin, neighbour = plantedCase()
    gidx = GkIndex.fromVariants(sidx.variants, genes=sidx.genes, exons=sidx.exons)
    rec, table = packed.packSample(sample, gidx)
    tab = Tabulation(DeviceIndex(device, gidx), rec)
    data = SampleData(tab, gidx, tab.novelVariants(table.strings))
    typer = TypingWithPosNegAllele(data, variant_correction=False, call_alternatives=True, call_alternatives_within=1)
    calls, _ = typer.typing({gene: 1})
    assert calls in ([truth], [twin])
    entry = typer.call_alternatives[gene]
    assert entry.cn == 1 and entry.scope == "all" and entry.out_of_range == 0 and len(entry.alleles) == 1
    called = entry.alleles[0]
    other = twin if called.allele == truth else truth
    assert (called.allele, called.copies) == (calls[0], 1)
    assert (called.n_better, called.n_identical, called.n_balanced, called.n_near) == (0, 1, 0, 1)
    by_name = {x.allele: x for x in called.listed}
    assert list(by_name) == [other, neighbour]
    t = by_name[other]
    assert (t.cls, t.delta, t.loss, t.gain, t.rows_for, t.rows_against) == ("identical", 0, 0, 0, 0, 0)
    n = by_name[neighbour]
    assert (n.cls, n.delta, n.loss, n.gain, n.rows_for, n.rows_against) == ("near", 1, 1, 0, 1, 0)
    # the twin differs in the last two digits: exactly that field goes
    assert truth[:-2] == twin[:-2] and called.resolved == truth[:-2] and len(called.resolved) == len(called.allele) - 2
    tab.close()
