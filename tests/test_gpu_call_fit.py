"""GPU: the fit report of a likelihood call (gk_call_fit: callfit_profile; gk_call_fit_extra: callfit_extra) against the
numpy restatement of tests/callfit_reference.py, and through TypingWithPosNegAllele and the command line.  Everything is
an integer: every comparison is an equality.

Shapes follow the kernels of csrc/gk_callfit.hip: a lane takes 16 rows, a wave 1024, a workgroup C = 4096 rows per turn;
callfit_extra takes 16 columns per workgroup."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import callfit_reference as fr  # noqa: E402

from kir_graph_amd import _lib, packed, synth  # noqa: E402
from kir_graph_amd.call_bootstrap import homoFactor  # noqa: E402
from kir_graph_amd.call_report import modelOf  # noqa: E402
from kir_graph_amd.call_fit import CALL_FIT_COLUMNS, fitCall  # noqa: E402
from kir_graph_amd.engine import DeviceIndex, Tabulation  # noqa: E402
from kir_graph_amd.hisat2 import SampleData  # noqa: E402
from kir_graph_amd.kir_typing import TypingWithPosNegAllele  # noqa: E402
from oracle import tabulate as ot, typing as oty  # noqa: E402

pytestmark = pytest.mark.gpu

C = 4096                  # kFitChunk
SENTINEL = 0xA5A5A5A5A5A5A5A5
MIN_SENTINEL = 0xA5
KINDS = ("ties", "equal", "smallest", "out_of_range", "large")


def makeTable(rng, kind, n_rows, n_table_cols, cols, ldm, pad):
    """uint8 [n_table_cols][ldm]: the rows beyond n_rows of every column hold ``pad``."""
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
    elif kind == "large":                                                   # bins 15, 16 and 17 and their edges: the listed
        levels = np.array([0, 1, 14, 15, 16, 17, 99, 100, 254, 255])       # columns of a row start at the row's own level
        t = rng.choice(levels, (n_table_cols, n_rows))
        t[cols] = np.maximum(t[cols], rng.choice(levels, n_rows))
    full = np.full((n_table_cols, ldm), pad, dtype=np.uint8)
    full[:, :n_rows] = t
    return full


def callFit(dev, table, n_rows, cols, want_min=True):
    """gk_call_fit with every host output pre-filled: (hist, per_col [K, 3], M, d_min or None)."""
    n_table_cols, ldm = table.shape
    cols = np.ascontiguousarray(cols, dtype=np.int32)
    d_table = dev.put(table)
    hist = np.full(18 + 2, SENTINEL, dtype=np.uint64)
    per_col = np.full(3 * len(cols) + 2, SENTINEL, dtype=np.uint64)
    m = np.full(1 + 2, SENTINEL, dtype=np.uint64)
    d_min = dev.put(np.full(ldm + 16, MIN_SENTINEL, dtype=np.uint8)) if want_min else None
    try:
        _lib.check(_lib.lib().gk_call_fit(dev.ctx, d_table.ptr, ldm, n_rows, n_table_cols, cols.ctypes.data, len(cols),
                                          hist.ctypes.data, per_col.ctypes.data, m.ctypes.data, d_min.ptr if want_min else 0))
        mins = d_min.download() if want_min else None
    finally:
        d_table.free()
        if d_min is not None:
            d_min.free()
    assert (hist[18:] == SENTINEL).all() and (per_col[3 * len(cols):] == SENTINEL).all() and (m[1:] == SENTINEL).all()
    if want_min:
        assert (mins[n_rows:] == MIN_SENTINEL).all()                 # nothing at or beyond n_rows is written
        mins = mins[:n_rows].astype(np.int64)
    return hist[:18].astype(np.int64), per_col[:3 * len(cols)].reshape(-1, 3).astype(np.int64), int(m[0]), mins


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("k", [1, 2, 3, 8, 16])
@pytest.mark.parametrize("n_rows", [1, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1, 2 * C + 5])
def test_profile_equals_the_restatement(device, n_rows, k):
    rng = np.random.default_rng(1000 * n_rows + k)
    case = 0
    for n_table_cols in (k, k + 3, 40):
        cols = rng.permutation(n_table_cols)[:k]                      # scattered and unordered
        for more in (0, 64):
            ldm = (n_rows + 63) // 64 * 64 + more
            for pad in (7, 255):
                for kind in KINDS:
                    where = (n_table_cols, ldm, pad, kind)
                    table = makeTable(rng, kind, n_rows, n_table_cols, cols, ldm, pad)
                    case += 1
                    hist, per_col, m, d_min = callFit(device, table, n_rows, cols, want_min=case % 7 != 0)
                    want_hist, want_m, want_cols, want_min = fr.profile(table[:, :n_rows], cols)
                    assert np.array_equal(hist, want_hist) and m == want_m, where
                    assert np.array_equal(per_col, want_cols), where
                    assert hist.sum() == n_rows, where
                    if d_min is not None:
                        assert np.array_equal(d_min, want_min) and m == d_min.sum(), where
                    # the test's own data is what it is meant to be
                    if kind == "equal" and k > 1:
                        assert not per_col[:, 1:].any() and (per_col[:, 0] == n_rows).all(), where
                    if kind == "smallest" or k == 1:
                        assert per_col[k // 2].tolist()[:2] == [n_rows, n_rows], where
                    if k == 1:
                        assert per_col[0, 2] == 0, where
                    if kind == "out_of_range":
                        assert hist[17] >= 1 and (k == 1 or n_rows < 64 or hist[17] < n_rows), where
                    if kind == "large" and n_rows >= 255:
                        assert hist[16] >= 1 and hist[15] + hist[14] >= 1, where


@pytest.mark.parametrize("n_rows", [65, C + 1])
@pytest.mark.parametrize("n_table_cols", [1, 5, 64, 65, 577])
def test_extra_equals_the_restatement(device, n_table_cols, n_rows):
    rng = np.random.default_rng(77 * n_table_cols + n_rows)
    k = min(3, n_table_cols)
    cols = np.ascontiguousarray(rng.permutation(n_table_cols)[:k], dtype=np.int32)
    ldm = (n_rows + 63) // 64 * 64 + 64
    table = makeTable(rng, "large" if n_table_cols % 2 else "ties", n_rows, n_table_cols, cols, ldm, 255)
    d_table = device.put(table)
    d_min = device.put(np.full(ldm + 16, MIN_SENTINEL, dtype=np.uint8))
    hist, per_col, m = np.zeros(18, dtype=np.uint64), np.zeros(3 * k, dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    lib = _lib.lib()
    _lib.check(lib.gk_call_fit(device.ctx, d_table.ptr, ldm, n_rows, n_table_cols, cols.ctypes.data, k, hist.ctypes.data,
                               per_col.ctypes.data, m.ctypes.data, d_min.ptr))
    got = np.full(n_table_cols + 2, SENTINEL, dtype=np.uint64)
    _lib.check(lib.gk_call_fit_extra(device.ctx, d_table.ptr, ldm, n_rows, n_table_cols, d_min.ptr, got.ctypes.data))
    mins = d_min.download()
    d_table.free()
    d_min.free()
    assert (got[n_table_cols:] == SENTINEL).all() and (mins[n_rows:] == MIN_SENTINEL).all()
    got = got[:n_table_cols].astype(np.int64)
    _, want_m, _, m1 = fr.profile(table[:, :n_rows], cols)
    assert np.array_equal(mins[:n_rows], m1) and int(m[0]) == want_m
    assert np.array_equal(got, fr.extra(table[:, :n_rows], m1))
    assert (got[cols] == want_m).all()                                 # a called allele once more explains nothing new
    assert (got <= want_m).all()


def test_arguments_are_checked(device):
    n, ldm, a = 100, 128, 5
    d_table = device.put(np.zeros((a, ldm), dtype=np.uint8))
    d_min = device.put(np.zeros(ldm, dtype=np.uint8))
    hist, per_col, m = np.zeros(18, dtype=np.uint64), np.zeros(48, dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    with_a = np.zeros(a, dtype=np.uint64)
    lib, ctx = _lib.lib(), device.ctx
    h, p, mm, w = hist.ctypes.data, per_col.ctypes.data, m.ctypes.data, with_a.ctypes.data

    def cols(*c):
        arr = np.array(c, dtype=np.int32)
        return arr, arr.ctypes.data

    good, good_p = cols(0, 3)
    seventeen, seventeen_p = cols(*range(17))
    twice, twice_p = cols(1, 2, 1)
    outside, outside_p = cols(0, 5)
    negative, negative_p = cols(-1)
    t, dm = d_table.ptr, d_min.ptr
    bad = [
        lambda: lib.gk_call_fit(ctx, t, ldm, 0, a, good_p, 2, h, p, mm, dm),
        lambda: lib.gk_call_fit(ctx, t, 1 << 31, 1 << 31, a, good_p, 2, h, p, mm, dm),
        lambda: lib.gk_call_fit(ctx, t, 64, n, a, good_p, 2, h, p, mm, dm),              # ldm < n_rows
        lambda: lib.gk_call_fit(ctx, t, 120, n, a, good_p, 2, h, p, mm, dm),             # ldm % 64 != 0
        lambda: lib.gk_call_fit(ctx, t, ldm, n, a, good_p, 0, h, p, mm, dm),
        lambda: lib.gk_call_fit(ctx, t, ldm, n, 20, seventeen_p, 17, h, p, mm, dm),
        lambda: lib.gk_call_fit(ctx, t, ldm, n, a, twice_p, 3, h, p, mm, dm),
        lambda: lib.gk_call_fit(ctx, t, ldm, n, a, outside_p, 2, h, p, mm, dm),
        lambda: lib.gk_call_fit(ctx, t, ldm, n, a, negative_p, 1, h, p, mm, dm),
        lambda: lib.gk_call_fit(ctx, 0, ldm, n, a, good_p, 2, h, p, mm, dm),
        lambda: lib.gk_call_fit(ctx, t, ldm, n, a, None, 2, h, p, mm, dm),
        lambda: lib.gk_call_fit(ctx, t, ldm, n, a, good_p, 2, None, p, mm, dm),
        lambda: lib.gk_call_fit(ctx, t, ldm, n, a, good_p, 2, h, None, mm, dm),
        lambda: lib.gk_call_fit(ctx, t, ldm, n, a, good_p, 2, h, p, None, dm),
        lambda: lib.gk_call_fit_extra(ctx, t, ldm, 0, a, dm, w),
        lambda: lib.gk_call_fit_extra(ctx, t, 1 << 31, 1 << 31, a, dm, w),
        lambda: lib.gk_call_fit_extra(ctx, t, 64, n, a, dm, w),
        lambda: lib.gk_call_fit_extra(ctx, t, 120, n, a, dm, w),
        lambda: lib.gk_call_fit_extra(ctx, t, ldm, n, 0, dm, w),
        lambda: lib.gk_call_fit_extra(ctx, 0, ldm, n, a, dm, w),
        lambda: lib.gk_call_fit_extra(ctx, t, ldm, n, a, 0, w),
        lambda: lib.gk_call_fit_extra(ctx, t, ldm, n, a, dm, None),
    ]
    for k, call in enumerate(bad):
        assert call() == -3, k                                  # GK_ERR_ARG, and nothing was launched
        assert lib.gk_last_error(), k
    assert not hist.any() and not per_col.any() and not m.any() and not with_a.any()
    # the context still works: a table of zeros
    _lib.check(lib.gk_call_fit(ctx, t, ldm, n, a, good_p, 2, h, p, mm, dm))
    assert hist[0] == n and m[0] == 0 and per_col[:6].tolist() == [n, 0, 0, n, 0, 0]
    _lib.check(lib.gk_call_fit_extra(ctx, t, ldm, n, a, dm, w))
    assert not with_a.any()
    d_table.free()
    d_min.free()


# ------------------------------------------------------------------------------------------------ the drivers
STRATEGIES = {"full": {}, "exonfirst": {"exon_first": True}}
LOG999 = float(np.log10(.999))

# what the oracle gives for small_case, variant_correction=True, top_n=300 (gene prefix: cn, copies of the distinct called
# alleles in ascending ordinal, hist bins 0 and 1, M, best, unique, only_explains, the gains listed)
LITERALS = {
    "KIR2DL1S1": (3, [865, 577], [605, 317], [1438, 667], (1179, 3), 3, [1, 1, 1]),
    "KIR2DL2": (2, [566], [566], [None], (566, 0), 0, []),
    "KIR2DL3": (3, [231, 435], [229, 433], [1002, 1912], (653, 11), 11, [1, 1, 1]),
    "KIR2DL4": (3, [627, 646, 622], [376, 321, 352], [624, 516, 568], (1416, 6), 6, [2, 1, 1]),
}


@pytest.fixture(scope="module")
def tabulated(device, small_case):
    sidx, gidx, sample = small_case
    rec, table = packed.packSample(sample, gidx)
    tab = Tabulation(DeviceIndex(device, gidx), rec)
    return SampleData(tab, gidx, tab.novelVariants(table.strings)), sample


@pytest.fixture(scope="module")
def typed(tabulated):
    """Per strategy: the sample typed without and with the fit report (the whole-sample paths)."""
    data, sample = tabulated
    out = {}
    for name, kw in STRATEGIES.items():
        plain = TypingWithPosNegAllele(data, variant_correction=True, **kw)
        plain_calls = plain.typing(sample.gene_cn)
        fit = TypingWithPosNegAllele(data, variant_correction=True, call_fit=True, **kw)
        fit_calls = fit.typing(sample.gene_cn)
        out[name] = (plain, plain_calls, fit, fit_calls)
    return out


@pytest.fixture(scope="module")
def oracle_models(small_case):
    """gene -> (oracle model, mismatch table [reads, alleles], listed variants per read): computed once on the CPU."""
    sidx, gidx, sample = small_case
    ref = ot.tabulateLines(synth.toSamLines(sample), gidx.variants)
    out = {}
    for gname in gidx.genes:
        reads = [dict(r) for r in ref["reads"] if r["backbone"] == gname and r["multiple"] == 1]
        variants = [v for v in ref["variants"] if v.ref == gname]
        om = oty.GeneModel(reads, variants, top_n=300, variant_correction=True)
        miss, nvar = oty.missTable(om.reads, om.variants, om.allele_to_id)
        out[gname] = (om, miss, nvar)
    return out


def expectedExtras(gain, called, extra, name_of):
    order = sorted((a for a in range(len(gain)) if a not in set(called) and gain[a] > 0), key=lambda a: (-gain[a], a))
    return [(name_of(a), int(gain[a])) for a in order[:extra]]


def checkEntry(fit, result, table, cols, name_of, where):
    """One CallFit against the restatement on ``table`` [columns][reads], ``cols`` the called columns in ascending
    allele ordinal."""
    hist, m, per_col, m1 = fr.profile(table, cols)
    assert np.array_equal(fit.hist, hist) and fit.mismatches == m and fit.out_of_range == hist[17], where
    assert fit.reads == table.shape[1] == hist.sum() and fit.cn == result.n, where
    called = list(result.selectBest())
    assert sorted(a.allele for a in fit.alleles for _ in range(a.copies)) == sorted(called), where
    assert [a.allele for a in fit.alleles] == [name_of(c) for c in cols], where
    assert [a.best for a in fit.alleles] == per_col[:, 0].tolist(), where
    assert [a.unique for a in fit.alleles] == per_col[:, 1].tolist(), where
    assert [a.only_explains for a in fit.alleles] == (per_col[:, 2].tolist() if len(cols) > 1 else [None]), where
    gain = m - np.minimum(m1[:, None], table.T).sum(0)
    assert fit.extra == expectedExtras(gain, list(cols), 3, name_of), where
    return m


def test_point_result_does_not_change(typed):
    for name, (plain, plain_calls, fit, fit_calls) in typed.items():
        assert fit_calls == plain_calls, name                   # calls and warnings
        assert plain.call_fit == {}
        assert list(plain._result) == list(fit._result)
        for gene in plain._result:
            a, b = list(plain._result[gene]), list(fit._result[gene])
            assert len(a) == len(b), (name, gene)
            for x, y in zip(a, b):
                assert x.n == y.n and list(x.allele_name) == list(y.allele_name)
                for f in ("value", "value_sum_indv", "allele_id", "fraction", "fraction_uniq"):
                    assert np.array_equal(getattr(x, f), getattr(y, f)), (name, gene, f)


def test_every_typed_gene_has_an_entry(tabulated, typed):
    data, sample = tabulated
    for name, (_, _, fit, _) in typed.items():
        want = {g for g, cn in sample.gene_cn.items() if cn and fit._result.get(g) and not fit._result[g][-1].isFail()}
        assert set(fit.call_fit) == want and len(want) >= 2, name


def test_full_entries_equal_the_oracle(small_case, typed, oracle_models):
    sidx, gidx, sample = small_case
    fit = typed["full"][2]
    seen = set()
    for gene, entry in fit.call_fit.items():
        om, miss, nvar = oracle_models[gene]
        result = fit._result[gene][-1]
        assert entry.reads == om.readsNum() and entry.extra_scope == "all", gene
        assert miss.max() < 100                                     # the byte table holds these counts as they are
        names = [a.allele for a in entry.alleles]
        cols = [om.allele_to_id[a] for a in names]
        assert cols == sorted(cols), gene
        m = checkEntry(entry, result, miss.T, cols, lambda a: om.id_to_allele[a], gene)
        # value = c N - (3 + c) M, N = the listed variants of the reads
        n_obs = (float(result.value[result.bestRank()]) / homoFactor(result) + (3 + LOG999) * m) / LOG999
        print(f"value identity {gene}: N {n_obs!r}, oracle {int(nvar.sum())}, M {m}")
        assert round(n_obs) == int(nvar.sum()) and abs(n_obs - round(n_obs)) < 1e-3, gene
        key = next(k for k in LITERALS if gene.startswith(k + "*"))
        cn, best, unique, only, bins, lit_m, gains = LITERALS[key]
        seen.add(key)
        assert entry.cn == cn and sum(a.copies for a in entry.alleles) == cn, gene
        assert [a.best for a in entry.alleles] == best and [a.unique for a in entry.alleles] == unique, gene
        assert [a.only_explains for a in entry.alleles] == only, gene
        assert (int(entry.hist[0]), int(entry.hist[1])) == bins and entry.mismatches == lit_m, gene
        assert [g for _, g in entry.extra] == gains, gene
    assert seen == set(LITERALS)


def test_exonfirst_entries_equal_the_table_in_hbm(small_case, typed):
    sidx, gidx, sample = small_case
    fit = typed["exonfirst"][2]
    n_restricted = 0
    for gene, entry in fit.call_fit.items():
        result = fit._result[gene][-1]
        model = modelOf(result)
        alleles = gidx.tables[gidx.gene_id[gene]].alleles
        before = model.tableColumns
        row = np.asarray(result.allele_id, dtype=np.int64)[result.bestRank()]
        miss8, ldm, n_table_cols, cols = model.missFor(np.unique(row))
        table = miss8.download().reshape(n_table_cols, ldm)[:, :model.n_rows].astype(np.int64)
        ordinal = (lambda c: int(c)) if before is None else (lambda c: int(before[c]))
        checkEntry(entry, result, table, cols.tolist(), lambda c: alleles[ordinal(c)], gene)
        assert entry.extra_scope == ("all" if before is None else "candidates"), gene
        # the report (made while the sample was typed) and this look wrote no all-allele table
        after = model.tableColumns
        assert (after is None) == (before is None) and n_table_cols == (len(alleles) if after is None else len(after)), gene
        info = getattr(fit, "exon_info", {}).get(gene)
        if info is not None and "table_columns" in info:
            assert info["table_columns"] == n_table_cols, gene
        n_restricted += before is not None
    print(f"exon-first: {n_restricted} of {len(fit.call_fit)} genes typed on a table of their candidates alone")


def test_per_gene_path_gives_the_same_entries(tabulated, typed):
    data, sample = tabulated
    for name, kw in STRATEGIES.items():
        whole = typed[name][2]
        per_gene = TypingWithPosNegAllele(data, variant_correction=True, call_fit=True, **kw)
        for gene, cn in sample.gene_cn.items():
            if cn:
                per_gene.typingPerGene(gene, int(cn))
        assert per_gene.call_fit.keys() == whole.call_fit.keys(), name
        for gene, a in whole.call_fit.items():
            b = per_gene.call_fit[gene]
            assert np.array_equal(a.hist, b.hist) and (a.cn, a.reads, a.mismatches, a.out_of_range) == \
                (b.cn, b.reads, b.mismatches, b.out_of_range), (name, gene)
            assert a.alleles == b.alleles, (name, gene)
            if a.extra_scope == b.extra_scope:
                assert a.extra == b.extra, (name, gene)
            else:       # the per-gene path of exon-first holds every allele's column: its extras are looked for among
                # all alleles, the whole-sample path's among the candidates -- a subset, so no gain there is larger
                assert (name, a.extra_scope, b.extra_scope) == ("exonfirst", "candidates", "all"), gene
                assert max((g for _, g in a.extra), default=0) <= max((g for _, g in b.extra), default=0), (name, gene)
                assert all(pair in b.extra for pair in a.extra if pair[1] > min((g for _, g in b.extra), default=0)), gene
    # no extras asked for: the same report without them
    fit = typed["full"][2]
    for gene, a in fit.call_fit.items():
        b = fitCall(fit._result[gene][-1], extra=0)
        assert b.extra == [] and b.alleles == a.alleles and np.array_equal(a.hist, b.hist) and b.mismatches == a.mismatches


def test_command_line_writes_the_fit_file(device, tmp_path, monkeypatch):
    """graphkir --allele-strategy exonfirst on a small BAM, without and with --call-fit (in-process, like
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
    for k, extra in enumerate(([], ["--call-fit", "--call-fit-extra", "2"])):
        run = tmp_path / f"run{k}"       # paths relative to the run's folder: the files name the sample's output
        run.mkdir()
        monkeypatch.chdir(run)
        cli.main(cli.createParser().parse_args(
            ["--step-skip-extraction", "--index-folder", "../index", "--output-folder", "out", "--allele-strategy", "exonfirst",
             "--cn-provided", "../s.cn.tsv", "--alignment", "../s.bam"] + extra))
        files.append({p.name: p for p in (run / "out").iterdir()})
    fit_files = [n for n in files[1] if n.endswith(".fit.tsv")]
    assert len(fit_files) == 1 and files[0].keys() | set(fit_files) == files[1].keys()
    assert not any(n.endswith(".fit.tsv") for n in files[0])
    stem = fit_files[0][:-len(".fit.tsv")]
    for n in (stem + ".tsv", stem + ".possible.tsv"):
        assert files[0][n].read_bytes() == files[1][n].read_bytes(), n
    assert len(typers) == 2 and typers[0].call_fit == {}
    typer = typers[1]
    typed_genes = [g for g, cn in s.gene_cn.items() if cn and typer._result.get(g) and not typer._result[g][-1].isFail()]
    assert list(typer.call_fit) == typed_genes and len(typed_genes) >= 2
    text = files[1][fit_files[0]].read_text().split("\n")
    width = max(len(f.extra) for f in typer.call_fit.values())
    assert width <= 2
    assert text[0].split("\t") == CALL_FIT_COLUMNS + [c for i in range(width) for c in (f"extra_{i + 1}", f"gain_{i + 1}")]
    assert text[-1] == ""
    rows = [line.split("\t") for line in text[1:-1]]
    assert all(len(r) == 15 + 2 * width for r in rows)
    assert [r[0] for r in rows] == [g for g in typed_genes for _ in typer.call_fit[g].alleles]
    for gene in typed_genes:
        f, mine = typer.call_fit[gene], [r for r in rows if r[0] == gene]
        h = [int(x) for x in f.hist]
        assert len(mine) == len(f.alleles) == len(set(typer._result[gene][-1].selectBest()))
        for r, a in zip(mine, f.alleles):
            assert [int(x) for x in r[1:9]] == [f.cn, f.reads, h[0], h[1], h[2], sum(h[3:17]), f.out_of_range, f.mismatches]
            assert r[9] == a.allele and [int(x) for x in r[10:13]] == [a.copies, a.best, a.unique]
            assert r[13] == ("" if a.only_explains is None else str(a.only_explains)) and r[14] == f.extra_scope
            assert [x for x in r[15:] if x] == [str(x) for pair in f.extra for x in pair]
