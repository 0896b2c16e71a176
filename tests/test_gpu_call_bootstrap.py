"""GPU: the call bootstrap of the likelihood strategies (gk_boot_row_counts: callboot_draw; gk_weighted_sums: callboot_sums
+ callboot_fold) against the CPU restatement of tests/callboot_reference.py, and through TypingWithPosNegAllele and the
command line.

Shapes follow the kernels of csrc/gk_callboot.hip: 2^14 draws per workgroup and turn; 4096 rows per workgroup of the sums,
64 lanes, 256 threads, a register tile of 4 replicates x 8 sets.

Measured on an MI355X (profiles/r10_call_bootstrap.txt), largest deviation over every typed gene of both strategies and the
forced homozygous one, as a share of the bound asserted: unit weights against the search's value 0.0017 of
``2 n 2^-53 sum|V|``, replicates against the restatement 0.0052 of ``2 n 2^-53 W @ |V|``."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import callboot_reference as cr  # noqa: E402

from kir_graph_amd import _lib, packed, synth  # noqa: E402
from kir_graph_amd.call_bootstrap import (CALL_CONFIDENCE_COLUMNS, bootstrapCall, homoFactor,  # noqa: E402
                                          summariseCall)
from kir_graph_amd.call_report import modelOf  # noqa: E402
from kir_graph_amd.engine import DeviceIndex, Tabulation  # noqa: E402
from kir_graph_amd.hisat2 import SampleData  # noqa: E402
from kir_graph_amd.kir_typing import TypingWithPosNegAllele, _GeneView  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 2022
DRAW_CHUNK = 1 << 14      # kDrawChunk
SUM_CHUNK = 4096          # kSumChunk
POISON = 0xFFFFFFFF


def rowCounts(dev, n_rows, n_boot, boot_first, stream, buf=None, seed=SEED):
    """gk_boot_row_counts into a [n_boot][n_rows + 5] table whose every entry was 0xFFFFFFFF (or into ``buf``)."""
    ldw = n_rows + 5
    if buf is None:
        buf = dev.put(np.full((n_boot, ldw), POISON, dtype=np.uint32))
    _lib.check(_lib.lib().gk_boot_row_counts(dev.ctx, n_rows, n_boot, boot_first, seed, stream, buf.ptr, ldw))
    return buf


def weightedSums(dev, V, ld, n_rows, n_sets, W, ldw, n_boot):
    out = np.full((n_boot, n_sets), np.nan)
    _lib.check(_lib.lib().gk_weighted_sums(dev.ctx, V.ptr, ld, n_rows, n_sets, W.ptr, ldw, n_boot, out.ctypes.data))
    return out


# ------------------------------------------------------------------------------------------------ the replicate weights
@pytest.mark.parametrize("boot_first", [0, 3])
@pytest.mark.parametrize("n_boot", [1, 5])
@pytest.mark.parametrize("n_rows", [1, 2, 1000, DRAW_CHUNK - 1, DRAW_CHUNK, DRAW_CHUNK + 1, 70001])
def test_counts_are_exact(device, n_rows, n_boot, boot_first):
    buf = rowCounts(device, n_rows, n_boot, boot_first, stream=3)
    got = buf.download().reshape(n_boot, n_rows + 5)
    buf.free()
    assert (got[:, n_rows:] == POISON).all()                   # the padding is not touched
    want = cr.weights(SEED, 3, range(boot_first, boot_first + n_boot), n_rows)
    assert np.array_equal(got[:, :n_rows].astype(np.int64), want)
    assert (got[:, :n_rows].sum(axis=1, dtype=np.int64) == n_rows).all()


def test_counts_of_two_calls_equal_one_call(device):
    n_rows, ldw = 20001, 20006
    whole = rowCounts(device, n_rows, 5, 0, stream=1)
    want = whole.download().reshape(5, ldw)
    whole.free()
    parts = device.put(np.full((5, ldw), POISON, dtype=np.uint32))
    _lib.check(_lib.lib().gk_boot_row_counts(device.ctx, n_rows, 3, 0, SEED, 1, parts.ptr, ldw))
    _lib.check(_lib.lib().gk_boot_row_counts(device.ctx, n_rows, 2, 3, SEED, 1, parts.ptr + 3 * ldw * 4, ldw))
    got = parts.download().reshape(5, ldw)
    parts.free()
    assert np.array_equal(got, want)
    # a second call on the same table starts from zero again, and another stream or seed draws other reads
    again = rowCounts(device, n_rows, 5, 0, stream=1, buf=rowCounts(device, n_rows, 5, 0, stream=1))
    assert np.array_equal(again.download().reshape(5, ldw), want)
    again.free()
    for stream, seed in ((2, SEED), (1, SEED + 1)):
        other = rowCounts(device, n_rows, 5, 0, stream=stream, seed=seed)
        assert not np.array_equal(other.download().reshape(5, ldw), want)
        other.free()


# ------------------------------------------------------------------------------------------------ the weighted sums
SUM_CASES = ([(n, 9, 5) for n in (1, 63, 64, 65, 255, 256, 257, SUM_CHUNK - 1, SUM_CHUNK, SUM_CHUNK + 1, 2 * SUM_CHUNK + 3)]
             + [(SUM_CHUNK + 1, t, 5) for t in (1, 7, 8, 9, 33, 256)]
             + [(SUM_CHUNK + 1, 9, b) for b in (1, 3, 4, 5, 17)])


@pytest.mark.parametrize("case", range(len(SUM_CASES)))
def test_sums_are_exact_on_dyadic_data(device, case):
    """V in multiples of 2^-10 in (-1024, 0], small integer weights: every product and partial sum is exact in float64
    (at most 8195 rows x 2^20 x a few draws, plus one product of 2^31 - 1, stays far below 2^53 units of 2^-10), so any
    summation order gives the restatement's bits.  The padding of V is NaN and that of W 0xFFFFFFFF: reading either one
    breaks the equality."""
    n_rows, n_sets, n_boot = SUM_CASES[case]
    rng = np.random.default_rng(100 + case)
    ld, ldw = n_rows + 3, n_rows + 5
    V = np.full((n_sets, ld), np.nan)
    V[:, :n_rows] = -rng.integers(0, 1 << 20, (n_sets, n_rows)) / 1024.0
    if case % 2 == 0:                   # the weights the library draws
        Wd = rowCounts(device, n_rows, n_boot, 0, stream=case)
        W = Wd.download().reshape(n_boot, ldw)
        assert (W[:, n_rows:] == POISON).all()
    else:                               # hand-made: a count of 2^31 - 1 on a row whose V is -1.0, a replicate of zeros
        W = np.full((n_boot, ldw), POISON, dtype=np.uint32)
        W[:, :n_rows] = rng.integers(0, 4, (n_boot, n_rows))
        big = int(rng.integers(0, n_rows))
        V[:, big] = -1.0
        W[0, big] = (1 << 31) - 1
        if n_boot > 1:
            W[1, :n_rows] = 0
        Wd = device.put(W)
    Vd = device.put(V)
    got = weightedSums(device, Vd, ld, n_rows, n_sets, Wd, ldw, n_boot)
    Vd.free()
    Wd.free()
    want = cr.scores(W[:, :n_rows], V[:, :n_rows])
    assert np.isfinite(want).all() and np.array_equal(got, want)
    if case % 2 and n_boot > 1:
        assert not got[1].any()


def test_bits_repeat(device):
    """Real log10 values: the same call twice gives the same bits, and so does a pair (b, t) whichever n_sets / n_boot it
    is computed with (its sum has one order, fixed by n_rows)."""
    rng = np.random.default_rng(9)
    n_rows, ld, ldw = 2 * SUM_CHUNK + 3, 2 * SUM_CHUNK + 6, 2 * SUM_CHUNK + 8
    V = np.full((33, ld), np.nan)
    V[:, :n_rows] = np.log10(rng.random((33, n_rows)) * 0.999 + 1e-9)
    Vd = device.put(V)
    Wd = rowCounts(device, n_rows, 17, 0, stream=4)
    W = Wd.download().reshape(17, ldw)[:, :n_rows]
    wide = weightedSums(device, Vd, ld, n_rows, 33, Wd, ldw, 17)
    again = weightedSums(device, Vd, ld, n_rows, 33, Wd, ldw, 17)
    assert np.array_equal(wide, again)
    for n_sets, n_boot in ((9, 5), (33, 5), (9, 17), (1, 1), (8, 4)):
        part = weightedSums(device, Vd, ld, n_rows, n_sets, Wd, ldw, n_boot)
        assert np.array_equal(part, wide[:n_boot, :n_sets]), (n_sets, n_boot)
    Vd.free()
    Wd.free()
    want = cr.scores(W, V[:, :n_rows])
    bound = 2 * n_rows * 2.0 ** -53 * (W.astype(np.float64) @ np.abs(V[:, :n_rows]).T)
    assert (np.abs(wide - want) <= bound).all()


def test_arguments_are_checked(device):
    n = 100
    Vd, Wd = device.put(np.zeros((2, n))), device.put(np.zeros((2, n), dtype=np.uint32))
    out = np.zeros(4)
    lib, ctx, o = _lib.lib(), device.ctx, out.ctypes.data
    bad = [
        lambda: lib.gk_boot_row_counts(ctx, 0, 2, 0, SEED, 0, Wd.ptr, n),
        lambda: lib.gk_boot_row_counts(ctx, n, 0, 0, SEED, 0, Wd.ptr, n),
        lambda: lib.gk_boot_row_counts(ctx, n, 10001, 0, SEED, 0, Wd.ptr, n),
        lambda: lib.gk_boot_row_counts(ctx, n, 2, -1, SEED, 0, Wd.ptr, n),
        lambda: lib.gk_boot_row_counts(ctx, n, 2, 0, SEED, 0, Wd.ptr, n - 1),
        lambda: lib.gk_boot_row_counts(ctx, n, 2, 0, SEED, 0, 0, n),
        lambda: lib.gk_boot_row_counts(ctx, 1 << 31, 2, 0, SEED, 0, Wd.ptr, 1 << 31),
        lambda: lib.gk_weighted_sums(ctx, Vd.ptr, n, 0, 2, Wd.ptr, n, 2, o),
        lambda: lib.gk_weighted_sums(ctx, Vd.ptr, n, n, 0, Wd.ptr, n, 2, o),
        lambda: lib.gk_weighted_sums(ctx, Vd.ptr, n, n, 257, Wd.ptr, n, 2, o),
        lambda: lib.gk_weighted_sums(ctx, Vd.ptr, n, n, 2, Wd.ptr, n, 0, o),
        lambda: lib.gk_weighted_sums(ctx, Vd.ptr, n, n, 2, Wd.ptr, n, 10001, o),
        lambda: lib.gk_weighted_sums(ctx, Vd.ptr, n, n, 2, Wd.ptr, n - 1, 2, o),
        lambda: lib.gk_weighted_sums(ctx, Vd.ptr, n - 1, n, 2, Wd.ptr, n, 2, o),
        lambda: lib.gk_weighted_sums(ctx, 0, n, n, 2, Wd.ptr, n, 2, o),
        lambda: lib.gk_weighted_sums(ctx, Vd.ptr, n, n, 2, 0, n, 2, o),
        lambda: lib.gk_weighted_sums(ctx, Vd.ptr, n, n, 2, Wd.ptr, n, 2, None),
    ]
    for k, call in enumerate(bad):
        assert call() == -3, k                                  # GK_ERR_ARG, and nothing was launched
        assert lib.gk_last_error(), k
    assert not out.any()
    # the context still works
    _lib.check(lib.gk_boot_row_counts(ctx, n, 2, 0, SEED, 0, Wd.ptr, n))
    assert (Wd.download().reshape(2, n).sum(axis=1) == n).all()
    Vd.free()
    Wd.free()


# ------------------------------------------------------------------------------------------------ the drivers
N_BOOT = 8
STRATEGIES = {"full": {}, "exonfirst": {"exon_first": True}}


@pytest.fixture(scope="module")
def tabulated(device, small_case):
    sidx, gidx, sample = small_case
    rec, table = packed.packSample(sample, gidx)
    tab = Tabulation(DeviceIndex(device, gidx), rec)
    return SampleData(tab, gidx, tab.novelVariants(table.strings)), sample


@pytest.fixture(scope="module")
def typed(tabulated):
    """Per strategy: the sample typed without and with 8 replicates (the whole-sample paths)."""
    data, sample = tabulated
    out = {}
    for name, kw in STRATEGIES.items():
        plain = TypingWithPosNegAllele(data, variant_correction=True, **kw)
        plain_calls = plain.typing(sample.gene_cn)
        boot = TypingWithPosNegAllele(data, variant_correction=True, call_bootstrap=N_BOOT, **kw)
        boot_calls = boot.typing(sample.gene_cn)
        out[name] = (plain, plain_calls, boot, boot_calls)
    return out


@pytest.fixture(scope="module")
def log_probs(tabulated):
    """gene -> (backbone ordinal, log10 table [reads, alleles]) of a model of the gene made for this purpose alone:
    the reference the replicates are restated from (``AlleleTyping.log_probs``)."""
    data, sample = tabulated
    typer = TypingWithPosNegAllele(data, variant_correction=True)
    tab, logs = typer._context()
    prep = tab.prepared(tab.dev, False)
    out = {}
    for gene, cn in sample.gene_cn.items():
        view = _GeneView(data, gene, False, tab=tab)
        if cn and view.g is not None and view.alleles:
            out[gene] = (view.g, view.model(logs, view.prepared(prep), top_n=300, variant_correction=True).log_probs)
    return out


@pytest.fixture(scope="module")
def forced_homo(tabulated):
    """One gene typed with cn = 2 as homozygous whatever its reads say: (gene, result, its bootstrap)."""
    data, sample = tabulated
    typer = TypingWithPosNegAllele(data, variant_correction=True)
    tab, logs = typer._context()
    gene = next(g for g, cn in sample.gene_cn.items() if cn)
    view = _GeneView(data, gene, False, tab=tab)
    typ = view.model(logs, view.prepared(tab.prepared(tab.dev, False)), force_homo=True, top_n=300, variant_correction=True,
                     _defer_log=True)
    res = typ.typing(2)
    assert res.n == 2 and homoFactor(res) == 2 and (res.allele_id[:, 0] == res.allele_id[:, 1]).all()
    return gene, res, bootstrapCall(res, homoFactor(res), N_BOOT, SEED, view.g, 32)


def everyCall(typed, forced_homo):
    """(label, last result, its CallBootstrap) of every typed gene of both strategies and of the forced homozygous one."""
    for name, (_, _, boot, _) in typed.items():
        for gene, cb in boot.call_bootstrap.items():
            yield f"{name}:{gene}", gene, boot._result[gene][-1], cb
    gene, res, cb = forced_homo
    yield f"homo:{gene}", gene, res, cb


def test_every_typed_gene_has_an_entry(tabulated, typed):
    data, sample = tabulated
    for name, (plain, _, boot, _) in typed.items():
        assert plain.call_bootstrap == {}
        want = {g for g, cn in sample.gene_cn.items() if cn and boot._result.get(g) and not boot._result[g][-1].isFail()}
        assert set(boot.call_bootstrap) == want and len(want) >= 2, name
        for gene, cb in boot.call_bootstrap.items():
            res = boot._result[gene][-1]
            assert cb.scores.shape == (N_BOOT, len(cb.rows)) and 1 <= len(cb.rows) <= 33
            assert cb.rows[cb.called] == res.bestRank() and cb.cn == res.n == int(sample.gene_cn[gene])
            assert cb.alleles[cb.called] == res.selectBest()
            assert np.array_equal(cb.value, res.value[cb.rows])
            ids = np.sort(np.asarray(res.allele_id)[cb.rows], axis=1)
            assert len(np.unique(ids, axis=0)) == len(ids)       # no multiset twice


def test_point_result_does_not_change(typed):
    for name, (plain, plain_calls, boot, boot_calls) in typed.items():
        assert boot_calls == plain_calls, name                   # calls and warnings
        assert list(plain._result) == list(boot._result)
        for gene in plain._result:
            a, b = list(plain._result[gene]), list(boot._result[gene])
            assert len(a) == len(b), (name, gene)
            for x, y in zip(a, b):
                assert x.n == y.n and list(x.allele_name) == list(y.allele_name)
                for field in ("value", "value_sum_indv", "allele_id", "fraction", "fraction_uniq"):
                    assert np.array_equal(getattr(x, field), getattr(y, field)), (name, gene, field)


def test_unit_weights_give_the_point_value(device, typed, forced_homo):
    """gk_weighted_sums on weights of one, on the table and columns ``DeviceModel.tableFor`` hands out, is the search's own
    ``value`` (divided by cn for a homozygous-model result) within the first-order bound of any summation order."""
    worst = 0.0
    for label, gene, res, cb in everyCall(typed, forced_homo):
        model = modelOf(res)
        n = model.n_rows
        table, ld, cols = model.tableFor(np.asarray(res.allele_id)[cb.rows])
        dev = model.dev
        Vd = dev.alloc((len(cols), n), np.float64)
        _lib.check(_lib.lib().gk_setmax(dev.ctx, table.ptr, n, ld, cols.ctypes.data, len(cols), cols.shape[1], Vd.ptr))
        Wd = dev.put(np.ones((1, n), dtype=np.uint32))
        got = weightedSums(dev, Vd, n, n, len(cols), Wd, n, 1)[0]
        V = Vd.download().reshape(len(cols), n)
        Vd.free()
        Wd.free()
        want = res.value[cb.rows] / homoFactor(res)
        bound = 2 * n * 2.0 ** -53 * np.abs(V).sum(axis=1)
        share = np.abs(got - want) / bound
        print(f"unit weights {label}: n_rows {n}, sets {len(cols)}, worst share of the bound {share.max():.3g}")
        worst = max(worst, float(share.max()))
        assert (np.abs(got - want) <= bound).all(), label
    print(f"unit weights: worst share of the bound {worst:.3g}")


def test_every_replicate_equals_the_restatement(typed, forced_homo, log_probs):
    worst = 0.0
    for label, gene, res, cb in everyCall(typed, forced_homo):
        g, L = log_probs[gene]
        f = homoFactor(res)
        n = L.shape[0]
        assert n == modelOf(res).n_rows
        V = np.array([L[:, row].max(axis=1) for row in np.asarray(res.allele_id)[cb.rows]])
        W = cr.weights(SEED, g, range(N_BOOT), n)
        want = f * cr.scores(W, V)
        bound = f * 2 * n * 2.0 ** -53 * (W.astype(np.float64) @ np.abs(V).T)
        share = np.abs(cb.scores - want) / bound
        print(f"replicates {label}: n_rows {n}, sets {len(V)}, worst share of the bound {share.max():.3g}")
        worst = max(worst, float(share.max()))
        assert (np.abs(cb.scores - want) <= bound).all(), label
        support, mean, lo, hi = summariseCall(cb.scores, cb.called)
        assert np.array_equal(cb.support, support) and np.array_equal(cb.delta_mean, mean)
        assert np.array_equal(cb.delta_lo, lo) and np.array_equal(cb.delta_hi, hi)
        assert cb.call_support == support[cb.called] and support.sum() == pytest.approx(1.0, abs=1e-12)
    print(f"replicates: worst share of the bound {worst:.3g}")


def test_per_gene_path_gives_the_same_bootstrap(tabulated, typed):
    data, sample = tabulated
    for name, kw in STRATEGIES.items():
        boot = typed[name][2]
        per_gene = TypingWithPosNegAllele(data, variant_correction=True, call_bootstrap=N_BOOT, **kw)
        for gene, cn in sample.gene_cn.items():
            if cn:
                per_gene.typingPerGene(gene, int(cn))
        assert per_gene.call_bootstrap.keys() == boot.call_bootstrap.keys(), name
        for gene, cb in boot.call_bootstrap.items():
            other = per_gene.call_bootstrap[gene]
            assert np.array_equal(other.rows, cb.rows) and other.called == cb.called and other.alleles == cb.alleles
            assert np.array_equal(other.scores, cb.scores), (name, gene)          # bit for bit
            assert np.array_equal(other.value, cb.value)
    # replicate b does not depend on how many there are or how many sets are kept; another seed draws other reads
    boot = typed["full"][2]
    fewer = TypingWithPosNegAllele(data, variant_correction=True, call_bootstrap=3, call_bootstrap_top=4)
    fewer.typing(sample.gene_cn)
    reseeded = TypingWithPosNegAllele(data, variant_correction=True, call_bootstrap=N_BOOT, call_bootstrap_seed=7)
    reseeded.typing(sample.gene_cn)
    for gene, cb in boot.call_bootstrap.items():
        few = fewer.call_bootstrap[gene]
        at = [int(np.flatnonzero(cb.rows == r)[0]) for r in few.rows]
        assert np.array_equal(few.scores, cb.scores[:3][:, at]), gene
    assert any(not np.array_equal(reseeded.call_bootstrap[g].scores, boot.call_bootstrap[g].scores) for g in boot.call_bootstrap)


def test_command_line_writes_the_call_confidence_file(device, tmp_path, monkeypatch):
    """graphkir --allele-strategy exonfirst on a small BAM, without and with --call-bootstrap 8 (in-process, like
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
    for k, extra in enumerate(([], ["--call-bootstrap", "8", "--call-bootstrap-top", "5"])):
        run = tmp_path / f"run{k}"       # paths relative to the run's folder: the files name the sample's output
        run.mkdir()
        monkeypatch.chdir(run)
        cli.main(cli.createParser().parse_args(
            ["--step-skip-extraction", "--index-folder", "../index", "--output-folder", "out", "--allele-strategy", "exonfirst",
             "--cn-provided", "../s.cn.tsv", "--alignment", "../s.bam"] + extra))
        files.append({p.name: p for p in (run / "out").iterdir()})
    conf = [n for n in files[1] if n.endswith(".call_confidence.tsv")]
    assert len(conf) == 1 and files[0].keys() | set(conf) == files[1].keys()
    assert not any(n.endswith(".call_confidence.tsv") for n in files[0])
    stem = conf[0][:-len(".call_confidence.tsv")]
    for n in (stem + ".tsv", stem + ".possible.tsv"):
        assert files[0][n].read_bytes() == files[1][n].read_bytes(), n
    assert len(typers) == 2 and typers[0].call_bootstrap == {}
    typer = typers[1]
    typed_genes = [g for g, cn in s.gene_cn.items() if cn and typer._result.get(g) and not typer._result[g][-1].isFail()]
    assert list(typer.call_bootstrap) == typed_genes and len(typed_genes) >= 2
    text = files[1][conf[0]].read_text().split("\n")
    width = max(int(s.gene_cn[g]) for g in typed_genes)
    assert text[0].split("\t") == CALL_CONFIDENCE_COLUMNS + [str(i + 1) for i in range(width)] and text[-1] == ""
    assert CALL_CONFIDENCE_COLUMNS == ["gene", "cn", "rank", "called", "value", "support", "delta_mean", "delta_q025", "delta_q975"]
    rows = [line.split("\t") for line in text[1:-1]]
    assert all(len(r) == 9 + width for r in rows)
    for gene in typed_genes:
        cb, mine = typer.call_bootstrap[gene], [r for r in rows if r[0] == gene]
        assert len(mine) == len(cb.rows) <= 6 and [r[3] for r in mine].count("1") == 1
        assert [int(r[2]) for r in mine] == cb.rows.tolist() and mine[cb.called][3] == "1"
        assert all(r[1] == str(int(s.gene_cn[gene])) for r in mine)
        for k, field in enumerate(("value", "support", "delta_mean", "delta_lo", "delta_hi")):
            assert [float(r[4 + k]) for r in mine] == getattr(cb, field).tolist(), (gene, field)
        assert [[a for a in r[9:] if a] for r in mine] == cb.alleles
    assert {r[0] for r in rows} == set(typed_genes)
