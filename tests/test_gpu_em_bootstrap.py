"""GPU: the read bootstrap of the EM strategy (gk_em_bootstrap: boot_resample + boot_em_batch) against the CPU
restatement of tests/boot_reference.py and the EM oracle, and through TypingWithReport and the command line."""
import ctypes as C
import os
import sys
from collections import Counter

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import boot_reference as br  # noqa: E402

from kir_graph_amd import _lib, packed, synth  # noqa: E402
from kir_graph_amd.engine import DeviceIndex, Tabulation  # noqa: E402
from kir_graph_amd.hisat2 import SampleData  # noqa: E402
from kir_graph_amd.kir_typing import TypingWithReport, _GeneView, selectKirTypingModel  # noqa: E402
from kir_graph_amd.typing_em import bootstrapEM, callsByAbundance, candidateSetsDistinct  # noqa: E402
from oracle import em as oem  # noqa: E402

pytestmark = pytest.mark.gpu

LDS_HIST_SETS = 8192      # kBootLdsSets of gk_boot.hip: prefix sums + histogram of a gene in LDS up to this many sets
LDS_SCALE_SETS = 4096     # kBootScaleLds of gk_boot.hip: the scale row of a replicate in LDS up to this many sets
SEED = 2022


def randomSets(rng, n_sets: int, words: int, n_allele: int, empty_first: bool = False, density: float = 0.3) -> np.ndarray:
    """``n_sets`` distinct non-empty bit sets over ``n_allele`` alleles, ascending (word 0 first, like
    ``candidateSetsDistinct``); ``empty_first``: the first of them is the empty set instead."""
    rows = np.zeros((0, words), dtype=np.uint32)
    while len(rows) < n_sets:
        bits = np.zeros((2 * n_sets + 8, words * 32), dtype=np.uint8)
        bits[:, :n_allele] = rng.random((len(bits), n_allele)) < density
        new = np.packbits(bits, axis=1, bitorder="little").view(np.uint32)
        rows = np.unique(np.concatenate([rows, new[new.any(axis=1)]]), axis=0)
    rows = rows[np.sort(rng.choice(len(rows), size=n_sets, replace=False))]
    if empty_first:
        rows[0] = 0
    order = np.lexsort(rows.T[::-1])
    return np.ascontiguousarray(rows[order])


def mixedCounts(rng, n_sets: int, big_every: int = 4) -> np.ndarray:
    """Multiplicities that mix 1 and 100 000 (a big one every ``big_every`` sets) and a few sets without reads."""
    count = np.ones(n_sets, dtype=np.int64)
    count[rng.integers(0, big_every)::big_every] = 100_000
    if n_sets > 4:
        count[rng.choice(n_sets, size=max(1, n_sets // 8), replace=False)] = 0
    if not count.any():
        count[0] = 1
    return count


def wantCounts(jobs, n_boot: int, seed: int = SEED) -> np.ndarray:
    return np.array([np.concatenate([br.replicateCounts(seed, g, b, count) for _, count, _, g in jobs]) for b in range(n_boot)],
                    dtype=np.int64).reshape(n_boot, -1)


# (words, n_allele, n_sets, replicates, empty first row, a big count every ... sets)
# The 33 alleles of the issue's list need two words (n_allele <= words * 32 is a requirement of the call): one word is
# run with 32 alleles, and one word with 33 is checked to be refused below.
WEIGHT_CASES = [
    (1, 32, 1, 1, False, 1),
    (1, 32, 17, 3, True, 4),
    (2, 33, 17, 3, False, 4),
    (5, 150, 17, 3, True, 4),
    (16, 512, 17, 1, False, 4),
    (1, 32, LDS_HIST_SETS - 1, 1, True, 1000),
    (1, 32, LDS_HIST_SETS, 3, False, 1000),
    (16, 512, LDS_HIST_SETS + 1, 3, True, 1000),
    (5, 150, 3 * LDS_HIST_SETS + 5, 1, False, 3000),
]


@pytest.mark.parametrize("words,n_allele,n_sets,n_boot,empty_first,big_every", WEIGHT_CASES)
def test_replicate_weights_are_exact(device, words, n_allele, n_sets, n_boot, empty_first, big_every):
    rng = np.random.default_rng(n_sets * 31 + words)
    sets = randomSets(rng, n_sets, words, n_allele, empty_first)
    count = mixedCounts(rng, n_sets, big_every) if n_sets > 1 else np.array([1])
    jobs = [(sets, count, n_allele, 3)]
    prob, iters, got = bootstrapEM(device, jobs, n_boot, SEED, want_counts=True)
    assert got.dtype == np.uint32 and got.shape == (n_boot, n_sets)
    assert np.array_equal(got.astype(np.int64), wantCounts(jobs, n_boot))
    assert (got.sum(axis=1) == count.sum()).all() and not got[:, count == 0].any()
    assert np.isfinite(prob).all() and prob.shape == (n_boot, n_allele)
    named = prob.sum(axis=1) > 0
    assert np.allclose(prob[named].sum(axis=1), 1.0, rtol=0, atol=1e-9)
    if not empty_first:
        assert named.all()


def test_two_jobs_of_different_width_in_one_call(device):
    rng = np.random.default_rng(5)
    jobs = [(randomSets(rng, 17, 1, 20), mixedCounts(rng, 17), 20, 4),
            (randomSets(rng, LDS_HIST_SETS + 3, 5, 150, empty_first=True), mixedCounts(rng, LDS_HIST_SETS + 3, 1000), 150, 9),
            (np.zeros((0, 2), dtype=np.uint32), np.zeros(0, dtype=np.int64), 40, 1)]      # a job without sets: zeros
    prob, iters, got = bootstrapEM(device, jobs, 3, SEED, want_counts=True)
    assert np.array_equal(got.astype(np.int64), wantCounts(jobs, 3))
    assert prob.shape == (3, 210) and iters.shape == (3, 3)
    assert not prob[:, 170:].any() and not iters[:, 2].any()
    assert np.allclose(prob[:, :20].sum(axis=1), 1.0, atol=1e-9) and np.allclose(prob[:, 20:170].sum(axis=1), 1.0, atol=1e-9)


def test_arguments_are_checked(device):
    rng = np.random.default_rng(6)
    sets, count = randomSets(rng, 5, 1, 20), np.arange(1, 6)
    prob, iters = bootstrapEM(device, [], 2, SEED)                         # no jobs: nothing to do
    assert prob.shape == (2, 0) and iters.shape == (2, 0)
    for bad in (0, 10001):
        with pytest.raises(_lib.GkError):
            bootstrapEM(device, [(sets, count, 20, 0)], bad, SEED)
    with pytest.raises(_lib.GkError):
        bootstrapEM(device, [(sets, count, 33, 0)], 2, SEED)               # 33 alleles do not fit one word
    with pytest.raises(_lib.GkError):
        bootstrapEM(device, [(np.zeros((5, 17), dtype=np.uint32), count, 20, 0)], 2, SEED)      # more than 16 words
    with pytest.raises(ValueError):
        bootstrapEM(device, [(sets, np.full(5, 1 << 29), 20, 0)], 2, SEED)      # 2^31 reads or more
    many = np.full(5, 1 << 29, dtype=np.uint32)
    job = _lib.BootJob(sets=sets.ctypes.data, count=many.ctypes.data, n_sets=5, words=1, n_allele=20, stream=0)
    out_p, out_i = np.zeros(40), np.zeros(2, dtype=np.int32)
    assert _lib.lib().gk_em_bootstrap(device.ctx, C.byref(job), 1, 2, SEED, 300, 1e-4, out_p.ctypes.data, out_i.ctypes.data, None) == -3
    # the context still works
    prob, iters = bootstrapEM(device, [(sets, count, 20, 0)], 2, SEED)
    assert np.allclose(prob.sum(axis=1), 1.0, atol=1e-9)


def test_replicates_depend_on_seed_stream_and_number_only(device):
    rng = np.random.default_rng(7)
    a = (randomSets(rng, 300, 2, 40, empty_first=True), rng.integers(1, 50, 300), 40, 6)
    b = (randomSets(rng, LDS_SCALE_SETS + 9, 1, 24), rng.integers(1, 3, LDS_SCALE_SETS + 9), 24, 2)
    five = bootstrapEM(device, [a, b], 5, SEED, want_counts=True)
    three = bootstrapEM(device, [a, b], 3, SEED, want_counts=True)
    again = bootstrapEM(device, [a, b], 5, SEED, want_counts=True)
    for x, y, z in zip(five, three, again):
        assert np.array_equal(x[:3], y) and np.array_equal(x, z)        # bit for bit
    other = bootstrapEM(device, [a, b], 5, SEED + 1, want_counts=True)
    assert not np.array_equal(other[2], five[2])
    # job b alone, and behind another job: its replicates stay (its stream number is its own)
    alone = bootstrapEM(device, [b], 5, SEED, want_counts=True)
    behind = bootstrapEM(device, [(a[0], a[1], a[2], 11), b], 5, SEED, want_counts=True)
    for x in (five, behind):
        assert np.array_equal(x[0][:, 40:], alone[0]) and np.array_equal(x[1][:, 1], alone[1][:, 0])
        assert np.array_equal(x[2][:, 300:], alone[2])
    assert not np.array_equal(behind[2][:, :300], five[2][:, :300])      # job a on another stream: other draws


@pytest.fixture(scope="module")
def tabulated(device, small_case):
    sidx, gidx, sample = small_case
    rec, table = packed.packSample(sample, gidx)
    tab = Tabulation(DeviceIndex(device, gidx), rec)
    return SampleData(tab, gidx, tab.novelVariants(table.strings)), sample


@pytest.fixture(scope="module")
def typed(tabulated):
    """The sample typed without and with 8 replicates (whole-sample path)."""
    data, sample = tabulated
    plain = TypingWithReport(data)
    plain_calls = plain.typing(sample.gene_cn)
    boot = TypingWithReport(data, bootstrap=8)
    boot_calls = boot.typing(sample.gene_cn)
    return plain, plain_calls, boot, boot_calls


def sameAsOracle(sets, count, alleles, stream, prob, iters, seed=SEED):
    """Every replicate (rows of ``prob`` over ``alleles``) against oracle.em.squaremEM on the replicate's reads:
    abundances at the project's EM tolerance (BASELINE.json north_star), never-named alleles exactly 0, same steps."""
    for b in range(len(prob)):
        weights = br.replicateCounts(seed, stream, b, count)
        want, want_iters = oem.squaremEM(br.replicateReads(sets, weights, alleles))
        for a, name in enumerate(alleles):
            if name in want:
                assert prob[b, a] == pytest.approx(want[name], rel=1e-5, abs=1e-9), (b, name)
            else:
                assert prob[b, a] == 0.0, (b, name)
        # The oracle's count is its Python loop variable, iter_max - 1 for a run that uses up iter_max; the solver says
        # iter_max then (csrc/gk_squarem.h).  The equality holds for runs that stop, which all of these do.
        assert int(iters[b]) == want_iters, b


def test_solver_equals_the_oracle_on_every_replicate(tabulated, typed):
    data, sample = tabulated
    _, _, boot, _ = typed
    assert set(boot.bootstrap) == {g for g, cn in sample.gene_cn.items() if cn and boot._result.get(g)}
    for gene, res in boot.bootstrap.items():
        view = _GeneView(data, gene, multiple=False)
        t = data.index.tables[view.g]
        sets, count = candidateSetsDistinct(data.tab, view.rows, view.n_rows, view.vbeg, view.vbeg + view.n_span, view.mask, t.words)
        assert res.prob.shape == (8, len(res.alleles)) and res.iterations.shape == (8,)
        # the replicate's abundances of the point report's alleles; no other allele of the gene is named by any read
        col = {a: i for i, a in enumerate(view.alleles)}
        full = np.zeros((8, len(view.alleles)))
        full[:, [col[a] for a in res.alleles]] = res.prob
        sameAsOracle(sets, count, view.alleles, view.g, full, res.iterations)


def test_solver_equals_the_oracle_beyond_the_scale_row_in_lds(device):
    """A gene of more sets than a replicate's scale row holds in LDS (the row then lives in HBM), two replicates.  The
    reads favour two alleles, so the abundances are well determined."""
    rng = np.random.default_rng(11)
    n_sets, n_allele = LDS_SCALE_SETS + 150, 24
    alleles = [f"G*{a:03d}" for a in range(n_allele)]
    bits = (rng.random((3 * n_sets, n_allele)) < 0.15).astype(np.uint8)
    truth = rng.random(len(bits)) < 0.6
    bits[truth, 3] = 1
    bits[~truth, 7] = 1
    wide = np.zeros((len(bits), 32), dtype=np.uint8)
    wide[:, :n_allele] = bits
    rows = np.unique(np.packbits(wide, axis=1, bitorder="little").view(np.uint32), axis=0)
    assert len(rows) >= n_sets
    sets = np.ascontiguousarray(rows[:n_sets])
    count = rng.integers(1, 3, n_sets)
    prob, iters = bootstrapEM(device, [(sets, count, n_allele, 5)], 2, SEED)
    sameAsOracle(sets, count, alleles, 5, prob, iters[:, 0])


# (words, n_allele, n_sets, empty first row, a big count every ... sets): the widths of the bit sets, and the numbers of
# sets either side of the batch kernel's scale row leaving LDS (the point kernel keeps its own there) and past the point
# kernel's limit of 8192 (both keep it in HBM).  Every case has sets of 100 000 reads: no replicate is empty.
# Then the edges of the rounds: a workgroup of 512 threads takes 32 sets or alleles per round, one of 1024 takes 64 -- 31,
# 32, 33 and 65 sets, 65 and 129 alleles.  The sets of the 512-allele case have some 150 members each (density 0.3):
# more than one stride of the 16 lanes.  tests/test_gpu_squarem_edges.py ties the point solver to a plain reference;
# with this test, so is the batch solver.
SAME_SOLVER_CASES = [
    (1, 20, 17, False, 4),
    (2, 33, 17, True, 4),
    (16, 512, 17, False, 4),
    (1, 24, LDS_SCALE_SETS, False, 1000),
    (1, 24, LDS_SCALE_SETS + 1, False, 1000),
    (1, 24, 8193, False, 1000),
    (2, 33, 31, False, 4),
    (2, 33, 32, False, 4),
    (2, 33, 33, True, 4),
    (2, 33, 65, False, 4),
    (3, 65, 40, False, 4),
    (5, 129, 40, True, 4),
]


def batchIsPoint(device, words, n_allele, n_sets, empty_first, big_every, iter_max):
    rng = np.random.default_rng(n_sets * 37 + words)
    sets = randomSets(rng, n_sets, words, n_allele, empty_first)
    count = mixedCounts(rng, n_sets, big_every)
    prob, iters, got = bootstrapEM(device, [(sets, count, n_allele, 3)], 2, SEED, iter_max=iter_max, want_counts=True)
    keep = sets.any(axis=1)
    assert keep.sum() == n_sets - empty_first
    uniq = np.ascontiguousarray(sets[keep])
    for b in range(2):
        weight = np.ascontiguousarray(got[b][keep].astype(np.float64))
        assert weight.sum() > 0
        point, point_iters = np.zeros(n_allele, dtype=np.float64), C.c_int32(-1)
        _lib.check(_lib.lib().gk_em_run(device.ctx, uniq.ctypes.data, weight.ctypes.data, len(uniq), words, n_allele, iter_max, 1e-4,
                                        point.ctypes.data, C.byref(point_iters)))
        assert np.array_equal(prob[b], point), b
        assert int(iters[b, 0]) == point_iters.value, b
    return prob, iters


@pytest.mark.parametrize("words,n_allele,n_sets,empty_first,big_every", SAME_SOLVER_CASES)
def test_batch_solver_is_the_point_solver(device, words, n_allele, n_sets, empty_first, big_every):
    """boot_em_batch and em_kernel_genes instantiate one solver (csrc/gk_squarem.h) whose sums do not depend on the
    workgroup size: a replicate's counts handed to gk_em_run as weights (sets that drew no read included: weight 0 gives
    scale 0 in both) give the replicate's abundances and step count, bit for bit."""
    batchIsPoint(device, words, n_allele, n_sets, empty_first, big_every, 300)


@pytest.mark.parametrize("words,n_allele,n_sets,empty_first,big_every", SAME_SOLVER_CASES)
def test_batch_solver_is_the_point_solver_after_two_passes(device, words, n_allele, n_sets, empty_first, big_every):
    """The same at iter_max = 2: the state after exactly two passes, before any stop (a run that is used up says 2)."""
    prob, iters = batchIsPoint(device, words, n_allele, n_sets, empty_first, big_every, 2)
    assert (iters <= 2).all()


def test_point_result_does_not_change(typed):
    plain, plain_calls, boot, boot_calls = typed
    assert plain.bootstrap == {} and boot_calls == plain_calls
    assert plain._result.keys() == boot._result.keys()
    for gene in plain._result:
        a = [(r.allele, r.count, r.prob, r.cn) for r in plain._result[gene]]
        b = [(r.allele, r.count, r.prob, r.cn) for r in boot._result[gene]]
        assert a == b, gene           # bit for bit
    assert plain.em_info == boot.em_info


def test_support_follows_from_the_replicates(tabulated, typed):
    data, sample = tabulated
    _, _, boot, _ = typed
    for gene, res in boot.bootstrap.items():
        cn = int(sample.gene_cn[gene])
        report = boot._result[gene]
        assert res.alleles == [r.allele for r in report]
        point = Counter(callsByAbundance(res.alleles, [r.prob for r in report], cn)[0])
        calls = [callsByAbundance(res.alleles, res.prob[b].tolist(), cn)[0] for b in range(8)]
        assert calls == res.calls
        assert res.call_support == sum(Counter(c) == point for c in calls) / 8
        for i, (rec, row) in enumerate(zip(report, res.rows)):
            need = max(1, point.get(rec.allele, 0))
            assert row["support"] == sum(Counter(c).get(rec.allele, 0) >= need for c in calls) / 8
            assert (row["gene"], row["allele"], row["cn"], row["count"], row["prob"]) == (gene, rec.allele, rec.cn, rec.count, rec.prob)
            assert row["boot_mean"] == float(res.prob[:, i].mean()) and row["boot_sd"] == float(res.prob[:, i].std(ddof=1))
            assert [row["boot_lo"], row["boot_hi"]] == [float(v) for v in np.percentile(res.prob[:, i], [2.5, 97.5])]
            assert row["call_support"] == res.call_support


def test_per_gene_path_gives_the_same_bootstrap(tabulated, typed):
    data, sample = tabulated
    _, _, boot, _ = typed
    per_gene = selectKirTypingModel("em", data, bootstrap=8, bootstrap_seed=2022)
    for gene, cn in sample.gene_cn.items():
        if cn:
            per_gene.typingPerGene(gene, int(cn))
    assert per_gene.bootstrap.keys() == boot.bootstrap.keys()
    for gene, res in boot.bootstrap.items():
        other = per_gene.bootstrap[gene]
        assert other.alleles == res.alleles and other.calls == res.calls and other.rows == res.rows
        assert np.array_equal(other.prob, res.prob) and np.array_equal(other.iterations, res.iterations)
    reseeded = TypingWithReport(data, bootstrap=8, bootstrap_seed=7)
    reseeded.typing(sample.gene_cn)
    assert any(not np.array_equal(reseeded.bootstrap[g].prob, boot.bootstrap[g].prob) for g in boot.bootstrap)


def test_command_line_writes_the_confidence_file(device, tmp_path, monkeypatch):
    """graphkir --allele-strategy em on a small BAM, without and with --em-bootstrap 8 (in-process, like
    tests/test_gpu_cn_cli.py): the typing files do not change, the confidence file holds the typer's numbers."""
    from bamwriter import samToBam
    from kir_graph_amd import main as cli
    sidx = synth.makeIndex(seed=11, n_genes=3, var_range=(200, 300), allele_range=(12, 20))
    folder = tmp_path / "index"
    folder.mkdir()
    prefix = str(folder / "kir_2100_withexon_ab_2dl1s1.leftalign.mut01")
    sidx.write(prefix)
    s = synth.makeSample(sidx, seed=50, n_pairs=2500)
    lines = synth.toSamLines(s)
    header = ["@HD\tVN:1.0\tSO:coordinate"] + [f"@SQ\tSN:{g}\tLN:{len(sidx.backbone[g])}" for g in sidx.genes]
    samToBam(header + sorted(lines, key=lambda l: (l.split("\t")[2], int(l.split("\t")[3]))), str(tmp_path / "s.bam"))
    (tmp_path / "s.cn.tsv").write_text("gene\tcn\n" + "".join(f"{g}\t{c}\n" for g, c in s.gene_cn.items()))
    files, typers = [], []
    write = cli.writeTyping
    monkeypatch.setattr(cli, "writeTyping", lambda name, typer, *rest: (typers.append(typer), write(name, typer, *rest))[1])
    for k, extra in enumerate(([], ["--em-bootstrap", "8"])):
        # every path relative to the run's own folder: {name}.tsv holds the sample's output name, which must be the same
        # text in both runs for the files to be comparable byte for byte (and short enough for a file name)
        run = tmp_path / f"run{k}"
        run.mkdir()
        monkeypatch.chdir(run)
        cli.main(cli.createParser().parse_args(
            ["--step-skip-extraction", "--index-folder", "../index", "--output-folder", "out", "--allele-strategy", "em",
             "--cn-provided", "../s.cn.tsv", "--alignment", "../s.bam"] + extra))
        files.append({p.name: p for p in (run / "out").iterdir()})
    assert files[0].keys() | {n for n in files[1] if n.endswith(".confidence.tsv")} == files[1].keys()
    typing = [n for n in files[0] if n.endswith(".em.tsv") or n.endswith(".em.possible.tsv")]
    assert len(typing) == 2
    for n in typing:
        assert files[0][n].read_bytes() == files[1][n].read_bytes(), n
    conf = [n for n in files[1] if n.endswith(".confidence.tsv")]
    assert len(conf) == 1 and conf[0] == [n for n in typing if n.endswith(".em.tsv")][0][:-4] + ".confidence.tsv"
    assert not any(n.endswith(".confidence.tsv") for n in files[0])
    text = files[1][conf[0]].read_text().split("\n")
    assert text[0] == "gene\tallele\tcn\tcount\tprob\tboot_mean\tboot_sd\tboot_lo\tboot_hi\tsupport\tcall_support" and text[-1] == ""
    rows = [line.split("\t") for line in text[1:-1]]
    assert len(typers) == 2 and typers[0].bootstrap == {} and len(typers[1].bootstrap) == 3
    typer = typers[1]              # the typer of the second run, as the finish step saw it
    for gene, report in typers[0]._result.items():
        assert [(r.allele, r.count, r.prob, r.cn) for r in report] == [(r.allele, r.count, r.prob, r.cn) for r in typer._result[gene]]
    want = [(gene, r.allele, str(r.cn), str(r.count), repr(float(r.prob))) for gene, report in typer._result.items() for r in report]
    assert [tuple(r[:5]) for r in rows] == want and len(want) > 3
    assert [[float(x) for x in r[5:]] for r in rows] == [
        [row[k] for k in ("boot_mean", "boot_sd", "boot_lo", "boot_hi", "support", "call_support")]
        for boot in typer.bootstrap.values() for row in boot.rows]
