"""Host side of the copy-number bootstrap (kir_graph_amd/cn_bootstrap.py, the parser of main.py): no GPU."""
import numpy as np
import pandas as pd
import pytest

from kir_graph_amd import cn_bootstrap as cb


class StubModel:
    """Copy number = depth // 10; ``assignCN`` fails beyond its bins like ``CNgroup.assignCN`` does."""

    def __init__(self, x_max=100.0, bin_num=50):
        self.x_max, self.bin_num, self.base = x_max, bin_num, 10.0
        self.seen = []

    def assignCN(self, values):
        space = self.x_max / self.bin_num
        table = [int(i * space // 10) for i in range(self.bin_num)]
        self.seen.append(list(values))
        return [table[int(v / space)] for v in values]          # IndexError at or beyond x_max


class CutModel:
    """A model without bins (``KDEcut``): nothing to clamp."""

    def assignCN(self, values):
        return list(np.searchsorted([10.0, 20.0], np.array(values)))


def makeBoot(columns, point=None):
    genes = list(columns)
    reps = np.array([columns[g] for g in genes], dtype=np.float64).T
    return cb.DepthBootstrap(genes=genes, point=np.array(point if point is not None else reps[0], dtype=np.float64),
                             replicates=reps, seed=5, select_mode="p75")


def test_confidence_rows():
    boot = makeBoot({
        "A": [21, 22, 23, 24, 25, 26, 27, 28],                  # every replicate gets the called 2
        "B": [21, 22, 11, 12, 31, 32, 25, 26],                  # 1 and 3 tie as the alternative: the smaller
        "C": [35, 36, 37, 38, 39, 41, 42, 1000],                # a depth beyond x_max: the last bin
        "D": [5, 5, 5, 5, 15, 15, 15, 25],                      # the called copy number is not the most frequent
        "E": [1, 2, 3, 4, 5, 6, 7, 8],                          # not in the CN file: no row
    }, point=[24.5, 22.0, 38.0, 5.0, 1.0])
    model = StubModel()
    rows = cb.cnConfidence(boot, model, {"A": 2, "B": 2, "C": 3, "D": 1, "Z": 4})
    assert [r["gene"] for r in rows] == ["A", "B", "C", "D"] and len(model.seen) == 1          # one call for all genes
    a, b, c, d = rows
    assert (a["cn"], a["depth"], a["support"], a["cn_lo"], a["cn_hi"], a["alt_cn"], a["alt_share"]) == (2, 24.5, 1.0, 2, 2, None, None)
    x = np.arange(21.0, 29.0)
    assert a["depth_mean"] == x.mean() and a["depth_sd"] == x.std(ddof=1)
    assert (a["depth_lo"], a["depth_hi"]) == tuple(np.percentile(x, [2.5, 97.5]))
    assert (b["support"], b["cn_lo"], b["cn_hi"], b["alt_cn"], b["alt_share"]) == (0.5, 1, 3, 1, 0.25)
    assert (c["support"], c["cn_lo"], c["cn_hi"], c["alt_cn"], c["alt_share"]) == (5 / 8, 3, 9, 4, 0.25)      # 1000 -> bin 49 -> 9
    assert c["depth_hi"] > 100 and max(model.seen[0]) < 100                                   # clamped for the model only
    assert (d["cn"], d["support"], d["alt_cn"], d["alt_share"]) == (1, 3 / 8, 0, 0.5)
    # a depth exactly at x_max is the last bin too; a model without bins is asked as it is
    assert cb.assignReplicates(StubModel(), [100.0, 99.99, 0.0]) == [9, 9, 0]
    assert cb.assignReplicates(CutModel(), [5.0, 1e9]) == [0, 2]
    one = cb.cnConfidence(makeBoot({"A": [21.0]}), StubModel(), {"A": 2})[0]
    assert one["depth_sd"] == 0.0 and one["depth_lo"] == one["depth_hi"] == 21.0


def test_confidence_text():
    boot = makeBoot({"A": [21, 22, 23, 24], "B": [21, 22, 11, 31]}, point=[22.5, 0.1 + 0.2])
    rows = cb.cnConfidence(boot, StubModel(), {"A": 2, "B": 2})
    text = cb.cnConfidenceText(rows)
    lines = text.split("\n")
    assert lines[0].startswith("# conditional on the copy-number model") and lines[-1] == "" and len(lines) == 5
    assert lines[1].split("\t") == cb.CN_CONFIDENCE_COLUMNS == ["gene", "cn", "depth", "depth_mean", "depth_sd", "depth_lo",
                                                                 "depth_hi", "support", "cn_lo", "cn_hi", "alt_cn", "alt_share"]
    a, b = (line.split("\t") for line in lines[2:4])
    assert a[:3] == ["A", "2", "22.5"] and a[7:] == ["1.0", "2", "2", "", ""]
    assert b[2] == repr(0.1 + 0.2) and float(b[2]) == 0.1 + 0.2 and b[7:] == ["0.5", "1", "3", "1", "0.25"]
    named = cb.cnConfidenceText(rows, name="s1").split("\n")
    assert named[1].split("\t") == ["name"] + cb.CN_CONFIDENCE_COLUMNS and named[2].split("\t") == ["s1"] + a
    assert cb.cnConfidenceText([]).split("\n")[1:] == ["\t".join(cb.CN_CONFIDENCE_COLUMNS), ""]


def test_merged_table(tmp_path):
    rows = cb.cnConfidence(makeBoot({"A": [21, 22, 23, 24], "B": [21, 22, 11, 31]}), StubModel(), {"A": 2, "B": 2})
    for name in ("x", "y"):
        (tmp_path / f"{name}.confidence.tsv").write_text(cb.cnConfidenceText(rows if name == "x" else rows[:1]))
    out = cb.mergeCnConfidence([("y.tsv", str(tmp_path / "y.confidence.tsv")), ("x.tsv", str(tmp_path / "x.confidence.tsv"))],
                               str(tmp_path / "cohort.cn.confidence.tsv"))
    want = cb.cnConfidenceText(rows[:1], name="y.tsv") + cb.cnConfidenceText(rows, name="x.tsv", header=False)
    assert open(out).read() == want
    back = pd.read_csv(out, sep="\t", comment="#")
    assert list(back["name"]) == ["y.tsv", "x.tsv", "x.tsv"] and list(back["gene"]) == ["A", "A", "B"]


def test_boot_file_round_trip_is_bit_exact(tmp_path):
    rng = np.random.default_rng(1)
    reps = rng.random((6, 3)) * np.array([1.0, 1e-300, 1e300])
    reps[2, 1] = np.nan                                          # a gene without a selected position
    reps[3, 0] = 5e-324
    boot = cb.DepthBootstrap(genes=["KIR2DL1*BACKBONE", "b", "c"], point=np.array([0.1 + 0.2, 1 / 3, 2.0 ** 70]),
                             replicates=reps, seed=(1 << 63) + 12345, select_mode="median")
    path = cb.writeDepthBootstrap(boot, str(tmp_path / "s.depth.boot.tsv"))
    back = cb.readDepthBootstrap(path)
    assert back.genes == boot.genes and (back.seed, back.select_mode) == (boot.seed, "median")
    assert back.point.tobytes() == boot.point.tobytes() and back.replicates.shape == (6, 3)
    same = np.ascontiguousarray(back.replicates).view(np.uint64) == np.ascontiguousarray(boot.replicates).view(np.uint64)
    assert same[~np.isnan(boot.replicates)].all() and np.isnan(boot.replicates).sum() == 1
    assert np.isnan(back.replicates[2, 1])
    lines = open(path).read().split("\n")
    assert lines[1].split("\t") == ["gene", "point", "b0", "b1", "b2", "b3", "b4", "b5"] and len(lines) == 2 + 3 + 1
    assert cb.writeDepthBootstrap(back, str(tmp_path / "again.tsv")) and open(tmp_path / "again.tsv").read() == open(path).read()


def test_parser_defaults_and_range():
    from kir_graph_amd import main as cli
    p = cli.createParser()
    ns = p.parse_args([])
    assert ns.cn_bootstrap is None and ns.cn_bootstrap_seed == 2022 and cli._cnBootstrapArgs(ns) is None
    ns = p.parse_args(["--cn-bootstrap", "100", "--cn-bootstrap-seed", "7", "--cn-select", "mean"])
    assert cli._cnBootstrapArgs(ns) == {"n_boot": 100, "seed": 7, "select_mode": "mean"}
    assert p.parse_args(["--cn-bootstrap", "1"]).cn_bootstrap == 1 and p.parse_args(["--cn-bootstrap", "10000"]).cn_bootstrap == 10000
    for bad in ("0", "-3", "10001", "many"):
        with pytest.raises(SystemExit):
            p.parse_args(["--cn-bootstrap", bad])
    assert cb.CN_BOOT_STREAM == 0x434E and cb.MAX_BOOT == 10000


@pytest.mark.parametrize("q", [0.75, 0.5])
def test_interpolation_equals_pandas(q):
    rng = np.random.default_rng(int(q * 100))
    for n in list(range(1, 40)) + [100, 101, 102, 103, 4097, 17000]:
        values = np.sort(rng.integers(0, rng.choice([3, 50, 1 << 12, 1 << 32]), n)).astype(np.int64)
        lo, hi = cb.quantileRanks(q, n)
        assert 0 <= lo <= hi <= n - 1 and hi - lo <= 1
        got = cb.quantileOf(values[[lo]], values[[hi]], q, n)
        want = pd.Series(values).quantile(q)
        assert got.dtype == np.float64 and float(got[0]).hex() == float(want).hex(), (q, n)
        # what aggrDepths asks pandas for: the same bits
        frame = pd.DataFrame({"gene": "g", "depth": values}).groupby("gene", as_index=False)["depth"]
        assert float(frame.quantile(q)["depth"][0]).hex() == float(got[0]).hex(), (q, n)
        if q == 0.5:
            assert float(frame.median()["depth"][0]).hex() == float(got[0]).hex(), n
    assert cb.quantileRanks(q, 0) == (0, 0)


def test_region_mask():
    off = np.array([0, 10, 30], dtype=np.int64)
    mask = cb.regionMask(["a", "b"], off, {"a": [(2, 4), (8, 50)], "b": [(0, 1)], "c": [(1, 5)]})
    # 1-based inclusive, as kir_cn.selectSamtoolsDepth compares them, clipped to the backbone
    assert mask[:10].tolist() == [0, 1, 1, 1, 0, 0, 0, 1, 1, 1] and mask[10:].tolist() == [1] + [0] * 19
    frame = pd.DataFrame({"gene": ["a"] * 10 + ["b"] * 20, "pos": list(range(1, 11)) + list(range(1, 21)), "depth": 0})
    from kir_graph_amd.kir_cn import selectSamtoolsDepth
    kept = selectSamtoolsDepth(frame, {"a": [(2, 4), (8, 50)], "b": [(0, 1)]})
    assert sorted(kept.index.tolist()) == np.flatnonzero(mask).tolist()
    assert not cb.regionMask(["a", "b"], off, {}).any()
    for overlapping in ({"a": [(2, 4), (4, 6)]}, {"b": [(1, 9), (3, 5)]}, {"a": [(3, 3), (3, 3)]}):
        with pytest.raises(ValueError):
            cb.regionMask(["a", "b"], off, overlapping)
    assert cb.regionMask(["a", "b"], off, {"a": [(2, 4), (5, 6)]})[:10].tolist() == [0, 1, 1, 1, 1, 1, 0, 0, 0, 0]
