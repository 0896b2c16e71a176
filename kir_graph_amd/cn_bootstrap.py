"""
Read-bootstrap confidence of the copy numbers (``--cn-bootstrap``).

Every likelihood and EM call is conditioned on the copy number of its gene, and that number is one integer read off one
gene depth (``kir_cn.aggrDepths``: p75 / mean / median of the depth track).  This module says how far the gene depth moves
under another draw of the reads, and how often the copy number moves with it:

1. a replicate draws ``n_valid`` pairs with replacement from the sample's ``n_valid`` filter-passing pairs -- over the WHOLE
   sample, not per gene: a gene's share of the reads is the signal -- as weights ``W[b][i]`` (``gk_boot_row_counts``: the
   generator of the EM and call bootstraps, stream ``CN_BOOT_STREAM``; a replicate depends on (seed, b, n_valid) alone);
2. ``gk_depth_weighted`` (``depthw_mark``, one scan, ``depthw_finish``, ``depthw_select``): the depth of the sample with pair
   ``i`` counted ``W[b][i]`` times, and per gene the sum and two order statistics of its (selected) positions -- the tracks
   stay in HBM;
3. on the host the gene statistic from those integers, interpolated as ``pandas.Series.quantile`` does
   (``quantileOf``); the POINT value is the same computation with all weights 1 and equals ``aggrDepths`` of the depth file;
4. ``cnConfidence``: every replicate's statistic assigned a copy number by the model the point estimate fitted.  The model
   is NOT refitted per replicate: the table is conditional on it.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ._lib import check, lib
from .utils import logger

MAX_BOOT = 10000                 # replicates of one library call (include/graphkir_hip.h)
CN_BOOT_STREAM = 0x434E          # "CN": the generator stream of this bootstrap -- the EM bootstrap uses 0, 1, ... (a gene's job),
                                 # the call bootstrap a gene's ordinal in the index (< 256): the draws share nothing with theirs
W_BYTES = 256 << 20              # the weights of a slice of the replicates
QUANTILE = {"p75": 0.75, "median": 0.5}

CN_CONFIDENCE_COLUMNS = ["gene", "cn", "depth", "depth_mean", "depth_sd", "depth_lo", "depth_hi", "support", "cn_lo", "cn_hi",
                         "alt_cn", "alt_share"]
CN_CONFIDENCE_NOTE = ("# conditional on the copy-number model fitted to the point estimate: a replicate's gene depth is assigned "
                      "by that model, which is not refitted")


@dataclass
class DepthBootstrap:
    """Read bootstrap of one sample's gene depths.  ``genes``: the backbones in index order, ``point[g]``: the statistic
    ``select_mode`` of the sample's depth (all weights 1), ``replicates[b, g]``: that of replicate ``b``; NaN for a gene
    without a selected position."""

    genes: list[str]
    point: np.ndarray
    replicates: np.ndarray
    seed: int = 2022
    select_mode: str = "p75"


def quantileRanks(q: float, n: int) -> tuple[int, int]:
    """The two 0-based ranks ``pandas.Series.quantile(q)`` of ``n`` values interpolates between: ``floor(q (n - 1))`` and
    the next one, clamped."""
    lo = int(np.floor(q * (n - 1)))
    lo = min(max(lo, 0), max(n - 1, 0))
    return lo, min(lo + 1, max(n - 1, 0))


def quantileOf(a, b, q: float, n: int) -> np.ndarray:
    """``pandas.Series.quantile(q)`` (numpy's ``linear`` method) of ``n`` sorted values whose ranks ``quantileRanks(q, n)``
    hold ``a`` and ``b`` (arrays): ``a + (b - a) t`` with ``t`` the fractional part of ``q (n - 1)``, taken from the upper
    end from ``t = 0.5`` on as numpy does."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    t = q * (n - 1) - np.floor(q * (n - 1))
    diff = b - a
    return np.where(t >= 0.5, b - diff * (1 - t), a + diff * t) if t > 0 else a.copy()


def regionMask(genes: list[str], off: np.ndarray, regions: dict[str, list[tuple[int, int]]]) -> np.ndarray:
    """uint8 over the concatenated positions: 1 where ``kir_cn.selectSamtoolsDepth`` keeps the position -- 1-based position
    ``p`` of a gene with ``start <= p <= end`` for one of the gene's ``regions``.  Regions that overlap inside a gene raise
    ``ValueError``: ``selectSamtoolsDepth`` would list their positions twice."""
    mask = np.zeros(int(off[-1]), dtype=np.uint8)
    for g, gene in enumerate(genes):
        length = int(off[g + 1] - off[g])
        last = None
        for start, end in sorted((int(s), int(e)) for s, e in regions.get(gene, [])):
            if end < start:
                continue
            if last is not None and start <= last:
                raise ValueError(f"cn bootstrap: the regions of {gene} overlap at position {start}")
            last = end
            a, b = max(start, 1), min(end, length)      # 1-based inclusive, clipped to the backbone
            if b >= a:
                mask[int(off[g]) + a - 1:int(off[g]) + b] = 1
    return mask


def _records(tab) -> tuple[int, int]:
    """(d_mates, d_compact) of the sample's records in HBM: of ``packed.DeviceCompactMates`` the compact words."""
    words = getattr(tab.mates, "words", None) if hasattr(tab.mates, "records") else None
    return (0, words.ptr) if words is not None else (tab.mates.ptr, 0)


def hasRecords(data) -> bool:
    """Are the sample's packed records in HBM with a tabulation that knows its pair sources?"""
    tab = getattr(data, "tab", None)
    return (tab is not None and getattr(tab, "mates", None) is not None
            and bool(getattr(getattr(tab, "info", None), "d_pair_src", 0)))


def bootstrapGeneDepths(data, gene_len: dict[str, int], n_boot: int, seed: int = 2022, select_mode: str = "p75",
                        regions: dict[str, list[tuple[int, int]]] | None = None, multiple: bool = False,
                        slice: int | None = None) -> DepthBootstrap:
    """The read bootstrap of the gene depths of one tabulated sample whose records are in HBM (``samtools_utils.depthOfSample``
    needs the same).  ``regions``: what ``index.readExons`` returns, used as ``kir_cn.filterDepth`` uses it (``--cn-exon``).
    ``slice``: replicates per library call (default: what ``W_BYTES`` of weights hold); the result does not depend on it."""
    if select_mode not in ("p75", "mean", "median"):
        raise NotImplementedError(select_mode)
    n_boot = int(n_boot)
    if not 1 <= n_boot <= MAX_BOOT:
        raise ValueError(f"cn bootstrap: the number of replicates must lie in 1 .. {MAX_BOOT}, got {n_boot}")
    if not hasRecords(data):
        raise ValueError("cn bootstrap: the sample's packed records are not in HBM")
    tab = data.tab
    dev = tab.dev
    genes = list(data.index.genes)
    lens = np.array([gene_len[g] for g in genes], dtype=np.int64)
    off = np.zeros(len(genes) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    sel = None if regions is None else regionMask(genes, off, regions)
    n_sel = lens if sel is None else np.add.reduceat((sel != 0).astype(np.int64), off[:-1])
    q = QUANTILE.get(select_mode, 0.5)
    rank = np.array([quantileRanks(q, int(n)) for n in n_sel], dtype=np.int64).reshape(len(genes), 2)
    n_valid = int(tab.n_valid)
    ldw = max(n_valid, 1)
    per_call = int(slice) if slice else max(1, W_BYTES // (4 * ldw))
    per_call = max(1, min(per_call, n_boot, MAX_BOOT))
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    d_mates, d_compact = _records(tab)

    def statistic(W, nb: int) -> np.ndarray:
        stat = np.zeros((nb, len(genes), 2), dtype=np.uint32)
        total = np.zeros((nb, len(genes)), dtype=np.uint64)
        check(lib().gk_depth_weighted(dev.ctx, tab.handle, d_mates, d_compact, int(multiple), off.ctypes.data, len(genes), W.ptr,
                                      ldw, nb, sel.ctypes.data if sel is not None else None, rank.ctypes.data,
                                      stat.ctypes.data, total.ctypes.data, None))
        out = np.full((nb, len(genes)), np.nan)
        for g, n in enumerate(n_sel):
            if n == 0:
                continue
            if select_mode == "mean":
                out[:, g] = total[:, g].astype(np.float64) / float(n)      # exact integers below 2^53: one rounding, pandas' value
            else:
                out[:, g] = quantileOf(stat[:, g, 0], stat[:, g, 1], q, int(n))
        return out

    ones = dev.put(np.ones((1, ldw), dtype=np.uint32))      # the point estimate: one more "replicate", through the same kernels
    try:
        point = statistic(ones, 1)[0]
    finally:
        ones.free()
    replicates = np.empty((n_boot, len(genes)), dtype=np.float64)
    W = dev.alloc((per_call, ldw), np.uint32)
    try:
        for b0 in range(0, n_boot, per_call):
            nb = min(per_call, n_boot - b0)
            if n_valid:
                check(lib().gk_boot_row_counts(dev.ctx, n_valid, nb, b0, seed, CN_BOOT_STREAM, W.ptr, ldw))
            replicates[b0:b0 + nb] = statistic(W, nb)
    finally:
        W.free()
    return DepthBootstrap(genes=genes, point=point, replicates=replicates, seed=int(seed), select_mode=select_mode)


# ------------------------------------------------------------------------------------------------ {depth_name}.boot.tsv
def depthBootstrapText(boot: DepthBootstrap) -> str:
    """``gene``, ``point``, ``b0`` .. ``b{N-1}``, tab separated, one row per gene; floats as ``repr(float)`` (they round-trip);
    a first ``#`` line holds the seed and the statistic."""
    n_boot = len(boot.replicates)
    lines = [f"# seed={int(boot.seed)} select_mode={boot.select_mode}", "\t".join(["gene", "point"] + [f"b{b}" for b in range(n_boot)])]
    for g, gene in enumerate(boot.genes):
        lines.append("\t".join([gene, repr(float(boot.point[g]))] + [repr(float(x)) for x in boot.replicates[:, g]]))
    return "\n".join(lines) + "\n"


def writeDepthBootstrap(boot: DepthBootstrap, filename: str) -> str:
    with open(filename, "w") as f:
        f.write(depthBootstrapText(boot))
    return filename


def readDepthBootstrap(filename: str) -> DepthBootstrap:
    with open(filename) as f:
        lines = f.read().split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    seed, select_mode = 2022, "p75"
    if lines and lines[0].startswith("#"):
        for word in lines.pop(0)[1:].split():
            key, _, value = word.partition("=")
            if key == "seed":
                seed = int(value)
            elif key == "select_mode":
                select_mode = value
    header = lines[0].split("\t")
    assert header[:2] == ["gene", "point"] and header[2:] == [f"b{b}" for b in range(len(header) - 2)], header
    rows = [line.split("\t") for line in lines[1:]]
    assert all(len(r) == len(header) for r in rows)
    return DepthBootstrap(genes=[r[0] for r in rows], point=np.array([float(r[1]) for r in rows], dtype=np.float64),
                          replicates=np.array([[float(x) for x in r[2:]] for r in rows], dtype=np.float64).reshape(len(rows), -1).T.copy(),
                          seed=seed, select_mode=select_mode)


# ------------------------------------------------------------------------------------------------ {cn_name}.confidence.tsv
def assignReplicates(dist, depths) -> list[int]:
    """``dist.assignCN`` of replicate depths.  ``CNgroup.assignCN`` looks a depth up in ``bin_num`` bins over [0, x_max) and
    fails beyond them; a replicate may lie there (the model saw the point estimates only), so a depth at or beyond ``x_max``
    is assigned as the last bin."""
    depths = [float(d) for d in depths]
    bins = getattr(dist, "bin_num", None)
    if bins is not None and getattr(dist, "base", None) is not None:      # CNgroup
        space = dist.x_max / dist.bin_num
        inside = (bins - 0.5) * space                                     # int(inside / space) == bins - 1
        depths = [d if int(d / space) < bins else inside for d in depths]
    return [int(c) for c in dist.assignCN(depths)]


def cnConfidence(boot: DepthBootstrap, dist, cn: dict[str, int]) -> list[dict]:
    """One row per gene of ``boot`` that ``cn`` (the sample's called copy numbers) lists: ``depth`` = the point value,
    mean / sd (n - 1) / 2.5 % / 97.5 % (``numpy.percentile``) of the replicates' depths, ``support`` = the share of replicates
    the model gives the called ``cn``, ``cn_lo`` / ``cn_hi`` = the smallest / largest copy number of any replicate,
    ``alt_cn`` / ``alt_share`` = the most frequent other copy number (the smaller on a tie; None when there is none)."""
    kept = [(g, gene) for g, gene in enumerate(boot.genes) if gene in cn and np.isfinite(boot.replicates[:, g]).all()]
    n_boot = len(boot.replicates)
    flat = [x for g, _ in kept for x in boot.replicates[:, g]]
    assigned = np.array(assignReplicates(dist, flat) if flat else [], dtype=np.int64).reshape(len(kept), n_boot)
    rows = []
    for (g, gene), cns in zip(kept, assigned):
        x = boot.replicates[:, g]
        lo, hi = np.percentile(x, [2.5, 97.5])
        called = int(cn[gene])
        values, counts = np.unique(cns[cns != called], return_counts=True)
        alt = int(values[np.argmax(counts)]) if len(values) else None      # the first of equal maxima: the smaller
        rows.append({"gene": gene, "cn": called, "depth": float(boot.point[g]), "depth_mean": float(x.mean()),
                     "depth_sd": float(x.std(ddof=1)) if n_boot > 1 else 0.0, "depth_lo": float(lo), "depth_hi": float(hi),
                     "support": float((cns == called).sum() / n_boot), "cn_lo": int(cns.min()), "cn_hi": int(cns.max()),
                     "alt_cn": alt, "alt_share": float(counts.max() / n_boot) if alt is not None else None})
    return rows


def _cell(x) -> str:
    if x is None:
        return ""
    return repr(float(x)) if isinstance(x, (float, np.floating)) else str(x)


def cnConfidenceText(rows: list[dict], name: str | None = None, header: bool = True) -> str:
    """``{cn_name}.confidence.tsv``: the note that the table is conditional on the fitted model, the column names, one row
    per gene; floats as ``repr(float)``, ``alt_cn`` / ``alt_share`` empty when every replicate got the called copy number.
    ``name``: a leading ``name`` column with this value (the cohort's table); ``header=False``: the rows alone."""
    lead = [] if name is None else ["name"]
    lines = [CN_CONFIDENCE_NOTE, "\t".join(lead + CN_CONFIDENCE_COLUMNS)] if header else []
    for r in rows:
        lines.append("\t".join(([] if name is None else [name]) + [_cell(r[c]) for c in CN_CONFIDENCE_COLUMNS]))
    return "\n".join(lines) + "\n" if lines else ""


def writeCnConfidence(boot_file: str, dist, cn_file: str, filename: str) -> str:
    """The confidence table of one sample from its ``.boot.tsv``, the model its copy numbers were assigned by and its CN
    file."""
    from .kir_cn import loadCN
    with open(filename, "w") as f:
        f.write(cnConfidenceText(cnConfidence(readDepthBootstrap(boot_file), dist, loadCN(cn_file))))
    logger.info(f"[CN] Bootstrap confidence of the copy numbers in {filename}")
    return filename


def mergeCnConfidence(files: list[tuple[str, str]], filename: str) -> str:
    """``{cohort}.cn.confidence.tsv``: the per-sample tables ``(name, file)`` one after the other, in the order given, with
    a leading ``name`` column."""
    lines = [CN_CONFIDENCE_NOTE, "\t".join(["name"] + CN_CONFIDENCE_COLUMNS)]
    for name, path in files:
        with open(path) as f:
            rows = [line for line in f.read().split("\n") if line and not line.startswith("#")]
        assert rows and rows[0].split("\t") == CN_CONFIDENCE_COLUMNS, path
        lines.extend(name + "\t" + row for row in rows[1:])
    with open(filename, "w") as f:
        f.write("\n".join(lines) + "\n")
    return filename
