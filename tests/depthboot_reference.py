"""numpy / plain-Python restatement of the read bootstrap of the copy-number stage (csrc/gk_depthboot.hip,
include/graphkir_hip.h, kir_graph_amd/cn_bootstrap.py): what gk_depth_weighted must return and what the host makes of it, in
exact integers.  Slow and plain on purpose: one loop per mate, selection by sorting."""
import numpy as np

import callboot_reference
from callcov_reference import SPILLED, mateRuns

CN_BOOT_STREAM = 0x434E
MASK32 = 0xFFFFFFFF


def weights(seed, boots, n_valid):
    """int64 [len(boots), n_valid]: the draws of the listed replicates on every valid pair (the documented generator)."""
    boots = list(boots)
    if n_valid == 0:
        return np.zeros((len(boots), 0), dtype=np.int64)
    return np.array([callboot_reference.rowCounts(seed, CN_BOOT_STREAM, b, n_valid) for b in boots],
                    dtype=np.int64).reshape(len(boots), n_valid)


def pairMarks(records, pair_src, pair_nh, multiple, gene_off, wide=None):
    """Per valid pair the (position in the concatenated space, +1 / -1) marks of both mates, as depth_mark makes them."""
    n_gene = len(gene_off) - 1
    out = []
    for i in range(len(pair_src)):
        marks = []
        if multiple or int(pair_nh[i]) == 1:
            p = int(pair_src[i])
            for side in (0, 1):
                rec = records[2 * p + side]
                ref = int(rec["ref"])
                if ref >= n_gene:
                    continue
                far = None
                if int(rec["n_cig"]) == SPILLED:
                    if wide is None:
                        continue
                    far = wide[2 * int(rec["ins"][0]) + side]
                base, length = int(gene_off[ref]), int(gene_off[ref + 1] - gene_off[ref])
                for a, b in mateRuns(rec, far):
                    a, b = max(a, 0), min(b, length)
                    if b > a:
                        marks += [(base + a, 1), (base + b, -1)]
        out.append(marks)
    return out


def weightedDepth(marks, W, total):
    """uint32-valued int64 [n_boot][total]: the depth with pair i counted W[b][i] times, mod 2^32."""
    W = np.asarray(W, dtype=np.int64)
    diff = np.zeros((len(W), total + 1), dtype=np.int64)
    for i, pair in enumerate(marks):
        for at, sign in pair:
            diff[:, at] += sign * W[:, i]
    return np.cumsum(diff, axis=1)[:, :total] & MASK32


def select(depth, gene_off, sel, rank):
    """(stat int64 [n_boot][n_gene][2], sum [n_boot][n_gene] as Python integers in an object array) by sorting."""
    n_boot, n_gene = len(depth), len(gene_off) - 1
    stat = np.zeros((n_boot, n_gene, 2), dtype=np.int64)
    total = np.zeros((n_boot, n_gene), dtype=object)
    for g in range(n_gene):
        a, b = int(gene_off[g]), int(gene_off[g + 1])
        keep = np.ones(b - a, dtype=bool) if sel is None else np.asarray(sel[a:b]) != 0
        if not keep.any():
            continue
        for r in range(n_boot):
            v = np.sort(depth[r, a:b][keep])
            stat[r, g] = v[int(rank[g][0])], v[int(rank[g][1])]
            total[r, g] = sum(int(x) for x in v)
    return stat, total


def statistic(depth, gene_off, sel, select_mode):
    """float64 [n_boot][n_gene]: pandas' own p75 / mean / median of every gene's selected depths (NaN when none)."""
    import pandas as pd
    n_boot, n_gene = len(depth), len(gene_off) - 1
    out = np.full((n_boot, n_gene), np.nan)
    for g in range(n_gene):
        a, b = int(gene_off[g]), int(gene_off[g + 1])
        keep = np.ones(b - a, dtype=bool) if sel is None else np.asarray(sel[a:b]) != 0
        if not keep.any():
            continue
        for r in range(n_boot):
            s = pd.Series(depth[r, a:b][keep].astype(np.int64))
            out[r, g] = {"p75": lambda: s.quantile(0.75), "mean": s.mean, "median": s.median}[select_mode]()
    return out
