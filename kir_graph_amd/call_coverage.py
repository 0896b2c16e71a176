"""
Per-allele coverage of a likelihood call (``--call-coverage``).

``--call-bootstrap`` and ``--call-fit`` reduce a gene to a few numbers.  This module says WHERE along the gene the support
of the called set lies -- a called allele with reads of its own over exons 1 - 5 and none behind them (a fusion), a called
copy with no reads of its own anywhere (one copy too many), the unexplained reads piled up in one intron (a variant the
index does not list) -- in exact integers, from the ``u8`` mismatch table ``miss8[column][read]`` the search left in HBM
(``DeviceModel.missFor``) joined with the sample's records, which stay in HBM for it.

1. the called set and its columns of the table (``call_report.calledSet``);
2. ``gk_call_coverage`` (``callcov_mark``, one scan, ``callcov_finish``): per read ``m1`` = the smallest byte over the
   called columns and ``A`` = the columns that hold it (``--call-fit``'s rule); the read's pair counts, with the M runs of
   both mates as in the depth of the sample, in the tracks ``informative`` (always), ``mismatch`` (``m1 > 0``), ``best_k``
   (``k`` in ``A``) and ``unique_k`` (``A == {k}``): ``depth[2 + 2K][length]``.  No search runs again;
3. on the host: the gene cut into ``upstream, exon1, intron1, ..., downstream`` (``regionsOf``), per region and track the
   summed depth and the positions covered, and per called allele its PRIVATE sites -- the index variants at which its
   membership differs from that of every other distinct called allele -- with those no read of its own covers.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from ._lib import check, lib
from .index import KEY_POS_SHIFT
from .utils import logger

CALL_COVERAGE_COLUMNS = ["gene", "cn", "reads", "region", "start", "end", "length", "informative_bases", "mismatch_bases",
                         "mismatch_covered", "allele", "copies", "best_bases", "unique_bases", "best_covered",
                         "unique_covered", "private_sites", "private_unsupported"]
CALL_COVERAGE_DEPTH_COLUMNS = ["gene", "track", "allele", "start", "end", "depth"]


@dataclass
class CallCoverage:
    """Coverage of one gene's called set.  ``alleles``: (name, copies) of the K distinct called alleles, ascending ordinal.
    ``depth[t][p]``: mates of track ``t`` whose aligned bases cover position ``p`` -- tracks 0 ``informative`` (every read
    of the model), 1 ``mismatch`` (reads the call does not fully explain), ``2 + k`` ``best_k`` (allele ``k`` is among the
    best of the set), ``2 + K + k`` ``unique_k`` (it alone is).  ``regions``: (name, start, end), 0-based half-open, the
    whole gene first.  ``bases[r][t]`` = the depth summed over region ``r``, ``covered[r][t]`` = its positions with depth
    > 0; ``private_sites[r][k]`` = the private sites of allele ``k`` in the region, ``private_unsupported[r][k]`` = those
    with ``unique_k`` depth 0."""

    cn: int
    reads: int
    length: int
    alleles: list[tuple[str, int]] = field(default_factory=list)
    depth: np.ndarray | None = None
    regions: list[tuple[str, int, int]] = field(default_factory=list)
    bases: np.ndarray | None = None
    covered: np.ndarray | None = None
    private_sites: np.ndarray | None = None
    private_unsupported: np.ndarray | None = None


def regionsOf(exons, length: int) -> list[tuple[str, int, int]]:
    """(name, start, end) of the regions of a backbone of ``length`` positions whose exons cover ``[s, e)`` (0-based, as
    ``index.readExons`` gives them): ``gene`` = everything first, then the maximal runs left to right -- ``upstream``,
    ``exon1``, ``intron1``, ..., ``exonN``, ``downstream`` -- each clipped to [previous end, length), empty ones dropped (a
    dropped exon still uses its number).  Without exons: ``gene`` alone."""
    length = int(length)
    regions = [("gene", 0, length)]
    prev = 0
    ordered = sorted((int(s), int(e)) for s, e in (exons or []))

    def add(name: str, a: int, b: int) -> None:
        nonlocal prev
        a, b = max(a, prev), min(b, length)
        if b > a:
            regions.append((name, a, b))
            prev = b

    for i, (s, e) in enumerate(ordered):
        add("upstream" if i == 0 else f"intron{i}", prev, s)
        add(f"exon{i + 1}", s, e)
    if ordered:
        add("downstream", prev, length)
    return regions


def privateSites(mask: np.ndarray, ids) -> list[np.ndarray]:
    """Per allele of ``ids`` (distinct ordinals) the rows of the bit rows ``mask`` [variants, words] at which its
    membership differs from that of EVERY other allele of ``ids``; with one allele there are none."""
    ids = np.asarray(ids, dtype=np.int64)
    if len(ids) < 2:
        return [np.zeros(0, dtype=np.int64) for _ in ids]
    mask = np.asarray(mask, dtype=np.uint32)
    bits = ((mask[:, ids >> 5] >> (ids & 31).astype(np.uint32)) & 1).astype(bool)      # [variants, K]
    carried = bits.sum(axis=1)
    k = len(ids)
    # allele j differs from all others: it alone carries the variant, or it alone does not
    return [np.flatnonzero(np.where(bits[:, j], carried == 1, carried == k - 1)) for j in range(k)]


def summarise(depth: np.ndarray, regions, sites: list[np.ndarray]):
    """(bases [R][T], covered [R][T], private_sites [R][K], private_unsupported [R][K]) of ``depth`` [2 + 2K][length];
    ``sites[k]``: the positions (clipped already) of allele ``k``'s private sites."""
    depth = np.asarray(depth)
    k = len(sites)
    starts = np.array([a for _, a, _ in regions], dtype=np.int64)
    ends = np.array([b for _, _, b in regions], dtype=np.int64)

    def perRegion(x: np.ndarray) -> np.ndarray:      # sums of x [T][length] over the regions, by prefix sums: [R][T]
        run = np.zeros((x.shape[0], x.shape[1] + 1), dtype=np.int64)
        np.cumsum(x, axis=1, dtype=np.int64, out=run[:, 1:])
        return (run[:, ends] - run[:, starts]).T

    bases, covered = perRegion(depth), perRegion(depth > 0)
    n_sites = np.zeros((len(regions), k), dtype=np.int64)
    unsupported = np.zeros((len(regions), k), dtype=np.int64)
    for j, pos in enumerate(sites):
        pos = np.asarray(pos, dtype=np.int64)
        bare = depth[2 + k + j][pos] == 0
        inside = (pos[None, :] >= starts[:, None]) & (pos[None, :] < ends[:, None])      # [R][sites]
        n_sites[:, j] = inside.sum(axis=1)
        unsupported[:, j] = (inside & bare[None, :]).sum(axis=1)
    return bases, covered, n_sites, unsupported


def coverageTracks(tab, mates, rows, n_rows: int, miss8, ldm: int, n_table_cols: int, cols: np.ndarray, gene: int,
                   gene_len: int) -> np.ndarray:
    """``gk_call_coverage``: ``uint32 [2 + 2K][gene_len]``.  ``mates``: the sample's records in HBM -- of
    ``packed.DeviceCompactMates`` the compact WORDS are passed (asking for ``.ptr`` would write the 128-byte records)."""
    cols = np.ascontiguousarray(cols, dtype=np.int32)
    depth = np.zeros((2 + 2 * len(cols), int(gene_len)), dtype=np.uint32)
    words = getattr(mates, "words", None) if hasattr(mates, "records") else None
    d_mates, d_compact = (0, words.ptr) if words is not None else (mates.ptr, 0)
    check(lib().gk_call_coverage(tab.dev.ctx, tab.handle, d_mates, d_compact, rows.ptr, n_rows, miss8.ptr, ldm, n_table_cols,
                                 cols.ctypes.data, len(cols), gene, int(gene_len), depth.ctypes.data))
    return depth


def coverCall(result, gene_len: int, exons, table, names=None) -> CallCoverage | None:
    """The coverage of one gene's adopted result (the last step's ``TypingResult``).  ``gene_len``: the backbone's length;
    ``exons``: its exons ``[(s, e)]`` (``index.readExons``); ``table``: its ``GeneTable`` (the bit rows name the private
    sites); ``names``: allele ordinal -> name, as ``call_fit.fitCall`` takes it (the called row names its own alleles: not
    needed here).  None -- with one warning --
    when the result's sets do not sit on one device table, the model has no mismatch table, more than 16 distinct alleles
    are called, or the sample has no records in HBM (a ``.json`` / CSR hand-off)."""
    called = calledSet(result, "call coverage", names, table=False)
    if called is None:
        return None
    tab = called.model.tab
    mates = getattr(getattr(tab, "_root", tab), "mates", None)
    host = getattr(getattr(tab, "dindex", None), "host", None)
    if mates is None or host is None or not tab.info.d_pair_src:
        logger.warning("[Allele] call coverage: the sample's records are not in HBM (a hand-off file, or released); skipped")
        return None
    called = called.withTable()
    if called is None:
        return None
    n, length = called.reads, int(gene_len)
    depth = coverageTracks(tab, mates, called.model.rows, n, called.miss8, called.ldm, called.n_table_cols, called.cols,
                           host.gene_id[table.name], length)
    regions = regionsOf(exons, length)
    pos = (host.key[table.vbeg:table.vend] >> np.uint64(KEY_POS_SHIFT)).astype(np.int64) & 0xFFFFFF
    sites = [np.minimum(pos[rows_k], length - 1) for rows_k in privateSites(table.mask, called.ids)]
    bases, covered, n_sites, unsupported = summarise(depth, regions, sites)
    return CallCoverage(cn=called.cn, reads=n, length=length, alleles=list(zip(called.labels, called.copies)), depth=depth,
                        regions=regions, bases=bases, covered=covered, private_sites=n_sites, private_unsupported=unsupported)


def callCoverageText(covers: dict[str, CallCoverage]) -> str:
    """``{result}.coverage.tsv``: tab separated, one row per gene, region and distinct called allele, the gene's and the
    region's cells repeated on each row; integers as integers; ``start`` / ``end`` 0-based half-open, ``length`` = end - start."""
    lines = ["\t".join(CALL_COVERAGE_COLUMNS)]
    for gene, c in covers.items():
        k = len(c.alleles)
        for r, (name, a, b) in enumerate(c.regions):
            head = [gene, c.cn, c.reads, name, a, b, b - a, int(c.bases[r, 0]), int(c.bases[r, 1]), int(c.covered[r, 1])]
            for j, (allele, copies) in enumerate(c.alleles):
                cells = head + [allele, copies, int(c.bases[r, 2 + j]), int(c.bases[r, 2 + k + j]), int(c.covered[r, 2 + j]),
                                int(c.covered[r, 2 + k + j]), int(c.private_sites[r, j]), int(c.private_unsupported[r, j])]
                lines.append("\t".join(str(x) for x in cells))
    return "\n".join(lines) + "\n"


def depthRuns(track: np.ndarray) -> list[tuple[int, int, int]]:
    """(start, end, depth) of the runs of equal depth of one track: 0-based half-open, ascending, tiling [0, length)."""
    track = np.asarray(track)
    if not len(track):
        return []
    starts = np.concatenate([[0], np.flatnonzero(track[1:] != track[:-1]) + 1])
    ends = np.concatenate([starts[1:], [len(track)]])
    return [(int(a), int(b), int(track[a])) for a, b in zip(starts, ends)]


def callCoverageDepthText(covers: dict[str, CallCoverage]) -> str:
    """``{result}.coverage.depth.tsv``: the tracks as runs of equal depth (``depthRuns``), per gene in the order
    ``informative``, ``mismatch``, ``best`` of every called allele, ``unique`` of every called allele; the ``allele`` cell
    is empty for the first two."""
    lines = ["\t".join(CALL_COVERAGE_DEPTH_COLUMNS)]
    for gene, c in covers.items():
        k = len(c.alleles)
        labels = [("informative", ""), ("mismatch", "")] + [("best", a) for a, _ in c.alleles] + [("unique", a) for a, _ in c.alleles]
        assert len(labels) == 2 + 2 * k == len(c.depth)
        for (track, allele), d in zip(labels, c.depth):
            for a, b, x in depthRuns(d):
                lines.append(f"{gene}\t{track}\t{allele}\t{a}\t{b}\t{x}")
    return "\n".join(lines) + "\n"


# at the end, not at the top: call_report's table of reports names this module, and whichever of the two is imported first
# finds what it needs of the other already defined
from .call_report import calledSet  # noqa: E402
