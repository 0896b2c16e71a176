"""numpy / plain-Python restatement of the per-allele coverage of a call (csrc/gk_callcov.hip, include/graphkir_hip.h,
kir_graph_amd/call_coverage.py): what gk_call_coverage must return and what the host makes of it, in exact integers.  Slow
and plain on purpose: one loop per mate, per position and per site."""
import numpy as np

SPILLED, CIG_M, CIG_D = 0xFF, 0, 2
COLUMNS = ("gene cn reads region start end length informative_bases mismatch_bases mismatch_covered allele copies best_bases "
           "unique_bases best_covered unique_covered private_sites private_unsupported").split()
DEPTH_COLUMNS = "gene track allele start end depth".split()


def mateRuns(rec, wide=None):
    """The M runs [(start, end)] of one 128-byte record (``_lib.MATE_DTYPE``), unclipped.  ``wide``: for a record with
    ``n_cig == 0xFF`` the wide record (``_lib.MATE_WIDE_DTYPE``) that holds its CIGAR -- number ``2 * ins[0] + side`` of the
    sample's; None: such a mate has no runs."""
    if int(rec["n_cig"]) == SPILLED:
        if wide is None:
            return []
        ops = [(int(c) & 15, int(c) >> 4) for c in wide["cig"][:min(int(wide["n_cig"]), 128)]]
    else:
        ops = [(int(c) & 15, int(c) >> 4) for c in rec["cig"][:min(int(rec["n_cig"]), 14)]]
    cur, runs = int(rec["pos0"]), []
    for op, n in ops:
        if op == CIG_M:
            runs.append((cur, cur + n))
            cur += n
        elif op == CIG_D:
            cur += n
    return runs


def tieSets(table, cols):
    """(m1 [rows], tie [rows, K] bool) of the listed columns of ``table`` [columns][rows]: bytes as stored."""
    b = np.asarray(table, dtype=np.int64)[np.asarray(cols, dtype=np.int64)].T
    m1 = b.min(axis=1)
    return m1, b == m1[:, None]


def tracks(records, pair_src, rows, table, cols, gene, gene_len, wide=None):
    """int64 [2 + 2K][gene_len]: row r of ``table`` belongs to the valid pair ``rows[r]`` = input pair
    ``pair_src[rows[r]]`` = records 2 p and 2 p + 1."""
    k = len(cols)
    m1, tie = tieSets(table, cols)
    diff = np.zeros((2 + 2 * k, gene_len + 1), dtype=np.int64)
    for r, row in enumerate(np.asarray(rows).tolist()):
        member = [True, bool(m1[r] > 0)] + tie[r].tolist() + (tie[r] & (tie[r].sum() == 1)).tolist()
        on = np.flatnonzero(member)
        p = int(pair_src[row])
        for side in (0, 1):
            rec = records[2 * p + side]
            if int(rec["ref"]) != gene:
                continue
            far = wide[2 * int(rec["ins"][0]) + side] if wide is not None and int(rec["n_cig"]) == SPILLED else None
            for a, b in mateRuns(rec, far):
                a, b = max(a, 0), min(b, gene_len)
                if b > a:
                    diff[on, a] += 1
                    diff[on, b] -= 1
    return np.cumsum(diff, axis=1)[:, :gene_len]


def regions(exons, length):
    """[(name, start, end)]: the gene, then upstream / exon i / intron i / downstream, clipped and non-empty."""
    out = [("gene", 0, length)]
    exons = sorted((int(s), int(e)) for s, e in exons)
    if not exons:
        return out
    label = ["?"] * length                       # the region of every position, written left to right, first writer wins
    taken = 0
    for i, (s, e) in enumerate(exons):
        for p in range(taken, min(max(s, taken), length)):
            label[p] = "upstream" if i == 0 else f"intron{i}"
        taken = max(taken, min(s, length))
        for p in range(max(s, taken), min(e, length)):
            label[p] = f"exon{i + 1}"
        taken = max(taken, min(e, length))
    for p in range(taken, length):
        label[p] = "downstream"
    start = 0
    for p in range(1, length + 1):
        if p == length or label[p] != label[start]:
            out.append((label[start], start, p))
            start = p
    return out


def privateSites(mask, ids):
    """Per allele of ``ids`` the variant rows at which its bit differs from the bit of every other allele of ``ids``."""
    out = []
    for a in ids:
        mine = []
        for v in range(len(mask)):
            bit = lambda x: (int(mask[v][x >> 5]) >> (x & 31)) & 1      # noqa: E731
            if len(ids) > 1 and all(bit(a) != bit(o) for o in ids if o != a):
                mine.append(v)
        out.append(mine)
    return out


def summary(depth, regs, site_pos):
    """Per region: (bases [T], covered [T], private sites [K], unsupported private sites [K])."""
    k = len(site_pos)
    out = []
    for _, a, b in regs:
        bases = [int(sum(int(x) for x in d[a:b])) for d in depth]
        covered = [int(sum(1 for x in d[a:b] if x > 0)) for d in depth]
        sites = [sum(1 for p in site_pos[j] if a <= p < b) for j in range(k)]
        bare = [sum(1 for p in site_pos[j] if a <= p < b and depth[2 + k + j][p] == 0) for j in range(k)]
        out.append((bases, covered, sites, bare))
    return out


def coverageText(entries):
    """entries: [(gene, cn, reads, [(allele, copies)], regs, summary)] -> the text of {result}.coverage.tsv."""
    lines = ["\t".join(COLUMNS)]
    for gene, cn, reads, alleles, regs, summ in entries:
        k = len(alleles)
        for (name, a, b), (bases, covered, sites, bare) in zip(regs, summ):
            for j, (allele, copies) in enumerate(alleles):
                cells = [gene, cn, reads, name, a, b, b - a, bases[0], bases[1], covered[1], allele, copies, bases[2 + j],
                         bases[2 + k + j], covered[2 + j], covered[2 + k + j], sites[j], bare[j]]
                lines.append("\t".join(str(c) for c in cells))
    return "\n".join(lines) + "\n"


def depthText(entries):
    """entries: [(gene, [(allele, copies)], depth [2 + 2K][length])] -> the text of {result}.coverage.depth.tsv."""
    lines = ["\t".join(DEPTH_COLUMNS)]
    for gene, alleles, depth in entries:
        names = [a for a, _ in alleles]
        labels = [("informative", ""), ("mismatch", "")] + [("best", a) for a in names] + [("unique", a) for a in names]
        for (track, allele), d in zip(labels, depth):
            start = 0
            for p in range(1, len(d) + 1):
                if p == len(d) or d[p] != d[start]:
                    lines.append(f"{gene}\t{track}\t{allele}\t{start}\t{p}\t{int(d[start])}")
                    start = p
    return "\n".join(lines) + "\n"


def expandDepthText(text):
    """The depth file back as {(gene, track, allele): int64 [length]}; asserts that the runs tile from 0 without gaps."""
    rows = [line.split("\t") for line in text.split("\n")[1:] if line]
    out = {}
    for gene, track, allele, a, b, x in rows:
        key = (gene, track, allele)
        have = out.setdefault(key, [])
        assert int(a) == len(have) and int(b) > int(a), (key, a, b)
        have.extend([int(x)] * (int(b) - int(a)))
    return {key: np.array(v, dtype=np.int64) for key, v in out.items()}
