"""numpy restatements of the row selections and of the plain depth (csrc/gk_scan.hip behind gk_select_nonempty, part_pass /
part_offsets behind gk_select_gene, csrc/gk_depth.hip): what the kernels must return, each as one obvious expression.  Slow
and plain on purpose."""
import numpy as np


def packLists(rows):
    """CSR of rows of four id lists (lpv, rpv, lnv, rnv): (off uint32 [4 n + 1], ids uint32)."""
    off, ids = [0], []
    for four in rows:
        assert len(four) == 4
        for one in four:
            ids += [int(v) for v in one]
            off.append(len(ids))
    return np.array(off, dtype=np.uint32), np.array(ids, dtype=np.uint32)


def aliveRows(off, ids, vflag):
    """bool [n_rows]: the row has an id that survives its drop flag -- bit 0 for the positive ids (those before
    off[4 row + 2]), bit 1 for the rest."""
    n = (len(off) - 1) // 4
    return np.array([any(not (int(vflag[ids[k]]) & (1 if k < off[4 * r + 2] else 2)) for k in range(off[4 * r], off[4 * r + 4]))
                     for r in range(n)], dtype=bool)


def selectRows(rows, alive):
    """The rows that survive, in the order given."""
    rows = np.asarray(rows)
    return rows[alive[rows]]


def genePartition(gene, nh, g, multiple):
    """The rows of backbone g in ascending order; without ``multiple`` only those with NH == 1."""
    return np.flatnonzero((np.asarray(gene) == g) & (bool(multiple) | (np.asarray(nh) == 1)))


def depth(marks, total):
    """int64 [total]: the depth from the (position, +1 / -1) marks of depthboot_reference.pairMarks."""
    diff = np.zeros(total + 1, dtype=np.int64)
    for pair in marks:
        for at, sign in pair:
            diff[at] += sign
    return np.cumsum(diff)[:total]
