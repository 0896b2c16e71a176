"""tests/select_reference.py against cases small enough to work out by hand."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import select_reference as sr  # noqa: E402

# row 0: nothing; row 1: +0; row 2: -1; row 3: +2 and -2; row 4: +3 (left) and +4 (right)
ROWS = [[[], [], [], []], [[0], [], [], []], [[], [], [], [1]], [[2], [], [2], []], [[3], [4], [], []]]


def test_pack_lists():
    off, ids = sr.packLists(ROWS)
    assert off.dtype == np.uint32 and ids.dtype == np.uint32
    assert off.tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 2, 3, 3, 4, 4, 5, 6, 6, 6]
    assert ids.tolist() == [0, 1, 2, 2, 3, 4]


def test_alive_rows_by_hand():
    off, ids = sr.packLists(ROWS)
    alive = lambda flags: sr.aliveRows(off, ids, np.array(flags, dtype=np.uint8)).tolist()      # noqa: E731
    assert alive([0, 0, 0, 0, 0]) == [False, True, True, True, True]
    assert alive([3, 3, 3, 3, 3]) == [False] * 5
    assert alive([1, 1, 1, 1, 1]) == [False, False, True, True, False]       # bit 0 drops positive ids only
    assert alive([2, 2, 2, 2, 2]) == [False, True, False, True, True]        # bit 1 drops negative ids only
    assert alive([2, 1, 0, 0, 0]) == [False, True, True, True, True]         # the wrong bit for the id's side: kept
    assert alive([0, 0, 3, 1, 0]) == [False, True, True, False, True]        # row 4 lives on its second id
    assert alive([0, 0, 0, 1, 1]) == [False, True, True, True, False]


def test_select_rows_keeps_order_and_repeats():
    alive = np.array([False, True, True, False, True])
    rows = np.array([4, 0, 1, 1, 3, 2, 4, 0], dtype=np.int32)
    assert sr.selectRows(rows, alive).tolist() == [4, 1, 1, 2, 4]
    assert sr.selectRows(rows[:0], alive).tolist() == []
    assert sr.selectRows(np.array([0, 3, 3]), alive).tolist() == []


def test_gene_partition_by_hand():
    gene = np.array([5, 0, 255, 5, 5, 0, 255], dtype=np.uint8)
    nh = np.array([1, 2, 1, 2, 1, 1, 2], dtype=np.uint8)
    assert sr.genePartition(gene, nh, 5, 0).tolist() == [0, 4]
    assert sr.genePartition(gene, nh, 5, 1).tolist() == [0, 3, 4]
    assert sr.genePartition(gene, nh, 0, 0).tolist() == [5]
    assert sr.genePartition(gene, nh, 0, 1).tolist() == [1, 5]
    assert sr.genePartition(gene, nh, 255, 0).tolist() == [2]
    assert sr.genePartition(gene, nh, 255, 1).tolist() == [2, 6]
    assert sr.genePartition(gene, nh, 7, 1).tolist() == []


def test_depth_by_hand():
    # pair 0: [1, 4) and [3, 6); pair 1: nothing; pair 2: [5, 6), clipped at the end of the space
    marks = [[(1, 1), (4, -1), (3, 1), (6, -1)], [], [(5, 1), (6, -1)]]
    got = sr.depth(marks, 6)
    assert got.dtype == np.int64 and got.tolist() == [0, 1, 1, 2, 1, 2]
    assert sr.depth([], 3).tolist() == [0, 0, 0]
    assert sr.depth([[(0, 1), (1, -1)]] * 5, 1).tolist() == [5]


def test_depth_marks_of_a_record():
    """With the marks of depthboot_reference.pairMarks: one pair on two backbones, M / D / M and a clipped run."""
    import depthboot_reference as dr
    from kir_graph_amd import _lib
    rec = np.zeros(2, dtype=_lib.MATE_DTYPE)
    rec["pos0"] = [2, 1]
    rec["ref"] = [0, 1]
    rec["n_cig"] = [3, 1]
    rec["cig"][0][:3] = [(3 << 4) | 0, (2 << 4) | 2, (2 << 4) | 0]        # 3M 2D 2M from 2: [2, 5) and [7, 9)
    rec["cig"][1][:1] = [(10 << 4) | 0]                                 # 10M from 1 on a backbone of 4: [1, 4)
    gene_off = np.array([0, 8, 12], dtype=np.int64)
    marks = dr.pairMarks(rec, [0], [1], 0, gene_off)
    assert sr.depth(marks, 12).tolist() == [0, 0, 1, 1, 1, 0, 0, 1] + [0, 1, 1, 1]
    assert sr.depth(dr.pairMarks(rec, [0], [2], 0, gene_off), 12).tolist() == [0] * 12         # NH == 2 without `multiple`
    assert sr.depth(dr.pairMarks(rec, [0], [2], 1, gene_off), 12).tolist() == [0, 0, 1, 1, 1, 0, 0, 1] + [0, 1, 1, 1]
    assert sr.depth(dr.pairMarks(rec, [0], [1], 0, gene_off[:2]), 8).tolist() == [0, 0, 1, 1, 1, 0, 0, 1]      # one backbone known
