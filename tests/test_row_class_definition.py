"""The definition the row classes rest on (csrc/gk_rowclass.hip), on the CPU: rows of equal KEPT (id, sign) sequence
(tests/rowclass_reference.py) have equal rows in the reference table of tests/compat_reference.py -- products, counts and
kept ids, bit for bit -- whatever else differs between them; and the neighbours that must NOT merge do differ in the
table for some bit rows."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import compat_reference as cr  # noqa: E402
import rowclass_reference as rr  # noqa: E402


def table(lists, bits, vflag=None, keep_empty=False):
    off, ids, rows = rr.packed(lists, filler_every=3)
    vflag = rr.geneFlags() if vflag is None else vflag
    ref = cr.compatReference(off, ids, rows, vflag, rr.VBEG, rr.VEND, bits, keep_empty)
    return ref, rr.classOf(off, ids, rows, vflag)


def test_equal_kept_sequences_have_equal_reference_rows():
    rng = np.random.default_rng(77)
    bits = rr.geneBits(70)
    lists = []
    for _ in range(60):
        pos = rng.permutation(rr.KEEPABLE)[:rng.integers(0, 9)].tolist()
        neg = rng.permutation(rr.KEEPABLE)[:rng.integers(0, 9)].tolist()
        if rng.random() < 0.3:
            pos.append(int(rng.choice([2, 315, 350])))          # an id outside the gene's span: a factor like any other
        for _ in range(3):      # the same kept sequence three times: other dropped ids between, another split of the mates
            p, q = list(pos), list(neg)
            for d in rng.permutation(rr.DROPPED)[:rng.integers(0, 5)].tolist():
                p.insert(int(rng.integers(0, len(p) + 1)), d)
            for d in rng.permutation(rr.DROPPED)[:rng.integers(0, 5)].tolist():
                q.insert(int(rng.integers(0, len(q) + 1)), d)
            p += [105, 107][:rng.integers(0, 3)]                 # kept: these are dropped from negative lists only
            q += [100, 101][:rng.integers(0, 3)]
            cp, cq = int(rng.integers(0, len(p) + 1)), int(rng.integers(0, len(q) + 1))
            lists.append([p[:cp], p[cp:], q[:cq], q[cq:]])
    order = rng.permutation(len(lists))
    lists = [lists[k] for k in order]
    ref, cls = table(lists, bits)
    assert 1 < cls.max() + 1 < len(lists)
    for c in range(cls.max() + 1):
        members = np.flatnonzero(cls == c)
        for m in members[1:]:
            assert np.array_equal(ref.probs[m].view(np.uint64), ref.probs[members[0]].view(np.uint64))
            assert np.array_equal(ref.miss[m], ref.miss[members[0]]) and ref.nvar[m] == ref.nvar[members[0]]


def test_neighbours_that_are_other_classes():
    a, b, c, d, e = 12, 13, 14, 15, 16
    pairs = {
        "boundary one place apart": ([[a, b, c], [], [d, e], []], [[a, b], [], [c, d, e], []]),
        "another order": ([[a, b, c], [], [d], []], [[a, c, b], [], [d], []]),
        "one id outside the span more": ([[a, b], [], [d], []], [[a, b, 2], [], [d], []]),
        "positive here, negative there": ([[a, b], [], [], []], [[a], [], [b], []]),
    }
    bits = rr.geneBits(70)
    for name, (x, y) in pairs.items():
        ref, cls = table([x, y], bits)
        assert cls.tolist() == [0, 1], name
        if name != "another order":      # the order only shows in the rounding of a long product: not in these three factors
            assert not np.array_equal(ref.probs[0], ref.probs[1]), name


def test_rows_that_keep_nothing_are_one_class_of_the_empty_value():
    lists = [[[], [], [], []], [rr.DROPPED[:5], [], rr.DROPPED[5:9], []], [[100, 104], [], [105], [109]]]
    for keep_empty in (False, True):
        ref, cls = table(lists, rr.geneBits(5), keep_empty=keep_empty)
        assert cls.tolist() == [0, 0, 0] and not ref.nvar.any()
        assert (ref.probs == (cr.HIT if keep_empty else 1.0)).all()
