"""numpy restatement of the alternatives of a called allele (csrc/gk_callswap.hip, include/graphkir_hip.h): what gk_call_swap
must return, in exact integers, by brute force.  ``table`` is the mismatch table [columns][rows] (rows beyond ``n_rows`` are
cut off by the caller).  For every called column k and every column a of the table the column list is formed with k
replaced by a and the row minima are taken: no m1 / m2 / own shortcut."""
import numpy as np


def swaps(table, cols):
    """dict: loss [K, A], rows_for [K, A], gain [A], rows_against [A], delta [K, A], m, out_of_range."""
    t = np.asarray(table, dtype=np.int64)
    cols = [int(c) for c in cols]
    n_table_cols, n_rows = t.shape
    k_n = len(cols)
    m1 = t[cols].min(axis=0)
    m = int(m1.sum())
    loss, rows_for = np.zeros((k_n, n_table_cols), dtype=np.int64), np.zeros((k_n, n_table_cols), dtype=np.int64)
    gain, against = np.zeros((k_n, n_table_cols), dtype=np.int64), np.zeros((k_n, n_table_cols), dtype=np.int64)
    for k in range(k_n):
        kept = [c for j, c in enumerate(cols) if j != k]
        # the list with k replaced by a is `kept` and a, for every a at once: min over `kept` (a set of one allele has
        # nothing kept, and 255 is the largest byte), then the minimum with column a
        rest = t[kept].min(axis=0) if kept else np.full(n_rows, 255, dtype=np.int64)
        new = np.minimum(rest[None, :], t)                                  # [A, rows]
        diff = new - m1[None, :]
        loss[k] = np.maximum(diff, 0).sum(axis=1)
        rows_for[k] = (diff > 0).sum(axis=1)
        gain[k] = np.maximum(-diff, 0).sum(axis=1)
        against[k] = (diff < 0).sum(axis=1)
        assert np.array_equal(loss[k] - gain[k], new.sum(axis=1) - m)      # delta = M(S(k -> a)) - M(S)
    # what a column takes from the call does not depend on the allele it replaces
    assert (gain == gain[0]).all() and (against == against[0]).all()
    return {"loss": loss, "rows_for": rows_for, "gain": gain[0], "rows_against": against[0], "delta": loss - gain[0], "m": m,
            "out_of_range": int((m1 == 255).sum())}


def swapOne(table, cols, k, a):
    """(loss, rows_for, gain, rows_against, delta) of ONE swap, literally: the column list with cols[k] replaced by a."""
    t = np.asarray(table, dtype=np.int64)
    m1 = t[[int(c) for c in cols]].min(axis=0)
    new = t[[int(a) if j == k else int(c) for j, c in enumerate(cols)]].min(axis=0)
    out = (int(np.maximum(new - m1, 0).sum()), int((new > m1).sum()), int(np.maximum(m1 - new, 0).sum()), int((new < m1).sum()))
    assert out[0] - out[2] == int(new.sum() - m1.sum())
    return out + (out[0] - out[2],)


def rowState(table, cols):
    """(m1, m2, own) per row as callswap_rows leaves them: m2 = the smallest byte outside the unique holder of m1 (255 for
    one listed column, m1 on a tie), own = the index of the unique holder, 255 on a tie."""
    b = np.asarray(table, dtype=np.int64)[[int(c) for c in cols]]           # [K, rows]
    m1 = b.min(axis=0)
    hit = b == m1[None, :]
    single = hit.sum(axis=0) == 1
    second = np.sort(b, axis=0)[1] if len(cols) > 1 else np.full(b.shape[1], 255, dtype=np.int64)
    return m1, np.where(single, second, m1), np.where(single, hit.argmax(axis=0), 255)
