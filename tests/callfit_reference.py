"""numpy restatement of the fit report's two kernels (csrc/gk_callfit.hip, include/graphkir_hip.h): what gk_call_fit and
gk_call_fit_extra must return, in exact integers.  ``table`` is the mismatch table [columns][rows] (rows beyond ``n_rows``
are cut off by the caller)."""
import numpy as np


def profile(table, cols):
    """(hist [18], M, per listed column [K, 3] = best / unique / only, d_min [rows]) of the listed columns."""
    b = np.asarray(table, dtype=np.int64)[np.asarray(cols, dtype=np.int64)].T          # [rows, K]
    n, k = b.shape
    m1 = b.min(axis=1)
    tie = b == m1[:, None]                                                              # A as a mask
    single = tie.sum(axis=1) == 1
    second = np.sort(b, axis=1)[:, 1] if k > 1 else m1                                  # the second value when |A| == 1
    bins = np.where(m1 < 16, m1, np.where(m1 == 255, 17, 16))
    hist = np.bincount(bins, minlength=18)
    alone = tie & single[:, None]
    per_col = np.stack([tie.sum(axis=0), alone.sum(axis=0), (alone * (second - m1)[:, None]).sum(axis=0)], axis=1)
    return hist.astype(np.int64), int(m1.sum()), per_col.astype(np.int64), m1


def extra(table, m1):
    """with[a] = sum_r min(m1[r], table[a][r]) of every column."""
    t = np.asarray(table, dtype=np.int64)
    return np.minimum(m1[:, None], t.T).sum(0)
