"""GPU: the grid of the copy-number fit (csrc/gk_cn.hip: cn_fit_kernel, one workgroup of 256 threads per candidate base, and
cn_assign_kernel, one thread per bin) against the 40-digit decimal reference of tests/cn_reference.py, at every bins /
n_bases / n_cn / first_cn the entry points take and at the values where the arithmetic has an edge.

Launch arithmetic, read from gk_cn_fit / cn_fit_kernel: thread t of a workgroup takes bins t, t + 256, ...; bins < 256 (1, 2,
255) leave threads without a bin, whose zero partial sums the LDS tree still adds; bins = 256 fills every thread once; bin 256
(bins = 257, 300, 513) is thread 0's second trip -- the ``lane256`` cases put the whole histogram there, ``lane255`` in the last
thread's only bin; bins = 513 gives thread 0 a third trip.  cn_assign_kernel launches ceil(bins / 256) workgroups.

Tolerance of gk_cn_fit, relative to S = sum |term|: eight times the error of the float64 numpy restatement against the decimal
reference, measured over the case list of cn_reference.py by

    python tests/cn_reference.py

and never less than 8 * 2^-53.  The factor covers device exp / log being one to two ulp where numpy's are one, and the other
order of the tree reduction."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cn_reference as cr  # noqa: E402

from kir_graph_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

CN_FIT_MEASURED = 3.971284757253312e-16                       # max |float64 restatement - decimal| / S, all cases
CN_FIT_BOUND = max(8 * CN_FIT_MEASURED, 8 * 2.0 ** -53)       # = 3.177e-15, what the kernel is allowed relative to S
GK_ERR_ARG = -3
SENTINEL = -12345.678
SENTINEL32 = 0x5A5A5A5A - (1 << 31)
TAIL = 8


def baseGap(ref):
    """The distance of the two largest likelihoods over the bases, relative to the largest S (inf with one base)."""
    if len(ref.loglik) < 2:
        return float("inf")
    top = sorted(ref.loglik)[-2:]
    scale = max(ref.S)
    return 0.0 if scale == 0 else float((top[1] - top[0]) / scale)


def fit(device, case, n_bases=None, n_cn=None, bins=None):
    out = np.full(case.n_bases + TAIL, SENTINEL, dtype=np.float64)
    rc = _lib.lib().gk_cn_fit(device.ctx, case.x.ctypes.data, case.density.ctypes.data, case.bins if bins is None else bins,
                              case.bases.ctypes.data, case.n_bases if n_bases is None else n_bases, case.dev.ctypes.data,
                              case.n_cn if n_cn is None else n_cn, case.first_cn, case.space, out.ctypes.data)
    return rc, out


def assign(device, case, base, n_cn=None, bins=None):
    out = np.full(case.bins + TAIL, SENTINEL32, dtype=np.int32)
    rc = _lib.lib().gk_cn_assign(device.ctx, case.x.ctypes.data, case.bins if bins is None else bins, float(base),
                                 case.dev.ctypes.data, case.n_cn if n_cn is None else n_cn, case.first_cn, case.space,
                                 out.ctypes.data)
    return rc, out


@pytest.mark.parametrize("name", [c.name for c in cr.cases()])
def test_fit_and_assign_equal_the_decimal_reference(device, name):
    case = next(c for c in cr.cases() if c.name == name)
    ref = cr.referenceOf(name)
    rc, out = fit(device, case)
    _lib.check(rc)
    got = out[:case.n_bases]
    assert (out[case.n_bases:] == SENTINEL).all()
    worst = cr.relativeError(got, ref)              # asserts an exact 0.0 wherever S == 0
    print(f"{name}: |kernel - decimal| / S = {worst:.3e} (bound {CN_FIT_BOUND:.3e}), "
          f"float64 restatement {cr.relativeError(cr.float64Loglik(case), ref):.3e}")
    assert worst <= CN_FIT_BOUND
    if case.kind == "zeros":
        assert all(float(v).hex() == (0.0).hex() for v in got)
    # the best base: excused only where the two best are within the tolerance; equal bases give equal values
    want_best = max(range(case.n_bases), key=lambda j: ref.loglik[j])
    if baseGap(ref) > CN_FIT_BOUND:
        assert int(np.argmax(got)) == want_best
    elif len(set(case.bases.tolist())) == 1:
        assert len(set(got.tolist())) == 1 and int(np.argmax(got)) == want_best == 0
    # the copy number of every bin, at every base
    excused = ref.gap <= cr.EXCUSE_GAP
    for j, b in enumerate(case.bases):
        rc, cn = assign(device, case, b)
        _lib.check(rc)
        assert (cn[case.bins:] == SENTINEL32).all()
        if case.kind == "tie":                     # every candidate equal in every bin: the first maximum, row 0
            assert excused[j].all() and not cn[:case.bins].any()
        else:
            assert not excused[j].any()
            assert np.array_equal(cn[:case.bins], ref.argmax[j]), (name, j)


def test_production_shape_equals_the_float64_restatement(device):
    """bins = n_bases = 300, n_cn = 7, first_cn = 0: 630 000 candidates are too many for the decimal reference inside a test,
    so the float64 restatement (oracle/cn.py's arithmetic) stands in, S in doubles, under the same tolerance."""
    case = cr.productionCase()
    want = cr.float64Loglik(case)
    S = np.array([np.sum(np.abs(np.log(cr.float64Table(case, b).max(axis=0) + cr.EPS) * case.density)) for b in case.bases])
    rc, out = fit(device, case)
    _lib.check(rc)
    assert (out[case.n_bases:] == SENTINEL).all() and (S > 0).all()
    err = np.abs(out[:case.n_bases] - want) / S
    print(f"production shape: max |kernel - float64| / S = {err.max():.3e} (bound {CN_FIT_BOUND:.3e})")
    assert err.max() <= CN_FIT_BOUND
    order = np.sort(want)
    if (order[-1] - order[-2]) / S.max() > CN_FIT_BOUND:
        assert int(np.argmax(out[:case.n_bases])) == int(np.argmax(want))
    best = float(case.bases[int(np.argmax(want))])
    rc, cn = assign(device, case, best)
    _lib.check(rc)
    table = cr.float64Table(case, best)
    top = np.sort(table, axis=0)
    clear = (top[-1] - top[-2]) > cr.EXCUSE_GAP * top[-1]
    assert clear.sum() >= case.bins - 8 and (cn[case.bins:] == SENTINEL32).all()
    assert np.array_equal(cn[:case.bins][clear], table.argmax(axis=0)[clear])


def test_refusals_write_nothing(device):
    case = next(c for c in cr.cases() if c.name == "two_peak-300x8x7+0")
    wide = cr.Case("wide", "two_peak", case.x, case.density, case.bases, np.full(17, 1.0), 0, case.space)
    lib = _lib.lib()
    for what, (rc, out) in {
        "n_cn = 0": fit(device, case, n_cn=0), "n_cn = 17": fit(device, wide), "bins = 0": fit(device, case, bins=0),
        "n_bases = 0": fit(device, case, n_bases=0), "bins < 0": fit(device, case, bins=-1),
    }.items():
        assert rc == GK_ERR_ARG and b"bad CN fit geometry" in lib.gk_last_error(), what
        assert (out == SENTINEL).all(), what
    for what, (rc, out) in {
        "n_cn = 0": assign(device, case, 1.0, n_cn=0), "n_cn = 17": assign(device, wide, 1.0),
        "bins = 0": assign(device, case, 1.0, bins=0),
    }.items():
        assert rc == GK_ERR_ARG and b"bad CN assign arguments" in lib.gk_last_error(), what
        assert (out == SENTINEL32).all(), what
    # the context still works, and 16 candidates are taken
    ok = next(c for c in cr.cases() if c.name == "two_peak-256x3x16+2")
    rc, out = fit(device, ok)
    _lib.check(rc)
    assert cr.relativeError(out[:ok.n_bases], cr.referenceOf(ok.name)) <= CN_FIT_BOUND
