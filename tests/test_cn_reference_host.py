"""tests/cn_reference.py: the decimal reference of the copy-number grid against mpmath and against the float64 restatement of
oracle/cn.py, the case list it is used on, and the tolerance that tests/test_gpu_cn_fit.py derives from it."""
import os
import sys
from decimal import Decimal

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cn_reference as cr  # noqa: E402
import test_gpu_cn_fit as gpu_test  # noqa: E402

from oracle import cn as ocn  # noqa: E402


def test_case_list_covers_every_value_of_every_axis():
    cases = cr.cases()
    assert {c.bins for c in cases} == set(cr.BINS) and {c.n_bases for c in cases} == set(cr.N_BASES)
    assert {c.n_cn for c in cases} == set(cr.N_CN) and {c.first_cn for c in cases} == set(cr.FIRST_CN)
    assert {c.kind for c in cases} == {"two_peak", "zeros", "lane255", "lane256", "underflow_all", "underflow_part", "base0", "tie"}
    for c in cases:
        if c.kind == "two_peak" and c.bins > 2:
            filled = np.flatnonzero(c.density)
            assert c.density.sum() == 100 and len(filled) > 3 and filled.max() - filled.min() > c.bins // 4
        if c.kind.startswith("lane"):
            assert np.flatnonzero(c.density).tolist() == [int(c.kind[4:])]
        if c.kind in ("base0", "tie"):
            assert not c.bases.any()


@pytest.mark.parametrize("name", ["two_peak-2x3x7+1", "lane255-256x3x7+0", "underflow_part-257x8x1+2", "underflow_all-255x1x16+2"])
def test_decimal_equals_mpmath(name):
    mp = pytest.importorskip("mpmath")
    case = next(c for c in cr.cases() if c.name == name)
    ref = cr.referenceOf(name)
    with mp.workdps(60):
        C, eps, space = mp.mpf(cr.SQRT_2PI), mp.mpf(cr.EPS), mp.mpf(case.space)
        for j, b in enumerate(case.bases):
            acc = mp.mpf(0)
            for i in range(case.bins):
                best = max(mp.exp(-(((mp.mpf(float(case.x[i])) - mp.mpf(float(b)) * (case.first_cn + k)) / mp.mpf(float(d))) ** 2) / 2)
                           / C / mp.mpf(float(d)) * space for k, d in enumerate(case.dev))
                acc += mp.log(best + eps) * mp.mpf(float(case.density[i]))
            want = Decimal(mp.nstr(acc, 50))
            assert abs(want - ref.loglik[j]) <= Decimal("1e-36") * ref.S[j], (name, j)


def test_float64_restatement_is_the_oracle():
    """On the model's own geometry the numpy restatement is oracle/cn.py's table and likelihood, bit for bit."""
    case = cr.productionCase()
    model = ocn.LCND()
    model.x_max = float(case.x[-1])
    model.base_dev *= model.x_max
    assert np.array_equal(np.linspace(0, model.x_max, model.bin_num), case.x) and case.space == model.x_max / model.bin_num
    for b in case.bases[[0, 1, 77, 299]]:
        assert np.array_equal(model.groupProb(b), cr.float64Table(case, b))
    mine = cr.float64Loglik(case)
    theirs = np.array([np.sum(np.log(model.groupProb(b).max(axis=0) + 1e-9) * case.density) for b in case.bases])
    assert np.array_equal(mine, theirs)


def test_special_values():
    for c in cr.cases():
        ref = cr.referenceOf(c.name)
        f64 = cr.float64Loglik(c)
        if c.kind == "zeros":
            assert all(v == 0 for v in ref.loglik) and all(s == 0 for s in ref.S) and not f64.any()
        if c.kind == "underflow_all":            # every term is log(1e-9) density, and the nearest mean is k = 0
            want = np.log(cr.EPS) * c.density.sum()
            assert not cr.float64Table(c, c.bases[0]).any()
            assert all(abs(float(v) - want) <= 1e-15 * abs(want) for v in ref.loglik) and not ref.argmax.any()
        if c.kind == "underflow_part":
            table = cr.float64Table(c, c.bases[0])
            assert (table == 0).any() and (table > 1e-3).any()
        if c.kind == "tie":
            assert not ref.argmax.any() and not ref.gap.any()


def test_no_bin_is_excused_outside_the_tie_cases():
    """So the GPU test leaves no bin out; and numpy's own argmax already agrees with the reference everywhere."""
    for c in cr.cases():
        ref = cr.referenceOf(c.name)
        excused = ref.gap <= cr.EXCUSE_GAP
        if c.kind == "tie":
            assert excused.all()
        else:
            assert not excused.any(), c.name
        for j, b in enumerate(c.bases):
            assert np.array_equal(cr.float64Table(c, b).argmax(axis=0), ref.argmax[j]), (c.name, j)


def test_best_base_is_clear_or_an_exact_tie():
    """Over the bases the two largest likelihoods are either further apart than twice the kernel's bound (relative to S), or
    equal because the bases are, or equal to every digit a double has: no case lies where the GPU test's excuse for the
    argmax over bases would decide anything."""
    seen = 0
    for c in cr.cases():
        if c.n_bases == 1:
            continue
        ref = cr.referenceOf(c.name)
        gap = gpu_test.baseGap(ref)
        if c.kind in ("zeros", "base0", "tie"):
            assert gap == 0 and len(set(ref.loglik)) == 1
        elif c.kind == "underflow_all":      # the bases differ by exp(-10^5) against 1e-9: no double can tell them apart
            assert gap < 1e-300
        else:
            assert gap > 2 * gpu_test.CN_FIT_BOUND, (c.name, gap)
            seen += 1
    assert seen >= 8


def test_the_recorded_tolerance_follows_the_rule():
    measured = cr.measure()
    # the constant in the GPU test is this measurement (numpy's exp / log may round differently on another CPU: a factor of
    # two either way says the constant is not stale, the bound itself is the constant's)
    assert gpu_test.CN_FIT_MEASURED / 2 <= measured <= gpu_test.CN_FIT_MEASURED * 2
    assert gpu_test.CN_FIT_BOUND == max(8 * gpu_test.CN_FIT_MEASURED, 8 * 2.0 ** -53)
    assert 1e-16 <= gpu_test.CN_FIT_MEASURED <= 1e-15
