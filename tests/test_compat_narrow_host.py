"""Bookkeeping of the tables of at most 8 columns (csrc/gk_compat_narrow.hip), no GPU needed: the name such a table's
launches carry in ``Device.call_log`` and the price ``roofmodel`` puts on them."""
import numpy as np
import pytest

from kir_graph_amd import roofmodel
from kir_graph_amd.typing_mulit_allele import compatKernelOf


def test_call_log_labels_by_column_count(monkeypatch):
    monkeypatch.delenv("GK_TEST_HOOKS", raising=False)
    assert compatKernelOf(None) == "compat_kernel"                            # no column list: every allele
    for n in (1, 4, 8):
        assert compatKernelOf(np.arange(n, dtype=np.int32)) == "compat_rows8"
    for n in (9, 64, 300):
        assert compatKernelOf(np.arange(n, dtype=np.int32)) == "compat_kernel"
    monkeypatch.setenv("GK_TEST_HOOKS", "two_walks,wide_compat")
    assert compatKernelOf(np.arange(3, dtype=np.int32)) == "compat_kernel"


def test_roofmodel_prices_a_compat_rows8_entry():
    n_rows, n_cols, n_ids = 750_000, 4, 68.0 * 750_000
    calls = [("compat_rows8", n_rows, n_cols, n_ids, 8)]
    by, ops, bound, peak = roofmodel._priced("compat_rows8", calls)
    assert by == roofmodel.compatLaunch(n_rows, n_cols, n_ids, 8)[0] == 4 * n_ids + 16 * n_rows + 9 * n_rows * n_cols
    assert (ops, bound, peak) == (0.0, "hbm", 0.0)
    entry = roofmodel.summarise(calls, "compat_rows8", total_ms=0.2, launches=1)
    assert entry["bound"] == "hbm" and entry["unit"] == "GB/s"
    assert entry["achieved"] == pytest.approx(by / 0.2e-3 / 1e9)
    # the launches of compat_kernel are priced without it
    both = calls + [("compat_kernel", n_rows, 300, n_ids, 8)]
    assert roofmodel._priced("compat_kernel", [c for c in both if c[0] == "compat_kernel"])[0] == \
        roofmodel.compatLaunch(n_rows, 300, n_ids, 8)[0]
    step = roofmodel.stepRoofline(both, 1, 1.0)
    assert step["kernels"]["compat_rows8"]["bound"] == "hbm" and step["kernels"]["compat_rows8"]["ops_per_step"] == 0.0
