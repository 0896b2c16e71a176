"""GPU: the SQUAREM solver (em_step / em_solve of csrc/gk_squarem.h through gk_em_run: 1024 threads, double weights) against
the plain longdouble reference of tests/squarem_reference.py at lane, round and stop edges.  The 512-thread instantiation
(boot_em_batch) is tied to this one bit for bit by tests/test_gpu_em_bootstrap.py.

Exact cases compare bits.  Every other run of the table (a case at iter_max 0, 1, 2, 3 -- the state after exactly that many
passes, no stop decision involved -- and at 300) has to lie within ``32 * max(dev64, 2^-52)`` of the longdouble run, absolute,
per allele, where dev64 is the distance of the reference's own float64 run from its longdouble run: kernel and float64
restatement evaluate the same formulas in float64 and differ in the order of their sums only (a tree over 16 lanes against
row-sequential sums), and the extrapolation amplifies both alike.  ``iterations`` is asserted every time, ``== iter_max``
for a run that is used up included.  tests/test_squarem_reference_host.py asserts, without a GPU, that every case reaches the
edge it names, that no stop of a run is a matter of rounding (margin >= 0.05, same passes in float64) and that the
reference's own float64 runs in other summation orders stay within the bound.

Measured on an MI355X, per group of cases and for the runs of at most 5 passes / the runs to the stop: the largest GPU
deviation from the longdouble run | the largest dev64 | the smallest bound of the group's runs | the largest ratio of a
run's deviation to its bound.  The kernel's 16-lane trees are nearer to the longdouble run than numpy's sequential sums.

    rounds of sets            <= 3 passes  2.7e-15 | 2.7e-15 | 7.1e-15 | 0.039      stop  6.8e-13 | 2.3e-12 | 7.1e-15 | 0.037
    members per set           <= 3 passes  2.3e-16 | 2.8e-16 | 7.1e-15 | 0.026      stop  6.1e-12 | 2.8e-12 | 9.1e-11 | 0.067
    sets per allele           <= 3 passes  3.9e-17 | 3.9e-17 | 7.1e-15 | 0.005      stop  3.9e-17 | 3.9e-17 | 7.1e-15 | 0.005
    allele counts             <= 3 passes  6.4e-16 | 6.4e-16 | 7.1e-15 | 0.051      stop  3.0e-13 | 2.1e-13 | 7.1e-15 | 0.108
    scale row in LDS or HBM   <= 3 passes  3.0e-15 | 1.4e-14 | 2.4e-14 | 0.038      stop  4.0e-16 | 2.6e-15 | 2.4e-14 | 0.005
    weights                   <= 3 passes  2.4e-15 | 3.3e-15 | 7.1e-15 | 0.046      stop  8.6e-14 | 4.0e-13 | 7.1e-15 | 0.042
    clamp and zero-sum sets   <= 3 passes  2.9e-16 | 3.4e-16 | 7.1e-15 | 0.027      stop  6.5e-15 | 2.7e-14 | 7.1e-15 | 0.008
    thresholds                5 passes     1.2e-17 | 2.4e-17 | 7.1e-15 | 0.002      stop  6.8e-18 | 1.3e-17 | 7.1e-15 | 0.001

The largest bound of the table is 9.1e-11 (members-per-set at the stop, 29 passes); none comes near the ceiling of 1e-9.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import squarem_reference as sq  # noqa: E402

from kir_graph_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

LD = np.longdouble


def emRun(device, packed, weight, n_allele, iter_max, threshold):
    packed = np.ascontiguousarray(packed, dtype=np.uint32)
    weight = np.ascontiguousarray(weight, dtype=np.float64)
    assert packed.ndim == 2 and len(weight) == len(packed) and 1 <= n_allele <= packed.shape[1] * 32 <= 512
    prob, iters = np.full(n_allele, np.nan), C.c_int32(-1)
    _lib.check(_lib.lib().gk_em_run(device.ctx, packed.ctypes.data, weight.ctypes.data, len(packed), packed.shape[1], n_allele,
                                    iter_max, threshold, prob.ctypes.data, C.byref(iters)))
    return prob, int(iters.value)


def runCase(device, name, iter_max):
    c = sq.case(name)
    return emRun(device, c.packed, c.weight, c.n_allele, iter_max, c.threshold)


EXACT = [c.name for c in sq.cases() if c.exact is not None]


@pytest.mark.parametrize("name", EXACT)
def test_exact_cases(device, name):
    """Every intermediate of these is exact in float64 (dyadic fractions): the bits derived by hand, the vs == 0 branch,
    the stop in pass 0 -- at every iter_max."""
    c = sq.case(name)
    for iter_max in c.iter_maxes:
        prob, iters = runCase(device, name, iter_max)
        assert np.array_equal(prob, c.exact), iter_max
        assert iters == 0, iter_max
        assert not prob[~c.sets.any(axis=0)].any()


@pytest.mark.parametrize("name,iter_max", [run for run in sq.RUNS if run[0] not in EXACT])
def test_run_meets_the_reference(device, name, iter_max):
    c = sq.case(name)
    want = sq.reference(name, iter_max)
    dev64, limit = sq.bound(name, iter_max)
    prob, iters = runCase(device, name, iter_max)
    dev = float(np.abs(prob.astype(LD) - want.prob).max())
    print(f"SQUAREM-DEV\t{c.group}\t{name}\t{iter_max}\t{dev64:.3g}\t{limit:.3g}\t{dev:.3g}\t{iters}\t{want.iterations}")
    assert limit <= sq.BOUND_CEILING
    assert iters == want.iterations
    assert np.isfinite(prob).all()
    assert (np.abs(prob.astype(LD) - want.prob) <= limit).all(), (dev, limit)
    assert not prob[~c.sets.any(axis=0)].any()      # alleles that no set names: exactly 0.0


def test_threshold_one_returns_the_first_step(device):
    """diff_threshold = 1: the stop in pass 0 returns the p from before the pass -- the first step's, bit for bit what
    iter_max = 0 gives."""
    c = sq.case("threshold-1")
    first, _ = emRun(device, c.packed, c.weight, c.n_allele, 0, 1.0)
    prob, iters = emRun(device, c.packed, c.weight, c.n_allele, 300, 1.0)
    assert iters == 0 and np.array_equal(prob, first)


@pytest.mark.parametrize("name", ["members-per-set", "scale-row-8193", "clamp-random"])
def test_two_runs_give_equal_bits(device, name):
    for iter_max in (2, 300):
        a, b = runCase(device, name, iter_max), runCase(device, name, iter_max)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1]


def test_weights_that_name_nobody_give_zeros(device):
    """All weights zero, or the only non-zero weight on a set whose bits all lie past n_allele: the first step's total
    would be 0 and every abundance NaN after iter_max passes.  gk_em_run answers zeros and 0 steps, as boot_em_batch does
    for a replicate that drew nothing.  Weights that are partly zero are a run like any other (weights-zeros above)."""
    c = sq.case("alleles-33")
    for iter_max in (0, 3, 300):
        prob, iters = emRun(device, c.packed, np.zeros(len(c.packed)), c.n_allele, iter_max, 1e-4)
        assert np.array_equal(prob, np.zeros(c.n_allele)) and not np.signbit(prob).any() and iters == 0
    ghost_only = ~c.sets.any(axis=1)
    assert ghost_only.sum() == 1
    prob, iters = emRun(device, c.packed, ghost_only.astype(np.float64), c.n_allele, 300, 1e-4)
    assert np.array_equal(prob, np.zeros(c.n_allele)) and iters == 0
    # one set of positive weight among zeros: its members share the abundance, exactly
    bits = np.zeros((3, 64), dtype=bool)
    bits[0, :4], bits[1, 4], bits[2, 5:7] = True, True, True
    packed = sq.pack(bits)
    packed = packed[sq.ascending(packed)]
    for u in range(3):
        w = np.zeros(3)
        w[u] = 7.0
        members = sq.unpack(packed, 40)[u]      # 4, 1 or 2 of them
        prob, iters = emRun(device, packed, w, 40, 300, 1e-4)
        assert np.array_equal(prob, np.where(members, 1.0 / members.sum(), 0.0)) and iters == 0
