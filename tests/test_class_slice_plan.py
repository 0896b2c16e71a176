"""The slice planner of the bound over pseudo-rows (csrc/gk_classrows.h: gk_class_planes + gk_class_slices, through
gk_class_slice_plan; no GPU): planes of 0, 1, 127, 128 and 129 classes in any mix, and planes large enough for several
slices.  No slice crosses a plane, every block lies in exactly one slice, and a slice carries its plane's shift."""
import itertools

import numpy as np
import pytest

from kir_graph_amd._lib import check, lib

PLANES = 24
BLOCK = 128


def plan(counts, want):
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    assert len(counts) == PLANES
    n = np.zeros(1, dtype=np.int32)
    blk0 = np.zeros(PLANES + 1, dtype=np.int64)
    check(lib().gk_class_slice_plan(counts.ctypes.data, want, None, 0, n.ctypes.data, blk0.ctypes.data))
    out = np.full((int(n[0]) + 1, 4), -5, dtype=np.int32)
    check(lib().gk_class_slice_plan(counts.ctypes.data, want, out.ctypes.data, int(n[0]), n.ctypes.data, None))
    assert (out[-1] == -5).all()                # nothing behind the capacity
    return out[:-1], blk0


def check_plan(counts, want):
    slices, blk0 = plan(counts, want)
    blocks = [-(-int(c) // BLOCK) for c in counts]
    assert blk0.tolist() == np.r_[0, np.cumsum(blocks)].tolist()
    owner = np.full(int(blk0[-1]), -1, dtype=np.int64)
    for first, end, shift, pad in slices.tolist():
        assert pad == 0 and 0 <= shift < PLANES and first < end
        assert blk0[shift] <= first and end <= blk0[shift + 1]          # inside ONE plane, and that plane is its shift
        assert (owner[first:end] == -1).all()
        owner[first:end] = shift
    assert (owner >= 0).all()                                            # every block in exactly one slice
    for b in range(PLANES):
        mine = slices[slices[:, 2] == b]
        assert (len(mine) == 0) == (blocks[b] == 0)
        if len(mine) > 1:                                                # several slices: at least 16 blocks each but the last
            assert ((mine[:-1, 1] - mine[:-1, 0]) >= 16).all()
    return slices


@pytest.mark.parametrize("want", [1, 7, 2048])
def test_small_planes_in_any_mix(want):
    for mix in itertools.product([0, 1, 127, 128, 129], repeat=4):
        for at in ((0, 1, 2, 3), (0, 5, 22, 23)):
            counts = np.zeros(PLANES, dtype=np.uint32)
            counts[list(at)] = mix
            slices = check_plan(counts, want)
            assert len(slices) == sum(1 for c in mix if c)               # a small plane is one short slice


@pytest.mark.parametrize("want", [1, 3, 32, 2048])
def test_large_planes_take_their_share(want):
    counts = np.zeros(PLANES, dtype=np.uint32)
    counts[[0, 1, 2, 5, 9, 23]] = [300000, 129, 5000, 2048 * 16, 1, 70000]
    slices = check_plan(counts, want)
    assert len(slices) <= want + 6                                       # about `want`: at most one more per plane
    if want == 1:
        assert len(slices) == 6


def test_no_plane():
    slices, blk0 = plan(np.zeros(PLANES, dtype=np.uint32), 4)
    assert len(slices) == 0 and (blk0 == 0).all()


def test_bad_arguments():
    counts = np.ones(PLANES, dtype=np.uint32)
    n = np.zeros(1, dtype=np.int32)
    assert lib().gk_class_slice_plan(None, 1, None, 0, n.ctypes.data, None) != 0
    assert lib().gk_class_slice_plan(counts.ctypes.data, 0, None, 0, n.ctypes.data, None) != 0
    assert lib().gk_class_slice_plan(counts.ctypes.data, 1, None, 3, n.ctypes.data, None) != 0
    assert lib().gk_class_slice_plan(counts.ctypes.data, 1, None, 0, None, None) != 0
