// numpy's pairwise summation tree (pairwise_sum in numpy's loops_utils.h), as every exact reduction of the library walks
// it: n rows above the leaf size are split into the first n2 = n / 2 rounded down to a multiple of 8, and the rest.
// Host code only: no kernel is compiled from this header, so it is in no kernel's source digest (build.KERNEL_SOURCES).
#pragma once

inline int gk_pairwise_split(int n) {
  const int n2 = n / 2;
  return n2 - n2 % 8;
}

// Post-order walk of the tree over rows [start, start + n) with leaves of at most `leaf_rows` rows.
//   leaf(start, n, slot) -> index of the leaf       (slot: 0 at the root, + 1 with every step into a RIGHT child -- the
//                                                    stack slot a leaf's sum is pushed to when sub-trees are folded as
//                                                    soon as they are complete)
//   join(a, b)                                      after both children: the sum of the node is "a += b"
// Returns the index that holds the node's sum (its leftmost leaf).
template <typename LeafFn, typename JoinFn>
int gk_pairwise_walk(int start, int n, int leaf_rows, int slot, LeafFn&& leaf, JoinFn&& join) {
  if (n <= leaf_rows) return leaf(start, n, slot);
  const int n2 = gk_pairwise_split(n);
  const int a = gk_pairwise_walk(start, n2, leaf_rows, slot, leaf, join);
  const int b = gk_pairwise_walk(start + n2, n - n2, leaf_rows, slot + 1, leaf, join);
  join(a, b);
  return a;
}
