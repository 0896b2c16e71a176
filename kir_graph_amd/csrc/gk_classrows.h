// Weighted row classes as bit planes (gk_classrows.hip): the integer bound of a search step (gk_bound.hip) is a sum of
// integers over the rows, and rows of one class hold the same byte in every column of the mismatch table, so
//     sum_r f(r) = sum_c w_c f(rep_c) = sum_b 2^b sum_{c: bit b of w_c} f(rep_c).
// Every set bit b of a class's weight w_c is one PSEUDO-ROW of PLANE b; a plane is a contiguous run of pseudo-rows padded
// with zero rows to a multiple of the staged block of minsum_sad (128 rows), and the table Q [column][ldq] of all planes
// is what the kernels of the bound run over, their inner loops unchanged: a slice of the reads lies inside one plane, and
// its partial sums are shifted left by the plane's bit when the slices are added.
// Everything is queued on the context's stream; nothing is waited for.
#pragma once
#include <algorithm>
#include <vector>

#include "gk_blocks.h"

constexpr int kClassPlanes = 24;          // weights are below 2^24: a table has fewer than 16 M rows
constexpr int kClassBlockRows = 128;      // the staged block of minsum_sad
constexpr int kClassCounters = 32;        // words of GkClassWeights::counts that the host fetches
constexpr int kClassCounterWords = 64;    // all of them: the cursors of the planes lie behind the fetched ones

// Weights and representatives of the classes of one table; they depend on the rows alone, so they serve every pass that
// writes the table's entries again.
struct GkClassWeights {
  const uint32_t* class_of = nullptr;     // [n_rows], not owned
  int64_t n_rows = 0;
  uint32_t* w = nullptr;                  // [n_rows]: rows of class c; zero from the class count on
  uint32_t* rep = nullptr;                // [n_rows]: the lowest row of class c
  // [b < 24]: classes whose weight has bit b; [24]: classes; [25]: the flag word given to the enqueue, as it stood then
  uint32_t* counts = nullptr;
  GkBlocks blocks;
};

// The pseudo-row table of one mismatch table
struct GkClassRows {
  uint8_t* Q = nullptr;                   // [n_cols][ldq]
  int64_t ldq = 0;                        // padded pseudo-rows, a multiple of 128
  int64_t n_rows = 0;                     // rows of the table Q stands for
  int n_cols = 0;
  uint8_t* blk_shift = nullptr;           // device [ldq / 128]: the plane of every block
  int64_t plane_blk0[kClassPlanes + 1] = {};      // first block of plane b; [24] = blocks of all planes
  GkBlocks blocks;
  bool ready() const { return Q != nullptr; }
};

// first blocks of the planes from the plane counts; -> padded pseudo-rows
inline int64_t gk_class_planes(const uint32_t* counts, int64_t* plane_blk0) {
  int64_t blk = 0;
  for (int b = 0; b < kClassPlanes; ++b) {
    plane_blk0[b] = blk;
    blk += ((int64_t)counts[b] + kClassBlockRows - 1) / kClassBlockRows;
  }
  plane_blk0[kClassPlanes] = blk;
  return blk * kClassBlockRows;
}

// The slices of minsum_sad over the planes: (first block, end block, shift, 0) per slice, four int32 each.  `want` slices
// fill the GPU (gk_bound.hip); a plane gets its share of them by its blocks, at least 16 blocks a slice -- a plane of
// fewer blocks is one short slice -- and no slice crosses a plane.
inline void gk_class_slices(const int64_t* plane_blk0, int64_t want, std::vector<int32_t>& out) {
  out.clear();
  const int64_t n_blk = plane_blk0[kClassPlanes];
  for (int b = 0; b < kClassPlanes; ++b) {
    const int64_t b0 = plane_blk0[b], nb = plane_blk0[b + 1] - b0;
    if (nb <= 0) continue;
    int64_t share = (want * nb + n_blk - 1) / n_blk;
    share = std::max<int64_t>(1, std::min<int64_t>(share, std::max<int64_t>(1, nb / 16)));
    const int64_t per = (nb + share - 1) / share;
    for (int64_t s = b0; s < b0 + nb; s += per) {
      const int32_t row[4] = {(int32_t)s, (int32_t)std::min<int64_t>(s + per, b0 + nb), b, 0};
      out.insert(out.end(), row, row + 4);
    }
  }
}

// w, rep and the counters of class_of (device, [n_rows]); d_flags (may be null): a device word copied to counts[25], so
// that one fetch of `counts` brings both; msum [n_msum] (may be null): cleared on the way, for gk_classrows_build.  The
// weights serve ONE gk_classrows_build (the cursors of the planes are cleared here)
int gk_classweights_enqueue(gk_ctx* ctx, const uint32_t* class_of, int64_t n_rows, const uint32_t* d_flags, uint32_t* msum,
                            int n_msum, GkClassWeights* out);
// The pseudo-row table of the FINAL miss8 from the plane counts the host has fetched (cw.counts), and on the way the
// column sums of miss8 (gk_miss_colsum) into msum [n_cols], which gk_classweights_enqueue has cleared.  A pool that cannot
// serve the table is no error: GK_OK and !out->ready() -- msum is untouched then, and the bound runs on the rows
int gk_classrows_build(gk_ctx* ctx, const GkClassWeights& cw, const uint32_t* counts_host, const uint8_t* miss8, int64_t ldm,
                       int n_cols, uint32_t* msum, GkClassRows* out);
// GK_TEST_HOOKS=class_bound=on|off, read per call, forces either route wherever a class record exists; otherwise the
// pseudo-row table is taken when its padded rows are at most half the rows
bool gk_use_class_bound(int64_t padded_pseudo_rows, int64_t n_rows);
