// Read bootstrap of the copy-number stage (gk_depth_weighted): the depth of the sample with every valid pair counted
// W[b][i] times instead of once, for a slice of replicates b at a time, and per (replicate, gene) the exact sum and two
// order statistics of the gene's selected positions -- what p75 / mean / median of a replicate's depth track are made of.
// Only those numbers cross PCIe; the tracks stay in HBM (depth_out exists for the tests).
//
// A mate counts as in depth_mark (gk_depth.hip; the walk of its M runs is gk_materuns.h, shared): pairs with NH != 1 are
// skipped unless `multiple`; every clipped M run adds +w at its start and -w at its end into the replicate's difference
// array.  With every weight 1 the result is gk_depth's integers.  All adds are integer atomics mod 2^32: exact
// whatever the schedule.
//
//   depthw_mark    one thread per mate (a workgroup holds 128 pairs) and per group of kBootPerThread replicates of the
//                  slice (blockIdx.y).  The header is read once and the CIGAR of a 128-byte / compact record is held in 7
//                  registers; per replicate the thread loads W[b][i] (the lanes of a wave read consecutive pairs), skips
//                  on 0 and marks replicate b's array of total + 1 slots.  A wide pair's CIGAR (up to 128 operations) is
//                  walked from its record per replicate: such pairs are rare.
//   gk_scan_u32    ONE exclusive scan over the slice: a replicate's +w / -w cancel inside its own total + 1 slots, so
//                  nothing carries over into the next replicate (as in gk_callcov.hip).
//   depthw_finish  depth = excl + diff, in place; a replicate keeps its total + 1 slots, the last one holds 0.
//   depthw_select  one workgroup per (replicate, gene): over the gene's selected positions the sum in 64 bits and the values
//                  of two 0-based ranks by a radix select -- three passes over the track with LDS histograms of 11 / 11 /
//                  10 bits, most significant first, both ranks carried through each pass (a histogram each from the second
//                  pass on).  Nothing is sorted.  Exact for any uint32 values, ties included.
//
// The replicates are processed in slices so that the difference arrays and their scan copy stay within kDepthwBudget
// (GK_TEST_HOOKS=depthw_budget=BYTES lowers it: the tests force several slices); a replicate's result does not depend on
// the slice it falls in.  tests/test_gpu_cn_bootstrap.py takes its pair counts from the workgroup's 128 pairs and its depth
// values from the digit boundaries 2^10 and 2^21: move them together.
#include <algorithm>
#include <vector>

#include "gk_calls.h"
#include "gk_materuns.h"

namespace {

constexpr int kDwThreads = 256;
constexpr int kMaxBoot = 10000;
constexpr int kBootPerThread = 8;                           // replicates a thread of depthw_mark takes
constexpr size_t kDepthwBudget = (size_t)1 << 30;           // bytes of a slice's difference arrays + their scan copy
constexpr int64_t kDwMaxLen = 1ll << 24;                    // a backbone position has 24 bits in a variant key
constexpr int kSelBins = 2048;                              // 11 bits; the last pass uses the first 1024

template <bool kCompact>
__global__ __launch_bounds__(kDwThreads) void depthw_mark(GkMateSample s, int multiple, const int64_t* __restrict__ gene_off,
                                                          int n_gene, const uint32_t* __restrict__ W, int64_t ldw, int n_boot,
                                                          int64_t slots, uint32_t* __restrict__ diff) {
  const int64_t t = (int64_t)blockIdx.x * kDwThreads + threadIdx.x;
  if (t >= 2 * s.n_valid) return;
  const int64_t i = t >> 1;
  const int side = (int)(t & 1);
  if (!multiple && s.pair_nh[i] != 1) return;
  GkMateRuns m;
  if (!gk_mate_find<kCompact>(s, i, side, [&](uint32_t ref) { return (int)ref < n_gene; }, m)) return;
  const int64_t base = gene_off[m.ref], len = gene_off[m.ref + 1] - base;
  GkMateCigar cig;
  if (!gk_mate_stage<kCompact>(s, m, side, cig)) return;
  const int b0 = blockIdx.y * kBootPerThread;
  const int b1 = min(b0 + kBootPerThread, n_boot);
  for (int b = b0; b < b1; ++b) {
    const uint32_t wt = W[(int64_t)b * ldw + i];
    if (wt == 0) continue;
    uint32_t* d = diff + (int64_t)b * slots + base;
    gk_mate_walk_staged(m, cig, len, [&](int64_t a, int64_t e) {
      atomicAdd(&d[a], wt);
      atomicAdd(&d[e], 0u - wt);      // -w (mod 2^32); a replicate's array has one slot past the end
    });
  }
}

__global__ __launch_bounds__(kDwThreads) void depthw_finish(const uint32_t* __restrict__ excl, uint32_t* __restrict__ diff,
                                                            int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kDwThreads + threadIdx.x;
  if (i < n) diff[i] += excl[i];
}

// The bin of `hist` (bins = per * kDwThreads) that holds 0-based rank k, and k's rank inside that bin -- by every thread
// of the workgroup: a thread sums its `per` bins, adds up the sums before it, and the one whose bins hold k walks them.
// k must be below the histogram's total.  Ends with a barrier.
__device__ inline void sel_find(const uint32_t* hist, int per, uint32_t k, uint32_t* part, uint32_t* digit_out, uint32_t* rank_out) {
  const int tid = threadIdx.x;
  uint32_t mine = 0;
  for (int j = 0; j < per; ++j) mine += hist[tid * per + j];
  __syncthreads();      // part may still be read by a previous call
  part[tid] = mine;
  __syncthreads();
  uint32_t before = 0;
  for (int x = 0; x < tid; ++x) before += part[x];
  if (k >= before && k - before < mine) {
    uint32_t left = k - before;
    for (int j = 0; j < per; ++j) {
      const uint32_t c = hist[tid * per + j];
      if (left < c) {
        *digit_out = (uint32_t)(tid * per + j);
        *rank_out = left;
        break;
      }
      left -= c;
    }
  }
  __syncthreads();
}

// Workgroup (g, b): gene g of replicate b.  depth: the slice's tracks, `slots` words per replicate; sel: nullable mask over
// the concatenated positions; rank [n_gene][2]; stat [n_boot][n_gene][2], sum [n_boot][n_gene] of the slice.
__global__ __launch_bounds__(kDwThreads) void depthw_select(const uint32_t* __restrict__ depth, int64_t slots,
                                                            const int64_t* __restrict__ gene_off, const uint8_t* __restrict__ sel,
                                                            const int64_t* __restrict__ rank, uint32_t* __restrict__ stat,
                                                            unsigned long long* __restrict__ sum) {
  __shared__ uint32_t hists[2 * kSelBins];      // one histogram per rank; the first pass shares the first
  uint32_t* const hist[2] = {hists, hists + kSelBins};
  __shared__ uint32_t part[kDwThreads];
  __shared__ uint32_t digit[2], left[2], count;
  __shared__ unsigned long long total;
  const int tid = threadIdx.x, g = blockIdx.x, n_gene = gridDim.x;
  const int64_t base = gene_off[g], len = gene_off[g + 1] - base;
  const uint32_t* d = depth + (int64_t)blockIdx.y * slots + base;
  const uint8_t* m = sel ? sel + base : nullptr;
  const int64_t cell = (int64_t)blockIdx.y * n_gene + g;

  // pass 1: bits 31 .. 21 of every selected value, their number and their sum
  for (int x = tid; x < kSelBins; x += kDwThreads) hist[0][x] = 0;
  if (tid == 0) {
    count = 0;
    total = 0;
  }
  __syncthreads();
  uint32_t n_mine = 0;
  unsigned long long s_mine = 0;
  for (int64_t p = tid; p < len; p += kDwThreads) {
    if (m && !m[p]) continue;
    const uint32_t v = d[p];
    atomicAdd(&hist[0][v >> 21], 1u);
    s_mine += v;
    ++n_mine;
  }
  if (n_mine) {
    atomicAdd(&count, n_mine);
    atomicAdd(&total, s_mine);
  }
  __syncthreads();
  const uint32_t n = count;      // <= 2^24
  if (n == 0) {      // no selected position: 0 / 0, the ranks are not looked at
    if (tid == 0) {
      stat[2 * cell] = stat[2 * cell + 1] = 0;
      sum[cell] = 0;
    }
    return;
  }
  uint32_t k[2], prefix[2];
  for (int j = 0; j < 2; ++j) {
    const int64_t r = rank[2 * g + j];
    k[j] = (uint32_t)(r < 0 ? 0 : r >= n ? n - 1 : r);      // checked on the host; clamped all the same
    sel_find(hist[0], kSelBins / kDwThreads, k[j], part, &digit[j], &left[j]);
    prefix[j] = digit[j];
    k[j] = left[j];
  }

  // pass 2: bits 20 .. 10 of the values under each rank's first digit
  for (int x = tid; x < 2 * kSelBins; x += kDwThreads) hists[x] = 0;
  __syncthreads();
  for (int64_t p = tid; p < len; p += kDwThreads) {
    if (m && !m[p]) continue;
    const uint32_t v = d[p], hi = v >> 21, mid = (v >> 10) & 0x7FFu;
    if (hi == prefix[0]) atomicAdd(&hist[0][mid], 1u);
    if (hi == prefix[1]) atomicAdd(&hist[1][mid], 1u);
  }
  __syncthreads();
  for (int j = 0; j < 2; ++j) {
    sel_find(hist[j], kSelBins / kDwThreads, k[j], part, &digit[j], &left[j]);
    prefix[j] = (prefix[j] << 11) | digit[j];
    k[j] = left[j];
  }

  // pass 3: bits 9 .. 0 of the values under each rank's first two digits
  for (int x = tid; x < 2 * kSelBins; x += kDwThreads) hists[x] = 0;
  __syncthreads();
  for (int64_t p = tid; p < len; p += kDwThreads) {
    if (m && !m[p]) continue;
    const uint32_t v = d[p], hi = v >> 10, low = v & 0x3FFu;
    if (hi == prefix[0]) atomicAdd(&hist[0][low], 1u);
    if (hi == prefix[1]) atomicAdd(&hist[1][low], 1u);
  }
  __syncthreads();
  for (int j = 0; j < 2; ++j) {
    sel_find(hist[j], 1024 / kDwThreads, k[j], part, &digit[j], &left[j]);
    prefix[j] = (prefix[j] << 10) | digit[j];
  }
  if (tid == 0) {
    stat[2 * cell] = prefix[0];
    stat[2 * cell + 1] = prefix[1];
    sum[cell] = total;
  }
}

size_t depthw_budget() {
  const long v = gk_test_hook_value("depthw_budget", 0);
  return v > 0 ? (size_t)v : kDepthwBudget;
}

}  // namespace

extern "C" {

/* The weighted depth of a slice of bootstrap replicates and its per-gene statistics; waits for the result.  See
 * include/graphkir_hip.h. */
int gk_depth_weighted(gk_ctx* ctx, gk_tab* tab, gk_dptr d_mates, gk_dptr d_compact, int32_t multiple, const int64_t* gene_off,
                      int32_t n_gene, gk_dptr d_W, int64_t ldw, int32_t n_boot, const uint8_t* sel, const int64_t* rank,
                      uint32_t* stat_out, uint64_t* sum_out, uint32_t* depth_out) {
  gk_bind(ctx);
  GK_REQUIRE(ctx && tab && gene_off && rank && stat_out && sum_out, "null pointer");
  GK_REQUIRE(tab->d_pair_src, "weighted depth needs a tabulation made from packed records");
  GK_REQUIRE((d_mates != 0) != (d_compact != 0), "weighted depth needs the sample's records in exactly one form");
  GK_REQUIRE(n_gene >= 1 && n_gene <= 256, "weighted depth: the number of backbones must lie in 1 .. 256");
  GK_REQUIRE(n_boot >= 1 && n_boot <= kMaxBoot, "the number of bootstrap replicates must lie in 1 .. 10000");
  GK_REQUIRE(d_W && ldw >= tab->n_valid, "weighted depth: a row of the weights is shorter than the valid pairs");
  GK_REQUIRE(gene_off[0] == 0, "weighted depth: the first backbone must start at 0");
  for (int g = 0; g < n_gene; ++g) {
    const int64_t len = gene_off[g + 1] - gene_off[g];
    GK_REQUIRE(len >= 1 && len <= kDwMaxLen, "weighted depth: a backbone's length must lie in 1 .. 2^24");
    int64_t n_sel = len;
    if (sel) {
      n_sel = 0;
      for (int64_t p = gene_off[g]; p < gene_off[g + 1]; ++p) n_sel += sel[p] != 0;
    }
    for (int j = 0; j < 2; ++j)
      GK_REQUIRE(n_sel == 0 || (rank[2 * g + j] >= 0 && rank[2 * g + j] < n_sel),
                 "weighted depth: a rank lies outside the gene's selected positions");
  }
  const int64_t total = gene_off[n_gene], slots = total + 1;
  const size_t n_cells = (size_t)n_boot * n_gene;
  if (tab->n_valid == 0) {      // nothing to mark: zeros, nothing launched
    std::fill(stat_out, stat_out + 2 * n_cells, 0u);
    std::fill(sum_out, sum_out + n_cells, (uint64_t)0);
    if (depth_out) std::fill(depth_out, depth_out + (size_t)n_boot * total, 0u);
    return GK_OK;
  }
  // replicates of one slice: their difference arrays and the scan copy stay within the budget
  const int64_t slice = std::max<int64_t>(1, std::min<int64_t>(n_boot, (int64_t)(depthw_budget() / (2 * sizeof(uint32_t) * (size_t)slots))));
  hipStream_t st = ctx->stream;
  GkCall call(ctx);
  uint32_t *diff = nullptr, *scan = nullptr, *d_stat = nullptr;
  int64_t *d_off = nullptr, *d_rank = nullptr;
  unsigned long long* d_sum = nullptr;
  uint8_t* d_sel = nullptr;
  if (call.take(&diff, (size_t)slice * slots * sizeof(uint32_t)) != hipSuccess ||
      call.take(&scan, (size_t)slice * slots * sizeof(uint32_t)) != hipSuccess ||
      call.take(&d_off, (size_t)(n_gene + 1) * sizeof(int64_t)) != hipSuccess ||
      call.take(&d_rank, (size_t)2 * n_gene * sizeof(int64_t)) != hipSuccess ||
      call.take(&d_stat, 2 * n_cells * sizeof(uint32_t)) != hipSuccess ||
      call.take(&d_sum, n_cells * sizeof(unsigned long long)) != hipSuccess ||
      (sel && call.take(&d_sel, (size_t)total) != hipSuccess)) {
    gk_set_error("out of device memory for the replicates of a weighted depth");
    return GK_ERR_HIP;
  }
  GK_TRY("weighted depth", call.send(d_off, gene_off, (size_t)(n_gene + 1) * sizeof(int64_t)));      // at most 257 words
  GK_TRY("weighted depth", call.send(d_rank, rank, (size_t)2 * n_gene * sizeof(int64_t)));
  // From here on the stream may read `sel` (a selection too large for the ring is copied straight from it, and the wait
  // at the end covers that copy) and write `depth_out`: a way out before that wait drains the stream
  call.expect();
  if (sel) GK_TRY("weighted depth", gk_send(ctx, d_sel, sel, (size_t)total));      // once, for every slice
  const GkMateSample s = gk_mate_sample(tab, d_mates, d_compact);
  const uint32_t* W = gk_ptr<const uint32_t>(d_W);
  const unsigned mate_groups = (unsigned)((2 * tab->n_valid + kDwThreads - 1) / kDwThreads);
  for (int64_t b0 = 0; b0 < n_boot; b0 += slice) {
    const int nb = (int)std::min<int64_t>(slice, n_boot - b0);
    const int64_t n = (int64_t)nb * slots;
    GK_TRY("weighted depth", hipMemsetAsync(diff, 0, (size_t)n * sizeof(uint32_t), st));
    const dim3 grid(mate_groups, (unsigned)((nb + kBootPerThread - 1) / kBootPerThread));
    if (s.c_off)
      GK_PROF(ctx, "depthw_mark", GK_KERNEL(depthw_mark<true>, grid, dim3(kDwThreads), 0, st, s, (int)multiple, d_off, (int)n_gene,
                                            W + b0 * ldw, ldw, nb, slots, diff));
    else
      GK_PROF(ctx, "depthw_mark", GK_KERNEL(depthw_mark<false>, grid, dim3(kDwThreads), 0, st, s, (int)multiple, d_off, (int)n_gene,
                                            W + b0 * ldw, ldw, nb, slots, diff));
    GK_TRY("weighted depth", hipGetLastError());
    GK_TRY("weighted depth", hipMemcpyAsync(scan, diff, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    const int rc = gk_scan_u32(ctx, scan, n, nullptr);
    if (rc) return rc;
    GK_PROF(ctx, "depthw_finish", GK_KERNEL(depthw_finish, dim3((unsigned)((n + kDwThreads - 1) / kDwThreads)), dim3(kDwThreads), 0,
                                            st, scan, diff, n));
    GK_PROF(ctx, "depthw_select", GK_KERNEL(depthw_select, dim3((unsigned)n_gene, (unsigned)nb), dim3(kDwThreads), 0, st, diff, slots,
                                            d_off, d_sel, d_rank, d_stat + 2 * b0 * n_gene, d_sum + b0 * n_gene));
    GK_TRY("weighted depth", hipGetLastError());
    if (depth_out)      // the tracks without their extra slots (the tests ask for them)
      GK_TRY("weighted depth",
             hipMemcpy2DAsync(depth_out + b0 * total, (size_t)total * sizeof(uint32_t), diff, (size_t)slots * sizeof(uint32_t),
                              (size_t)total * sizeof(uint32_t), (size_t)nb, hipMemcpyDeviceToHost, st));
  }
  GK_TRY("weighted depth", call.fetch(stat_out, d_stat, 2 * n_cells * sizeof(uint32_t)));
  GK_TRY("weighted depth", call.fetch(sum_out, d_sum, n_cells * sizeof(uint64_t)));
  GK_TRY("weighted depth", call.wait());
  return GK_OK;
}

}  // extern "C"
