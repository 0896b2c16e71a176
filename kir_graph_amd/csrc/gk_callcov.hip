// Per-allele coverage of a likelihood call: WHERE along the gene the called set's support lies, in exact integers, from
// the u8 mismatch table the search left in HBM joined with the sample's records (gk_call_coverage).  No search runs again.
//
// For row r of the model, b_k = miss8[cols[k]][r] over the K distinct called columns (1 .. 16), m1 = min_k b_k and
// A = {k : b_k == m1} -- callfit_profile's rule (gk_callfit.hip), bytes as stored, 255 included; the row loops of the
// call reports stay apart because their registers are counted per kernel.  The row's pair then
// counts, with both mates, in the tracks
//
//   0          informative   always
//   1          mismatch      m1 > 0
//   2 + k      best_k        k in A
//   2 + K + k  unique_k      A == {k}
//
// and a mate counts as in depth_mark (gk_depth.hip; the walk of its M runs is gk_materuns.h, shared): every clipped M run
// adds +1 at its start and -1 at its end into the difference array of every track the row counts in; mates are counted
// independently (no overlap removal); a mate on another backbone marks nothing.
//
// Marking: one thread per mate, mate t of row t >> 1, 256 threads -- a wave holds 32 rows, a workgroup 128.  The thread
// issues the K byte loads of its row together and unconditionally with clamped indices (a column beyond the list reads the
// last listed one and never wins; DESIGN.md section 8, "what reading the ISA gave"), keeps the tie set as a 16-bit mask in
// a register, then loads its row number, the pair's source and the record's header words and walks the CIGAR.  The marks
// are integer atomicAdds into difference arrays of gene_len + 1 slots per track: exact whatever the schedule.
//
//   callcov_mark      the direct form: a mate marks every track of its row in the concatenated arrays in HBM.
//   callcov_mark_lds  workgroup (x, y) owns track y and every gridDim.x-th turn of 256 mates; the track's whole array is in
//                     its LDS (up to kCovLdsBytes), marked with ds atomics, and its non-zero slots go to HBM contiguously
//                     at the end.  A row outside the track costs its K bytes only; the records are read once per track.
//                     On an MI355X it marks the 14 genes of a 10 M-pair sample in 3.1 ms, the direct form in 13.4 ms
//                     (profiles/r14_call_coverage.txt), so it takes every gene whose track fits; the direct form takes the
//                     longer ones, and all under GK_CALLCOV=direct.
//   gk_scan_u32     ONE exclusive scan over all tracks concatenated: a track's +1 / -1 cancel inside its own
//                   gene_len + 1 slots, so nothing carries over from one track into the next.
//   callcov_finish  depth = excl + diff, each track's extra slot dropped.
//
// tests/test_gpu_call_coverage.py takes its row counts from the wave's 32 rows and the workgroup's 128, and its gene
// lengths from kCovLdsBytes: move them together.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "gk_called.h"
#include "gk_calls.h"
#include "gk_materuns.h"

namespace {

constexpr int kCovThreads = 256;
constexpr int64_t kCovMaxLen = 1ll << 24;                    // a backbone position has 24 bits in a variant key
constexpr size_t kCovLdsBytes = 144 * 1024;                  // a track's difference array in LDS: gene_len <= 36863
constexpr int64_t kCovLdsTurns = 16;                         // turns of 256 mates a workgroup of the LDS form takes at least
constexpr int64_t kCovLdsGroups = 1024;                      // workgroups of the LDS form over all tracks, about

// b_k of row r over the listed columns, loaded together and unconditionally: the tie set A as a mask, m1 in *m1_out.
// KT: the columns a thread loads, K <= KT of them listed; off[k] = where column k starts (k >= K: the last listed one)
template <int KT>
__device__ inline uint32_t cov_ties(const uint8_t* __restrict__ miss8, const int64_t* off, int K, int64_t r, uint32_t* m1_out) {
  uint32_t b[KT];
#pragma unroll
  for (int k = 0; k < KT; ++k) b[k] = miss8[off[k] + r];
  uint32_t m1 = 256u;
#pragma unroll
  for (int k = 0; k < KT; ++k) {
    if (k >= K) b[k] = 256u;      // a column beyond the list never wins
    m1 = min(m1, b[k]);
  }
  uint32_t ties = 0;
#pragma unroll
  for (int k = 0; k < KT; ++k) ties |= (uint32_t)(b[k] == m1) << k;
  *m1_out = m1;
  return ties;
}

// the tracks of a row as a mask over 2 + 2K: informative, mismatch, best_k, unique_k
__device__ inline uint64_t cov_tracks(uint32_t ties, uint32_t m1, int K) {
  uint64_t tracks = 1ull | (m1 > 0 ? 2ull : 0ull) | ((uint64_t)ties << 2);
  if ((ties & (ties - 1)) == 0) tracks |= (uint64_t)ties << (2 + K);
  return tracks;
}

// Mate `side` of valid pair `row`: mark(a, e) for every clipped M run of its CIGAR, when it lies on `gene`.
template <bool kCompact, class Mark>
__device__ inline void cov_walk(const GkMateSample& s, int64_t row, int side, int gene, int64_t len, Mark mark) {
  if (row < 0 || row >= s.n_valid) return;      // not a valid pair of this tabulation
  GkMateRuns m;
  if (!gk_mate_find<kCompact>(s, row, side, [&](uint32_t ref) { return (int)ref == gene; }, m)) return;
  gk_mate_walk<kCompact>(s, m, side, len, mark);
}

// The direct form: one thread per mate marks every track of its row in HBM.
template <bool kCompact, int KT>
__global__ __launch_bounds__(kCovThreads) void callcov_mark(GkMateSample s, const int32_t* __restrict__ rows, int64_t n_rows,
                                                            const uint8_t* __restrict__ miss8, int64_t ldm, GkCalledCols cols, int K,
                                                            int gene, int64_t len, uint32_t* __restrict__ diff) {
  const int64_t t = (int64_t)blockIdx.x * kCovThreads + threadIdx.x;
  if (t >= 2 * n_rows) return;
  const int64_t r = t >> 1;
  const int64_t row = rows[r];
  int64_t off[KT];
#pragma unroll
  for (int k = 0; k < KT; ++k) off[k] = (int64_t)cols.c[min(k, K - 1)] * ldm;
  uint32_t m1;
  const uint32_t ties = cov_ties<KT>(miss8, off, K, r, &m1);
  const uint64_t tracks = cov_tracks(ties, m1, K);
  const int64_t ld = len + 1;      // a difference array has one slot past the end
  cov_walk<kCompact>(s, row, (int)(t & 1), gene, len, [&](int64_t a, int64_t e) {
    for (uint64_t m = tracks; m; m &= m - 1) {
      uint32_t* d = diff + (int64_t)__builtin_ctzll(m) * ld;
      atomicAdd(&d[a], 1u);
      atomicAdd(&d[e], 0xFFFFFFFFu);      // -1 (mod 2^32)
    }
  });
}

// The LDS form: workgroup (x, y) owns track y and the mates x * 256 + tid, + gridDim.x * 256, ...; it keeps the track's
// whole difference array (len + 1 words of dynamic LDS) to itself, marks it with ds atomics and adds its non-zero slots to
// HBM at the end, contiguously.  A row that does not count in the track costs its K bytes and nothing else; the records
// of a row are read once per track it counts in.
template <bool kCompact, int KT>
__global__ __launch_bounds__(kCovThreads) void callcov_mark_lds(GkMateSample s, const int32_t* __restrict__ rows, int64_t n_rows,
                                                                const uint8_t* __restrict__ miss8, int64_t ldm, GkCalledCols cols,
                                                                int K, int gene, int64_t len, uint32_t* __restrict__ diff) {
  extern __shared__ uint32_t lds_diff[];
  __shared__ int64_t col_off[kCalledMaxCols];      // in LDS, not in 32 scalar registers across the loop (they spilled at KT = 16)
  const int ld = (int)len + 1;
  const int trk = blockIdx.y;
  if (threadIdx.x < kCalledMaxCols) col_off[threadIdx.x] = (int64_t)cols.c[min((int)threadIdx.x, K - 1)] * ldm;
  for (int i = threadIdx.x; i < ld; i += kCovThreads) lds_diff[i] = 0;
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * kCovThreads;
  for (int64_t t = (int64_t)blockIdx.x * kCovThreads + threadIdx.x; t < 2 * n_rows; t += stride) {
    const int64_t r = t >> 1;
    uint32_t m1;
    const uint32_t ties = cov_ties<KT>(miss8, col_off, K, r, &m1);
    if (!((cov_tracks(ties, m1, K) >> trk) & 1)) continue;
    cov_walk<kCompact>(s, rows[r], (int)(t & 1), gene, len, [&](int64_t a, int64_t e) {
      atomicAdd(&lds_diff[a], 1u);
      atomicAdd(&lds_diff[e], 0xFFFFFFFFu);      // -1 (mod 2^32)
    });
  }
  __syncthreads();
  uint32_t* d = diff + (int64_t)trk * ld;
  for (int i = threadIdx.x; i < ld; i += kCovThreads) {
    const uint32_t v = lds_diff[i];
    if (v != 0) atomicAdd(&d[i], v);
  }
}

// depth[track][p] = excl[track][p] + diff[track][p], p < len: the tracks' extra slots are dropped
__global__ __launch_bounds__(kCovThreads) void callcov_finish(const uint32_t* __restrict__ excl, const uint32_t* __restrict__ diff,
                                                              int64_t len, int64_t total, uint32_t* __restrict__ depth) {
  const int64_t i = (int64_t)blockIdx.x * kCovThreads + threadIdx.x;
  if (i >= total) return;
  const int64_t at = i + i / len;      // track * (len + 1) + p
  depth[i] = excl[at] + diff[at];
}

// Which form marks: the LDS form when a track's difference array fits a workgroup's LDS, unless GK_CALLCOV=direct asks
// for the direct one (tests and tools/time_call_coverage.py run both; read at every call).
bool cov_lds_form(size_t lds_bytes) {
  const char* want = getenv("GK_CALLCOV");
  if (want && !strcmp(want, "direct")) return false;
  return lds_bytes <= kCovLdsBytes;
}

}  // namespace

extern "C" {

/* The coverage tracks of the called columns; waits for the result.  See include/graphkir_hip.h. */
int gk_call_coverage(gk_ctx* ctx, gk_tab* tab, gk_dptr d_mates, gk_dptr d_compact, gk_dptr d_rows, int64_t n_rows,
                     gk_dptr d_miss8, int64_t ldm, int32_t n_table_cols, const int32_t* cols, int32_t n_cols, int32_t gene,
                     int64_t gene_len, uint32_t* depth_out) {
  gk_bind(ctx);
  GK_REQUIRE(ctx && tab && cols && depth_out && d_rows, "null pointer");
  GK_REQUIRE(tab->d_pair_src, "call coverage needs a tabulation made from packed records");
  GK_REQUIRE((d_mates != 0) != (d_compact != 0), "call coverage needs the sample's records in exactly one form");
  GkCalledCols cc;
  const int bad = gk_called_cols("call coverage", d_miss8, ldm, n_rows, n_table_cols, cols, n_cols, &cc, [&]() -> int {
    GK_REQUIRE(gene_len >= 1 && gene_len <= kCovMaxLen, "call coverage: gene_len must lie in 1 .. 2^24");
    GK_REQUIRE(gene >= 0 && gene < 256 && (!tab->idx || gene < tab->idx->n_gene), "call coverage: no such backbone");
    return GK_OK;
  });
  if (bad) return bad;
  const int64_t n_tracks = 2 + 2 * (int64_t)n_cols;
  const int64_t slots = n_tracks * (gene_len + 1), total = n_tracks * gene_len;
  hipStream_t st = ctx->stream;
  GkCall call(ctx);
  // the depths get a block of their own: written over the scan, word i would be gone before the thread that reads it
  // as slot i = at' of an earlier track's position runs
  uint32_t *diff = nullptr, *scan = nullptr, *depth = nullptr;
  if (call.take(&diff, (size_t)slots * sizeof(uint32_t)) != hipSuccess ||
      call.take(&scan, (size_t)slots * sizeof(uint32_t)) != hipSuccess) {
    gk_set_error("out of device memory for the tracks of a call coverage");
    return GK_ERR_HIP;
  }
  GK_TRY("call coverage", hipMemsetAsync(diff, 0, (size_t)slots * sizeof(uint32_t), st));
  {
    hipError_t e = hipSuccess;      // of the LDS attribute of a launch
    const GkMateSample s = gk_mate_sample(tab, d_mates, d_compact);
    const dim3 block(kCovThreads);
    const int32_t* rows = gk_ptr<const int32_t>(d_rows);
    const uint8_t* m = gk_ptr<const uint8_t>(d_miss8);
    const int64_t mate_groups = (2 * n_rows + kCovThreads - 1) / kCovThreads;
    const size_t lds = (size_t)(gene_len + 1) * sizeof(uint32_t);
    if (cov_lds_form(lds)) {
      // a workgroup takes kCovLdsTurns turns of 256 mates at least (its LDS array is zeroed and flushed once), and there
      // are about kCovLdsGroups workgroups over all tracks at most
      const int64_t slices = std::max<int64_t>(1, std::min((mate_groups + kCovLdsTurns - 1) / kCovLdsTurns, kCovLdsGroups / n_tracks));
      const dim3 grid((unsigned)slices, (unsigned)n_tracks);
#define GK_COV_LDS(C, KT)                                                                                                  \
  do {                                                                                                                     \
    if (lds > 48 * 1024)                                                                                                   \
      e = hipFuncSetAttribute((const void*)callcov_mark_lds<C, KT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
    if (e == hipSuccess)                                                                                                   \
      GK_PROF(ctx, "callcov_mark_lds", GK_KERNEL((callcov_mark_lds<C, KT>), grid, block, lds, st, s, rows, n_rows, m, ldm, \
                                                 cc, (int)n_cols, (int)gene, gene_len, diff));                             \
  } while (0)
#define GK_COV_LAUNCH(KT)     \
  do {                        \
    if (s.c_off)              \
      GK_COV_LDS(true, KT);   \
    else                      \
      GK_COV_LDS(false, KT);  \
  } while (0)
      GK_CALLED_LAUNCH(n_cols, GK_COV_LAUNCH)
#undef GK_COV_LAUNCH
#undef GK_COV_LDS
    } else {
      const dim3 grid((unsigned)mate_groups);
#define GK_COV_LAUNCH(KT)                                                                                               \
  do {                                                                                                                  \
    if (s.c_off)                                                                                                        \
      GK_PROF(ctx, "callcov_mark", GK_KERNEL((callcov_mark<true, KT>), grid, block, 0, st, s, rows, n_rows, m, ldm, cc,  \
                                             (int)n_cols, (int)gene, gene_len, diff));                                  \
    else                                                                                                                \
      GK_PROF(ctx, "callcov_mark", GK_KERNEL((callcov_mark<false, KT>), grid, block, 0, st, s, rows, n_rows, m, ldm, cc, \
                                             (int)n_cols, (int)gene, gene_len, diff));                                  \
  } while (0)
      GK_CALLED_LAUNCH(n_cols, GK_COV_LAUNCH)
#undef GK_COV_LAUNCH
    }
    GK_TRY("call coverage", e);
  }
  GK_TRY("call coverage", hipGetLastError());
  GK_TRY("call coverage", hipMemcpyAsync(scan, diff, (size_t)slots * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  const int rc = gk_scan_u32(ctx, scan, slots, nullptr);
  if (rc) return rc;
  if (call.take(&depth, (size_t)total * sizeof(uint32_t)) != hipSuccess) {
    gk_set_error("out of device memory for the tracks of a call coverage");
    return GK_ERR_HIP;
  }
  GK_PROF(ctx, "callcov_finish", GK_KERNEL(callcov_finish, dim3((unsigned)((total + kCovThreads - 1) / kCovThreads)),
                                           dim3(kCovThreads), 0, st, scan, diff, gene_len, total, depth));
  GK_TRY("call coverage", hipGetLastError());
  GK_TRY("call coverage", call.fetch(depth_out, depth, (size_t)total * sizeof(uint32_t)));
  GK_TRY("call coverage", call.wait());
  return GK_OK;
}

}  // extern "C"
