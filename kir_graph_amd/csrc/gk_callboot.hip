// Read bootstrap of a likelihood call: replicate weights per read, and the weighted sums of the per-read values of the
// candidate sets (gk_boot_row_counts, gk_weighted_sums).  A replicate RESCORES the sets the point search ranked; no
// search runs again.
//
//   callboot_draw    replicate b draws n reads with replacement from the gene's n reads: a thread per draw (the counter
//                    based generator of gk_draw.h, DESIGN.md section 8c, shared with gk_boot.hip), one integer atomicAdd into
//                    W[b][row].  Draws scatter over n rows, about one per row: there is nothing to privatise in LDS.
//                    Integer adds only: exact, whatever the schedule.
//   callboot_sums    S[b][t] = sum_r W[b][r] * V[t][r].  Lanes run across rows, so both tables are read as whole lines.
//                    A workgroup of kSumThreads takes kSumChunk rows and a tile of kTileBoot replicates x kTileSets sets;
//                    a lane keeps the tile in registers (kTileBoot * kTileSets f64) over its rows r = chunk + tid,
//                    chunk + tid + kSumThreads, ...; the tile is summed across the 64 lanes of a wave by a butterfly of
//                    shuffles (offsets 32, 16, ... 1) and across the waves through LDS in wave order.  One partial per
//                    (chunk, b, t).
//   callboot_fold    adds the partials of a (b, t) in chunk order.
//
// The sum of a (b, t) has ONE order -- rows of a lane ascending, the butterfly, waves ascending, chunks ascending -- that
// depends on n_rows alone: the same bits on every run and whichever tile the pair sits in.  No float atomics.  w < 2^31
// converts to f64 exactly and a product is rounded once, inside the fma.  Rows, sets and replicates beyond the end are
// predicated off: nothing at or beyond n_rows is read from either table.
// tests/test_gpu_call_bootstrap.py takes its shapes from kSumChunk (4096), the wave (64), kSumThreads (256) and the tile
// (4 x 8): move them together.
#include <algorithm>

#include "gk_calls.h"
#include "gk_draw.h"

namespace {

constexpr int kMaxBoot = 10000;
constexpr int kMaxSets = 256;

// ------------------------------------------------------------------------------------------------ replicate weights
constexpr int kDrawThreads = 256;
constexpr uint32_t kDrawChunk = 1u << 14;      // draws of a workgroup per turn
constexpr uint32_t kDrawMaxGroups = 2048;      // workgroups per replicate; they stride over the chunks beyond

__global__ __launch_bounds__(kDrawThreads) void callboot_draw(uint32_t n, uint32_t boot_first, uint64_t seed, uint32_t stream,
                                                              uint32_t* __restrict__ W, int64_t ldw) {
  const uint32_t b = blockIdx.y;
  uint32_t* row = W + (int64_t)b * ldw;
  const uint64_t stride = (uint64_t)gridDim.x * kDrawChunk;
  for (uint64_t begin = (uint64_t)blockIdx.x * kDrawChunk; begin < n; begin += stride) {
    const uint64_t end = min(begin + (uint64_t)kDrawChunk, (uint64_t)n);
    for (uint64_t i = begin + threadIdx.x; i < end; i += kDrawThreads)
      atomicAdd(&row[gk_boot_draw(seed, i, (uint64_t)boot_first + b, stream, n)], 1u);
  }
}

// ------------------------------------------------------------------------------------------------ weighted sums
constexpr int kSumThreads = 256;
constexpr int kSumWaves = kSumThreads / 64;
constexpr int kSumChunk = 4096;      // rows of a workgroup: kSumChunk / kSumThreads per lane
constexpr int kTileBoot = 4;
constexpr int kTileSets = 8;
constexpr int kTile = kTileBoot * kTileSets;

__global__ __launch_bounds__(kSumThreads) void callboot_sums(const double* __restrict__ V, int64_t ld, int64_t n_rows, int n_sets,
                                                             const uint32_t* __restrict__ W, int64_t ldw, int n_boot,
                                                             int tiles_boot, int tiles_sets, double* __restrict__ partial) {
  __shared__ double wave_sum[kSumWaves][kTile];
  // tiles fastest: the workgroups that share a chunk's lines run together
  const int64_t n_tiles = (int64_t)tiles_boot * tiles_sets;
  const int64_t chunk = blockIdx.x / n_tiles;
  const int tile = (int)(blockIdx.x - chunk * n_tiles);
  const int b0 = (tile / tiles_sets) * kTileBoot;
  const int t0 = (tile % tiles_sets) * kTileSets;
  const int tid = threadIdx.x;
  const int64_t r_begin = chunk * kSumChunk;
  const int64_t r_end = min(r_begin + (int64_t)kSumChunk, n_rows);

  double acc[kTileBoot][kTileSets];
#pragma unroll
  for (int i = 0; i < kTileBoot; ++i)
#pragma unroll
    for (int j = 0; j < kTileSets; ++j) acc[i][j] = 0.0;

  for (int64_t r = r_begin + tid; r < r_end; r += kSumThreads) {
    double w[kTileBoot], v[kTileSets];
#pragma unroll
    for (int i = 0; i < kTileBoot; ++i) w[i] = b0 + i < n_boot ? (double)W[(int64_t)(b0 + i) * ldw + r] : 0.0;
#pragma unroll
    for (int j = 0; j < kTileSets; ++j) v[j] = t0 + j < n_sets ? V[(int64_t)(t0 + j) * ld + r] : 0.0;
#pragma unroll
    for (int i = 0; i < kTileBoot; ++i)
#pragma unroll
      for (int j = 0; j < kTileSets; ++j) acc[i][j] = fma(w[i], v[j], acc[i][j]);
  }

  // across the lanes of a wave: a butterfly, every lane ends with the wave's sum
#pragma unroll
  for (int i = 0; i < kTileBoot; ++i)
#pragma unroll
    for (int j = 0; j < kTileSets; ++j) {
      double x = acc[i][j];
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
      acc[i][j] = x;
    }
  const int wave = tid >> 6, lane = tid & 63;
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < kTileBoot; ++i)
#pragma unroll
      for (int j = 0; j < kTileSets; ++j) wave_sum[wave][i * kTileSets + j] = acc[i][j];
  }
  __syncthreads();
  if (tid < kTile) {
    const int b = b0 + tid / kTileSets, t = t0 + tid % kTileSets;
    if (b < n_boot && t < n_sets) {
      double x = wave_sum[0][tid];
#pragma unroll
      for (int k = 1; k < kSumWaves; ++k) x += wave_sum[k][tid];
      partial[(chunk * n_boot + b) * n_sets + t] = x;
    }
  }
}

__global__ __launch_bounds__(kSumThreads) void callboot_fold(const double* __restrict__ partial, int64_t n_chunks, int64_t n_cells,
                                                             double* __restrict__ out) {
  const int64_t cell = (int64_t)blockIdx.x * kSumThreads + threadIdx.x;
  if (cell >= n_cells) return;
  double x = partial[cell];
  for (int64_t c = 1; c < n_chunks; ++c) x += partial[c * n_cells + cell];
  out[cell] = x;
}

}  // namespace

extern "C" {

/* The replicate weights of a gene's reads: W[b][r] = how many of the n_rows draws of replicate boot_first + b fell on row
 * r.  Queued on the context's stream.  See include/graphkir_hip.h. */
int gk_boot_row_counts(gk_ctx* ctx, int64_t n_rows, int32_t n_boot, int32_t boot_first, uint64_t seed, uint32_t stream,
                       gk_dptr d_W, int64_t ldw) {
  gk_bind(ctx);
  GK_REQUIRE(ctx && d_W, "null pointer");
  GK_REQUIRE(n_rows >= 1 && n_rows < (1ll << 31), "call bootstrap: the number of reads must lie in 1 .. 2^31 - 1");
  GK_REQUIRE(n_boot >= 1 && n_boot <= kMaxBoot, "the number of bootstrap replicates must lie in 1 .. 10000");
  GK_REQUIRE(boot_first >= 0, "call bootstrap: the first replicate cannot be negative");
  GK_REQUIRE(ldw >= n_rows, "call bootstrap: a row of the weights is shorter than the reads");
  uint32_t* W = gk_ptr<uint32_t>(d_W);
  hipStream_t st = ctx->stream;
  GK_HIP(hipMemset2DAsync(W, (size_t)ldw * sizeof(uint32_t), 0, (size_t)n_rows * sizeof(uint32_t), (size_t)n_boot, st));
  const uint32_t chunks = (uint32_t)((n_rows + kDrawChunk - 1) / kDrawChunk);
  GK_PROF(ctx, "callboot_draw", GK_KERNEL(callboot_draw, dim3(std::min(chunks, kDrawMaxGroups), (unsigned)n_boot), dim3(kDrawThreads),
                                          0, st, (uint32_t)n_rows, (uint32_t)boot_first, seed, stream, W, ldw));
  GK_HIP(hipGetLastError());
  return GK_OK;
}

/* out[b * n_sets + t] = sum_r W[b][r] * V[t][r] in one fixed order; waits for the result.  See include/graphkir_hip.h. */
int gk_weighted_sums(gk_ctx* ctx, gk_dptr d_V, int64_t ld, int64_t n_rows, int32_t n_sets, gk_dptr d_W, int64_t ldw,
                     int32_t n_boot, double* out) {
  gk_bind(ctx);
  GK_REQUIRE(ctx && d_V && d_W && out, "null pointer");
  GK_REQUIRE(n_rows >= 1 && n_rows < (1ll << 31), "call bootstrap: the number of reads must lie in 1 .. 2^31 - 1");
  GK_REQUIRE(n_sets >= 1 && n_sets <= kMaxSets, "call bootstrap: the number of candidate sets must lie in 1 .. 256");
  GK_REQUIRE(n_boot >= 1 && n_boot <= kMaxBoot, "the number of bootstrap replicates must lie in 1 .. 10000");
  GK_REQUIRE(ld >= n_rows && ldw >= n_rows, "call bootstrap: a row of a table is shorter than the reads");
  const int64_t n_chunks = (n_rows + kSumChunk - 1) / kSumChunk;
  const int tiles_boot = (n_boot + kTileBoot - 1) / kTileBoot, tiles_sets = (n_sets + kTileSets - 1) / kTileSets;
  const int64_t n_groups = n_chunks * tiles_boot * tiles_sets;
  const int64_t n_cells = (int64_t)n_boot * n_sets;
  if (n_groups > 0x7FFFFFFFll || n_chunks * n_cells > (1ll << 28)) {
    gk_set_error("call bootstrap: %lld reads x %d replicates x %d sets in one call: pass the replicates in slices",
                 (long long)n_rows, (int)n_boot, (int)n_sets);
    return GK_ERR_CAPACITY;
  }
  hipStream_t st = ctx->stream;
  GkCall call(ctx);
  double *d_partial = nullptr, *d_out = nullptr;
  if (call.take(&d_partial, (size_t)(n_chunks * n_cells) * sizeof(double)) != hipSuccess) {
    gk_set_error("out of device memory for the partial sums of a call bootstrap");
    return GK_ERR_HIP;
  }
  if (call.take(&d_out, (size_t)n_cells * sizeof(double)) != hipSuccess) {
    gk_set_error("out of device memory for the sums of a call bootstrap");
    return GK_ERR_HIP;
  }
  GK_PROF(ctx, "callboot_sums", GK_KERNEL(callboot_sums, dim3((unsigned)n_groups), dim3(kSumThreads), 0, st,
                                          gk_ptr<const double>(d_V), ld, n_rows, (int)n_sets, gk_ptr<const uint32_t>(d_W), ldw,
                                          (int)n_boot, tiles_boot, tiles_sets, d_partial));
  GK_PROF(ctx, "callboot_fold", GK_KERNEL(callboot_fold, dim3((unsigned)((n_cells + kSumThreads - 1) / kSumThreads)),
                                          dim3(kSumThreads), 0, st, d_partial, n_chunks, n_cells, d_out));
  GK_TRY("call bootstrap: weighted sums", hipGetLastError());
  GK_TRY("call bootstrap: weighted sums", call.fetch(out, d_out, (size_t)n_cells * sizeof(double)));
  GK_TRY("call bootstrap: weighted sums", call.wait());
  return GK_OK;
}

}  // extern "C"
