// Fit report of a likelihood call: how the called set explains the reads, in exact integers, from the u8 mismatch table
// the search left in HBM (gk_call_fit, gk_call_fit_extra).  No search runs again.
//
// The search's value of a set S is c N - (3 + c) M(S), c = log10(.999), N = the reads' listed variants, M(S) = sum_r
// min_{a in S} miss8[a][r] (gk_bound.hip): one mismatching observation is worth about 2.9996.  So
//
//   callfit_profile  over the K distinct called columns (1 .. 16): per read m1 = the smallest byte, A = the columns that
//                    hold it, second = the smallest byte outside A.  hist[18] of m1 (bins 0 .. 15, 16 .. 254, 255), M = sum
//                    m1 (bytes as stored, 255 included, as gk_bound_step sums them), per column best = reads with k in A,
//                    unique = reads with A == {k}, only = sum over those of second - m1 = M(S \ {k}) - M(S); optionally
//                    d_min[r] = m1.
//   callfit_extra    with[a] = sum_r min(d_min[r], miss8[a][r]) for every column a of the table: M of the called set with
//                    a as one more copy.  min(x, y) = (x + y - |x - y|) / 2, so a 16-byte word of 16 reads costs four
//                    v_sad_u8 against d_min and four against zero (gk_bound.hip's identity, restated: that file's digest
//                    pins committed profiles).
//
// Lanes run across rows: a lane takes kFitLaneRows = 16 rows of a column per 16-byte load (columns start 64-byte aligned,
// ldm % 64 == 0), a workgroup kFitChunk = 4096 rows per turn, and the grid strides over the chunks.  The loads of a turn --
// one per column -- are issued together and unconditionally: a lane whose rows lie beyond the end reads row 0 and a column
// beyond the list reads the last listed one ("what reading the ISA gave"); such rows and columns are
// masked out of every count, so the padding of the table may hold anything.  Almost every read has m1 == 0 on one or two
// columns: a lane counts bin 0, M and the per-column figures in registers (u32: a lane sees at most 4096 rows), a wave
// adds them with shuffles, the workgroup through LDS, and then there is ONE 64-bit atomicAdd per non-zero counter and
// workgroup.  The rare reads with m1 > 0 go to a histogram in LDS (18 counters with a runtime index would leave the
// registers).  Integer adds only: exact whatever the schedule.  The library zeroes the counters on the stream first.
// tests/test_gpu_call_fit.py takes its shapes from kFitChunk (4096), the lane's 16 rows, the wave (64) and kExtraCols (16):
// move them together.
#include <algorithm>

#include "gk_called.h"
#include "gk_calls.h"

namespace {

constexpr int kFitThreads = 256;
constexpr int kFitWaves = kFitThreads / 64;
constexpr int kFitLaneRows = 16;                          // rows of a 16-byte load
constexpr int kFitChunk = kFitThreads * kFitLaneRows;     // rows of a workgroup per turn (4096)
constexpr int64_t kFitMaxGroups = 2048;                   // workgroups; they stride over the chunks beyond
constexpr int kFitBins = 18;
constexpr int kFitCounters = kFitBins + 1 + 3 * kCalledMaxCols;      // hist, M, [column][best, unique, only]
constexpr int kExtraCols = 16;                            // columns of a workgroup of callfit_extra

// KT: the columns a lane loads per turn, K <= KT of them listed
template <int KT>
__global__ __launch_bounds__(kFitThreads) void callfit_profile(const uint8_t* __restrict__ miss8, int64_t ldm, int64_t n_rows,
                                                               GkCalledCols cols, int K, unsigned long long* __restrict__ out,
                                                               uint8_t* __restrict__ d_min) {
  constexpr int kLane = 2 + 3 * KT;      // a lane's counters: bin 0, M, best / unique / only of KT columns
  __shared__ uint32_t lds_hist[kFitBins];
  __shared__ uint32_t wave_part[kFitWaves][kLane];
  const int tid = threadIdx.x;
  if (tid < kFitBins) lds_hist[tid] = 0;
  __syncthreads();

  const uint8_t* col[KT];
#pragma unroll
  for (int k = 0; k < KT; ++k) col[k] = miss8 + (int64_t)cols.c[min(k, K - 1)] * ldm;

  uint32_t bin0 = 0, msum = 0, best[KT], uniq[KT], only[KT];
#pragma unroll
  for (int k = 0; k < KT; ++k) best[k] = uniq[k] = only[k] = 0;

  const int64_t stride = (int64_t)gridDim.x * kFitChunk;
  for (int64_t begin = (int64_t)blockIdx.x * kFitChunk; begin < n_rows; begin += stride) {
    const int64_t r0 = begin + (int64_t)tid * kFitLaneRows;
    const int64_t left = n_rows - r0;
    const int nv = left >= kFitLaneRows ? kFitLaneRows : left > 0 ? (int)left : 0;      // rows of this lane that count
    const int64_t at = nv ? r0 : 0;                     // r0 < n_rows <= ldm, both multiples of 16: r0 + 16 <= ldm
    uint32_t w[KT][4];
#pragma unroll
    for (int k = 0; k < KT; ++k) {
      const uint4 v = *reinterpret_cast<const uint4*>(col[k] + at);
      w[k][0] = v.x; w[k][1] = v.y; w[k][2] = v.z; w[k][3] = v.w;
    }
    // one row (byte) at a time, the words shifted through w[k][0]: rolled loops keep the registers to the loaded words
    // and the counters (unrolled over the 16 rows, the compiler kept every row's compare masks alive and spilled)
    uint32_t mins[4] = {0, 0, 0, 0};
#pragma unroll 1
    for (int q = 0; q < 4; ++q) {
      uint32_t cur[KT], mw = 0;
#pragma unroll
      for (int k = 0; k < KT; ++k) {
        cur[k] = w[k][0];
        w[k][0] = w[k][1]; w[k][1] = w[k][2]; w[k][2] = w[k][3];
      }
#pragma unroll 1
      for (int s = 0; s < 4; ++s) {
        const bool valid = 4 * q + s < nv;
        uint32_t b[KT];
#pragma unroll
        for (int k = 0; k < KT; ++k) {
          b[k] = k < K ? cur[k] & 255u : 256u;      // a column beyond the list never wins
          cur[k] >>= 8;
        }
        uint32_t m1 = b[0];
#pragma unroll
        for (int k = 1; k < KT; ++k) m1 = min(m1, b[k]);
        uint32_t ties = 0, second = 256u;
#pragma unroll
        for (int k = 0; k < KT; ++k) {
          ties += b[k] == m1;
          second = min(second, b[k] == m1 ? 256u : b[k]);
        }
        mw = (mw >> 8) | (m1 << 24);
        const bool single = valid && ties == 1;
        const uint32_t gain = K > 1 ? second - m1 : 0u;      // ties == 1 among K > 1 columns: second <= 255
#pragma unroll
        for (int k = 0; k < KT; ++k) {
          const bool hit = b[k] == m1;
          best[k] += valid && hit;
          uniq[k] += single && hit;
          only[k] += single && hit ? gain : 0u;
        }
        bin0 += valid && m1 == 0;
        msum += valid ? m1 : 0u;
        if (valid && m1 != 0) atomicAdd(&lds_hist[m1 < 16 ? m1 : m1 == 255 ? 17 : 16], 1u);      // rare
      }
      mins[0] = mins[1]; mins[1] = mins[2]; mins[2] = mins[3]; mins[3] = mw;
    }
    if (d_min != nullptr) {
      if (nv == kFitLaneRows) {
        *reinterpret_cast<uint4*>(d_min + r0) = make_uint4(mins[0], mins[1], mins[2], mins[3]);
      } else {
        for (int i = 0; i < nv; ++i) d_min[r0 + i] = (uint8_t)(mins[i >> 2] >> (8 * (i & 3)));
      }
    }
  }

  // lanes -> wave -> workgroup -> one atomicAdd per non-zero counter
  const int wave = tid >> 6, lane = tid & 63;
  bin0 = wave_sum(bin0);
  msum = wave_sum(msum);
#pragma unroll
  for (int k = 0; k < KT; ++k) {
    best[k] = wave_sum(best[k]);
    uniq[k] = wave_sum(uniq[k]);
    only[k] = wave_sum(only[k]);
  }
  if (lane == 0) {
    wave_part[wave][0] = bin0;
    wave_part[wave][1] = msum;
#pragma unroll
    for (int k = 0; k < KT; ++k) {
      wave_part[wave][2 + 3 * k] = best[k];
      wave_part[wave][3 + 3 * k] = uniq[k];
      wave_part[wave][4 + 3 * k] = only[k];
    }
  }
  __syncthreads();
  if (tid < kLane) {
    uint32_t x = wave_part[0][tid];
#pragma unroll
    for (int v = 1; v < kFitWaves; ++v) x += wave_part[v][tid];
    // bin 0 -> out[0], M -> out[18], column k's three -> out[19 + 3 k ..]
    const int slot = tid == 0 ? 0 : kFitBins + tid - 1;
    if (x != 0 && (tid < 2 || (tid - 2) / 3 < K)) atomicAdd(&out[slot], (unsigned long long)x);
  }
  if (tid >= 64 && tid < 64 + kFitBins - 1) {      // bins 1 .. 17, by lanes of another wave
    const int bin = tid - 63;
    const uint32_t x = lds_hist[bin];
    if (x != 0) atomicAdd(&out[bin], (unsigned long long)x);
  }
}

// a workgroup: kExtraCols columns from tile * kExtraCols on, the chunks slice, slice + n_slices, ...
__global__ __launch_bounds__(kFitThreads) void callfit_extra(const uint8_t* __restrict__ miss8, int64_t ldm, int64_t n_rows,
                                                             int n_table_cols, const uint8_t* __restrict__ d_min, int n_tiles,
                                                             int n_slices, unsigned long long* __restrict__ with) {
  __shared__ uint32_t wave_part[kFitWaves][kExtraCols];
  const int tid = threadIdx.x;
  const int tile = blockIdx.x % n_tiles, slice = blockIdx.x / n_tiles;      // tiles fastest: they share d_min's lines
  const int a0 = tile * kExtraCols;
  const uint8_t* col[kExtraCols];
#pragma unroll
  for (int j = 0; j < kExtraCols; ++j) col[j] = miss8 + (int64_t)min(a0 + j, n_table_cols - 1) * ldm;

  // twice the sum of the minima: sum d + sum x - sum |d - x| over the lane's rows
  uint32_t twice[kExtraCols];
#pragma unroll
  for (int j = 0; j < kExtraCols; ++j) twice[j] = 0;

  const int64_t stride = (int64_t)n_slices * kFitChunk;
  for (int64_t begin = (int64_t)slice * kFitChunk; begin < n_rows; begin += stride) {
    const int64_t r0 = begin + (int64_t)tid * kFitLaneRows;
    const int64_t left = n_rows - r0;
    const int nv = left >= kFitLaneRows ? kFitLaneRows : left > 0 ? (int)left : 0;
    const int64_t at = nv ? r0 : 0;
    // d_min holds n_rows bytes and no more: the last lane with rows reads them one by one
    uint32_t d[4];
    if (nv == kFitLaneRows) {
      const uint4 v = *reinterpret_cast<const uint4*>(d_min + at);
      d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    } else {
      d[0] = d[1] = d[2] = d[3] = 0;
      for (int i = 0; i < nv; ++i) d[i >> 2] |= (uint32_t)d_min[at + i] << (8 * (i & 3));
    }
    uint4 x[kExtraCols];
#pragma unroll
    for (int j = 0; j < kExtraCols; ++j) x[j] = *reinterpret_cast<const uint4*>(col[j] + at);
    uint32_t keep[4], dsum = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      keep[q] = row_mask(nv, q);
      dsum = sad4(d[q], 0, dsum);
    }
#pragma unroll
    for (int j = 0; j < kExtraCols; ++j) {
      const uint32_t xw[4] = {x[j].x & keep[0], x[j].y & keep[1], x[j].z & keep[2], x[j].w & keep[3]};
      uint32_t plus = dsum, minus = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        plus = sad4(xw[q], 0, plus);
        minus = sad4(xw[q], d[q], minus);
      }
      twice[j] += plus - minus;
    }
  }

  const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int j = 0; j < kExtraCols; ++j) {
    const uint32_t x = wave_sum(twice[j]);
    if (lane == 0) wave_part[wave][j] = x;
  }
  __syncthreads();
  if (tid < kExtraCols && a0 + tid < n_table_cols) {
    uint32_t x = wave_part[0][tid];
#pragma unroll
    for (int v = 1; v < kFitWaves; ++v) x += wave_part[v][tid];
    if (x != 0) atomicAdd(&with[a0 + tid], (unsigned long long)(x >> 1));
  }
}

}  // namespace

extern "C" {

/* The fit of the called columns; waits for the result.  See include/graphkir_hip.h. */
int gk_call_fit(gk_ctx* ctx, gk_dptr d_miss8, int64_t ldm, int64_t n_rows, int32_t n_table_cols, const int32_t* cols,
                int32_t n_cols, uint64_t* hist_out, uint64_t* col_out, uint64_t* m_out, gk_dptr d_min) {
  gk_bind(ctx);
  GK_REQUIRE(ctx && cols && hist_out && col_out && m_out, "null pointer");
  GkCalledCols fc;
  const int bad = gk_called_cols("call fit", d_miss8, ldm, n_rows, n_table_cols, cols, n_cols, &fc, [&]() -> int {
    GK_REQUIRE(d_min % 16 == 0, "call fit: d_min must be 16-byte aligned");
    return GK_OK;
  });
  if (bad) return bad;
  hipStream_t st = ctx->stream;
  unsigned long long host[kFitCounters];      // before the record that delivers into it (GkCall::fetch)
  GkCall call(ctx);
  unsigned long long* d_out = nullptr;
  if (call.take(&d_out, kFitCounters * sizeof(unsigned long long)) != hipSuccess) {
    gk_set_error("out of device memory for the counters of a call fit");
    return GK_ERR_HIP;
  }
  GK_TRY("call fit", hipMemsetAsync(d_out, 0, kFitCounters * sizeof(unsigned long long), st));
  {
    const int64_t chunks = (n_rows + kFitChunk - 1) / kFitChunk;
    const dim3 grid((unsigned)std::min(chunks, kFitMaxGroups)), block(kFitThreads);
    const uint8_t* m = gk_ptr<const uint8_t>(d_miss8);
    uint8_t* dm = gk_ptr<uint8_t>(d_min);
#define GK_FIT_LAUNCH(KT) \
  GK_PROF(ctx, "callfit_profile", GK_KERNEL(callfit_profile<KT>, grid, block, 0, st, m, ldm, n_rows, fc, (int)n_cols, d_out, dm))
    GK_CALLED_LAUNCH(n_cols, GK_FIT_LAUNCH)
#undef GK_FIT_LAUNCH
  }
  GK_TRY("call fit", hipGetLastError());
  GK_TRY("call fit", call.fetch(host, d_out, sizeof(host)));
  GK_TRY("call fit", call.wait());
  for (int i = 0; i < kFitBins; ++i) hist_out[i] = host[i];
  m_out[0] = host[kFitBins];
  for (int i = 0; i < 3 * n_cols; ++i) col_out[i] = host[kFitBins + 1 + i];
  return GK_OK;
}

/* with_out[a] = sum_r min(d_min[r], miss8[a][r]); waits for the result.  See include/graphkir_hip.h. */
int gk_call_fit_extra(gk_ctx* ctx, gk_dptr d_miss8, int64_t ldm, int64_t n_rows, int32_t n_table_cols, gk_dptr d_min,
                      uint64_t* with_out) {
  gk_bind(ctx);
  GK_REQUIRE(ctx && d_min && with_out, "null pointer");
  GK_REQUIRE(gk_called_table_ok(d_miss8, ldm, n_rows, n_table_cols),
             "call fit: needs a 16-byte aligned table, 1 <= n_rows < 2^31 and n_rows <= ldm, a multiple of 64");
  GK_REQUIRE(d_min % 16 == 0, "call fit: d_min must be 16-byte aligned");
  const int64_t chunks = (n_rows + kFitChunk - 1) / kFitChunk;
  const int64_t n_tiles = ((int64_t)n_table_cols + kExtraCols - 1) / kExtraCols;
  const int64_t n_slices = std::min(chunks, std::max<int64_t>(1, kFitMaxGroups / n_tiles));
  GK_REQUIRE(n_tiles * n_slices <= 0x7FFFFFFFll, "call fit: too many columns for one call");
  hipStream_t st = ctx->stream;
  unsigned long long* d_with = nullptr;
  const size_t bytes = (size_t)n_table_cols * sizeof(unsigned long long);
  GkCall call(ctx);
  if (call.take(&d_with, bytes) != hipSuccess) {
    gk_set_error("out of device memory for the sums of a call fit");
    return GK_ERR_HIP;
  }
  GK_TRY("call fit: extra copies", hipMemsetAsync(d_with, 0, bytes, st));
  GK_PROF(ctx, "callfit_extra", GK_KERNEL(callfit_extra, dim3((unsigned)(n_tiles * n_slices)), dim3(kFitThreads), 0, st,
                                          gk_ptr<const uint8_t>(d_miss8), ldm, n_rows, (int)n_table_cols,
                                          gk_ptr<const uint8_t>(d_min), (int)n_tiles, (int)n_slices, d_with));
  GK_TRY("call fit: extra copies", hipGetLastError());
  GK_TRY("call fit: extra copies", call.fetch(with_out, d_with, bytes));
  GK_TRY("call fit: extra copies", call.wait());
  return GK_OK;
}

}  // extern "C"
