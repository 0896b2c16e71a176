// Alternatives of a likelihood call: what the reads say about replacing ONE called allele by any other allele of the table,
// in exact integers, from the u8 mismatch table the search left in HBM (gk_call_swap).  No search runs again.
//
// S = the K distinct called columns (1 .. 16), b_k[r] = miss8[cols[k]][r], m1[r] = min_k b_k[r], M = sum_r m1[r] (bytes as
// stored, 255 included, as gk_bound.hip and gk_callfit.hip sum them).  The swap S(k -> a) puts column a in the place of k:
// new[r] = min(rest_k[r], miss8[a][r]) with rest_k[r] = min_{j != k} b_j[r] (255 when K == 1), and
//
//   loss[k][a] = sum_r max(0, new - m1)     rows_for[k][a] = #{r : new > m1}      the reads that prefer k
//   gain[a]    = sum_r max(0, m1 - new)     rows_against[a] = #{r : new < m1}     (new < m1 <=> miss8[a][r] < m1[r]: no k)
//
// so that loss[k][a] - gain[a] = M(S(k -> a)) - M(S).  Three bytes per row carry every k:
//
//   callswap_rows   m1, m2 = the smallest byte outside the unique holder of m1 (255 when K == 1; m1 itself on a tie) and
//                   own = the index k of that unique holder, 255 on a tie.  rest_k[r] is m2[r] where own[r] == k and m1[r]
//                   elsewhere.  Also M and the rows with m1 == 255.
//   callswap_sums   for a tile of table columns and all K called alleles at once.  With x = miss8[a][r]:
//                   max(0, m1 - new) = m1 -sat x, and on a row that k owns max(0, new - m1) = min(x, m2) -sat m1, 0 on
//                   every other row.  Both are formed ONCE per column, sixteen rows to a 16-byte word, with packed u16
//                   min / saturating subtract on the even and the odd bytes; every k then costs an AND with the bytes it
//                   owns and a v_sad_u8 against zero, for the sum and for the count (the bytes clamped to 1).  The tile is
//                   32 / KT columns (at most 16), so the loss / rows_for counters stay 2 x 32 registers for every KT.
//
// Lanes run across rows: a lane takes kSwapLaneRows = 16 rows of a column per 16-byte load (columns start 64-byte aligned,
// ldm % 64 == 0), a workgroup kSwapChunk = 4096 rows per turn.  The loads of a turn are issued together and unconditionally:
// a lane whose rows lie beyond the end reads row 0, a column beyond the list or the table reads the last one; such rows and
// columns are masked out of every count, so the padding of the table may hold anything, and nothing at or beyond n_rows is
// written.  The state of the rows is read back in whole 16-byte words (its buffer has ldm bytes per plane) and masked.
//
// The 32-bit counters of a lane: n_rows < 2^31 (GK_REQUIRE) is at most 2^19 chunks; callswap_rows runs min(chunks,
// kSwapMaxGroups = 2048) workgroups and callswap_sums at least chunks / kSwapMaxTurns slices per tile, so a lane takes at
// most kSwapMaxTurns = 256 turns = 4096 rows of at most 255 each (a saturated difference of two bytes; callfit's doubled
// 255 + 255 does not arise): 1 044 480 per lane, x 64 lanes x 4 waves = 267 386 880 < 2^32.  Then there is ONE 64-bit
// atomicAdd per non-zero counter and workgroup.  Integer adds only: exact whatever the schedule.  The library zeroes the
// counters on the stream first.
// tests/test_gpu_call_alternatives.py takes its shapes from kSwapChunk (4096), the lane's 16 rows, the wave (64) and the
// tiles 32 / KT (16, 16, 8, 4, 2 columns for KT = 1, 2, 4, 8, 16): move them together.
#include <algorithm>

#include "gk_called.h"
#include "gk_calls.h"

namespace {

constexpr int kSwapThreads = 256;
constexpr int kSwapWaves = kSwapThreads / 64;
constexpr int kSwapLaneRows = 16;                          // rows of a 16-byte load
constexpr int kSwapChunk = kSwapThreads * kSwapLaneRows;   // rows of a workgroup per turn (4096)
constexpr int64_t kSwapMaxGroups = 2048;                   // workgroups; they stride over the chunks beyond
constexpr int64_t kSwapMaxTurns = (1ll << 31) / kSwapChunk / kSwapMaxGroups;      // 256: the turns of a lane
constexpr int kSwapNone = 255;                             // own: no unique holder

// columns of a workgroup of callswap_sums
constexpr int swapTile(int KT) { return 32 / KT < 16 ? 32 / KT : 16; }

typedef unsigned short swap_u16x2 __attribute__((ext_vector_type(2)));

// per 16-bit half: max(0, a - b) and min(a, b)
__device__ inline uint32_t swap_subsat(uint32_t a, uint32_t b) {
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_sub_sat(__builtin_bit_cast(swap_u16x2, a), __builtin_bit_cast(swap_u16x2, b)));
}
__device__ inline uint32_t swap_min(uint32_t a, uint32_t b) {
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(swap_u16x2, a), __builtin_bit_cast(swap_u16x2, b)));
}

// 0xFF in every byte of `w` that equals `k`
__device__ inline uint32_t swap_bytes_equal(uint32_t w, uint32_t k) {
  const uint32_t t = w ^ (k * 0x01010101u);
  const uint32_t nz = (((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t) & 0x80808080u;      // 0x80 in the bytes that differ
  return ((nz ^ 0x80808080u) >> 7) * 255u;
}

// KT: the columns a lane loads per turn, K <= KT of them listed.  state: m1 [ld], m2 [ld], own [ld]
template <int KT>
__global__ __launch_bounds__(kSwapThreads) void callswap_rows(const uint8_t* __restrict__ miss8, int64_t ldm, int64_t n_rows,
                                                              GkCalledCols cols, int K, uint8_t* __restrict__ state, int64_t ld,
                                                              unsigned long long* __restrict__ out) {
  __shared__ uint32_t wave_part[kSwapWaves][2];
  __shared__ int64_t col_at[KT];      // in LDS: as 32 scalar registers live across the loop they spilled at 16 columns
  const int tid = threadIdx.x;
  if (tid < KT) col_at[tid] = (int64_t)cols.c[min(tid, K - 1)] * ldm;
  __syncthreads();

  uint32_t msum = 0, beyond = 0;      // M, rows with m1 == 255
  const int64_t stride = (int64_t)gridDim.x * kSwapChunk;
  for (int64_t begin = (int64_t)blockIdx.x * kSwapChunk; begin < n_rows; begin += stride) {
    const int64_t r0 = begin + (int64_t)tid * kSwapLaneRows;
    const int64_t left = n_rows - r0;
    const int nv = left >= kSwapLaneRows ? kSwapLaneRows : left > 0 ? (int)left : 0;      // rows of this lane that count
    const int64_t at = nv ? r0 : 0;                     // r0 < n_rows <= ldm, both multiples of 16: r0 + 16 <= ldm
    uint32_t w[KT][4];
#pragma unroll
    for (int k = 0; k < KT; ++k) {
      const uint4 v = *reinterpret_cast<const uint4*>(miss8 + col_at[k] + at);
      w[k][0] = v.x; w[k][1] = v.y; w[k][2] = v.z; w[k][3] = v.w;
    }
    // one row (byte) at a time, the words shifted through w[k][0]: rolled loops keep the registers to the loaded words
    uint32_t o1[4] = {0, 0, 0, 0}, o2[4] = {0, 0, 0, 0}, oo[4] = {0, 0, 0, 0};
#pragma unroll 1
    for (int q = 0; q < 4; ++q) {
      uint32_t cur[KT], w1 = 0, w2 = 0, wo = 0;
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
        uint32_t ties = 0, holder = 0, second = 255u;
#pragma unroll
        for (int k = 0; k < KT; ++k) {
          const bool hit = b[k] == m1;
          ties += hit;
          holder += hit ? (uint32_t)k : 0u;
          second = min(second, hit ? 255u : b[k]);      // a column beyond the list holds 256
        }
        const bool single = ties == 1;
        w1 = (w1 >> 8) | (m1 << 24);
        w2 = (w2 >> 8) | ((single ? second : m1) << 24);
        wo = (wo >> 8) | ((single ? holder : (uint32_t)kSwapNone) << 24);
        msum += valid ? m1 : 0u;
        beyond += valid && m1 == 255u;
      }
      o1[0] = o1[1]; o1[1] = o1[2]; o1[2] = o1[3]; o1[3] = w1;
      o2[0] = o2[1]; o2[1] = o2[2]; o2[2] = o2[3]; o2[3] = w2;
      oo[0] = oo[1]; oo[1] = oo[2]; oo[2] = oo[3]; oo[3] = wo;
    }
    if (nv == kSwapLaneRows) {
      *reinterpret_cast<uint4*>(state + r0) = make_uint4(o1[0], o1[1], o1[2], o1[3]);
      *reinterpret_cast<uint4*>(state + ld + r0) = make_uint4(o2[0], o2[1], o2[2], o2[3]);
      *reinterpret_cast<uint4*>(state + 2 * ld + r0) = make_uint4(oo[0], oo[1], oo[2], oo[3]);
    } else {
      for (int i = 0; i < nv; ++i) {
        const int sh = 8 * (i & 3);
        state[r0 + i] = (uint8_t)(o1[i >> 2] >> sh);
        state[ld + r0 + i] = (uint8_t)(o2[i >> 2] >> sh);
        state[2 * ld + r0 + i] = (uint8_t)(oo[i >> 2] >> sh);
      }
    }
  }

  const int wave = tid >> 6, lane = tid & 63;
  msum = wave_sum(msum);
  beyond = wave_sum(beyond);
  if (lane == 0) {
    wave_part[wave][0] = msum;
    wave_part[wave][1] = beyond;
  }
  __syncthreads();
  if (tid < 2) {
    uint32_t x = wave_part[0][tid];
#pragma unroll
    for (int v = 1; v < kSwapWaves; ++v) x += wave_part[v][tid];
    if (x != 0) atomicAdd(&out[tid], (unsigned long long)x);
  }
}

// a workgroup: swapTile(KT) columns from tile * swapTile(KT) on, the chunks slice, slice + n_slices, ...
// out: gain [A], rows_against [A], loss [K][A], rows_for [K][A], A = n_table_cols
template <int KT>
__global__ __launch_bounds__(kSwapThreads) void callswap_sums(const uint8_t* __restrict__ miss8, int64_t ldm, int64_t n_rows,
                                                              int n_table_cols, const uint8_t* __restrict__ state, int64_t ld,
                                                              int K, int n_tiles, int n_slices,
                                                              unsigned long long* __restrict__ out) {
  constexpr int T = swapTile(KT);
  constexpr int kCounters = 2 * T + 2 * KT * T;      // gain, against, loss [KT][T], for [KT][T]
  __shared__ uint32_t wave_part[kSwapWaves][kCounters];
  const int tid = threadIdx.x;
  const int tile = blockIdx.x % n_tiles, slice = blockIdx.x / n_tiles;      // tiles fastest: they share the state's lines
  const int a0 = tile * T;
  const uint8_t* col[T];
#pragma unroll
  for (int j = 0; j < T; ++j) col[j] = miss8 + (int64_t)min(a0 + j, n_table_cols - 1) * ldm;

  uint32_t gain[T], against[T], loss[KT][T], rows_for[KT][T];
#pragma unroll
  for (int j = 0; j < T; ++j) {
    gain[j] = against[j] = 0;
#pragma unroll
    for (int k = 0; k < KT; ++k) loss[k][j] = rows_for[k][j] = 0;
  }

  const int64_t stride = (int64_t)n_slices * kSwapChunk;
  for (int64_t begin = (int64_t)slice * kSwapChunk; begin < n_rows; begin += stride) {
    const int64_t r0 = begin + (int64_t)tid * kSwapLaneRows;
    const int64_t left = n_rows - r0;
    const int nv = left >= kSwapLaneRows ? kSwapLaneRows : left > 0 ? (int)left : 0;
    const int64_t at = nv ? r0 : 0;
    const uint4 s1 = *reinterpret_cast<const uint4*>(state + at);
    const uint4 s2 = *reinterpret_cast<const uint4*>(state + ld + at);
    const uint4 so = *reinterpret_cast<const uint4*>(state + 2 * ld + at);
    uint4 x[T];
#pragma unroll
    for (int j = 0; j < T; ++j) x[j] = *reinterpret_cast<const uint4*>(col[j] + at);
    // rows beyond the end: m1 = m2 = 0 gives no difference either way, and nobody owns them
    const uint32_t m1w[4] = {s1.x, s1.y, s1.z, s1.w}, m2w[4] = {s2.x, s2.y, s2.z, s2.w}, ow[4] = {so.x, so.y, so.z, so.w};
    uint32_t m1e[4], m1o[4], m2e[4], m2o[4], mine[KT][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t keep = row_mask(nv, q);
      m1e[q] = m1w[q] & keep & 0x00FF00FFu;
      m1o[q] = m1w[q] & keep & 0xFF00FF00u;
      m2e[q] = m2w[q] & keep & 0x00FF00FFu;
      m2o[q] = m2w[q] & keep & 0xFF00FF00u;
      const uint32_t owner = ow[q] | ~keep;
#pragma unroll
      for (int k = 0; k < KT; ++k) mine[k][q] = swap_bytes_equal(owner, (uint32_t)k);
    }
#pragma unroll
    for (int j = 0; j < T; ++j) {
      const uint32_t xw[4] = {x[j].x, x[j].y, x[j].z, x[j].w};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t xe = xw[q] & 0x00FF00FFu, xo = xw[q] & 0xFF00FF00u;
        const uint32_t ge = swap_subsat(m1e[q], xe), go = swap_subsat(m1o[q], xo);                       // m1 -sat x
        const uint32_t ce = swap_subsat(swap_min(xe, m2e[q]), m1e[q]), co = swap_subsat(swap_min(xo, m2o[q]), m1o[q]);
        gain[j] = sad4(ge | go, 0, gain[j]);
        against[j] = sad4(swap_min(ge, 0x00010001u) | swap_min(go, 0x01000100u), 0, against[j]);
        const uint32_t c = ce | co;                                                                      // min(x, m2) -sat m1
        const uint32_t g = swap_min(ce, 0x00010001u) | swap_min(co, 0x01000100u);
#pragma unroll
        for (int k = 0; k < KT; ++k) {
          loss[k][j] = sad4(c & mine[k][q], 0, loss[k][j]);
          rows_for[k][j] = sad4(g & mine[k][q], 0, rows_for[k][j]);
        }
      }
    }
  }

  const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int j = 0; j < T; ++j) {
    const uint32_t a = wave_sum(gain[j]), b = wave_sum(against[j]);
    if (lane == 0) {
      wave_part[wave][j] = a;
      wave_part[wave][T + j] = b;
    }
#pragma unroll
    for (int k = 0; k < KT; ++k) {
      const uint32_t c = wave_sum(loss[k][j]), d = wave_sum(rows_for[k][j]);
      if (lane == 0) {
        wave_part[wave][2 * T + k * T + j] = c;
        wave_part[wave][2 * T + KT * T + k * T + j] = d;
      }
    }
  }
  __syncthreads();
  if (tid < kCounters) {
    uint32_t x = wave_part[0][tid];
#pragma unroll
    for (int v = 1; v < kSwapWaves; ++v) x += wave_part[v][tid];
    const int64_t A = n_table_cols;
    const int j = tid % T, part = tid / T;      // part: 0 gain, 1 against, 2 + k loss of k, 2 + KT + k rows_for of k
    const int k = part < 2 ? 0 : (part - 2) % KT;
    const int64_t plane = part < 2 ? part : part < 2 + KT ? 2 + k : 2 + K + k;
    if (x != 0 && a0 + j < n_table_cols && k < K) atomicAdd(&out[plane * A + a0 + j], (unsigned long long)x);
  }
}

}  // namespace

extern "C" {

/* The swaps of every called column against every column of the table; waits for the result.  See include/graphkir_hip.h. */
int gk_call_swap(gk_ctx* ctx, gk_dptr d_miss8, int64_t ldm, int64_t n_rows, int32_t n_table_cols, const int32_t* cols,
                 int32_t n_cols, uint64_t* loss_out, uint64_t* for_out, uint64_t* gain_out, uint64_t* against_out,
                 uint64_t* m_out, uint64_t* out_of_range_out, gk_dptr d_state) {
  gk_bind(ctx);
  GK_REQUIRE(ctx && cols && loss_out && for_out && gain_out && against_out && m_out && out_of_range_out, "null pointer");
  GkCalledCols sc;
  const int bad = gk_called_cols("call swap", d_miss8, ldm, n_rows, n_table_cols, cols, n_cols, &sc, [&]() -> int {
    GK_REQUIRE(d_state % 16 == 0, "call swap: d_state must be 16-byte aligned");
    return GK_OK;
  });
  if (bad) return bad;
  const int kt = calledKT(n_cols);
  const int64_t chunks = (n_rows + kSwapChunk - 1) / kSwapChunk;
  const int64_t n_tiles = ((int64_t)n_table_cols + swapTile(kt) - 1) / swapTile(kt);
  // enough slices to fill the GPU, and never more than kSwapMaxTurns turns for a lane
  const int64_t n_slices = std::max(std::min(chunks, std::max<int64_t>(1, kSwapMaxGroups / n_tiles)),
                                    (chunks + kSwapMaxTurns - 1) / kSwapMaxTurns);
  GK_REQUIRE(n_tiles * n_slices <= 0x7FFFFFFFll, "call swap: too many columns for one call");

  hipStream_t st = ctx->stream;
  unsigned long long head[2] = {0, 0};      // before the record that delivers into it (GkCall::fetch)
  GkCall call(ctx);
  const int64_t A = n_table_cols;
  const size_t n_counters = (size_t)(2 + 2 * A + 2 * (int64_t)n_cols * A);      // M, out of range, then callswap_sums' planes
  unsigned long long* d_out = nullptr;
  if (call.take(&d_out, n_counters * sizeof(unsigned long long)) != hipSuccess) {
    gk_set_error("out of device memory for the counters of a call swap");
    return GK_ERR_HIP;
  }
  uint8_t* state = gk_ptr<uint8_t>(d_state);
  if (state == nullptr && call.take(&state, 3 * (size_t)ldm) != hipSuccess) {
    gk_set_error("out of device memory for the row state of a call swap");
    return GK_ERR_HIP;
  }
  GK_TRY("call swap", hipMemsetAsync(d_out, 0, n_counters * sizeof(unsigned long long), st));
  {
    const dim3 grid_rows((unsigned)std::min(chunks, kSwapMaxGroups)), grid_sums((unsigned)(n_tiles * n_slices)), block(kSwapThreads);
    const uint8_t* m = gk_ptr<const uint8_t>(d_miss8);
#define GK_SWAP_LAUNCH(KT)                                                                                                   \
  do {                                                                                                                       \
    GK_PROF(ctx, "callswap_rows",                                                                                            \
            GK_KERNEL(callswap_rows<KT>, grid_rows, block, 0, st, m, ldm, n_rows, sc, (int)n_cols, state, ldm, d_out));      \
    GK_PROF(ctx, "callswap_sums",                                                                                            \
            GK_KERNEL(callswap_sums<KT>, grid_sums, block, 0, st, m, ldm, n_rows, (int)n_table_cols, (const uint8_t*)state, \
                      ldm, (int)n_cols, (int)n_tiles, (int)n_slices, d_out + 2));                                            \
  } while (0)
    GK_CALLED_LAUNCH(n_cols, GK_SWAP_LAUNCH)
#undef GK_SWAP_LAUNCH
  }
  GK_TRY("call swap", hipGetLastError());
  const size_t plane = (size_t)A * sizeof(unsigned long long);
  GK_TRY("call swap", call.fetch(head, d_out, sizeof(head)));
  GK_TRY("call swap", call.fetch(gain_out, d_out + 2, plane));
  GK_TRY("call swap", call.fetch(against_out, d_out + 2 + A, plane));
  GK_TRY("call swap", call.fetch(loss_out, d_out + 2 + 2 * A, plane * n_cols));
  GK_TRY("call swap", call.fetch(for_out, d_out + 2 + (2 + (int64_t)n_cols) * A, plane * n_cols));
  GK_TRY("call swap", call.wait());
  m_out[0] = head[0];
  out_of_range_out[0] = head[1];
  return GK_OK;
}

}  // extern "C"
