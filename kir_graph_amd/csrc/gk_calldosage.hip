// Copy dosage of a likelihood call: the rows of the u8 mismatch table the search left in HBM, collapsed over the K distinct
// called columns (1 .. 16) into (pattern, count) pairs in exact integers (gk_call_patterns).  No search runs again.
//
// b_k[r] = miss8[cols[k]][r], m1[r] = min_k b_k[r].  A row with m1 == 255 is out of range (gk_call_fit's bin 17) and has
// no pattern; every other row's pattern is the K bytes d_k = b_k - m1 (255 where b_k == 255), zero-extended to 16: what the
// mixture likelihood of call_dosage.py needs of the row, and no more.  A gene's rows take few patterns (a read in shared
// sequence is all-zero, a read private to one allele is zero there and 1 .. 3 elsewhere).
//
//   calldosage_patterns  one pass.  Lanes run across rows as in callfit_profile (gk_callfit.hip; the row loops stay apart,
//                        their registers are counted per kernel: DESIGN.md section 8j): a lane takes kPatLaneRows = 16 rows of a column per 16-byte load,
//                        a workgroup kPatChunk = 4096 rows per turn, the grid strides over the chunks; the K loads of a
//                        turn are issued together and unconditionally (a lane beyond the end reads row 0, a column beyond
//                        the list the last listed one) and such rows and columns are masked, so the padding may hold
//                        anything.
//
// Identity is exact and nobody waits.  A table maps a 64-bit KEY to the slot that holds it: open addressing, the slot
// claimed by ONE compare-and-swap of the key itself on an empty (all bits set) word, read before it is swapped.  The hash
// only says where the probe starts; a key is written once and never changes, so a stale read costs a swap, never the
// result, and no thread ever looks at a word another thread has yet to write.  K <= 8: the pattern IS the key (it has a
// zero byte, so it is never the empty word).  K > 8: the low and the high eight bytes are interned in a table each (eight
// bytes of 255 get the reserved number kAllFF instead of a slot) and the key is the pair of their slot numbers.  Three
// such tables per workgroup live in LDS, three in HBM:
//
//   lane       rows of the all-zero pattern and out-of-range rows are counted in registers; a run of equal patterns among
//              the lane's rows is one (pattern, count);
//   workgroup  runs go to the LDS tables (a u32 add per run; the zero rows once per wave); a run whose key finds no room
//              within kPatLdsProbes = 16 slots of its start goes to HBM directly (in HBM a probe may walk the whole table);
//   grid       at its end a workgroup makes ONE 64-bit add per occupied LDS entry into the HBM table.  A pattern the HBM
//              tables have no room for adds its rows to `unplaced`.
//
// Integer adds only: exact whatever the schedule; sum counts + unplaced + out_of_range == n_rows.  The host reads the
// tables back and turns pairs into bytes.  u32 counters: a workgroup sees at most 2^31 / kPatMaxGroups + kPatChunk < 2^22 rows.
// gfx950, -O3: no scratch and no VGPR spill in any instantiation; VGPRs 14 / 34 / 40 / 60 / 105 for KT = 1 / 2 / 4 / 8 /
// 16, static LDS 12 KiB (16 KiB for KT = 16).  KT = 8 keeps 8 and KT = 16 keeps 74 of its scalars (the column pointers and
// the table addresses live across the row loop) in lanes of a VGPR, not in memory; profiles/r25_call_dosage.txt.
// tests/test_gpu_call_dosage.py takes its shapes from kPatChunk (4096), the lane's 16 rows, the wave (64 x 16 rows),
// kPatMaxGroups (1024), kPatLdsSlots (1024) and kPatLdsProbes (16): move them together.
#include <algorithm>
#include <vector>

#include "gk_called.h"
#include "gk_calls.h"
#include "gk_env.h"

namespace {

constexpr int kPatThreads = 256;
constexpr int kPatLaneRows = 16;                          // rows of a 16-byte load
constexpr int kPatChunk = kPatThreads * kPatLaneRows;     // rows of a workgroup per turn (4096)
constexpr int64_t kPatMaxGroups = 1024;                   // workgroups; they stride over the chunks beyond
constexpr int kPatLdsSlots = 1024;                        // patterns (K <= 8) or pairs (K > 8) of a workgroup in LDS
constexpr uint32_t kPatLdsProbes = 16;                    // slots a key may lie from its start in LDS: a full table costs no more
constexpr int kPatLdsHalf = 256;                          // low / high halves of a workgroup in LDS (K > 8)
constexpr unsigned long long kPatEmpty = ~0ull;
constexpr int kAllFF = 0x7FFFFFFF;                        // the number of a half of eight bytes 255: no slot
constexpr int64_t kPatMinSlots = 16, kPatMaxSlots = 1ll << 24;

// the HBM tables: fin[n], lo[n], hi[n] (lo, hi: K > 8 only), counts[n]; counters[0] = unplaced, [1] = out of range
struct PatGlobal {
  unsigned long long *fin, *lo, *hi, *counts, *counters;
  uint32_t mask;
};

__device__ inline uint64_t pat_mix64(uint64_t x) {
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// The slot of `key` in a table of mask + 1 slots, claimed when the key is new; -1 when the `probes` slots from its start
// all hold other keys (the same answer for the same key ever after: a key lies within `probes` slots or nowhere).
template <int SCOPE>
__device__ inline int pat_intern(unsigned long long* keys, uint32_t mask, unsigned long long key, uint64_t hash_mask,
                                 uint32_t probes) {
  const uint64_t h = pat_mix64(key) & hash_mask;
  uint32_t s = (uint32_t)(h ^ (h >> 32)) & mask;
  for (uint32_t tries = 0; tries < probes; ++tries) {
    unsigned long long prev = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, SCOPE);
    if (prev == kPatEmpty) {
      if (__hip_atomic_compare_exchange_strong(&keys[s], &prev, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, SCOPE)) return (int)s;
    }
    if (prev == key) return (int)s;
    s = (s + 1u) & mask;
  }
  return -1;
}

// the slot of the pattern (lo, hi) in `fin`; -1 when a table is full
template <bool WIDE, int SCOPE>
__device__ inline int pat_slot(unsigned long long* fin, unsigned long long* lo_t, unsigned long long* hi_t, uint32_t mask,
                               uint32_t half_mask, unsigned long long lo, unsigned long long hi, uint64_t hash_mask,
                               uint32_t probes) {
  unsigned long long key = lo;
  if (WIDE) {
    const int a = lo == kPatEmpty ? kAllFF : pat_intern<SCOPE>(lo_t, half_mask, lo, hash_mask, probes);
    if (a < 0) return -1;
    const int b = hi == kPatEmpty ? kAllFF : pat_intern<SCOPE>(hi_t, half_mask, hi, hash_mask, probes);
    if (b < 0) return -1;
    key = ((unsigned long long)(uint32_t)a << 32) | (uint32_t)b;
  }
  return pat_intern<SCOPE>(fin, mask, key, hash_mask, probes);
}

template <bool WIDE>
__device__ inline void pat_add_global(const PatGlobal& g, unsigned long long lo, unsigned long long hi, uint32_t n,
                                      uint64_t hash_mask) {
  const int s = pat_slot<WIDE, __HIP_MEMORY_SCOPE_AGENT>(g.fin, g.lo, g.hi, g.mask, g.mask, lo, hi, hash_mask, g.mask + 1u);
  atomicAdd(s >= 0 ? &g.counts[s] : &g.counters[0], (unsigned long long)n);
}

// KT: the columns a lane loads per turn, K <= KT of them listed
template <int KT>
__global__ __launch_bounds__(kPatThreads) void calldosage_patterns(const uint8_t* __restrict__ miss8, int64_t ldm,
                                                                   int64_t n_rows, GkCalledCols cols, int K, uint64_t hash_mask,
                                                                   PatGlobal g) {
  constexpr bool WIDE = KT > 8;
  constexpr int kWords = KT <= 4 ? 1 : KT / 4;
  constexpr int kHalf = WIDE ? kPatLdsHalf : 1;
  __shared__ unsigned long long lds_fin[kPatLdsSlots];
  __shared__ unsigned long long lds_lo[kHalf], lds_hi[kHalf];
  __shared__ uint32_t lds_cnt[kPatLdsSlots];
  const int tid = threadIdx.x;
  for (int i = tid; i < kPatLdsSlots; i += kPatThreads) { lds_fin[i] = kPatEmpty; lds_cnt[i] = 0; }
  for (int i = tid; i < kHalf; i += kPatThreads) { lds_lo[i] = kPatEmpty; lds_hi[i] = kPatEmpty; }
  __syncthreads();

  // (pattern, rows) into the workgroup's tables, or past them into the grid's
  auto add = [&](unsigned long long lo, unsigned long long hi, uint32_t n) {
    const int s = pat_slot<WIDE, __HIP_MEMORY_SCOPE_WORKGROUP>(lds_fin, lds_lo, lds_hi, kPatLdsSlots - 1, kHalf - 1, lo, hi,
                                                               hash_mask, kPatLdsProbes);
    if (s >= 0) atomicAdd(&lds_cnt[s], n);
    else pat_add_global<WIDE>(g, lo, hi, n, hash_mask);
  };

  const uint8_t* col[KT];
#pragma unroll
  for (int k = 0; k < KT; ++k) col[k] = miss8 + (int64_t)cols.c[min(k, K - 1)] * ldm;

  uint32_t zero = 0, oor = 0, run_n = 0;
  unsigned long long run_lo = 0, run_hi = 0;

  const int64_t stride = (int64_t)gridDim.x * kPatChunk;
  for (int64_t begin = (int64_t)blockIdx.x * kPatChunk; begin < n_rows; begin += stride) {
    const int64_t r0 = begin + (int64_t)tid * kPatLaneRows;
    const int64_t left = n_rows - r0;
    const int nv = left >= kPatLaneRows ? kPatLaneRows : left > 0 ? (int)left : 0;      // rows of this lane that count
    const int64_t at = nv ? r0 : 0;                     // r0 < n_rows <= ldm, both multiples of 16: r0 + 16 <= ldm
    uint32_t w[KT][4];
#pragma unroll
    for (int k = 0; k < KT; ++k) {
      const uint4 v = *reinterpret_cast<const uint4*>(col[k] + at);
      w[k][0] = v.x; w[k][1] = v.y; w[k][2] = v.z; w[k][3] = v.w;
    }
    // one row (byte) at a time, the words shifted through w[k][0], as callfit_profile does: rolled loops keep the
    // registers to the loaded words
#pragma unroll 1
    for (int q = 0; q < 4; ++q) {
      uint32_t cur[KT];
#pragma unroll
      for (int k = 0; k < KT; ++k) {
        cur[k] = w[k][0];
        w[k][0] = w[k][1]; w[k][1] = w[k][2]; w[k][2] = w[k][3];
      }
#pragma unroll 1
      for (int s = 0; s < 4; ++s) {
        uint32_t b[KT];
#pragma unroll
        for (int k = 0; k < KT; ++k) {
          b[k] = k < K ? cur[k] & 255u : 256u;      // a column beyond the list never wins
          cur[k] >>= 8;
        }
        uint32_t m1 = b[0];
#pragma unroll
        for (int k = 1; k < KT; ++k) m1 = min(m1, b[k]);
        uint32_t p[kWords];
#pragma unroll
        for (int i = 0; i < kWords; ++i) p[i] = 0;
#pragma unroll
        for (int k = 0; k < KT; ++k) {
          const uint32_t d = b[k] == 256u ? 0u : b[k] == 255u ? 255u : b[k] - m1;
          p[k / 4] |= d << (8 * (k % 4));
        }
        unsigned long long lo = p[0], hi = 0;
        if (kWords > 1) lo |= (unsigned long long)p[kWords > 1 ? 1 : 0] << 32;
        if (kWords > 2) hi = p[kWords > 2 ? 2 : 0] | ((unsigned long long)p[kWords > 3 ? 3 : 0] << 32);
        if (4 * q + s >= nv) continue;
        if (m1 == 255u) {
          ++oor;
        } else if ((lo | hi) == 0ull) {
          ++zero;
        } else if (run_n != 0 && lo == run_lo && hi == run_hi) {
          ++run_n;
        } else {
          if (run_n != 0) add(run_lo, run_hi, run_n);
          run_lo = lo; run_hi = hi; run_n = 1;
        }
      }
    }
  }
  if (run_n != 0) add(run_lo, run_hi, run_n);
  zero = wave_sum(zero);
  oor = wave_sum(oor);
  if ((tid & 63) == 0) {
    if (zero != 0) add(0ull, 0ull, zero);
    if (oor != 0) atomicAdd(&g.counters[1], (unsigned long long)oor);
  }
  __syncthreads();

  // one 64-bit add per occupied entry of the workgroup's table
  for (int i = tid; i < kPatLdsSlots; i += kPatThreads) {
    const unsigned long long key = lds_fin[i];
    const uint32_t n = lds_cnt[i];
    if (key == kPatEmpty || n == 0) continue;
    unsigned long long lo = key, hi = 0;
    if (WIDE) {
      const uint32_t a = (uint32_t)(key >> 32), b = (uint32_t)key;
      lo = a == (uint32_t)kAllFF ? kPatEmpty : lds_lo[a & (kHalf - 1)];
      hi = b == (uint32_t)kAllFF ? kPatEmpty : lds_hi[b & (kHalf - 1)];
    }
    pat_add_global<WIDE>(g, lo, hi, n, hash_mask);
  }
}

}  // namespace

extern "C" {

/* The patterns of the called columns and their row counts; waits for the result.  See include/graphkir_hip.h. */
int gk_call_patterns(gk_ctx* ctx, gk_dptr d_miss8, int64_t ldm, int64_t n_rows, int32_t n_table_cols, const int32_t* cols,
                     int32_t n_cols, int64_t n_slots, uint8_t* patterns_out, uint64_t* counts_out, int64_t* n_out,
                     uint64_t* out_of_range_out, uint64_t* unplaced_out) {
  gk_bind(ctx);
  GK_REQUIRE(ctx && cols && patterns_out && counts_out && n_out && out_of_range_out && unplaced_out, "null pointer");
  GkCalledCols pc;
  const int bad = gk_called_cols("call patterns", d_miss8, ldm, n_rows, n_table_cols, cols, n_cols, &pc, [&]() -> int {
    GK_REQUIRE(n_slots >= kPatMinSlots && n_slots <= kPatMaxSlots && (n_slots & (n_slots - 1)) == 0,
               "call patterns: the slots must be a power of two in 16 .. 2^24");
    return GK_OK;
  });
  if (bad) return bad;
  // GK_TEST_HOOKS=calldosage_hashbits=N: the hash cut to N bits, so that different keys start their probes in one slot
  const long bits = gk_test_hook_value("calldosage_hashbits", 64);
  const uint64_t hash_mask = bits >= 64 ? ~0ull : bits <= 0 ? 0ull : (1ull << bits) - 1ull;
  const bool wide = n_cols > 8;
  const size_t n = (size_t)n_slots, n_key_tables = wide ? 3 : 1;
  const size_t key_bytes = n_key_tables * n * sizeof(unsigned long long), count_bytes = (n + 2) * sizeof(unsigned long long);
  hipStream_t st = ctx->stream;
  std::vector<unsigned long long> keys, counts;      // before the record that delivers into them (GkCall::fetch)
  GkCall call(ctx);
  unsigned long long *d_keys = nullptr, *d_counts = nullptr;      // [fin | lo | hi]; [counts | unplaced, out of range]
  if (call.take(&d_keys, key_bytes) != hipSuccess || call.take(&d_counts, count_bytes) != hipSuccess) {
    gk_set_error("out of device memory for the pattern tables of a call dosage");
    return GK_ERR_HIP;
  }
  GK_TRY("call patterns", hipMemsetAsync(d_keys, 0xFF, key_bytes, st));
  GK_TRY("call patterns", hipMemsetAsync(d_counts, 0, count_bytes, st));
  {
    PatGlobal g;
    g.fin = d_keys; g.lo = wide ? d_keys + n : d_keys; g.hi = wide ? d_keys + 2 * n : d_keys;
    g.counts = d_counts; g.counters = d_counts + n; g.mask = (uint32_t)(n - 1);
    const int64_t chunks = (n_rows + kPatChunk - 1) / kPatChunk;
    const dim3 grid((unsigned)std::min(chunks, kPatMaxGroups)), block(kPatThreads);
    const uint8_t* m = gk_ptr<const uint8_t>(d_miss8);
#define GK_PAT_LAUNCH(KT) \
  GK_PROF(ctx, "calldosage_patterns", GK_KERNEL(calldosage_patterns<KT>, grid, block, 0, st, m, ldm, n_rows, pc, (int)n_cols, hash_mask, g))
    GK_CALLED_LAUNCH(n_cols, GK_PAT_LAUNCH)
#undef GK_PAT_LAUNCH
  }
  GK_TRY("call patterns", hipGetLastError());
  keys.resize(n_key_tables * n);      // sized while the kernel runs
  counts.resize(n + 2);
  GK_TRY("call patterns", call.fetch(keys.data(), d_keys, key_bytes));
  GK_TRY("call patterns", call.fetch(counts.data(), d_counts, count_bytes));
  GK_TRY("call patterns", call.wait());
  int64_t found = 0;
  for (size_t s = 0; s < n; ++s) {
    if (keys[s] == kPatEmpty || counts[s] == 0) continue;
    unsigned long long lo = keys[s], hi = 0;
    if (wide) {
      const uint32_t a = (uint32_t)(keys[s] >> 32), b = (uint32_t)keys[s];
      lo = a == (uint32_t)kAllFF ? kPatEmpty : keys[n + (a & (n - 1))];
      hi = b == (uint32_t)kAllFF ? kPatEmpty : keys[2 * n + (b & (n - 1))];
    }
    uint8_t* const p = patterns_out + 16 * found;
    for (int i = 0; i < 8; ++i) {
      p[i] = (uint8_t)(lo >> (8 * i));
      p[8 + i] = (uint8_t)(hi >> (8 * i));
    }
    counts_out[found++] = counts[s];
  }
  *n_out = found;
  unplaced_out[0] = counts[n];
  out_of_range_out[0] = counts[n + 1];
  return GK_OK;
}

}  // extern "C"
