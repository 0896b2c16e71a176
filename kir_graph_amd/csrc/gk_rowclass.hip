// Row classes of one gene: rows of the compatibility table whose KEPT (id, sign) sequences are equal hold equal entries
// in every column (an entry is the ordered product over that sequence and depends on nothing else of the row), so the
// product chains run once per class (compat_kernel on the representatives, gk_typing.hip) and the results are copied
// into place (rowclass_expand).
//
//   rowclass_keys     16 lanes per row walk its lists the way count_ids_genes does (unconditional loads, clamped indices)
//                     and form a 64-bit hash of the kept sequence -- "kept" is compat_kernel's test,
//                     !(vflag[v] & (k < mid ? 1 : 2)); the sign of an entry is k >= mid; ids outside the gene's span are
//                     factors and therefore part of the sequence.  The group's first lane claims a slot of an
//                     open-addressing table by CAS on the hash; the slot's representative is its LOWEST row (atomicMin):
//                     the classes do not depend on which row came first.
//   rowclass_verify   every row's kept sequence against its representative's, element by element in list order (the
//                     row's kept tokens laid down in LDS by their kept rank, the representative's compared at the same
//                     rank).  A row that differs -- or keeps more than kCap ids -- is a class of its own: no hash decides
//                     equality.
//   (gk_compact_enqueue: the representatives in row order, their number left on the device)
//   rowclass_rank     rank_of[representative] = its place in that order; rep_rows[c] = rows[representative]
//   rowclass_classof  class_of[r] = rank_of[representative of r]
//   rowclass_expand   L[a][r] = Lc[class_of[r]][a], eight columns (gridDim.y) of four rows per thread: the compact table
//                     is held row by row, so a row's entries of the eight columns are 64 consecutive bytes (gathered
//                     column by column from [column][class], every 8-byte entry fetched a line of its own from the L2:
//                     profiles/r20_row_classes.txt); out go 32 bytes of float64 and one word of mismatch counts per
//                     store, as pass 2 of compat_kernel -- and as there the count is read back from the log-likelihood
//                     (the same arithmetic on the same double gives the same byte), so one gather serves both tables; the
//                     rows of miss8 from n_rows up to its stride are zeroed.
#include "gk_rowclass.h"

namespace {

constexpr int kThreads = 256;
constexpr int kGroup = 16, kDeep = 4;            // lanes per row; ids per lane and round: 64 list entries per round
constexpr int kRound = kGroup * kDeep;
constexpr int kCap = 256;                        // kept ids of a row that the comparison holds in LDS
constexpr uint64_t kEmptyKey = ~0ull;            // no hash has bit 63
constexpr int kExpandCols = 8;                   // columns per thread of the expansion: 64 bytes of a class's row

__device__ inline uint64_t mix64(uint64_t x) {
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// One round of a row's walk: the 64 list entries from k0 (this lane's are k0 + lane + 16 j).  f(token, rank) is called
// for every KEPT entry: token = id << 1 | sign, rank = kept entries of the row before it (kept_before counts those of
// the earlier rounds).  Returns the kept entries up to the end of the round.  e > k0.
template <class F>
__device__ inline uint32_t walk_round(const uint32_t* __restrict__ ids, const uint8_t* __restrict__ vflag, uint32_t k0,
                                      uint32_t mid, uint32_t e, int lane, int shift, uint32_t kept_before, F&& f) {
  uint32_t v[kDeep];
  uint8_t fl[kDeep];
  const uint32_t last = e - 1u;
#pragma unroll
  for (int j = 0; j < kDeep; ++j) {
    const uint32_t k = k0 + (uint32_t)lane + kGroup * j;
    v[j] = ids[k < e ? k : last];
  }
#pragma unroll
  for (int j = 0; j < kDeep; ++j) fl[j] = vflag[v[j]];
  uint32_t run = kept_before;
#pragma unroll
  for (int j = 0; j < kDeep; ++j) {
    const uint32_t k = k0 + (uint32_t)lane + kGroup * j;
    const bool positive = k < mid;
    const bool keep = k < e && !(fl[j] & (positive ? 1 : 2));
    const uint32_t mine = (uint32_t)(__ballot(keep) >> shift) & 0xFFFFu;      // the group's 16 lanes
    if (keep) f((v[j] << 1) | (positive ? 0u : 1u), run + (uint32_t)__builtin_popcount(mine & ((1u << lane) - 1u)));
    run += (uint32_t)__builtin_popcount(mine);
  }
  return run;
}

__global__ __launch_bounds__(kThreads) void rowclass_keys(const int32_t* __restrict__ rows, int64_t n_rows,
                                                          const uint32_t* __restrict__ off,
                                                          const uint32_t* __restrict__ ids,
                                                          const uint8_t* __restrict__ vflag, uint64_t hash_mask,
                                                          unsigned long long* slot_key, uint32_t* slot_rep,
                                                          uint32_t slot_mask, uint32_t* __restrict__ slot_of) {
  const int lane = threadIdx.x & (kGroup - 1);
  const int shift = (threadIdx.x & 63) & ~(kGroup - 1);
  const int64_t i = ((int64_t)blockIdx.x * kThreads + threadIdx.x) / kGroup;
  const bool active = i < n_rows;
  uint32_t b = 0, mid = 0, e = 0;
  if (active) {
    const int64_t row = rows[i];
    b = off[4 * row]; mid = off[4 * row + 2]; e = off[4 * row + 4];
  }
  uint64_t h = 0;
  uint32_t n = 0;
  for (uint32_t k0 = b; k0 < e; k0 += kRound)
    n = walk_round(ids, vflag, k0, mid, e, lane, shift, n,
                   [&](uint32_t token, uint32_t rank) { h += mix64(((uint64_t)rank << 32) | token); });
  // the sum over the group's lanes (every term is bound to its rank, so the sum depends on the order of the sequence)
  uint32_t lo = (uint32_t)h, hi = (uint32_t)(h >> 32);
#pragma unroll
  for (int d = kGroup / 2; d > 0; d >>= 1) {
    const uint64_t o = ((uint64_t)(uint32_t)__shfl_xor((int)hi, d, 64) << 32) | (uint32_t)__shfl_xor((int)lo, d, 64);
    h += o;
    lo = (uint32_t)h; hi = (uint32_t)(h >> 32);
  }
  if (!active || lane != 0) return;
  const unsigned long long key = mix64(h ^ n) & hash_mask & ~(1ull << 63);
  uint32_t s = (uint32_t)(key ^ (key >> 32)) & slot_mask;
  // A class of a deep sample has a hundred rows and more, which all meet in one slot: the slot is READ first, and the
  // atomics are left to the rows that change it (a key is written once, a representative only falls: a stale read costs
  // an atomic, never the result).  At least half of the slots are empty: the probe ends.
  for (;;) {
    unsigned long long prev = __hip_atomic_load(&slot_key[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (prev == kEmptyKey) prev = atomicCAS(&slot_key[s], (unsigned long long)kEmptyKey, key);
    if (prev == kEmptyKey || prev == key) break;
    s = (s + 1u) & slot_mask;
  }
  if (__hip_atomic_load(&slot_rep[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > (uint32_t)i)
    atomicMin(&slot_rep[s], (uint32_t)i);
  slot_of[i] = s;
}

__global__ __launch_bounds__(kThreads) void rowclass_verify(const int32_t* __restrict__ rows, int64_t n_rows,
                                                            const uint32_t* __restrict__ off,
                                                            const uint32_t* __restrict__ ids,
                                                            const uint8_t* __restrict__ vflag,
                                                            const uint32_t* __restrict__ slot_rep,
                                                            const uint32_t* __restrict__ slot_of,
                                                            uint32_t* __restrict__ is_rep, uint32_t* __restrict__ rep_of) {
  __shared__ uint32_t kept[kThreads / kGroup][kCap];
  const int lane = threadIdx.x & (kGroup - 1);
  const int shift = (threadIdx.x & 63) & ~(kGroup - 1);
  const int g = threadIdx.x / kGroup;
  const int64_t i = ((int64_t)blockIdx.x * kThreads + threadIdx.x) / kGroup;
  const bool active = i < n_rows;
  const uint32_t rep = active ? slot_rep[slot_of[i]] : 0u;      // <= i: row i is of that slot
  const bool compare = active && rep < (uint32_t)i;
  uint32_t b = 0, mid = 0, e = 0, rb = 0, rmid = 0, re = 0;
  if (compare) {
    const int64_t row = rows[i], rrow = rows[rep];
    b = off[4 * row]; mid = off[4 * row + 2]; e = off[4 * row + 4];
    rb = off[4 * rrow]; rmid = off[4 * rrow + 2]; re = off[4 * rrow + 4];
  }
  uint32_t* const mine = kept[g];
  uint32_t n = 0, rn = 0;
  for (uint32_t k0 = b; k0 < e; k0 += kRound)
    n = walk_round(ids, vflag, k0, mid, e, lane, shift, n, [&](uint32_t token, uint32_t rank) {
      if (rank < (uint32_t)kCap) mine[rank] = token;
    });
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();      // a group lies in one wave, whose LDS operations are executed in order
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  bool differs = false;
  for (uint32_t k0 = rb; k0 < re; k0 += kRound)
    rn = walk_round(ids, vflag, k0, rmid, re, lane, shift, rn, [&](uint32_t token, uint32_t rank) {
      // a rank beyond the row's own count reads what an earlier row left: the counts differ then, whatever it holds
      if (rank < (uint32_t)kCap && mine[rank] != token) differs = true;
    });
  const bool any = ((__ballot(differs) >> shift) & 0xFFFFull) != 0ull;
  const bool same = compare && n == rn && n <= (uint32_t)kCap && !any;
  if (active && lane == 0) {
    is_rep[i] = same ? 0u : 1u;
    rep_of[i] = same ? rep : (uint32_t)i;
  }
}

__global__ __launch_bounds__(kThreads) void rowclass_rank(const int32_t* __restrict__ rep_idx,
                                                          const uint32_t* __restrict__ n_classes, int64_t n_rows,
                                                          const int32_t* __restrict__ rows, uint32_t* __restrict__ rank_of,
                                                          int32_t* __restrict__ rep_rows) {
  const int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (c >= n_rows || c >= (int64_t)*n_classes) return;
  const int32_t r = rep_idx[c];
  rank_of[r] = (uint32_t)c;
  rep_rows[c] = rows[r];
}

__global__ __launch_bounds__(kThreads) void rowclass_classof(const uint32_t* __restrict__ rep_of,
                                                             const uint32_t* __restrict__ rank_of, int64_t n_rows,
                                                             uint32_t* __restrict__ class_of) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n_rows) class_of[i] = rank_of[rep_of[i]];
}

__global__ __launch_bounds__(kThreads) void rowclass_expand(const double* __restrict__ Lc, int64_t ldc,
                                                            const uint32_t* __restrict__ class_of, int64_t n_rows,
                                                            int n_cols, double* __restrict__ L,
                                                            uint8_t* __restrict__ miss8, int64_t ldm) {
  const int a0 = (int)blockIdx.y * kExpandCols;
  const int n_a = min(kExpandCols, n_cols - a0);
  const int64_t r0 = 4 * ((int64_t)blockIdx.x * kThreads + threadIdx.x);
  if (r0 >= ldm) return;
  if (r0 >= n_rows) {      // ldm is a multiple of 64: whole words
    for (int a = 0; a < n_a; ++a) *reinterpret_cast<uint32_t*>(miss8 + (int64_t)(a0 + a) * ldm + r0) = 0u;
    return;
  }
  const int n_r = (int)(n_rows - r0 < 4 ? n_rows - r0 : 4);
  uint32_t c[4];
  if (n_r == 4) {
    const uint4 q = *reinterpret_cast<const uint4*>(class_of + r0);
    c[0] = q.x; c[1] = q.y; c[2] = q.z; c[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = class_of[j < n_r ? r0 + j : n_rows - 1];
  }
  // a class's entries of these columns are 64 consecutive bytes of its row of the compact table (ldc is a multiple of 8
  // columns; the columns past n_cols of the last group are read and not used)
  double v[4][kExpandCols];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double2* const src = reinterpret_cast<const double2*>(Lc + (int64_t)c[j] * ldc + a0);
#pragma unroll
    for (int q = 0; q < kExpandCols / 2; ++q) {
      const double2 x = src[q];
      v[j][2 * q] = x.x; v[j][2 * q + 1] = x.y;
    }
  }
#pragma unroll
  for (int a = 0; a < kExpandCols; ++a) {
    if (a >= n_a) break;
    uint32_t packed = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {      // pass 2 of compat_kernel, to the letter: NaN and counts from 100 on are 255
      const double t = __builtin_fma(v[j][a], -1.0 / 3.0, 0.25);
      const uint32_t m = t < 100.0 ? (uint32_t)(int)t : 255u;
      if (j < n_r) packed |= m << (8 * j);
    }
    double* const dst = L + (int64_t)(a0 + a) * n_rows + r0;
    if (n_r == 4) {
#pragma unroll
      for (int j = 0; j < 4; ++j) dst[j] = v[j][a];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < n_r) dst[j] = v[j][a];
    }
    *reinterpret_cast<uint32_t*>(miss8 + (int64_t)(a0 + a) * ldm + r0) = packed;
  }
}

inline unsigned nblk(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

}  // namespace

int64_t gk_rowclass_ld(int n_cols) { return ((int64_t)n_cols + kExpandCols - 1) / kExpandCols * kExpandCols; }

int gk_rowclass_enqueue(gk_ctx* ctx, gk_tab* tab, const int32_t* d_rows, int64_t n_rows, const uint8_t* d_vflag,
                        gk_rowclass* rc) {
  GK_REQUIRE(ctx && tab && rc && d_rows && d_vflag && n_rows > 0 && n_rows <= 0x7FFFFFFFll, "bad row-class arguments");      // row numbers are int32
  hipStream_t st = ctx->stream;
  // GK_TEST_HOOKS=rowclass_hashbits=N: the hash cut to N bits, so that rows of different sequences meet in one slot
  const long bits = gk_test_hook_value("rowclass_hashbits", 63);
  const uint64_t hash_mask = bits >= 63 ? ~0ull : bits <= 0 ? 0ull : (1ull << bits) - 1ull;
  uint64_t n_slots = 64;
  while (n_slots < 2 * (uint64_t)n_rows) n_slots <<= 1;
  GkBlocks temps(ctx);
  char* slots = nullptr;      // [n_slots] keys, then [n_slots] representatives: all bits set = empty / no row yet
  uint32_t *slot_of = nullptr, *is_rep = nullptr, *rep_of = nullptr, *rank_of = nullptr, *class_of = nullptr, *n_classes = nullptr;
  int32_t *rep_idx = nullptr, *rep_rows = nullptr;
  const size_t per_row = (size_t)n_rows * sizeof(uint32_t);
  if (temps.take(&slots, (size_t)n_slots * 12) != hipSuccess || temps.take(&slot_of, per_row) != hipSuccess ||
      temps.take(&is_rep, per_row) != hipSuccess || temps.take(&rep_of, per_row) != hipSuccess ||
      temps.take(&rank_of, per_row) != hipSuccess || temps.take(&rep_idx, per_row) != hipSuccess ||
      temps.take(&rep_rows, per_row) != hipSuccess || temps.take(&class_of, per_row) != hipSuccess) {
    gk_set_error("out of device memory for the row classes");
    return GK_ERR_HIP;
  }
  unsigned long long* const slot_key = reinterpret_cast<unsigned long long*>(slots);
  uint32_t* const slot_rep = reinterpret_cast<uint32_t*>(slots + (size_t)n_slots * 8);
  if (hipMemsetAsync(slots, 0xFF, (size_t)n_slots * 12, st) != hipSuccess) {
    gk_set_error("row classes: clearing the slots failed");
    return GK_ERR_HIP;
  }
  const unsigned groups = nblk(n_rows * kGroup);
  GK_PROF(ctx, "rowclass_keys", GK_KERNEL(rowclass_keys, dim3(groups), dim3(kThreads), 0, st, d_rows, n_rows, tab->d_off,
                                          tab->d_ids, d_vflag, hash_mask, slot_key, slot_rep, (uint32_t)(n_slots - 1),
                                          slot_of));
  GK_PROF(ctx, "rowclass_verify", GK_KERNEL(rowclass_verify, dim3(groups), dim3(kThreads), 0, st, d_rows, n_rows,
                                            tab->d_off, tab->d_ids, d_vflag, slot_rep, slot_of, is_rep, rep_of));
  const int code = gk_compact_enqueue(ctx, is_rep, nullptr, n_rows, rep_idx, &n_classes, temps);
  if (code) return code;
  GK_PROF(ctx, "rowclass_rank", {
    GK_KERNEL(rowclass_rank, dim3(nblk(n_rows)), dim3(kThreads), 0, st, rep_idx, n_classes, n_rows, d_rows, rank_of,
              rep_rows);
    GK_KERNEL(rowclass_classof, dim3(nblk(n_rows)), dim3(kThreads), 0, st, rep_of, rank_of, n_rows, class_of);
  });
  if (hipGetLastError() != hipSuccess) {
    gk_set_error("row classes: a launch failed");
    return GK_ERR_HIP;
  }
  rc->rep_rows = rep_rows; rc->class_of = class_of; rc->n_classes = n_classes;
  rc->blocks = std::move(temps);
  return GK_OK;
}

int gk_rowclass_expand(gk_ctx* ctx, const gk_rowclass* rc, const double* Lc, int64_t ldc, int n_cols, int64_t n_rows,
                       double* L, uint8_t* miss8, int64_t ldm) {
  GK_REQUIRE(ctx && rc && rc->class_of && Lc && L && miss8 && n_cols > 0 && n_cols <= 65535 && n_rows > 0 &&
                 ldm >= n_rows && ldm % 64 == 0 && ldc == gk_rowclass_ld(n_cols), "bad expansion arguments");
  GK_PROF(ctx, "rowclass_expand", GK_KERNEL(rowclass_expand, dim3(nblk(ldm / 4), (unsigned)((n_cols + kExpandCols - 1) / kExpandCols)), dim3(kThreads), 0,
                                            ctx->stream, Lc, ldc, rc->class_of, n_rows, n_cols, L, miss8, ldm));
  GK_HIP(hipGetLastError());
  return GK_OK;
}

extern "C" int gk_row_classes(gk_ctx* ctx, gk_tab* tab, gk_dptr d_rows, int64_t n_rows, gk_dptr d_vflag, gk_dptr d_class_of,
                              int64_t* n_classes) {
  gk_bind(ctx);
  GK_REQUIRE(ctx && tab && n_classes && n_rows >= 0, "bad arguments");
  *n_classes = 0;
  if (n_rows == 0) return GK_OK;
  gk_rowclass rc;
  int code = gk_rowclass_enqueue(ctx, tab, gk_ptr<int32_t>(d_rows), n_rows, gk_ptr<uint8_t>(d_vflag), &rc);
  if (code) return code;
  if (d_class_of)
    (void)hipMemcpyAsync(gk_ptr<void>(d_class_of), rc.class_of, (size_t)n_rows * sizeof(uint32_t), hipMemcpyDeviceToDevice,
                         ctx->stream);
  uint32_t n = 0;
  GK_HIP(gk_fetch(ctx, &n, rc.n_classes, sizeof(uint32_t)));
  *n_classes = n;
  return GK_OK;
}
