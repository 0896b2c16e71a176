// Post-typing novel-variant discovery: the device side of graphkir/novel_discover.py.
//
//   gk_novel_assign     groupReadByAllele        novel_discover.py:48-70
//   gk_novel_confusion  variantConfusionInRead /  novel_discover.py:73-144
//                       statNovelConfusion /
//                       extractNovelVariant
//
// The products of the called alleles come from gk_compat with a mask restricted to the gene's distinct called alleles
// (one bit per column): a product depends on its own allele's bits only, so these K columns are bit-identical to the
// same columns of the full table (typing_mulit_allele.py:340-381), which is never built.
//
// Assignment: per row the maximum of the K products and the set of columns equal to it (np.equal, exact).  The group
// code of a row is the bitmask over CALLED-LIST ENTRIES (a homozygous call sets both of its entries), the histogram and
// the first row of every group are kept per distinct-column set: a per-block histogram in LDS, then one atomic per bin and
// block (cdna_hip_programming.md, Guideline 12).
//
// Confusion: rows whose code names one entry only (the singleton groups, novel_discover.py:311) walk their four lists
// with the sample's error-correction drop flags (errorCorrection mutates the reads in place, typing_mulit_allele.py:
// 333-337: the counts see the corrected lists).  An id is novel when its ordinal lies outside the gene's index span,
// otherwise tp / fp (positive lists) or fn / tn (negative lists) by the allele's bit.  Totals per entry: LDS, then one
// atomic per block.  novel / fp / fn also count per (entry, ordinal), with the first-seen key
// (row << 20 | offset of the id in the row's lists): the lists are stored lpv, rpv, lnv, rnv back to back, so the offset
// orders the ids of one row as every stat's concatenation does, and the smallest key is the Counter's insertion order
// (novel_discover.py:139-143).  All counts are integers: the result does not depend on the order of arrival.
#include <climits>

#include "gk_calls.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxEntries = 16;      // called-list entries of one gene (codes are uint16)
constexpr int kLdsCols = 10;         // up to 2^10 distinct-column sets are binned in LDS
constexpr int kStats = 5;            // novel, tp, tn, fp, fn
constexpr uint32_t kOffBits = 20;

inline unsigned nblk(int64_t n, int cap = 1024) {
  const int64_t b = (n + kThreads - 1) / kThreads;
  return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

template <bool kLds>
__global__ __launch_bounds__(kThreads) void novel_assign(const double* __restrict__ probs, int64_t n_rows, int n_cols,
                                                         const uint32_t* __restrict__ col_entries,
                                                         uint16_t* __restrict__ code_out, uint32_t* count,
                                                         int32_t* first) {
  extern __shared__ uint32_t lds[];     // [bins] counts, [bins] first rows
  const int bins = 1 << n_cols;
  uint32_t* l_count = lds;
  int32_t* l_first = (int32_t*)(lds + (kLds ? bins : 0));
  if (kLds) {
    for (int i = threadIdx.x; i < bins; i += kThreads) { l_count[i] = 0u; l_first[i] = INT_MAX; }
    __syncthreads();
  }
  for (int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x; r < n_rows; r += (int64_t)gridDim.x * kThreads) {
    double m = probs[r];
    for (int k = 1; k < n_cols; ++k) {
      const double v = probs[(int64_t)k * n_rows + r];
      m = v > m ? v : m;
    }
    uint32_t dc = 0u, ec = 0u;
    for (int k = 0; k < n_cols; ++k)
      if (probs[(int64_t)k * n_rows + r] == m) { dc |= 1u << k; ec |= col_entries[k]; }
    code_out[r] = (uint16_t)ec;
    if (kLds) {
      atomicAdd(&l_count[dc], 1u);
      atomicMin(&l_first[dc], (int32_t)r);
    } else {
      atomicAdd(&count[dc], 1u);
      atomicMin(&first[dc], (int32_t)r);
    }
  }
  if (kLds) {
    __syncthreads();
    for (int i = threadIdx.x; i < bins; i += kThreads) {
      const uint32_t c = l_count[i];
      if (c) { atomicAdd(&count[i], c); atomicMin(&first[i], l_first[i]); }
    }
  }
}

__global__ __launch_bounds__(kThreads) void novel_confusion(const int32_t* __restrict__ rows, int64_t n_rows,
                                                            const uint16_t* __restrict__ code,
                                                            const uint32_t* __restrict__ off,
                                                            const uint32_t* __restrict__ ids,
                                                            const uint8_t* __restrict__ vflag, int vbeg, int n_span,
                                                            const uint32_t* __restrict__ carry, const int32_t* entry_col,
                                                            const int32_t* entry_slot, int n_slots, int64_t n_var_total,
                                                            unsigned long long* totals, uint32_t* cnt,
                                                            unsigned long long* key) {
  __shared__ uint32_t l_tot[kMaxEntries * kStats];
  __shared__ int32_t s_col[kMaxEntries], s_slot[kMaxEntries];
  for (int i = threadIdx.x; i < kMaxEntries * kStats; i += kThreads) l_tot[i] = 0u;
  if (threadIdx.x < kMaxEntries) { s_col[threadIdx.x] = entry_col[threadIdx.x]; s_slot[threadIdx.x] = entry_slot[threadIdx.x]; }
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n_rows; i += (int64_t)gridDim.x * kThreads) {
    const uint32_t c = code[i];
    if (__builtin_popcount(c) != 1) continue;        // not a singleton group (novel_discover.py:311)
    const int e = __builtin_ctz(c);
    const int slot = s_slot[e];
    if (slot < 0) continue;
    const uint32_t bit = 1u << s_col[e];
    const int64_t row = rows[i];
    const uint32_t b = off[4 * row], mid = off[4 * row + 2], end = off[4 * row + 4];
    uint32_t t_novel = 0, t_tp = 0, t_tn = 0, t_fp = 0, t_fn = 0;
    for (uint32_t k = b; k < end; ++k) {         // every load guarded by k < end (no sentinel word is read)
      const uint32_t v = ids[k];
      if ((int64_t)v >= n_var_total) continue;         // not an ordinal of this tabulation (never for a sound one)
      const bool positive = k < mid;
      if (vflag[v] & (positive ? 1 : 2)) continue;       // dropped by the error correction
      const uint32_t local = v - (uint32_t)vbeg;
      bool counted;
      if (local >= (uint32_t)n_span) {
        ++t_novel;
        counted = true;
      } else {
        const bool has = (carry[local] & bit) != 0u;
        if (positive) { if (has) ++t_tp; else ++t_fp; }
        else { if (has) ++t_fn; else ++t_tn; }
        counted = positive != has;                      // fp or fn
      }
      if (counted) {
        const int64_t at = (int64_t)slot * n_var_total + v;
        const uint32_t rel = k - b < (1u << kOffBits) ? k - b : (1u << kOffBits) - 1u;
        atomicAdd(&cnt[at], 1u);
        atomicMin(&key[at], ((unsigned long long)i << kOffBits) | rel);
      }
    }
    uint32_t* t = &l_tot[slot * kStats];
    if (t_novel) atomicAdd(&t[0], t_novel);
    if (t_tp) atomicAdd(&t[1], t_tp);
    if (t_tn) atomicAdd(&t[2], t_tn);
    if (t_fp) atomicAdd(&t[3], t_fp);
    if (t_fn) atomicAdd(&t[4], t_fn);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < n_slots * kStats; j += kThreads)
    if (l_tot[j]) atomicAdd(&totals[j], (unsigned long long)l_tot[j]);
}

// (slot, ordinal, count, key) of every counted pair, in no particular order (the host orders them by key)
__global__ __launch_bounds__(kThreads) void novel_compact(const uint32_t* __restrict__ cnt,
                                                          const unsigned long long* __restrict__ key, int64_t n,
                                                          int64_t n_var_total, int64_t cap, uint32_t* n_out,
                                                          int32_t* slot_out, int32_t* ord_out, uint32_t* count_out,
                                                          unsigned long long* key_out) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const uint32_t c = cnt[i];
    if (!c) continue;
    const uint32_t at = atomicAdd(n_out, 1u);
    if ((int64_t)at >= cap) continue;
    slot_out[at] = (int32_t)(i / n_var_total);
    ord_out[at] = (int32_t)(i % n_var_total);
    count_out[at] = c;
    key_out[at] = key[i];
  }
}

}  // namespace

extern "C" {

int gk_novel_assign(gk_ctx* ctx, gk_dptr d_probs, int64_t n_rows, int32_t n_cols, const uint32_t* col_entries,
                    int32_t n_entries, gk_dptr d_code, uint16_t* code_out, uint32_t* count_out, int32_t* first_out) {
  gk_bind(ctx);
  GK_REQUIRE(ctx && col_entries && count_out && first_out, "null pointer");
  GK_REQUIRE(n_entries >= 1 && n_entries <= kMaxEntries,
             "novel discovery supports 1 to 16 called-list entries per gene (codes are 16-bit)");
  GK_REQUIRE(n_cols >= 1 && n_cols <= n_entries, "bad distinct-column count");
  GK_REQUIRE(n_rows >= 0 && n_rows < (int64_t)INT_MAX, "too many rows for 32-bit row numbers");
  for (int k = 0; k < n_cols; ++k)
    GK_REQUIRE(col_entries[k] && col_entries[k] < (1u << n_entries), "column without a called-list entry");
  const int bins = 1 << n_cols;
  if (n_rows == 0) {
    memset(count_out, 0, sizeof(uint32_t) * bins);
    for (int i = 0; i < bins; ++i) first_out[i] = INT_MAX;
    return GK_OK;
  }
  GK_REQUIRE(d_probs && d_code, "null device pointer");
  GkCall call(ctx);
  uint32_t *d_count = nullptr, *d_cols = nullptr;
  GK_HIP(call.take(&d_count, sizeof(uint32_t) * 2 * bins));
  int32_t* d_first = (int32_t*)(d_count + bins);
  if (call.take(&d_cols, sizeof(uint32_t) * kMaxEntries) != hipSuccess) {
    gk_set_error("device allocation failed");
    return GK_ERR_HIP;
  }
  GK_TRY("novel_assign: set-up failed", hipMemsetAsync(d_count, 0, sizeof(uint32_t) * bins, ctx->stream));
  GK_TRY("novel_assign: set-up failed", hipMemsetAsync(d_first, 0x7F, sizeof(int32_t) * bins, ctx->stream));
  GK_TRY("novel_assign: set-up failed", call.send(d_cols, col_entries, sizeof(uint32_t) * n_cols));      // at most 16 words
  const bool lds = n_cols <= kLdsCols;
  GK_PROF(ctx, "novel_assign", {
    if (lds)
      GK_KERNEL(novel_assign<true>, dim3(nblk(n_rows)), dim3(kThreads), sizeof(uint32_t) * 2 * bins, ctx->stream,
                gk_ptr<double>(d_probs), n_rows, (int)n_cols, d_cols, gk_ptr<uint16_t>(d_code), d_count, d_first);
    else
      GK_KERNEL(novel_assign<false>, dim3(nblk(n_rows)), dim3(kThreads), 0, ctx->stream, gk_ptr<double>(d_probs), n_rows,
                (int)n_cols, d_cols, gk_ptr<uint16_t>(d_code), d_count, d_first);
  });
  GK_TRY("novel_assign: launch failed", hipGetLastError());
  GK_TRY("novel_assign: fetch failed", call.fetch(count_out, d_count, sizeof(uint32_t) * bins));
  GK_TRY("novel_assign: fetch failed", call.fetch(first_out, d_first, sizeof(int32_t) * bins));
  if (code_out) GK_TRY("novel_assign: fetch failed", call.fetch(code_out, gk_ptr<void>(d_code), sizeof(uint16_t) * n_rows));
  GK_TRY("novel_assign: fetch failed", call.wait());
  return GK_OK;
}

int gk_novel_confusion(gk_ctx* ctx, gk_tab* tab, gk_dptr d_rows, int64_t n_rows, gk_dptr d_code, gk_dptr d_vflag,
                       int32_t vbeg, int32_t vend, gk_dptr d_carry, const int32_t* entry_col, const int32_t* entry_slot,
                       int32_t n_entries, int32_t n_slots, uint64_t* totals_out, int64_t max_out, int32_t* slot_out,
                       int32_t* ord_out, uint32_t* count_out, uint64_t* key_out, int64_t* n_out) {
  gk_bind(ctx);
  GK_REQUIRE(ctx && tab && entry_col && entry_slot && totals_out && n_out, "null pointer");
  GK_REQUIRE(n_entries >= 1 && n_entries <= kMaxEntries,
             "novel discovery supports 1 to 16 called-list entries per gene (codes are 16-bit)");
  GK_REQUIRE(n_slots >= 0 && n_slots <= n_entries && vend >= vbeg && max_out >= 0, "bad confusion arguments");
  GK_REQUIRE(n_rows >= 0 && n_rows < (1ll << 43), "too many rows for the first-seen key");
  GK_REQUIRE(max_out == 0 || (slot_out && ord_out && count_out && key_out), "null output array");
  for (int e = 0; e < n_entries; ++e) {
    GK_REQUIRE(entry_col[e] >= 0 && entry_col[e] < 32, "entry column out of range");
    GK_REQUIRE(entry_slot[e] >= -1 && entry_slot[e] < n_slots, "entry slot out of range");
  }
  const int64_t nvt = (int64_t)tab->n_var + tab->n_novel;
  memset(totals_out, 0, sizeof(uint64_t) * kStats * n_slots);
  *n_out = 0;
  if (n_rows == 0 || n_slots == 0 || nvt == 0) return GK_OK;
  GK_REQUIRE(d_rows && d_code && d_vflag && (d_carry || vend == vbeg), "null device pointer");
  const int64_t n_cells = nvt * n_slots;
  uint32_t found = 0;              // before the record that delivers into it (GkCall::fetch)
  GkCall call(ctx);
  const char* const no_memory = "novel_confusion: device allocation failed";
  uint32_t* d_cnt = nullptr;
  unsigned long long *d_key = nullptr, *d_tot = nullptr;
  int32_t* d_meta = nullptr;       // entry_col[16], entry_slot[16]
  uint32_t* d_n = nullptr;
  GK_TRY(no_memory, call.take(&d_cnt, sizeof(uint32_t) * n_cells));
  GK_TRY(no_memory, call.take(&d_key, sizeof(uint64_t) * n_cells));
  GK_TRY(no_memory, call.take(&d_tot, sizeof(uint64_t) * kStats * n_slots));
  GK_TRY(no_memory, call.take(&d_meta, sizeof(int32_t) * 2 * kMaxEntries));
  GK_TRY(no_memory, call.take(&d_n, sizeof(uint32_t)));
  int32_t meta[2 * kMaxEntries];
  for (int e = 0; e < kMaxEntries; ++e) {
    meta[e] = e < n_entries ? entry_col[e] : 0;
    meta[kMaxEntries + e] = e < n_entries ? entry_slot[e] : -1;
  }
  GK_TRY("novel_confusion: set-up failed", hipMemsetAsync(d_cnt, 0, sizeof(uint32_t) * n_cells, ctx->stream));
  GK_TRY("novel_confusion: set-up failed", hipMemsetAsync(d_key, 0xFF, sizeof(uint64_t) * n_cells, ctx->stream));
  GK_TRY("novel_confusion: set-up failed", hipMemsetAsync(d_tot, 0, sizeof(uint64_t) * kStats * n_slots, ctx->stream));
  GK_TRY("novel_confusion: set-up failed", hipMemsetAsync(d_n, 0, sizeof(uint32_t), ctx->stream));
  GK_TRY("novel_confusion: set-up failed", call.send(d_meta, meta, sizeof(meta)));      // 128 bytes
  GK_PROF(ctx, "novel_confusion",
          GK_KERNEL(novel_confusion, dim3(nblk(n_rows)), dim3(kThreads), 0, ctx->stream, gk_ptr<int32_t>(d_rows), n_rows,
                    gk_ptr<uint16_t>(d_code), tab->d_off, tab->d_ids, gk_ptr<uint8_t>(d_vflag), vbeg, vend - vbeg,
                    gk_ptr<uint32_t>(d_carry), d_meta, d_meta + kMaxEntries, n_slots, nvt, d_tot, d_cnt, d_key));
  GK_TRY("novel_confusion: launch failed", hipGetLastError());
  // first wait: the totals and the number of counted pairs
  int32_t* d_slot = nullptr;
  int32_t* d_ord = nullptr;
  uint32_t* d_count = nullptr;
  unsigned long long* d_okey = nullptr;
  const int64_t cap = std::min<int64_t>(n_cells, std::max<int64_t>(max_out, 1));
  GK_TRY(no_memory, call.take(&d_slot, sizeof(int32_t) * cap));
  GK_TRY(no_memory, call.take(&d_ord, sizeof(int32_t) * cap));
  GK_TRY(no_memory, call.take(&d_count, sizeof(uint32_t) * cap));
  GK_TRY(no_memory, call.take(&d_okey, sizeof(uint64_t) * cap));
  GK_PROF(ctx, "novel_compact",
          GK_KERNEL(novel_compact, dim3(nblk(n_cells)), dim3(kThreads), 0, ctx->stream, d_cnt, d_key, n_cells, nvt, cap,
                    d_n, d_slot, d_ord, d_count, d_okey));
  GK_TRY("novel_confusion: launch failed", hipGetLastError());
  GK_TRY("novel_confusion: fetch failed", call.fetch(totals_out, d_tot, sizeof(uint64_t) * kStats * n_slots));
  GK_TRY("novel_confusion: fetch failed", call.fetch(&found, d_n, sizeof(uint32_t)));
  GK_TRY("novel_confusion: fetch failed", call.wait());
  *n_out = found;
  if ((int64_t)found > max_out) {
    gk_set_error("novel_confusion: %u counted variants, room for %lld", found, (long long)max_out);
    return GK_ERR_CAPACITY;
  }
  if (!found) return GK_OK;
  GK_TRY("novel_confusion: fetch failed", call.fetch(slot_out, d_slot, sizeof(int32_t) * found));
  GK_TRY("novel_confusion: fetch failed", call.fetch(ord_out, d_ord, sizeof(int32_t) * found));
  GK_TRY("novel_confusion: fetch failed", call.fetch(count_out, d_count, sizeof(uint32_t) * found));
  GK_TRY("novel_confusion: fetch failed", call.fetch(key_out, d_okey, sizeof(uint64_t) * found));
  GK_TRY("novel_confusion: fetch failed", call.wait());
  return GK_OK;
}

}  // extern "C"
