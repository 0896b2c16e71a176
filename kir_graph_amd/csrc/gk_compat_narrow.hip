// The compatibility table of AT MOST 8 listed alleles of a gene (exon-first: the candidates' columns of the full model,
// typing_mulit_allele.py:506-520, 740-746) -- what gk_compat_log_miss_cols followed by gk_miss_colsum writes, bit for
// bit, by kernels of their own:
//   cols_bytes     colbits[v] = bit c <- bit table_cols[c] of variant v's bit row: ONE byte per variant of the gene's span
//   compat_rows8   a wavefront owns 8 rows at a time, lane = (row g = lane >> 3, column c = lane & 7) -- 16 rows of 4
//                  lanes each for a list of at most 4 columns
// (the factor phase of the 4-lane form issues half the instructions per row: 148 against 176 us per table of ~750 k rows
// and <= 4 columns, profiles/r11_compat_narrow.txt).
// compat_kernel (gk_typing.hip) gives a wavefront to ONE row with lanes = alleles: on a table of <= 4 columns 60 of its
// 64 lanes multiply factors nobody stores, and its time is the issue of those instructions whatever the column count.
#include <algorithm>

#include "gk_blocks.h"
#include "gk_lut.h"

namespace {

constexpr int kNarrowCols = 8;                         // columns a lane group carries
constexpr int kNarrowWaves = 8;
constexpr int kNarrowThreads = 64 * kNarrowWaves;
constexpr int kHalfRows = 8;                           // rows whose chunks are loaded and compacted together
constexpr int kWaveRows = 16;                          // rows of a wave per tile: two groups of 8 or one of 16
constexpr int kNarrowTile = kNarrowWaves * kWaveRows;  // 128 rows: whole 128-byte lines of the mismatch table
constexpr int kStripBytes = 68;     // a row's 64 kept bytes + 4: the strips of rows g and g + 2 start in different banks
constexpr int kTileStride = kNarrowTile + 8;           // doubles: column c starts 16 banks after column c - 1
constexpr int kColThreads = 256;

struct NarrowCols { int32_t c[kNarrowCols]; };

// One thread per variant of the gene's span.  Thread 0 also clears the flag word and the column sums of the launch
// that follows (at least one workgroup runs, whatever the span).
__global__ __launch_bounds__(kColThreads) void cols_bytes(const uint32_t* __restrict__ mask, int n_span, int words,
                                                         NarrowCols cols, int n_cols, uint8_t* __restrict__ colbits,
                                                         uint32_t* __restrict__ flags, uint32_t* __restrict__ msum) {
  const int64_t v = (int64_t)blockIdx.x * kColThreads + threadIdx.x;
  if (v == 0) {
    *flags = 0;
    for (int c = 0; c < n_cols; ++c) msum[c] = 0;
  }
  if (v >= n_span) return;
  const uint32_t* const row = mask + v * words;
  uint32_t x = 0;
#pragma unroll
  for (int c = 0; c < kNarrowCols; ++c) {
    if (c < n_cols) {
      const int a = cols.c[c];
      x |= ((row[a >> 5] >> (a & 31)) & 1u) << c;
    }
  }
  colbits[v] = (uint8_t)x;
}

// Compaction (per row and chunk of 64 ids, all 64 lanes, as compat_kernel does it): id, drop flag and the variant's
// byte of colbits by straight-line loads with clamped indices; the byte inverted for a negative id -- a set bit then
// means "allele and read agree" for both signs; the KEPT bytes back to back, in list order, into the row's strip of LDS.
// Factor phase (once for the kRows = 64 / kLanes rows of a group, kLanes = 4 or 8 lanes per row; the compaction takes
// them 8 at a time): for t below the largest kept count, a lane reads byte t of its row's strip, takes bit c and
// multiplies by 0.999 / 0.001 -- by 1.0 past its own row's count, which is exact -- so order and values per entry are
// compat_kernel's.  Rows longer than 64 ids take further rounds of both phases.
// On its way out every lane maps its own product through the log10 value table (one lookup per entry, 64 in flight per
// wave); the tile is transposed through LDS and leaves as 1 KB runs of d_log and whole lines of the mismatch table;
// the column sums of the bytes are added per workgroup.  Flag bits as compat_kernel raises them.
template <int kLanes>
__global__ __launch_bounds__(kNarrowThreads) void compat_rows8(const int32_t* __restrict__ rows, int64_t n_rows,
                                                              const uint32_t* __restrict__ off,
                                                              const uint32_t* __restrict__ ids,
                                                              const uint8_t* __restrict__ vflag, int vbeg, int n_span,
                                                              const uint8_t* __restrict__ colbits, int n_cols, LutView lut,
                                                              double empty_p, double* __restrict__ out_log,
                                                              uint8_t* __restrict__ miss8, int64_t ldm, int64_t n_tiles,
                                                              uint32_t* __restrict__ flags, uint32_t* __restrict__ msum) {
  __shared__ double tile[kNarrowCols * kTileStride];
  constexpr int kRows = 64 / kLanes;                   // rows of a group: one factor phase serves them
  constexpr int kGroups = kWaveRows / kRows, kHalves = kRows / kHalfRows;
  __shared__ __attribute__((aligned(4))) uint8_t strips[kNarrowWaves][kRows * kStripBytes];
  __shared__ uint32_t col_sum[kNarrowCols];
  // 0.999 = 0x3FEFF7CED916872B, 0.001 = 0x3F50624DD2F1A9FC, 1.0 = 0x3FF0000000000000
  constexpr int32_t kHi999 = 0x3FEFF7CE, kLo999 = (int32_t)0xD916872B, kHi001 = 0x3F50624D, kLo001 = (int32_t)0xD2F1A9FC;
  constexpr int32_t kHiOne = 0x3FF00000;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane / kLanes, c = lane % kLanes;
  const int64_t row0 = (int64_t)blockIdx.x * kNarrowTile;
  if (tid < kNarrowCols) col_sum[tid] = 0;

  // the list offsets of the wave's 16 rows, one row per lane: row number -> offsets for all of them at once.  A row past
  // the end of the table has an empty list (and stores nothing below).
  uint32_t lane_b = 0, lane_mid = 0, lane_e = 0;
  {
    const int64_t i = row0 + wid * kWaveRows + (lane & (kWaveRows - 1));
    const bool in = i < n_rows;
    const int64_t row = rows[in ? i : n_rows - 1];
    const uint32_t b = off[4 * row], mid = off[4 * row + 2], e = off[4 * row + 4];
    if (in) { lane_b = b; lane_mid = mid; lane_e = e; }
  }
  uint8_t* const wave_strips = strips[wid];
  const uint32_t* const my_strip = reinterpret_cast<const uint32_t*>(wave_strips + g * kStripBytes);
  int bitpos[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) bitpos[j] = c + 8 * j;
  uint32_t raise = 0;      // flag bits this lane wants raised: one atomic per wave

#pragma unroll 1
  for (int grp = 0; grp < kGroups; ++grp) {
    uint32_t longest = 0;
#pragma unroll
    for (int q = 0; q < kRows; ++q)
      longest = max(longest, (uint32_t)__builtin_amdgcn_readlane((int)(lane_e - lane_b), grp * kRows + q));
    double p = 1.0;
    uint32_t nvar = 0;      // kept ids of this lane's row so far
    for (uint32_t done = 0; done < longest; done += 64) {
      uint32_t my_kept = 0, most = 0, least = 64;
#pragma unroll 1
      for (int half = 0; half < kHalves; ++half) {
        // ---- compaction of this round's chunk of 8 rows.  A row that has no chunk left keeps nothing; its loads read
        // id 0 of the lists (some row of the group has a chunk, so the lists are not empty).
        const int first = grp * kRows + half * kHalfRows;
        uint32_t rb[kHalfRows], rmid[kHalfRows], re[kHalfRows];      // wave-uniform
#pragma unroll
        for (int q = 0; q < kHalfRows; ++q) {
          rb[q] = (uint32_t)__builtin_amdgcn_readlane((int)lane_b, first + q);
          rmid[q] = (uint32_t)__builtin_amdgcn_readlane((int)lane_mid, first + q);
          re[q] = (uint32_t)__builtin_amdgcn_readlane((int)lane_e, first + q);
        }
        uint32_t v[kHalfRows];
#pragma unroll
        for (int q = 0; q < kHalfRows; ++q) {
          const bool has = done < re[q] - rb[q];                       // uniform
          const uint32_t k = rb[q] + done + (uint32_t)lane;
          v[q] = ids[has ? (k < re[q] ? k : re[q] - 1u) : 0u];
        }
        uint8_t dropped[kHalfRows], bits[kHalfRows];
#pragma unroll
        for (int q = 0; q < kHalfRows; ++q) {
          const uint32_t local = v[q] - (uint32_t)vbeg;
          dropped[q] = vflag[v[q]];
          bits[q] = colbits[local < (uint32_t)n_span ? local : 0u];      // a variant outside the span: nobody carries it
        }
#pragma unroll
        for (int q = 0; q < kHalfRows; ++q) {
          const bool has = done < re[q] - rb[q];
          const uint32_t k = rb[q] + done + (uint32_t)lane;
          const bool in = has && k < re[q];
          const bool negative = k >= rmid[q];
          const uint32_t local = v[q] - (uint32_t)vbeg;
          const uint32_t x = (local < (uint32_t)n_span ? (uint32_t)bits[q] : 0u) ^ (negative ? 0xFFu : 0u);
          const bool keep = in && !(dropped[q] & (negative ? 2 : 1));
          const uint64_t kept = __ballot(keep);
          const uint32_t n_kept = (uint32_t)__builtin_popcountll(kept);
          const uint32_t place = __builtin_amdgcn_mbcnt_hi((uint32_t)(kept >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)kept, 0u));
          const int r = half * kHalfRows + q;                              // row inside the group
          if (keep) wave_strips[r * kStripBytes + place] = (uint8_t)x;      // place < 64
          my_kept = g == r ? n_kept : my_kept;
          most = max(most, n_kept);
          least = min(least, n_kept);
        }
      }
      nvar += my_kept;
      __builtin_amdgcn_wave_barrier();   // LDS operations of a wave are executed in order
      // ---- factors: bit -> select mask -> the factor's two halves -> multiply
      uint32_t t = 0;
      for (; t + 4 <= least; t += 4) {      // every row of the group keeps these
        const uint32_t w = my_strip[t >> 2];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int32_t m = __builtin_amdgcn_sbfe((int32_t)w, bitpos[j], 1);   // -1: allele and read agree
          p *= __hiloint2double((m & kHi999) | (~m & kHi001), (m & kLo999) | (~m & kLo001));
        }
      }
      for (; t < most; t += 4) {            // some rows have ended: 1.0 for them
        const uint32_t w = my_strip[t >> 2];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int32_t m = __builtin_amdgcn_sbfe((int32_t)w, bitpos[j], 1);
          const bool mine = t + j < my_kept;
          const int32_t hi = (m & kHi999) | (~m & kHi001), lo = (m & kLo999) | (~m & kLo001);
          p *= __hiloint2double(mine ? hi : kHiOne, mine ? lo : 0);
        }
      }
      __builtin_amdgcn_wave_barrier();   // the next round overwrites the strips
    }
    // ---- this lane's entry on its way out: a read without any kept variant counts 1.0, or 0.999 for every allele when
    // such reads stay in the model; then the log10 of the product from the value table
    const int rt = wid * kWaveRows + grp * kRows + g;      // row inside the tile
    if (c < n_cols && row0 + rt < n_rows) {
      // the mismatch count read back from the log-likelihood is exact only for rows of fewer than ~5000 factors
      if (nvar >= 4096u) raise |= 1u;
      const double prod = nvar ? p : empty_p;
      const uint64_t key = (uint64_t)__double_as_longlong(prod);
      bool found;
      double val = gk_lut_lookup(lut, key, &found);
      if (!found) {
        // no log10 yet: the PRODUCT itself is stored in the entry's place (strictly positive, which no log10 of a
        // probability is) and bit 2 raised; +0.0 cannot mark itself: bit 3, the table is written again
        gk_lut_insert(lut, key);
        const bool marks = (int64_t)key > 0;
        raise |= marks ? 4u : 12u;
        if (marks) val = prod;
      }
      tile[c * kTileStride + rt] = val;
    }
  }
  {
    const uint32_t b0 = __ballot((raise & 1u) != 0) ? 1u : 0u, b2 = __ballot((raise & 4u) != 0) ? 4u : 0u,
                   b3 = __ballot((raise & 8u) != 0) ? 8u : 0u;
    if ((b0 | b2 | b3) && lane == 0) atomicOr(flags, b0 | b2 | b3);
  }
  __syncthreads();
  // ---- the way out: a thread takes FOUR consecutive rows of one column -- 32 bytes of d_log and one word of the
  // mismatch table, the count read back from the log-likelihood as compat_kernel does (m = floor(-L / 3 + 1/4); 255 from
  // 100 on, with bit 0 unless the entry is a NaN).  Rows of the tile past the end of the table hold 0 up to the stride.
  const int n_r = (int)min<int64_t>(kNarrowTile, n_rows - row0);
  constexpr int kQuads = kNarrowTile / 4;
  bool capped = false;
  for (int it = tid; it < n_cols * kQuads; it += kNarrowThreads) {
    const int col = it / kQuads, r0 = 4 * (it % kQuads);
    uint32_t packed = 0, sum = 0;
    if (r0 < n_r) {
      const double* const cell = &tile[col * kTileStride + r0];
      double* const dst = out_log + (int64_t)col * n_rows + row0 + r0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (r0 + j < n_r) {
          const double val = cell[j];
          dst[j] = val;
          const double tq = __builtin_fma(val, -1.0 / 3.0, 0.25);
          uint32_t m;
          if (tq < 100.0) m = (uint32_t)(int)tq;
          else { m = 255u; capped |= val == val; }
          packed |= m << (8 * j);
          sum += m;
        }
      }
    }
    if (row0 + r0 < ldm) *reinterpret_cast<uint32_t*>(miss8 + (int64_t)col * ldm + row0 + r0) = packed;
    if (sum) atomicAdd(&col_sum[col], sum);
  }
  if (__ballot(capped) && lane == 0) atomicOr(flags, 1u);
  if (blockIdx.x == n_tiles - 1) {      // a stride beyond the last tile: zero as well
    const int64_t pad0 = n_tiles * kNarrowTile;
    const int64_t n_pad = ldm > pad0 ? (ldm - pad0) / 4 : 0;
    for (int64_t it = tid; it < n_cols * n_pad; it += kNarrowThreads) {
      const int64_t col = it / n_pad, w = it % n_pad;
      *reinterpret_cast<uint32_t*>(miss8 + col * ldm + pad0 + 4 * w) = 0u;
    }
  }
  __syncthreads();
  if (tid < n_cols && col_sum[tid]) atomicAdd(&msum[tid], col_sum[tid]);
}

}  // namespace

extern "C" {

/* gk_compat_log_miss_cols + gk_miss_colsum for a list of at most 8 alleles: d_log [n_table_cols][n_rows], d_miss8
 * [n_table_cols][ldm] (zero from n_rows up to ldm), *d_flags (bits 0, 2 and 3) and d_msum uint32 [n_table_cols] = the
 * column sums of the bytes written, all bit-identical to what those two calls leave. */
int gk_compat_log_miss_narrow(gk_ctx* ctx, gk_tab* tab, gk_dptr d_rows, int64_t n_rows, gk_dptr d_vflag, int32_t vbeg,
                              int32_t vend, gk_dptr d_mask, int32_t words, int32_t n_allele, int32_t keep_empty, gk_lut* lut,
                              const int32_t* table_cols, int32_t n_table_cols, gk_dptr d_log, gk_dptr d_miss8, int64_t ldm,
                              gk_dptr d_flags, gk_dptr d_msum) {
  gk_bind(ctx);
  GK_REQUIRE(ctx && tab && lut, "null pointer");
  GK_REQUIRE(words >= 1 && n_allele >= 0 && n_allele <= words * 32 && vend >= vbeg, "bad mask geometry");
  GK_REQUIRE(table_cols && n_table_cols >= 1 && n_table_cols <= n_allele, "bad column list");
  GK_REQUIRE(n_table_cols <= kNarrowCols, "the narrow table holds at most 8 columns");
  for (int c = 0; c < n_table_cols; ++c)
    GK_REQUIRE(table_cols[c] >= 0 && table_cols[c] < n_allele && (c == 0 || table_cols[c] > table_cols[c - 1]),
               "table columns must be allele ordinals, ascending and unique");
  if (n_rows == 0) return GK_OK;
  GK_REQUIRE(d_log && d_miss8 && d_flags && d_msum, "null output");
  GK_REQUIRE(ldm >= n_rows && ldm % 64 == 0, "mismatch table stride must be a multiple of 64 rows");
  const int n_span = vend - vbeg;
  NarrowCols cols{};
  for (int c = 0; c < n_table_cols; ++c) cols.c[c] = table_cols[c];
  GkBlocks temps(ctx);
  uint8_t* colbits = nullptr;
  if (temps.take(&colbits, (size_t)std::max(n_span, 4)) != hipSuccess) {
    gk_set_error("out of device memory for the column bytes");
    return GK_ERR_HIP;
  }
  const unsigned col_blocks = (unsigned)std::max(1, (n_span + kColThreads - 1) / kColThreads);
  GK_PROF(ctx, "cols_bytes",
          GK_KERNEL(cols_bytes, dim3(col_blocks), dim3(kColThreads), 0, ctx->stream, gk_ptr<uint32_t>(d_mask), n_span, words,
                    cols, n_table_cols, colbits, gk_ptr<uint32_t>(d_flags), gk_ptr<uint32_t>(d_msum)));
  const int64_t n_tiles = (n_rows + kNarrowTile - 1) / kNarrowTile;
#define GK_ROWS8_GO(LANES)                                                                                                  \
  GK_KERNEL(compat_rows8<LANES>, dim3((unsigned)n_tiles), dim3(kNarrowThreads), 0, ctx->stream, gk_ptr<int32_t>(d_rows),   \
            n_rows, tab->d_off, tab->d_ids, gk_ptr<uint8_t>(d_vflag), vbeg, n_span, colbits, n_table_cols, gk_lut_view(lut), \
            keep_empty ? 0.999 : 1.0, gk_ptr<double>(d_log), gk_ptr<uint8_t>(d_miss8), ldm, n_tiles,                        \
            gk_ptr<uint32_t>(d_flags), gk_ptr<uint32_t>(d_msum))
  GK_PROF(ctx, "compat_rows8", {
    if (n_table_cols <= 4) GK_ROWS8_GO(4);      // 16 rows of 4 lanes per wave
    else GK_ROWS8_GO(8);
  });
#undef GK_ROWS8_GO
  GK_HIP(hipGetLastError());
  return GK_OK;
}

}  // extern "C"
