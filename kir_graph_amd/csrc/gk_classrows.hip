// Weighted row classes as bit planes: see gk_classrows.h for the idea.
//
//   class_clear     the counters, the weights, the representatives and the column sums start from their identities
//   class_weights   w[class_of[r]] += 1 and rep[class_of[r]] = min(r) over the rows (vector atomics on a cleared array; the
//                   representative is read first and the atomic left to the rows that lower it)
//   class_planes    counts[b] = classes with bit b in their weight, [24] = classes, [26] = highest class + 1: one ballot per
//                   bit and wave into an LDS histogram, one global add per non-empty bin and workgroup; the grid covers
//                   n_rows, the upper bound of the class count
//   class_scatter   every (class, set bit) takes a slot of its plane from the plane's cursor, one atomic per wave and bit
//                   (the order inside a plane is free: the sums are integers); row_of[slot] = rep; and the plane of every
//                   block (blk_shift)
//   class_gather    Q[a][p] = miss8[a][row_of[p]] for the filled slots of a plane, 0 for its padding; whole words; and the
//                   column sums of the row table on the way, msum[a] += 2^plane x the bytes written: they take 3 to 9 % of
//                   the pass over the rows that colsum_u8 makes.  (Gathered per class from the row table they cost more
//                   than that pass: a byte per 64-byte line -- measured, profiles/r24_class_bound.txt.)
#include "gk_classrows.h"
#include "gk_calls.h"

namespace {

constexpr int kThreads = 256;
constexpr int kHi = 26;      // counter: highest class with a row, + 1
constexpr int kCursor0 = 32;      // counters from here: the cursors of the planes (class_scatter)

inline unsigned nblk(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

// [counters and cursors | w] = 0, rep = all bits set, msum = 0 (the column sums by class are accumulated): one launch
__global__ __launch_bounds__(kThreads) void class_clear(uint32_t* __restrict__ zero, int64_t n_zero, uint32_t* __restrict__ rep,
                                                        int64_t n_rep, uint32_t* __restrict__ msum, int n_msum) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n_zero) zero[i] = 0u;
  if (i < n_rep) rep[i] = 0xFFFFFFFFu;
  if (msum && i < n_msum) msum[i] = 0u;
}

// Adds to ONE word are served one after the other, and a class of a deep sample holds thousands of rows -- a third of
// the table is not rare.  So a workgroup takes 4096 rows; the rows of a wave that share the class of its first pending
// lane count as one (a few rounds of it); the counts go to a table of the workgroup in LDS, where a class owns the slot
// it is first to claim (whoever finds its slot taken adds in HBM at once); and the table is flushed with one add per
// class and workgroup.  Lanes and rounds rise with the rows, so a group's first lane holds its lowest row.
constexpr int kWeightRounds = 16, kWeightSlots = 1024;
constexpr uint32_t kNoClass = 0xFFFFFFFFu;

__device__ inline void weight_global(uint32_t* w, uint32_t* rep, uint32_t c, uint32_t n, uint32_t r) {
  atomicAdd(&w[c], n);
  if (__hip_atomic_load(&rep[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > r) atomicMin(&rep[c], r);
}

__global__ __launch_bounds__(kThreads) void class_weights(const uint32_t* __restrict__ class_of, int64_t n_rows,
                                                          uint32_t n_bound, uint32_t* w, uint32_t* rep) {
  __shared__ uint32_t tag[kWeightSlots], cnt[kWeightSlots], low[kWeightSlots];
  for (int i = threadIdx.x; i < kWeightSlots; i += kThreads) { tag[i] = kNoClass; cnt[i] = 0u; low[i] = kNoClass; }
  __syncthreads();
  auto add = [&](uint32_t c, uint32_t n, uint32_t r) {
    const uint32_t slot = c & (kWeightSlots - 1);
    uint32_t t = __hip_atomic_load(&tag[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (t == kNoClass) {
      t = atomicCAS(&tag[slot], kNoClass, c);
      if (t == kNoClass) t = c;
    }
    if (t == c) { atomicAdd(&cnt[slot], n); atomicMin(&low[slot], r); }
    else weight_global(w, rep, c, n, r);
  };
  const int lane = threadIdx.x & 63;
  const int64_t first = (int64_t)blockIdx.x * (kThreads * kWeightRounds);
  for (int k = 0; k < kWeightRounds; ++k) {
    const int64_t r = first + (int64_t)k * kThreads + threadIdx.x;
    const uint32_t c = r < n_rows ? class_of[r] : kNoClass;
    bool todo = c < n_bound;      // a class beyond the table's (the caller's array): the row counts nowhere
    for (int round = 0; round < 4; ++round) {
      const uint64_t pending = __ballot(todo);
      if (!pending) break;
      const int leader = __ffsll((unsigned long long)pending) - 1;
      const uint32_t lc = (uint32_t)__shfl((int)c, leader, 64);
      const bool same = todo && c == lc;
      const uint64_t group = __ballot(same);
      if (lane == leader) add(lc, (uint32_t)__popcll(group), (uint32_t)r);
      todo = todo && !same;
    }
    if (todo) add(c, 1u, (uint32_t)r);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kWeightSlots; i += kThreads)
    if (cnt[i]) weight_global(w, rep, tag[i], cnt[i], low[i]);
}

__global__ __launch_bounds__(kThreads) void class_planes(const uint32_t* __restrict__ w, uint32_t n_bound,
                                                         const uint32_t* __restrict__ flags, uint32_t* counts) {
  __shared__ uint32_t bins[kClassCounters];
  if (threadIdx.x < kClassCounters) bins[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t c = blockIdx.x * kThreads + threadIdx.x;
  const uint32_t wv = c < n_bound ? w[c] : 0u;
  const uint64_t any = __ballot(wv != 0u);
  if (any) {
    const int lane = threadIdx.x & 63;
    for (int b = 0; b < kClassPlanes; ++b) {
      const uint64_t has = __ballot((wv >> b) & 1u);
      if (has && lane == 0) atomicAdd(&bins[b], (uint32_t)__popcll(has));
    }
    if (lane == 0) {
      atomicAdd(&bins[kClassPlanes], (uint32_t)__popcll(any));
      atomicMax(&bins[kHi], c + 64u - (uint32_t)__builtin_clzll(any));      // the wave's highest lane with a row, + 1
    }
  }
  __syncthreads();
  if (threadIdx.x <= kClassPlanes && bins[threadIdx.x]) atomicAdd(&counts[threadIdx.x], bins[threadIdx.x]);
  if (threadIdx.x == kHi && bins[kHi]) atomicMax(&counts[kHi], bins[kHi]);
  if (blockIdx.x == 0 && threadIdx.x == 0 && flags) counts[kClassPlanes + 1] = *flags;
}

__device__ inline uint32_t sum_bytes(uint32_t x, uint32_t acc) { return __builtin_amdgcn_sad_u8(x, 0u, acc); }

// first pseudo-row and filled slots of every plane
struct Planes { uint32_t row0[kClassPlanes], count[kClassPlanes]; };

// A workgroup takes kScatterPer x 256 classes: its waves count their set bits plane by plane into LDS (what a wave finds
// there is its place in the workgroup), ONE add per plane and workgroup takes the workgroup's run of slots from the
// plane's cursor, and the ballots, formed again, place every lane.
constexpr int kScatterPer = 4;
__global__ __launch_bounds__(kThreads) void class_scatter(const uint32_t* __restrict__ w, const uint32_t* __restrict__ rep,
                                                          uint32_t hi, Planes pl, uint32_t n_blk, uint32_t* cursor,
                                                          int32_t* __restrict__ row_of, uint8_t* __restrict__ blk_shift) {
  __shared__ uint32_t total[kClassPlanes];
  __shared__ uint32_t place[kScatterPer * (kThreads / 64)][kClassPlanes];
  const uint32_t g = blockIdx.x * kThreads + threadIdx.x;
  if (g < n_blk) {      // the plane of block g: the last one that starts at or before it (empty planes start where the next does)
    int b = 0;
    for (int k = 1; k < kClassPlanes; ++k)
      if (pl.count[k] && pl.row0[k] / kClassBlockRows <= g) b = k;
    blk_shift[g] = (uint8_t)b;
  }
  if (threadIdx.x < kClassPlanes) total[threadIdx.x] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t wv[kScatterPer];
#pragma unroll
  for (int j = 0; j < kScatterPer; ++j) {
    const uint32_t c = (blockIdx.x * kScatterPer + j) * kThreads + threadIdx.x;
    wv[j] = c < hi ? w[c] : 0u;
    for (int b = 0; b < kClassPlanes; ++b) {
      const uint64_t has = __ballot((wv[j] >> b) & 1u);
      if (lane == 0) place[j * (kThreads / 64) + wave][b] = has ? atomicAdd(&total[b], (uint32_t)__popcll(has)) : 0u;
    }
  }
  __syncthreads();
  if (threadIdx.x < kClassPlanes && total[threadIdx.x]) total[threadIdx.x] = atomicAdd(&cursor[threadIdx.x], total[threadIdx.x]);
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kScatterPer; ++j) {
    if (!__ballot(wv[j] != 0u)) continue;
    const uint32_t c = (blockIdx.x * kScatterPer + j) * kThreads + threadIdx.x;
    const uint32_t r = wv[j] ? rep[c] : 0u;
    for (int b = 0; b < kClassPlanes; ++b) {
      const bool mine = (wv[j] >> b) & 1u;
      const uint64_t has = __ballot(mine);
      if (!mine) continue;
      const uint32_t k = total[b] + place[j * (kThreads / 64) + wave][b] + (uint32_t)__popcll(has & ((1ull << lane) - 1ull));
      if (k < pl.count[b]) row_of[pl.row0[b] + k] = (int32_t)r;
    }
  }
}

// Q[a][p] = miss8[a][row_of[p]] for the filled slots of a plane, 0 for its padding: a thread takes kGatherIter times four
// pseudo-rows of kGatherCols columns (the rows are looked up once per eight columns), whole words out.  And msum[a]
// (cleared) += the bytes written, 2^plane times: the column sums of the row table (32 bits: a sum over the rows, below
// 2^32), a workgroup's 4096 pseudo-rows in ONE add per column (adds to one word are served one after the other)
constexpr int kGatherCols = 8, kGatherIter = 4;
__global__ __launch_bounds__(kThreads) void class_gather(const uint8_t* __restrict__ miss8, int64_t ldm, int64_t n_rows,
                                                         int n_cols, const int32_t* __restrict__ row_of,
                                                         const uint8_t* __restrict__ blk_shift, Planes pl, int64_t ldq,
                                                         uint8_t* __restrict__ Q, uint32_t* msum) {
  const int a0 = (int)blockIdx.y * kGatherCols;
  uint32_t acc[kGatherCols];
#pragma unroll
  for (int q = 0; q < kGatherCols; ++q) acc[q] = 0u;
  for (int it = 0; it < kGatherIter; ++it) {
    const int64_t p0 = 4 * (((int64_t)blockIdx.x * kGatherIter + it) * kThreads + threadIdx.x);
    if (p0 >= ldq) break;
    const int b = blk_shift[p0 / kClassBlockRows];
    const int64_t filled = (int64_t)pl.row0[b] + pl.count[b];      // slots of this plane before its padding
    const int4 rows = *reinterpret_cast<const int4*>(row_of + p0);
    const int32_t r4[4] = {rows.x, rows.y, rows.z, rows.w};
    bool ok[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) ok[j] = p0 + j < filled && (int64_t)(uint32_t)r4[j] < n_rows;
#pragma unroll
    for (int q = 0; q < kGatherCols; ++q) {
      const int a = a0 + q;
      if (a >= n_cols) break;
      const uint8_t* col = miss8 + (int64_t)a * ldm;
      uint32_t packed = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (ok[j]) packed |= (uint32_t)col[r4[j]] << (8 * j);
      *reinterpret_cast<uint32_t*>(Q + (int64_t)a * ldq + p0) = packed;
      acc[q] += sum_bytes(packed, 0u) << b;
    }
  }
  __shared__ uint32_t part[kThreads / 64][kGatherCols];
#pragma unroll
  for (int q = 0; q < kGatherCols; ++q) {
    uint32_t sum = acc[q];
    for (int off = 32; off > 0; off >>= 1) sum += (uint32_t)__shfl_xor((int)sum, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][q] = sum;
  }
  __syncthreads();
  if (threadIdx.x < kGatherCols && a0 + (int)threadIdx.x < n_cols) {
    uint32_t sum = 0;
    for (int wv = 0; wv < kThreads / 64; ++wv) sum += part[wv][threadIdx.x];
    if (sum) atomicAdd(&msum[a0 + threadIdx.x], sum);
  }
}

}  // namespace

int gk_classweights_enqueue(gk_ctx* ctx, const uint32_t* class_of, int64_t n_rows, const uint32_t* d_flags, uint32_t* msum,
                            int n_msum, GkClassWeights* out) {
  GK_REQUIRE(ctx && class_of && out && n_rows > 0 && n_rows < (int64_t)16000000 && n_msum >= 0 && (msum || n_msum == 0),
             "bad class-weight arguments");
  hipStream_t st = ctx->stream;
  GkBlocks blocks(ctx);
  char* base = nullptr;      // [counters, cursors | w | rep]
  const size_t per = (size_t)n_rows * sizeof(uint32_t), head = kClassCounterWords * sizeof(uint32_t);
  if (blocks.take(&base, head + 2 * per) != hipSuccess) {
    gk_set_error("out of device memory for the class weights");
    return GK_ERR_HIP;
  }
  uint32_t* counts = reinterpret_cast<uint32_t*>(base);
  uint32_t* w = reinterpret_cast<uint32_t*>(base + head);
  uint32_t* rep = reinterpret_cast<uint32_t*>(base + head + per);
  const int64_t n_clear = std::max<int64_t>(n_rows + kClassCounterWords, n_msum);
  GK_PROF(ctx, "class_clear", GK_KERNEL(class_clear, dim3(nblk(n_clear)), dim3(kThreads), 0, st, counts,
                                        n_rows + kClassCounterWords, rep, n_rows, msum, n_msum));
  GK_PROF(ctx, "class_weights",
          GK_KERNEL(class_weights, dim3(nblk((n_rows + kWeightRounds - 1) / kWeightRounds)), dim3(kThreads), 0, st, class_of,
                    n_rows, (uint32_t)n_rows, w, rep));
  GK_PROF(ctx, "class_planes",
          GK_KERNEL(class_planes, dim3(nblk(n_rows)), dim3(kThreads), 0, st, w, (uint32_t)n_rows, d_flags, counts));
  GK_HIP(hipGetLastError());
  out->class_of = class_of; out->n_rows = n_rows; out->w = w; out->rep = rep; out->counts = counts;
  out->blocks = std::move(blocks);
  return GK_OK;
}

int gk_classrows_build(gk_ctx* ctx, const GkClassWeights& cw, const uint32_t* counts_host, const uint8_t* miss8, int64_t ldm,
                       int n_cols, uint32_t* msum, GkClassRows* out) {
  GK_REQUIRE(ctx && cw.w && counts_host && miss8 && msum && out && n_cols > 0 && n_cols <= 65535 && ldm >= cw.n_rows,
             "bad pseudo-row arguments");
  *out = GkClassRows();
  char form[8];      // GK_TEST_HOOKS=class_bound=nomem: as if the pool had refused the record
  if (gk_test_hook("class_bound", form, sizeof(form)) && !strcmp(form, "nomem")) return GK_OK;
  GkClassRows rec;
  const int64_t ldq = gk_class_planes(counts_host, rec.plane_blk0);
  const uint32_t hi = counts_host[kHi];
  // what the counters may say of a table of n_rows rows; anything else is not a record to build from
  GK_REQUIRE(ldq > 0 && hi >= 1 && (int64_t)hi <= cw.n_rows && (int64_t)counts_host[kClassPlanes] <= cw.n_rows,
             "class counters out of range");
  const int64_t n_blk = ldq / kClassBlockRows;
  Planes pl;
  for (int b = 0; b < kClassPlanes; ++b) {
    GK_REQUIRE(counts_host[b] <= counts_host[kClassPlanes], "class counters out of range");
    pl.row0[b] = (uint32_t)(rec.plane_blk0[b] * kClassBlockRows);
    pl.count[b] = counts_host[b];
  }
  rec.blocks.begin(ctx);
  uint32_t* cursor = nullptr;
  int32_t* row_of = nullptr;
  if (rec.blocks.take(&rec.Q, (size_t)n_cols * (size_t)ldq) != hipSuccess ||
      rec.blocks.take(&rec.blk_shift, (size_t)n_blk) != hipSuccess) return GK_OK;      // the bound runs on the rows
  GkBlocks temps(ctx);
  if (temps.take(&row_of, (size_t)ldq * sizeof(int32_t)) != hipSuccess) return GK_OK;
  hipStream_t st = ctx->stream;
  cursor = cw.counts + kCursor0;      // zero since class_clear: the weights serve ONE build
  GK_PROF(ctx, "class_scatter",
          GK_KERNEL(class_scatter, dim3(std::max(nblk((hi + kScatterPer - 1) / kScatterPer), nblk(n_blk))), dim3(kThreads), 0,
                    st, cw.w, cw.rep, hi, pl, (uint32_t)n_blk, cursor, row_of, rec.blk_shift));
  GK_PROF(ctx, "class_gather",
          GK_KERNEL(class_gather, dim3(nblk((ldq / 4 + kGatherIter - 1) / kGatherIter), (unsigned)((n_cols + kGatherCols - 1) / kGatherCols)), dim3(kThreads), 0,
                    st, miss8, ldm, cw.n_rows, n_cols, row_of, rec.blk_shift, pl, ldq, rec.Q, msum));
  GK_HIP(hipGetLastError());
  rec.ldq = ldq; rec.n_rows = cw.n_rows; rec.n_cols = n_cols;
  *out = std::move(rec);
  return GK_OK;
}

bool gk_use_class_bound(int64_t padded_pseudo_rows, int64_t n_rows) {
  char form[8];
  if (gk_test_hook("class_bound", form, sizeof(form))) {
    if (!strcmp(form, "on") || !strcmp(form, "nomem")) return true;
    if (!strcmp(form, "off")) return false;
  }
  return 2 * padded_pseudo_rows <= n_rows;
}

extern "C" {

int gk_miss_colsum(gk_ctx* ctx, gk_dptr d_miss8, int64_t ldm, int32_t n_cols, gk_dptr d_msum);

/* gk_bound_step on the pseudo-rows of a table whose rows fall into classes: d_class_of (device, uint32 [n_rows]) names the
 * class of every row, 0 <= class < n_classes, and rows of one class hold the same byte in every column (the caller's word
 * for it; the representative of a class is its lowest row).  d_msum (device, uint32, one entry per column up to the highest
 * one that ids or cols name) receives the column sums, formed by class.  Results as gk_bound_step. */
int gk_bound_step_classes(gk_ctx* ctx, gk_dptr d_miss8, int64_t ldm, int64_t n_rows, gk_dptr d_class_of, int64_t n_classes,
                          gk_dptr d_msum, const int32_t* ids, int32_t n_sets, int32_t c_prev, const int32_t* cols,
                          int32_t n_cols, const uint8_t* first, int32_t top_n, int32_t cap, uint32_t* hdr_out,
                          int32_t* idx_out, uint32_t* m_out) {
  gk_bind(ctx);
  GK_REQUIRE(ctx && d_miss8 && d_class_of && d_msum && ids && cols && first && hdr_out && idx_out && m_out, "null pointer");
  GK_REQUIRE(n_sets >= 1 && n_cols >= 1 && c_prev >= 1 && c_prev <= 8 && top_n >= 1 && cap >= 1, "bad bound arguments");
  GK_REQUIRE(ldm >= n_rows && ldm % 64 == 0 && n_rows > 0, "mismatch table stride must be a multiple of 64 rows");
  GK_REQUIRE(n_rows < (int64_t)16000000, "too many reads for 32-bit mismatch totals");
  GK_REQUIRE(n_classes >= 1 && n_classes <= n_rows, "the classes of a table are at least one and at most its rows");
  int32_t n_tab = 0;      // the columns the call names
  for (size_t i = 0; i < (size_t)n_sets * c_prev; ++i) { GK_REQUIRE(ids[i] >= 0, "negative column"); n_tab = std::max(n_tab, ids[i] + 1); }
  for (int a = 0; a < n_cols; ++a) { GK_REQUIRE(cols[a] >= 0, "negative column"); n_tab = std::max(n_tab, cols[a] + 1); }
  GK_REQUIRE(n_tab <= 65535, "too many columns");
  const uint8_t* miss8 = gk_ptr<uint8_t>(d_miss8);
  GkClassWeights cw;
  GkClassRows rec;
  int rc = gk_classweights_enqueue(ctx, gk_ptr<uint32_t>(d_class_of), n_rows, nullptr, gk_ptr<uint32_t>(d_msum), n_tab, &cw);
  if (rc) return rc;
  uint32_t counts[kClassCounters];
  GK_HIP(gk_fetch(ctx, counts, cw.counts, sizeof(counts)));
  GK_REQUIRE((int64_t)counts[kHi] <= n_classes && (int64_t)counts[kClassPlanes] >= 1, "a row names a class beyond n_classes");
  {
    uint64_t rows = 0;      // every row was counted: no class id lay outside the table
    for (int b = 0; b < kClassPlanes; ++b) rows += (uint64_t)counts[b] << b;
    GK_REQUIRE(rows == (uint64_t)n_rows, "a row names a class beyond n_classes");
  }
  int64_t plane_blk0[kClassPlanes + 1];
  if (gk_use_class_bound(gk_class_planes(counts, plane_blk0), n_rows)) {
    rc = gk_classrows_build(ctx, cw, counts, miss8, ldm, n_tab, gk_ptr<uint32_t>(d_msum), &rec);
    if (rc) return rc;
  }
  if (!rec.ready()) {      // the row route, or a pool that refused the pseudo-rows
    rc = gk_miss_colsum(ctx, d_miss8, ldm, n_tab, d_msum);
    if (rc) return rc;
  }
  GkBoundCall call;
  rc = gk_call_wait(ctx, call,
                    gk_bound_enqueue_classes(ctx, d_miss8, ldm, n_rows, d_msum, ids, n_sets, c_prev, cols, n_cols, first,
                                             top_n, cap, rec.ready() ? &rec : nullptr, call),
                    "bound step by classes");
  if (rc == GK_OK) gk_bound_collect(ctx, call, hdr_out, idx_out, m_out);
  return rc;
}

/* The slices of the bound over the planes of a pseudo-row table (the planner of gk_bound_enqueue_classes, for tests and
 * tools; no device): plane_counts[24] classes per plane, `want` slices to fill the GPU; slices_out receives (first block,
 * end block, shift, 0) per slice, at most `capacity` slices; *n_slices their number; plane_blk0_out[25] (may be null) the
 * first block of every plane and the number of blocks. */
int gk_class_slice_plan(const uint32_t* plane_counts, int64_t want, int32_t* slices_out, int32_t capacity, int32_t* n_slices,
                        int64_t* plane_blk0_out) {
  GK_REQUIRE(plane_counts && n_slices && want >= 1 && capacity >= 0 && (capacity == 0 || slices_out), "bad plan arguments");
  int64_t blk0[kClassPlanes + 1];
  gk_class_planes(plane_counts, blk0);
  std::vector<int32_t> tab;
  gk_class_slices(blk0, want, tab);
  *n_slices = (int32_t)(tab.size() / 4);
  std::copy(tab.begin(), tab.begin() + 4 * std::min<size_t>(tab.size() / 4, (size_t)capacity), slices_out);
  if (plane_blk0_out) std::copy(blk0, blk0 + kClassPlanes + 1, plane_blk0_out);
  return GK_OK;
}

}  // extern "C"
