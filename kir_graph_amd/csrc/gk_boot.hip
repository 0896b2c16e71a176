// Read bootstrap of the EM strategy: B replicates of every gene of a sample in one call (gk_em_bootstrap).
//
//   boot_resample    a replicate draws n reads with replacement from the gene's n reads (n = the sum of the multiplicities
//                    of its distinct candidate sets, the empty set included) and keeps, per distinct set, how many of the
//                    draws fell on it.  The draws are counter-based (gk_draw.h: a splitmix64 finish of seed, draw, replicate and the
//                    gene's stream number), so any thread makes any draw and a replicate depends on nothing but its own
//                    four numbers; draw j belongs to the set u with cum[u] <= j < cum[u + 1] (a bisection of the inclusive
//                    prefix sums).  A workgroup takes a chunk of the draws of one (gene, replicate): prefix sums and a
//                    histogram in LDS when the gene has at most kBootLdsSets sets (flushed with one global atomic per
//                    non-zero bin), prefix sums through L2 and global atomics beyond.  Integer adds only: exact, whatever
//                    the schedule.
//   boot_em_batch    hisatEMnp (typing_em.py:107-188) for every (gene, replicate): a workgroup each runs the solver of
//                    gk_squarem.h -- the one em_kernel_genes of gk_em.hip runs for the point estimate, so a replicate's
//                    abundances are what the point EM gives for the replicate's counts, bit for bit.  The two sparse
//                    forms of a gene (members of a set / sets of an allele) are built once and shared by its replicates;
//                    a replicate owns its weight row (the counts of boot_resample, read as they are) and its scale row
//                    (LDS up to kBootScaleLds sets, HBM / L2 beyond).
#include <algorithm>
#include <vector>

#include "gk_common.h"
#include "gk_calls.h"
#include "gk_draw.h"
#include "gk_squarem.h"

namespace {

constexpr int kMaxBoot = 10000;

// ------------------------------------------------------------------------------------------------ resampling
constexpr int kBootThreads = 256;
constexpr int kBootLdsSets = 8192;           // prefix sums + histogram of a gene in LDS up to this many sets (64 KB)
constexpr uint32_t kBootChunk = 1u << 14;    // draws of a workgroup, at least (16 per set where the sets are staged)

struct BootDraw {      // one gene of boot_resample (blockIdx.z)
  int64_t cum_off;     // inclusive prefix sums of the multiplicities [n_sets]
  int64_t cnt_off;     // the gene's counts within a replicate's row
  uint32_t n_sets, n, stream, chunk;
};

// the number of prefix sums <= j: the set the draw falls on (sets without reads are stepped over)
__device__ inline uint32_t boot_find(const uint32_t* cum, uint32_t n_sets, uint32_t j) {
  uint32_t lo = 0, hi = n_sets;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (cum[mid] <= j) lo = mid + 1; else hi = mid;
  }
  return min(lo, n_sets - 1);      // j < cum[n_sets - 1] by construction
}

__global__ __launch_bounds__(kBootThreads) void boot_resample(const BootDraw* __restrict__ jobs, const uint32_t* __restrict__ cum_all,
                                                              uint64_t seed, int64_t row_sets, uint32_t* __restrict__ cnt_all) {
  extern __shared__ __align__(16) unsigned char boot_lds[];
  const BootDraw J = jobs[blockIdx.z];
  const uint64_t begin = (uint64_t)blockIdx.x * J.chunk;
  if (begin >= J.n) return;
  const uint64_t end = min(begin + (uint64_t)J.chunk, (uint64_t)J.n);
  const uint32_t b = blockIdx.y;
  const uint32_t* cum = cum_all + J.cum_off;
  uint32_t* cnt = cnt_all + (int64_t)b * row_sets + J.cnt_off;
  const int tid = threadIdx.x;
  if (J.n_sets <= (uint32_t)kBootLdsSets) {
    uint32_t* lcum = (uint32_t*)boot_lds;
    uint32_t* hist = lcum + J.n_sets;
    for (uint32_t e = tid; e < J.n_sets; e += kBootThreads) { lcum[e] = cum[e]; hist[e] = 0u; }
    __syncthreads();
    for (uint64_t i = begin + tid; i < end; i += kBootThreads)
      atomicAdd(&hist[boot_find(lcum, J.n_sets, gk_boot_draw(seed, i, b, J.stream, J.n))], 1u);
    __syncthreads();
    for (uint32_t e = tid; e < J.n_sets; e += kBootThreads)
      if (hist[e]) atomicAdd(&cnt[e], hist[e]);
  } else {
    for (uint64_t i = begin + tid; i < end; i += kBootThreads)
      atomicAdd(&cnt[boot_find(cum, J.n_sets, gk_boot_draw(seed, i, b, J.stream, J.n))], 1u);
  }
}

// ------------------------------------------------------------------------------------------------ SQUAREM, batched
constexpr int kEmThreads = 512;
constexpr int kBootScaleLds = 4096;      // sets whose 1 / (sum of member abundances) live in LDS; more go through HBM / L2

// a gene of boot_em_batch (blockIdx.y) is an EmGene: its non-empty distinct sets, shared by the replicates; w_off: the first
// non-empty set's count within a replicate's row of counts, s_off: its scales within a replicate's row of scales (genes
// beyond kBootScaleLds only), job: the caller's number of the gene

struct BootArrays {
  const uint32_t* cnt;      // [n_boot][row_sets]
  double* scale;            // [n_boot][row_scale]
  const uint32_t* set_off;
  const uint16_t* members;
  const uint32_t* al_off;
  const uint32_t* al_sets;
  int64_t row_sets, row_scale;
};

__global__ __launch_bounds__(kEmThreads) void boot_em_batch(const EmGene* __restrict__ genes, BootArrays A, int n_jobs, int64_t row_prob,
                                                            int iter_max, double diff_threshold, double* __restrict__ prob_all,
                                                            int* __restrict__ iters_all) {
  extern __shared__ __align__(16) unsigned char boot_lds[];
  EmLds& sh = *reinterpret_cast<EmLds*>(boot_lds);
  const EmGene G = genes[blockIdx.y];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x;
  EmView<uint32_t> g;
  g.weight = A.cnt + b * A.row_sets + G.w_off;
  g.set_off = A.set_off + G.so_off;
  g.members = A.members + G.mem_off;
  g.al_off = A.al_off + G.ao_off;
  g.al_sets = A.al_sets + G.mem_off;
  g.scale = G.n_sets <= kBootScaleLds ? reinterpret_cast<double*>(boot_lds + sizeof(EmLds)) : A.scale + b * A.row_scale + G.s_off;
  g.n_sets = G.n_sets;
  g.n_allele = G.n_allele;
  double* prob_out = prob_all + b * row_prob + G.prob_off;      // zero when the kernel starts
  // a replicate whose draws all fell on the empty set names nobody: its abundances stay zero
  if (tid < 64) {
    uint32_t any = 0u;
    for (int u = tid; u < g.n_sets; u += 64) any |= g.weight[u];
    const unsigned long long some = __ballot(any != 0u);
    if (tid == 0) sh.flag = some != 0ull;
  }
  __syncthreads();
  if (!sh.flag) return;
  em_solve<kEmThreads>(sh, g, iter_max, diff_threshold, prob_out, iters_all + b * n_jobs + G.job);
}

bool empty_set(const uint32_t* row, int words) {
  for (int q = 0; q < words; ++q)
    if (row[q]) return false;
  return true;
}

}  // namespace

extern "C" {

/* B bootstrap replicates of the EM of every listed gene in one call: one launch that draws the replicate weights of all
 * (gene, replicate) pairs, one that runs their SQUAREM loops (a workgroup each), one wait.  See include/graphkir_hip.h. */
int gk_em_bootstrap(gk_ctx* ctx, const gk_boot_job* jobs, int32_t n_jobs, int32_t n_boot, uint64_t seed, int32_t iter_max,
                    double diff_threshold, double* prob_out, int32_t* iters_out, uint32_t* counts_out) {
  gk_bind(ctx);
  GK_REQUIRE(ctx && prob_out && iters_out && n_jobs >= 0 && (jobs || !n_jobs), "null pointer");
  GK_REQUIRE(n_boot >= 1 && n_boot <= kMaxBoot, "the number of bootstrap replicates must lie in 1 .. 10000");
  int64_t row_sets = 0, row_prob = 0;
  std::vector<int64_t> set_at((size_t)n_jobs, 0), prob_at((size_t)n_jobs, 0);
  std::vector<uint64_t> reads((size_t)n_jobs, 0);
  for (int i = 0; i < n_jobs; ++i) {
    const gk_boot_job& j = jobs[i];
    GK_REQUIRE(j.n_sets >= 0 && j.words >= 1 && j.words <= kMaxWords && j.n_allele >= 0 && j.n_allele <= j.words * 32,
               "bad bootstrap job: at most 16 words and words * 32 alleles per gene");
    GK_REQUIRE(!j.n_sets || (j.sets && j.count), "null pointer");
    for (int u = 0; u < j.n_sets; ++u) {
      reads[i] += j.count[u];
      GK_REQUIRE(u == 0 || !empty_set(j.sets + (size_t)u * j.words, j.words),
                 "bootstrap job: the sets must be distinct and ascending (an empty set can only come first)");
    }
    GK_REQUIRE(reads[i] < (1ull << 31), "bootstrap job: 2^31 reads or more");
    set_at[i] = row_sets;
    prob_at[i] = row_prob;
    row_sets += j.n_sets;
    row_prob += j.n_allele;
  }
  std::fill(prob_out, prob_out + (size_t)n_boot * row_prob, 0.0);
  std::fill(iters_out, iters_out + (size_t)n_boot * n_jobs, 0);
  if (counts_out) std::fill(counts_out, counts_out + (size_t)n_boot * row_sets, 0u);
  // ---- host: prefix sums of the genes that have reads, the sparse forms of those that have a non-empty set
  std::vector<BootDraw> draws;
  std::vector<uint32_t> cum((size_t)row_sets, 0u);
  EmForms h;
  int64_t row_scale = 0;      // a replicate's scales: the genes whose scale row does not fit LDS, one after the other
  uint32_t max_chunks = 1;
  size_t draw_lds = 0;
  for (int i = 0; i < n_jobs; ++i) {
    const gk_boot_job& j = jobs[i];
    if (!j.n_sets || !reads[i]) continue;
    uint32_t run = 0;
    for (int u = 0; u < j.n_sets; ++u) cum[(size_t)set_at[i] + u] = run += j.count[u];
    BootDraw d{set_at[i], set_at[i], (uint32_t)j.n_sets, (uint32_t)reads[i], j.stream, kBootChunk};
    if (j.n_sets <= kBootLdsSets) {
      d.chunk = std::max<uint32_t>(kBootChunk, (uint32_t)j.n_sets * 16u);
      draw_lds = std::max(draw_lds, (size_t)j.n_sets * 2 * sizeof(uint32_t));
    }
    max_chunks = std::max(max_chunks, (d.n + d.chunk - 1) / d.chunk);
    draws.push_back(d);
    const int first = empty_set(j.sets, j.words) ? 1 : 0;      // the empty set names nobody: its draws are dropped
    if (j.n_sets > first && j.n_allele > 0) {
      EmGene& g = h.add(j.sets + (size_t)first * j.words, j.n_sets - first, j.words, j.n_allele);
      g.w_off = set_at[i] + first;
      g.prob_off = prob_at[i];
      g.job = i;
      if (g.n_sets > kBootScaleLds) { g.s_off = row_scale; row_scale += g.n_sets; }
    }
  }
  if (draws.empty()) return GK_OK;
  // ---- device
  hipStream_t st = ctx->stream;
  GkCall call(ctx);      // after draws, cum and h, which the stream reads (below)
  BootDraw* d_draws = nullptr;
  EmGene* d_genes = nullptr;
  uint32_t *d_cum = nullptr, *d_cnt = nullptr, *d_so = nullptr, *d_ao = nullptr, *d_as = nullptr;
  uint16_t* d_mem = nullptr;
  double *d_scale = nullptr, *d_prob = nullptr;
  int* d_it = nullptr;
  const size_t cnt_bytes = (size_t)n_boot * row_sets * sizeof(uint32_t);
  const size_t prob_bytes = (size_t)n_boot * row_prob * sizeof(double);
  const size_t it_bytes = (size_t)n_boot * n_jobs * sizeof(int);
  if (call.take(&d_draws, draws.size() * sizeof(BootDraw)) != hipSuccess ||
      call.take(&d_cum, cum.size() * sizeof(uint32_t)) != hipSuccess ||
      call.take(&d_cnt, cnt_bytes) != hipSuccess ||
      call.take(&d_genes, h.genes.size() * sizeof(EmGene)) != hipSuccess ||
      call.take(&d_so, h.set_off.size() * sizeof(uint32_t)) != hipSuccess ||
      call.take(&d_mem, h.members.size() * sizeof(uint16_t)) != hipSuccess ||
      call.take(&d_ao, h.al_off.size() * sizeof(uint32_t)) != hipSuccess ||
      call.take(&d_as, h.al_sets.size() * sizeof(uint32_t)) != hipSuccess ||
      call.take(&d_scale, (size_t)n_boot * row_scale * sizeof(double)) != hipSuccess ||
      call.take(&d_prob, prob_bytes) != hipSuccess ||
      call.take(&d_it, it_bytes) != hipSuccess) {
    gk_set_error("out of device memory for the EM bootstrap of a sample");
    return GK_ERR_HIP;
  }
  const size_t em_lds = sizeof(EmLds) + (size_t)std::min(h.max_sets, kBootScaleLds) * sizeof(double);
  if ((draw_lds > 48 * 1024 && hipFuncSetAttribute((const void*)boot_resample, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                  (int)draw_lds) != hipSuccess) ||
      (em_lds > 48 * 1024 && hipFuncSetAttribute((const void*)boot_em_batch, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                (int)em_lds) != hipSuccess)) {
    gk_set_error("EM bootstrap: %zu / %zu bytes of LDS refused", draw_lds, em_lds);
    return GK_ERR_HIP;
  }
  // a copy too large for the ring is queued straight from its vector: no wait per copy -- the one at the end covers them
  // all, and a way out before it drains the stream while the vectors (declared before the record) still live
  call.expect();
  GK_TRY("EM bootstrap: queueing the draws", gk_send(ctx, d_draws, draws.data(), draws.size() * sizeof(BootDraw)));
  GK_TRY("EM bootstrap: queueing the draws", gk_send(ctx, d_cum, cum.data(), cum.size() * sizeof(uint32_t)));
  GK_TRY("EM bootstrap: queueing the draws", hipMemsetAsync(d_cnt, 0, cnt_bytes, st));
  GK_PROF(ctx, "boot_resample", GK_KERNEL(boot_resample, dim3(max_chunks, (unsigned)n_boot, (unsigned)draws.size()),
                                          dim3(kBootThreads), draw_lds, st, d_draws, d_cum, seed, row_sets, d_cnt));
  if (!h.genes.empty()) {
    const char* const what = "EM bootstrap: queueing the sparse forms";
    GK_TRY(what, gk_send(ctx, d_genes, h.genes.data(), h.genes.size() * sizeof(EmGene)));
    GK_TRY(what, gk_send(ctx, d_so, h.set_off.data(), h.set_off.size() * sizeof(uint32_t)));
    GK_TRY(what, gk_send(ctx, d_mem, h.members.data(), h.members.size() * sizeof(uint16_t)));
    GK_TRY(what, gk_send(ctx, d_as, h.al_sets.data(), h.al_sets.size() * sizeof(uint32_t)));
    GK_TRY(what, gk_send(ctx, d_ao, h.al_off.data(), h.al_off.size() * sizeof(uint32_t)));
    if (prob_bytes) GK_TRY(what, hipMemsetAsync(d_prob, 0, prob_bytes, st));
    GK_TRY(what, hipMemsetAsync(d_it, 0, it_bytes, st));
    const BootArrays A{d_cnt, d_scale, d_so, d_mem, d_ao, d_as, row_sets, row_scale};
    GK_PROF(ctx, "boot_em_batch", GK_KERNEL(boot_em_batch, dim3((unsigned)n_boot, (unsigned)h.genes.size()), dim3(kEmThreads),
                                            em_lds, st, d_genes, A, (int)n_jobs, row_prob, (int)iter_max, diff_threshold, d_prob,
                                            d_it));
    GK_TRY("EM bootstrap: queueing the results", call.fetch(prob_out, d_prob, prob_bytes));
    GK_TRY("EM bootstrap: queueing the results", call.fetch(iters_out, d_it, it_bytes));
  }
  if (counts_out) GK_TRY("EM bootstrap: queueing the counts", call.fetch(counts_out, d_cnt, cnt_bytes));
  GK_TRY("EM bootstrap: launch", hipGetLastError());
  GK_TRY("EM bootstrap: launch", call.wait());
  return GK_OK;
}

}  // extern "C"
