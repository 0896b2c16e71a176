// Read bootstrap of the EM strategy: B replicates of every gene of a sample in one call (gk_em_bootstrap).
//
//   boot_resample    a replicate draws n reads with replacement from the gene's n reads (n = the sum of the multiplicities
//                    of its distinct candidate sets, the empty set included) and keeps, per distinct set, how many of the
//                    draws fell on it.  The draws are counter-based (a splitmix64 finish of seed, draw, replicate and the
//                    gene's stream number), so any thread makes any draw and a replicate depends on nothing but its own
//                    four numbers; draw j belongs to the set u with cum[u] <= j < cum[u + 1] (a bisection of the inclusive
//                    prefix sums).  A workgroup takes a chunk of the draws of one (gene, replicate): prefix sums and a
//                    histogram in LDS when the gene has at most kBootLdsSets sets (flushed with one global atomic per
//                    non-zero bin), prefix sums through L2 and global atomics beyond.  Integer adds only: exact, whatever
//                    the schedule.
//   boot_em_batch    hisatEMnp (typing_em.py:107-188) for every (gene, replicate): a workgroup each, the SQUAREM loop of
//                    gk_em.hip restated for the batch.  The two sparse forms of a gene (members of a set / sets of an
//                    allele) are built once and shared by its replicates; a replicate owns its weight row (the counts of
//                    boot_resample, read as they are) and its scale row (LDS up to kBootScaleLds sets, HBM / L2 beyond).
//                    The solver of gk_em.hip lives in an anonymous namespace of a file whose digest pins committed PMC
//                    profiles, hence the restatement here.  Sums run in a fixed order: a replicate is bit-reproducible.
#include <algorithm>
#include <vector>

#include "gk_common.h"

namespace {

constexpr int kMaxWords = 16;      // up to 512 alleles per gene
constexpr int kMaxAllele = kMaxWords * 32;
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

__device__ inline uint32_t boot_draw(uint64_t seed, uint64_t i, uint64_t b, uint64_t g, uint32_t n) {
  uint64_t z = seed + (i + 1) * 0x9E3779B97F4A7C15ull + (b + 1) * 0xBF58476D1CE4E5B9ull + (g + 1) * 0x94D049BB133111EBull;
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (uint32_t)(((z >> 32) * (uint64_t)n) >> 32);      // < n
}

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
      atomicAdd(&hist[boot_find(lcum, J.n_sets, boot_draw(seed, i, b, J.stream, J.n))], 1u);
    __syncthreads();
    for (uint32_t e = tid; e < J.n_sets; e += kBootThreads)
      if (hist[e]) atomicAdd(&cnt[e], hist[e]);
  } else {
    for (uint64_t i = begin + tid; i < end; i += kBootThreads)
      atomicAdd(&cnt[boot_find(cum, J.n_sets, boot_draw(seed, i, b, J.stream, J.n))], 1u);
  }
}

// ------------------------------------------------------------------------------------------------ SQUAREM, batched
constexpr int kEmThreads = 512;
constexpr int kBootScaleLds = 4096;      // sets whose 1 / (sum of member abundances) live in LDS; more go through HBM / L2

// one gene of boot_em_batch (blockIdx.y): its non-empty distinct sets in two sparse forms, shared by the replicates
struct BootGene {
  int64_t w_off;          // the first non-empty set's count within a replicate's row of counts
  int64_t s_off;          // scale [n_sets] within a replicate's row of scales (genes beyond kBootScaleLds only)
  int64_t so_off;         // set_off [n_sets + 1]: members of set u = members[mem_off + set_off[u] .. set_off[u + 1])
  int64_t mem_off;        // members: allele numbers (uint16), and al_sets: set numbers (uint32) -- both nnz entries
  int64_t ao_off;         // al_off [n_allele + 1]: sets of allele a = al_sets[mem_off + al_off[a] .. al_off[a + 1])
  int64_t prob_off;
  int32_t n_sets, n_allele, job, pad;
};

struct BootArrays {
  const uint32_t* cnt;      // [n_boot][row_sets]
  double* scale;            // [n_boot][row_scale]
  const uint32_t* set_off;
  const uint16_t* members;
  const uint32_t* al_off;
  const uint32_t* al_sets;
  int64_t row_sets, row_scale;
};

struct BootLds {
  double p[kMaxAllele], p1[kMaxAllele], p2[kMaxAllele], p3[kMaxAllele];
  double scalar[4];
  int flag;
};

__device__ inline double lanes16_sum(double v) {
#pragma unroll
  for (int d = 8; d >= 1; d >>= 1) v += __shfl_xor(v, d, 16);
  return v;
}
__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

struct BootView {      // one (gene, replicate)
  const uint32_t* weight;
  const uint32_t* set_off;
  const uint16_t* members;
  const uint32_t* al_off;
  const uint32_t* al_sets;
  double* scale;
  int n_sets, n_allele;
};

// next(p): q[a] = sum_u w_u * p[a] / (sum_{b in u} p[b]) over the sets that contain a, then normalised
__device__ void em_step(const BootView& g, const double* in, double* out, double* scalar) {
  const int tid = threadIdx.x, l = tid & 15, grp = tid >> 4;
  constexpr int kGroups = kEmThreads / 16;
  for (int u0 = 0; u0 < g.n_sets; u0 += kGroups) {
    const int u = u0 + grp;
    double t = 0.0;
    if (u < g.n_sets)
      for (uint32_t k = g.set_off[u] + l, e = g.set_off[u + 1]; k < e; k += 16) t += in[g.members[k]];
    t = lanes16_sum(t);
    if (u < g.n_sets && l == 0) g.scale[u] = t != 0.0 ? (double)g.weight[u] / t : 0.0;
  }
  __syncthreads();
  for (int a0 = 0; a0 < g.n_allele; a0 += kGroups) {
    const int a = a0 + grp;
    double s = 0.0;
    if (a < g.n_allele)
      for (uint32_t k = g.al_off[a] + l, e = g.al_off[a + 1]; k < e; k += 16) s += g.scale[g.al_sets[k]];
    s = lanes16_sum(s);
    if (a < g.n_allele && l == 0) out[a] = in[a] * s;
  }
  __syncthreads();
  if (tid < 64) {
    double t = 0.0;
    for (int a = tid; a < g.n_allele; a += 64) t += out[a];
    t = wave_sum(t);
    if (tid == 0) scalar[0] = t;
  }
  __syncthreads();
  const double tot = scalar[0];
  for (int a = tid; a < g.n_allele; a += kEmThreads) out[a] = out[a] / tot;
  __syncthreads();
}

__global__ __launch_bounds__(kEmThreads) void boot_em_batch(const BootGene* __restrict__ genes, BootArrays A, int n_jobs, int64_t row_prob,
                                                            int iter_max, double diff_threshold, double* __restrict__ prob_all,
                                                            int* __restrict__ iters_all) {
  extern __shared__ __align__(16) unsigned char boot_lds[];
  BootLds& sh = *reinterpret_cast<BootLds*>(boot_lds);
  const BootGene G = genes[blockIdx.y];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x, n_allele = G.n_allele;
  BootView g;
  g.weight = A.cnt + b * A.row_sets + G.w_off;
  g.set_off = A.set_off + G.so_off;
  g.members = A.members + G.mem_off;
  g.al_off = A.al_off + G.ao_off;
  g.al_sets = A.al_sets + G.mem_off;
  g.scale = G.n_sets <= kBootScaleLds ? reinterpret_cast<double*>(boot_lds + sizeof(BootLds)) : A.scale + b * A.row_scale + G.s_off;
  g.n_sets = G.n_sets;
  g.n_allele = n_allele;
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
  for (int a = tid; a < n_allele; a += kEmThreads) sh.p3[a] = 1.0;
  __syncthreads();
  em_step(g, sh.p3, sh.p, sh.scalar);
  int iters = 0;
  for (iters = 0; iters < iter_max; ++iters) {
    em_step(g, sh.p, sh.p1, sh.scalar);
    em_step(g, sh.p1, sh.p2, sh.scalar);
    if (tid < 64) {
      double rs = 0.0, vs = 0.0;
      for (int a = tid; a < n_allele; a += 64) {
        const double r = sh.p1[a] - sh.p[a];
        const double v = sh.p2[a] - sh.p1[a] - r;
        rs += r * r;
        vs += v * v;
      }
      rs = wave_sum(rs);
      vs = wave_sum(vs);
      if (tid == 0) { sh.scalar[1] = rs; sh.scalar[2] = vs; }
    }
    __syncthreads();
    const double rs = sh.scalar[1], vs = sh.scalar[2];
    if (vs > 0.0) {
      const double gs = -sqrt(rs / vs);
      for (int a = tid; a < n_allele; a += kEmThreads) {
        const double r = sh.p1[a] - sh.p[a];
        const double v = sh.p2[a] - sh.p1[a] - r;
        const double x = sh.p[a] - r * gs * 2 + v * (gs * gs);
        sh.p3[a] = x > 0.0 ? x : 0.0;
      }
      __syncthreads();
      em_step(g, sh.p3, sh.p1, sh.scalar);
    }
    if (tid < 64) {
      double d = 0.0;
      for (int a = tid; a < n_allele; a += 64) d += fabs(sh.p[a] - sh.p1[a]);
      d = wave_sum(d);
      if (tid == 0) sh.flag = d <= diff_threshold;
    }
    __syncthreads();
    if (sh.flag) break;
    for (int a = tid; a < n_allele; a += kEmThreads) sh.p[a] = sh.p1[a];
    __syncthreads();
  }
  for (int a = tid; a < n_allele; a += kEmThreads) prob_out[a] = sh.p[a];
  if (tid == 0) iters_all[b * n_jobs + G.job] = iters;
}

// the sparse forms of a gene's non-empty distinct sets, appended to the call's arrays (as EmHost::add of gk_em.hip builds them)
struct BootHost {
  std::vector<BootGene> genes;
  std::vector<uint32_t> set_off, al_off, al_sets;
  std::vector<uint16_t> members;
  int max_sets = 0;
  int64_t row_scale = 0;
  void add(const uint32_t* sets, int n_sets, int words, int n_allele, int64_t w_off, int64_t prob_off, int job) {
    BootGene g{w_off, 0, (int64_t)set_off.size(), (int64_t)members.size(), (int64_t)al_off.size(), prob_off, n_sets, n_allele, job, 0};
    if (n_sets > kBootScaleLds) { g.s_off = row_scale; row_scale += n_sets; }
    std::vector<uint32_t> per_allele((size_t)n_allele + 1, 0);
    const size_t m0 = members.size();
    for (int u = 0; u < n_sets; ++u) {
      set_off.push_back((uint32_t)(members.size() - m0));
      for (int q = 0; q < words; ++q) {
        uint32_t bits = sets[(size_t)u * words + q];
        while (bits) {
          const int a = q * 32 + __builtin_ctz(bits);
          bits &= bits - 1;
          if (a >= n_allele) continue;
          members.push_back((uint16_t)a);
          per_allele[(size_t)a + 1]++;
        }
      }
    }
    set_off.push_back((uint32_t)(members.size() - m0));
    for (int a = 0; a < n_allele; ++a) per_allele[(size_t)a + 1] += per_allele[a];
    al_off.insert(al_off.end(), per_allele.begin(), per_allele.end());
    al_sets.resize(members.size());
    std::vector<uint32_t> at(per_allele.begin(), per_allele.end() - 1);
    for (int u = 0; u < n_sets; ++u)
      for (uint32_t k = set_off[(size_t)g.so_off + u]; k < set_off[(size_t)g.so_off + u + 1]; ++k)
        al_sets[m0 + at[members[m0 + k]]++] = (uint32_t)u;       // ascending set numbers per allele
    genes.push_back(g);
    max_sets = std::max(max_sets, n_sets);
  }
};

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
  BootHost h;
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
    if (j.n_sets > first && j.n_allele > 0)
      h.add(j.sets + (size_t)first * j.words, j.n_sets - first, j.words, j.n_allele, set_at[i] + first, prob_at[i], i);
  }
  if (draws.empty()) return GK_OK;
  // ---- device
  hipStream_t st = ctx->stream;
  std::vector<void*> temps;
  auto take = [&](void** p, size_t bytes) -> hipError_t {
    hipError_t e = gk_pool_malloc(ctx, p, bytes ? bytes : 16);
    if (e == hipSuccess) temps.push_back(*p);
    return e;
  };
  auto done = [&](int rc) { for (void* p : temps) gk_pool_free(ctx, p); return rc; };
  // a failure after the first queued copy: the stream still reads this call's vectors and may write its outputs
  auto fail = [&](const char* what) {
    const hipError_t e = hipGetLastError();
    gk_fetch_cancel(ctx);
    gk_set_error("EM bootstrap: %s: %s", what, hipGetErrorString(e));
    return done(GK_ERR_HIP);
  };
  BootDraw* d_draws = nullptr;
  BootGene* d_genes = nullptr;
  uint32_t *d_cum = nullptr, *d_cnt = nullptr, *d_so = nullptr, *d_ao = nullptr, *d_as = nullptr;
  uint16_t* d_mem = nullptr;
  double *d_scale = nullptr, *d_prob = nullptr;
  int* d_it = nullptr;
  const size_t cnt_bytes = (size_t)n_boot * row_sets * sizeof(uint32_t);
  const size_t prob_bytes = (size_t)n_boot * row_prob * sizeof(double);
  const size_t it_bytes = (size_t)n_boot * n_jobs * sizeof(int);
  if (take((void**)&d_draws, draws.size() * sizeof(BootDraw)) != hipSuccess ||
      take((void**)&d_cum, cum.size() * sizeof(uint32_t)) != hipSuccess ||
      take((void**)&d_cnt, cnt_bytes) != hipSuccess ||
      take((void**)&d_genes, h.genes.size() * sizeof(BootGene)) != hipSuccess ||
      take((void**)&d_so, h.set_off.size() * sizeof(uint32_t)) != hipSuccess ||
      take((void**)&d_mem, h.members.size() * sizeof(uint16_t)) != hipSuccess ||
      take((void**)&d_ao, h.al_off.size() * sizeof(uint32_t)) != hipSuccess ||
      take((void**)&d_as, h.al_sets.size() * sizeof(uint32_t)) != hipSuccess ||
      take((void**)&d_scale, (size_t)n_boot * h.row_scale * sizeof(double)) != hipSuccess ||
      take((void**)&d_prob, prob_bytes) != hipSuccess ||
      take((void**)&d_it, it_bytes) != hipSuccess) {
    gk_set_error("out of device memory for the EM bootstrap of a sample");
    return done(GK_ERR_HIP);
  }
  const size_t em_lds = sizeof(BootLds) + (size_t)std::min(h.max_sets, kBootScaleLds) * sizeof(double);
  if ((draw_lds > 48 * 1024 && hipFuncSetAttribute((const void*)boot_resample, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                  (int)draw_lds) != hipSuccess) ||
      (em_lds > 48 * 1024 && hipFuncSetAttribute((const void*)boot_em_batch, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                (int)em_lds) != hipSuccess)) {
    gk_set_error("EM bootstrap: %zu / %zu bytes of LDS refused", draw_lds, em_lds);
    return done(GK_ERR_HIP);
  }
  // the sources of the large copies live until the stream is waited for below
  if (gk_send(ctx, d_draws, draws.data(), draws.size() * sizeof(BootDraw)) != hipSuccess ||
      gk_send(ctx, d_cum, cum.data(), cum.size() * sizeof(uint32_t)) != hipSuccess ||
      hipMemsetAsync(d_cnt, 0, cnt_bytes, st) != hipSuccess)
    return fail("queueing the draws");
  GK_PROF(ctx, "boot_resample", GK_KERNEL(boot_resample, dim3(max_chunks, (unsigned)n_boot, (unsigned)draws.size()),
                                          dim3(kBootThreads), draw_lds, st, d_draws, d_cum, seed, row_sets, d_cnt));
  if (!h.genes.empty()) {
    if (gk_send(ctx, d_genes, h.genes.data(), h.genes.size() * sizeof(BootGene)) != hipSuccess ||
        gk_send(ctx, d_so, h.set_off.data(), h.set_off.size() * sizeof(uint32_t)) != hipSuccess ||
        gk_send(ctx, d_mem, h.members.data(), h.members.size() * sizeof(uint16_t)) != hipSuccess ||
        gk_send(ctx, d_as, h.al_sets.data(), h.al_sets.size() * sizeof(uint32_t)) != hipSuccess ||
        gk_send(ctx, d_ao, h.al_off.data(), h.al_off.size() * sizeof(uint32_t)) != hipSuccess ||
        (prob_bytes && hipMemsetAsync(d_prob, 0, prob_bytes, st) != hipSuccess) ||
        hipMemsetAsync(d_it, 0, it_bytes, st) != hipSuccess)
      return fail("queueing the sparse forms");
    const BootArrays A{d_cnt, d_scale, d_so, d_mem, d_ao, d_as, row_sets, h.row_scale};
    GK_PROF(ctx, "boot_em_batch", GK_KERNEL(boot_em_batch, dim3((unsigned)n_boot, (unsigned)h.genes.size()), dim3(kEmThreads),
                                            em_lds, st, d_genes, A, (int)n_jobs, row_prob, (int)iter_max, diff_threshold, d_prob,
                                            d_it));
    if (gk_fetch_queue(ctx, prob_out, d_prob, prob_bytes) != hipSuccess ||
        gk_fetch_queue(ctx, iters_out, d_it, it_bytes) != hipSuccess)
      return fail("queueing the results");
  }
  if (counts_out && gk_fetch_queue(ctx, counts_out, d_cnt, cnt_bytes) != hipSuccess) return fail("queueing the counts");
  if (hipGetLastError() != hipSuccess || gk_fetch_wait(ctx) != hipSuccess) return fail("launch");
  return done(GK_OK);
}

}  // extern "C"
