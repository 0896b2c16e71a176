// The SQUAREM solver of the EM strategy (hisatEMnp, typing_em.py:107-188), shared by the point estimate (em_kernel_genes of
// gk_em.hip: double weights, 1024 threads) and the read bootstrap (boot_em_batch of gk_boot.hip: a replicate's uint32 counts,
// 512 threads), and the host-side builder of the two sparse forms of a gene's distinct sets that both launches read.
// A workgroup runs the whole loop of one solve: 16 lanes per set or allele, the abundances in LDS, the totals over the first
// wave.  No sum depends on the workgroup size and every sum runs in a fixed order, so the two instantiations give the same
// bits for the same sets and weights, run after run.  Compiled into two translation units: everything here is a template
// or sits in the anonymous namespace.
#pragma once
#include <algorithm>
#include <vector>

#include "gk_common.h"

namespace {

constexpr int kMaxWords = 16;    // up to 512 alleles per gene
constexpr int kMaxAllele = kMaxWords * 32;

// ------------------------------------------------------------------------------------------------ device
struct EmLds {      // the scale row of the solve follows it in LDS when it fits
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

// one gene of a launch: where its distinct sets, in two sparse forms, and its rows lie within the launch's arrays
struct EmGene {
  int64_t w_off;          // weight [n_sets] (the bootstrap: within a replicate's row of counts)
  int64_t s_off;          // scale [n_sets] (the bootstrap: within a replicate's row of scales)
  int64_t so_off;         // set_off [n_sets + 1]: members of set u = members[mem_off + set_off[u] .. set_off[u + 1])
  int64_t mem_off;        // members: allele numbers (uint16), and al_sets: set numbers (uint32) -- both nnz entries
  int64_t ao_off;         // al_off [n_allele + 1]: sets of allele a = al_sets[mem_off + al_off[a] .. al_off[a + 1])
  int64_t prob_off;
  int32_t n_sets, n_allele, job, pad;
};

template <typename W>
struct EmView {      // one solve: W = double (the point estimate) or uint32_t (a replicate's counts, converted where read)
  const W* weight;
  const uint32_t* set_off;
  const uint16_t* members;
  const uint32_t* al_off;
  const uint32_t* al_sets;
  double* scale;
  int n_sets, n_allele;
};

// next(p): q[a] = sum_u w_u * p[a] / (sum_{b in u} p[b]) over the sets that contain a, then normalised
template <int kThreads, typename W>
__device__ void em_step(const EmView<W>& g, const double* in, double* out, double* scalar) {
  const int tid = threadIdx.x, l = tid & 15, grp = tid >> 4;
  constexpr int kGroups = kThreads / 16;
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
  for (int a = tid; a < g.n_allele; a += kThreads) out[a] = out[a] / tot;
  __syncthreads();
}

// the whole SQUAREM loop of one solve by a workgroup of kThreads; abundances to prob_out, the steps taken to *iters_out.
// *iters_out is the number of the pass (from 0) whose difference met diff_threshold -- the abundances are those from
// before that pass -- or iter_max when no pass did: iter_max says "did not stop", which no stopping pass can (they are
// 0 .. iter_max - 1).  The reference returns no count; a Python loop variable would be left at iter_max - 1 here.
template <int kThreads, typename W>
__device__ void em_solve(EmLds& sh, const EmView<W>& g, int iter_max, double diff_threshold, double* prob_out, int* iters_out) {
  const int tid = threadIdx.x;
  const int n_allele = g.n_allele;
  for (int a = tid; a < n_allele; a += kThreads) sh.p3[a] = 1.0;
  __syncthreads();
  em_step<kThreads>(g, sh.p3, sh.p, sh.scalar);
  int iters = 0;
  for (iters = 0; iters < iter_max; ++iters) {
    em_step<kThreads>(g, sh.p, sh.p1, sh.scalar);
    em_step<kThreads>(g, sh.p1, sh.p2, sh.scalar);
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
      for (int a = tid; a < n_allele; a += kThreads) {
        const double r = sh.p1[a] - sh.p[a];
        const double v = sh.p2[a] - sh.p1[a] - r;
        const double x = sh.p[a] - r * gs * 2 + v * (gs * gs);
        sh.p3[a] = x > 0.0 ? x : 0.0;
      }
      __syncthreads();
      em_step<kThreads>(g, sh.p3, sh.p1, sh.scalar);
    }
    if (tid < 64) {
      double d = 0.0;
      for (int a = tid; a < n_allele; a += 64) d += fabs(sh.p[a] - sh.p1[a]);
      d = wave_sum(d);
      if (tid == 0) sh.flag = d <= diff_threshold;
    }
    __syncthreads();
    if (sh.flag) break;
    for (int a = tid; a < n_allele; a += kThreads) sh.p[a] = sh.p1[a];
    __syncthreads();
  }
  for (int a = tid; a < n_allele; a += kThreads) prob_out[a] = sh.p[a];
  if (tid == 0) *iters_out = iters;
}

// ------------------------------------------------------------------------------------------------ host
// the sparse forms of the genes of a launch, one after the other.  The weights stay with the caller.
struct EmForms {
  std::vector<EmGene> genes;
  std::vector<uint32_t> set_off, al_off, al_sets;
  std::vector<uint16_t> members;
  int max_sets = 0;
  // sorted, non-empty distinct sets [n_sets][words] of a gene; the caller fills in w_off, s_off, prob_off and job
  EmGene& add(const uint32_t* sets, int n_sets, int words, int n_allele) {
    EmGene g{0, 0, (int64_t)set_off.size(), (int64_t)members.size(), (int64_t)al_off.size(), 0, n_sets, n_allele, 0, 0};
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
    max_sets = std::max(max_sets, n_sets);
    genes.push_back(g);
    return genes.back();
  }
};

}  // namespace
