// Exact value + shares of a FEW allele sets, and the column sums of a narrow table: one workgroup owns one chunk.
//
//   gk_few_enqueue, c >= 2  typing_mulit_allele.py:540-542 for one set + 575-580 (value and undivided shares per set)
//   gk_few_enqueue, c == 1  typing_mulit_allele.py:514 (log_probs[:, cols].sum(axis=0))
//
// The one-set steps of exon-first ask for ONE set of 2 .. 4 alleles over a table of ~750 k rows, a dozen times per
// sample.  setsum_leaves (gk_search.hip) gives such a call a 1024-thread workgroup per 128-row leaf, of which 8 lanes
// hold accumulators, stages the columns through LDS and hands the leaf sums to fold_leaves through HBM.  Here the grid
// is (chunks of 8192 rows, sets): a workgroup reads the rows of ITS chunk in the columns ITS set names, straight from
// global memory into registers, folds the leaves in LDS and leaves one sum per output; the workgroup that finishes last
// for its set adds the chunk sums.  One launch, the named columns read once, nothing staged.
//
// The summation tree is numpy's add.reduce, as in gk_search.hip.  The DEVICE side is restated here and shares no code with
// that file: the committed traffic measurements of a kernel are tied to the digest of its own file + gk_common.h
// (build.KERNEL_SOURCES), so an edit to one file leaves the other's profiles valid.  The host's walk of the tree is
// gk_tree.h for both; it is host code only, no kernel is compiled from it, and it is in neither digest -- an edit to it
// invalidates no profile.  Chunks of 8192 rows are added in sequence; a chunk is halved
// (n2 = n/2, n2 -= n2 % 8) down to leaves of <= 128 rows; a leaf summed by 8 strided accumulators combined as
// ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then its `len & 7` tail rows in sequence (a leaf shorter than 8 is all tail).
// The per-row terms are setsum_leaves': the row's maximum, and 1 / (number of alleles that reach it) for each that does.
#include <algorithm>

#include "gk_calls.h"
#include "gk_tree.h"

namespace {

#ifndef GK_FEW_THREADS
#define GK_FEW_THREADS 256
#endif
// 256: an eight-lane group takes two of the 64 leaves of a chunk in turn.  With 512 (one leaf per group, every load of the
// chunk in flight at once) the launches took a fifth to two fifths longer (profiles/r18_setsum_few.txt)
constexpr int kFewThreads = GK_FEW_THREADS;
constexpr int kFewGroups = kFewThreads / 8;
constexpr int kFewLeafRows = 128;                    // numpy PW_BLOCKSIZE
constexpr int kFewChunkRows = 8192;                  // numpy's buffer for add.reduce
constexpr int kFewMaxLeaves = kFewChunkRows / 64;    // a leaf of a split node has >= 64 rows
constexpr int kFewMaxC = 4;
constexpr int kFewSteps = kFewLeafRows / 8;          // row steps of a lane in a full leaf
constexpr int kFewMaxSets = 4096;
constexpr int kFewTile = 1024;                       // chunk sums the last workgroup of a set holds in LDS at a time

struct FewLeaf { int32_t start, len; };              // rows [start, start + len) of the chunk
struct FewOp { int32_t dst, src; };                  // leaf sum dst += leaf sum src
// the two chunk lengths of a call: [0] 8192 rows, [1] the last chunk's; offsets into the leaf and op arrays
struct FewPlan { int32_t leaf0[2], n_leaf[2], op0[2], n_op[2]; };

__device__ inline double few_max(double a, double b) {
  double r;
  asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));   // fmax() would add two canonicalising v_max
  return r;
}

constexpr int kFewSwap1 = 0xB1;        // quad_perm:[1,0,3,2]  lane ^ 1
constexpr int kFewSwap2 = 0x4E;        // quad_perm:[2,3,0,1]  lane ^ 2
constexpr int kFewHalfMirror = 0x141;  // row_half_mirror      lane -> 7 - lane inside its group of 8

template <int kCtrl>
__device__ inline uint32_t few_dpp(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kCtrl, 0xF, 0xF, true);
}
template <int kCtrl>
__device__ inline double few_dpp(double v) {
  return __hiloint2double((int)few_dpp<kCtrl>((uint32_t)__double2hiint(v)), (int)few_dpp<kCtrl>((uint32_t)__double2loint(v)));
}
// ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) over the 8 lanes of a group, in every lane: after two steps lanes 0-3 hold the left
// half-sum and lanes 4-7 the right one, the mirror partner supplies the other half (a + b == b + a bit for bit)
template <typename T>
__device__ inline T few_sum8(T v) {
  v += few_dpp<kFewSwap1>(v);
  v += few_dpp<kFewSwap2>(v);
  v += few_dpp<kFewHalfMirror>(v);
  return v;
}

// one row of a set: acc[0 .. kC) the shares, acc[kC] the value; kC == 1: acc[0] the column's sum.  Two alleles: a row's
// shares are 1 / 0, 0 / 1 or 1/2 / 1/2, whose sums are exact in any order, so the rows an allele reaches the maximum on
// are COUNTED and the shares formed from the counts at the end of the leaf
template <int kC>
__device__ inline void few_terms(const double (&v)[kC], double (&acc)[kC == 1 ? 1 : kC + 1], uint32_t (&hits)[2]) {
  if constexpr (kC == 1) {
    acc[0] += v[0];
  } else if constexpr (kC == 2) {
    acc[2] += few_max(v[0], v[1]);
    hits[0] += v[0] >= v[1] ? 1u : 0u;
    hits[1] += v[1] >= v[0] ? 1u : 0u;
  } else {
    double best = -__builtin_huge_val();
#pragma unroll
    for (int q = 0; q < kC; ++q) best = few_max(best, v[q]);
    int cnt = 0;
#pragma unroll
    for (int q = 0; q < kC; ++q) cnt += v[q] == best ? 1 : 0;
    double share = 1.0;   // exact IEEE quotients, as numpy's bool / int
#pragma unroll
    for (int q = 2; q <= kC; ++q) share = cnt == q ? (1.0 / (double)q) : share;
#pragma unroll
    for (int q = 0; q < kC; ++q) acc[q] += v[q] == best ? share : 0.0;   // 0.0 + x == x: first term exact
    acc[kC] += best;
  }
}

// grid (chunks, sets), kFewThreads threads.  `out`: per set kO sums (the pinned result ring)
template <int kC>
__global__ __launch_bounds__(kFewThreads) void setsum_few(const double* __restrict__ L, int64_t ld, int64_t n_rows,
                                                          const int32_t* __restrict__ ids,
                                                          const FewLeaf* __restrict__ leaves,
                                                          const FewOp* __restrict__ ops, FewPlan plan,
                                                          double* chunk_sums, uint32_t* __restrict__ tickets,
                                                          double* __restrict__ out) {
  constexpr int kO = kC == 1 ? 1 : kC + 1;
  // four alleles: the loads of a leaf come in two halves (64 float64 per lane would leave no room for the rest)
  constexpr int kHalves = kC == 4 ? 2 : 1;
  constexpr int kQ = kFewSteps / kHalves;
  __shared__ double lsum[kFewMaxLeaves * kO];        // [leaf of the chunk][output]
  __shared__ FewOp s_ops[kFewMaxLeaves];
  __shared__ double s_tile[kFewTile];                // chunk sums of the set, for the workgroup that adds them
  __shared__ uint32_t s_last;
  const int tid = threadIdx.x, j = tid & 7, g = tid >> 3;
  const int chunk = blockIdx.x, set = blockIdx.y, n_chunks = gridDim.x;
  const int kind = chunk == n_chunks - 1 ? 1 : 0;
  const int n_l = plan.n_leaf[kind], n_op = plan.n_op[kind];
  const FewLeaf* const my_leaves = leaves + plan.leaf0[kind];
  if (tid < n_op) s_ops[tid] = ops[plan.op0[kind] + tid];
  const double* col[kC];
#pragma unroll
  for (int q = 0; q < kC; ++q) col[q] = L + (int64_t)ids[set * kC + q] * ld + (int64_t)chunk * kFewChunkRows;

  for (int l = g; l < n_l; l += kFewGroups) {
    const FewLeaf lf = my_leaves[l];
    const int len = lf.len;
    const int n8 = len < 8 ? 0 : len - (len & 7);    // rows summed by the 8 strided accumulators
    double acc[kO];
    uint32_t hits[2] = {0u, 0u};
#pragma unroll
    for (int o = 0; o < kO; ++o) acc[o] = 0.0;
    if (n8) {
#pragma unroll
      for (int h = 0; h < kHalves; ++h) {
        double v[kQ][kC];
        // lane j reads rows j + 8 s: the 8 lanes of a group 64 contiguous bytes per step and column.  A step past the
        // leaf's end reads row j again (it is in the leaf: n8 >= 8) and is not added
#pragma unroll
        for (int s = 0; s < kQ; ++s) {
          const int r = 8 * (h * kQ + s);
          const int at = lf.start + (r < n8 ? r : 0) + j;
#pragma unroll
          for (int q = 0; q < kC; ++q) v[s][q] = col[q][at];
        }
#pragma unroll
        for (int s = 0; s < kQ; ++s)
          if (8 * (h * kQ + s) < n8) few_terms<kC>(v[s], acc, hits);       // r[j] += a[i + j], in row order
      }
#pragma unroll
      for (int o = (kC == 2 ? 2 : 0); o < kO; ++o) acc[o] = few_sum8(acc[o]);
      if constexpr (kC == 2) {              // the counts of the group's 8 lanes (integers: any order), in every lane
        hits[0] = few_sum8(hits[0]);
        hits[1] = few_sum8(hits[1]);
      }
    }
    for (int r = n8; r < len; ++r) {        // sequential tail rows, the same in every lane of the group
      double v[kC];
#pragma unroll
      for (int q = 0; q < kC; ++q) v[q] = col[q][lf.start + r];
      few_terms<kC>(v, acc, hits);
    }
    if constexpr (kC == 2) {
      const double tied = (double)(hits[0] + hits[1] - (uint32_t)len);
      acc[0] = (double)hits[0] - 0.5 * tied;         // exact: integers and halves
      acc[1] = (double)hits[1] - 0.5 * tied;
    }
    if (j == 0) {
#pragma unroll
      for (int o = 0; o < kO; ++o) lsum[l * kO + o] = acc[o];
    }
  }
  __syncthreads();
  // the leaves of the chunk in the order of numpy's pairwise recursion (dst += src, post-order), a thread per output;
  // the chunk's sum ends in leaf 0
  double* const my_chunks = chunk_sums + (int64_t)set * n_chunks * kO;
  if (tid < kO) {
    for (int k = 0; k < n_op; ++k) lsum[s_ops[k].dst * kO + tid] += lsum[s_ops[k].src * kO + tid];
    my_chunks[(int64_t)chunk * kO + tid] = lsum[tid];
  }
  // The workgroup that finishes LAST for its set adds the chunk sums in chunk order (numpy's outer reduce loop); the
  // ticket goes back to zero for the next launch on this stream
  __threadfence();                       // this chunk's sums are visible before the ticket is taken
  __syncthreads();
  if (tid == 0) {
    const uint32_t ticket = atomicAdd(&tickets[set], 1u);
    s_last = ticket == (uint32_t)n_chunks - 1 ? 1u : 0u;
    if (s_last) tickets[set] = 0u;
  }
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  // a tile of chunk sums into LDS with every thread loading (all loads of the tile in flight together), then a thread per
  // output adds them in chunk order
  constexpr int kTileChunks = kFewTile / kO;
  double total = 0.0;
  for (int c0 = 0; c0 < n_chunks; c0 += kTileChunks) {
    const int n_here = min(kTileChunks, n_chunks - c0);
    for (int i = tid; i < n_here * kO; i += kFewThreads)
      s_tile[i] = __hip_atomic_load(&my_chunks[(int64_t)c0 * kO + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (tid < kO) {
      for (int c = 0; c < n_here; ++c) {
        const double v = s_tile[c * kO + tid];
        total = c0 + c == 0 ? v : total + v;
      }
    }
    __syncthreads();
  }
  if (tid < kO) out[(int64_t)set * kO + tid] = total;
}

// ---------------------------------------------------------------------------------------------
// host: the leaves of a chunk of n rows and the additions that fold them (they depend on n only)
void few_nodes(std::vector<FewLeaf>& leaves, std::vector<FewOp>& ops, int n) {
  const int first_leaf = (int)leaves.size();
  gk_pairwise_walk(0, n, kFewLeafRows, 0,
                   [&](int start, int len, int) {
                     leaves.push_back(FewLeaf{start, len});
                     return (int)leaves.size() - 1 - first_leaf;
                   },
                   [&](int a, int b) { ops.push_back(FewOp{a, b}); });
}

}  // namespace

// `ids`: n_sets x c column ids; c == 1: the sums of n_sets columns.  Results: per set c shares then the value (c >= 2),
// one sum (c == 1), written by the kernel into call.back's slot of the result ring
int gk_few_enqueue(gk_ctx* ctx, const GkTable& L, int64_t n_rows, const int32_t* ids, int32_t n_sets, int32_t c, GkSumCall& call) {
  gk_bind(ctx);
  GK_REQUIRE(ctx && L.d && !L.indexed() && ids && n_rows > 0 && L.ld >= n_rows, "bad arguments of the sums of a few sets");
  GK_REQUIRE(n_sets > 0 && n_sets <= kFewMaxSets, "too many sets for the chunk-owning form");
  GK_REQUIRE(c >= 1 && c <= kFewMaxC, "set size beyond the chunk-owning form");
  for (int64_t i = 0; i < (int64_t)n_sets * c; ++i) GK_REQUIRE(ids[i] >= 0, "negative allele id");
  GK_REQUIRE((n_rows + kFewChunkRows - 1) / kFewChunkRows <= 0x7fffffff / kFewChunkRows, "too many rows");
  const int n_chunks = (int)((n_rows + kFewChunkRows - 1) / kFewChunkRows);
  const int kO = c == 1 ? 1 : c + 1;

  std::vector<FewLeaf> leaves;
  std::vector<FewOp> ops;
  FewPlan plan;
  const int lens[2] = {kFewChunkRows, (int)(n_rows - (int64_t)(n_chunks - 1) * kFewChunkRows)};
  for (int k = 0; k < 2; ++k) {
    plan.leaf0[k] = (int32_t)leaves.size();
    plan.op0[k] = (int32_t)ops.size();
    few_nodes(leaves, ops, lens[k]);
    plan.n_leaf[k] = (int32_t)leaves.size() - plan.leaf0[k];
    plan.n_op[k] = (int32_t)ops.size() - plan.op0[k];
    GK_REQUIRE(plan.n_leaf[k] <= kFewMaxLeaves && plan.n_op[k] < kFewMaxLeaves && plan.n_op[k] <= kFewThreads,
               "too many leaves in a chunk");
  }
  // one parameter block: ids | leaves | ops (all 4-byte fields; the structs are pairs of int32)
  const size_t n_id = (size_t)n_sets * c;
  const size_t o_leaf = (n_id + 3) / 4 * 4, o_op = o_leaf + 2 * leaves.size();
  std::vector<int32_t> par(o_op + 2 * ops.size() + 1, 0);
  memcpy(par.data(), ids, n_id * sizeof(int32_t));
  memcpy(par.data() + o_leaf, leaves.data(), leaves.size() * sizeof(FewLeaf));
  if (!ops.empty()) memcpy(par.data() + o_op, ops.data(), ops.size() * sizeof(FewOp));
  call.begin(ctx);
  int32_t* d_par = nullptr;
  GK_HIP(call.take((void**)&d_par, par.size() * sizeof(int32_t)));
  GK_HIP(call.send(d_par, par.data(), par.size() * sizeof(int32_t)));
  double *d_chunk = nullptr, *d_out = nullptr;
  const int64_t n_out = (int64_t)n_sets * kO;
  GK_HIP(call.take((void**)&d_chunk, (size_t)n_out * n_chunks * sizeof(double)));
  GK_HIP(call.result((size_t)n_out * sizeof(double), (void**)&d_out));
  uint32_t* tickets = nullptr;
  { const int trc = gk_ctx_tickets(ctx, (size_t)n_sets, &tickets); if (trc) return trc; }
  const dim3 grid((unsigned)n_chunks, (unsigned)n_sets);
#define GK_FEW_GO(C)                                                                                                    \
  GK_PROF(ctx, "setsum_few",                                                                                            \
          GK_KERNEL(setsum_few<C>, grid, dim3(kFewThreads), 0, ctx->stream, gk_ptr<double>(L.d), L.ld, n_rows, d_par,   \
                    (const FewLeaf*)(d_par + o_leaf), (const FewOp*)(d_par + o_op), plan, d_chunk, tickets, d_out))
  switch (c) {
    case 1: GK_FEW_GO(1); break;
    case 2: GK_FEW_GO(2); break;
    case 3: GK_FEW_GO(3); break;
    default: GK_FEW_GO(4); break;
  }
#undef GK_FEW_GO
  GK_HIP(hipGetLastError());
  GK_HIP(call.finish());
  call.n_rows = n_rows;
  call.n_sets = n_sets;
  call.c = c;
  call.with_value = c >= 2;
  call.form = kSumFew;
  return GK_OK;
}

extern "C" int gk_setsum_few(gk_ctx* ctx, gk_dptr d_L, int64_t n_rows, int64_t ld, const int32_t* ids, int32_t n_sets,
                             int32_t c, double* value_out, double* frac_out) {
  gk_bind(ctx);
  GK_REQUIRE(value_out && frac_out, "null output");
  GkSumCall call;
  const int rc = gk_call_wait(ctx, call, gk_few_enqueue(ctx, GkTable{d_L, ld, nullptr}, n_rows, ids, n_sets, c, call),
                              "sums of a few sets");
  if (rc != GK_OK) return rc;
  if (c == 1) {                          // one allele owns every row: its share is rows / rows
    gk_colsum_collect(ctx, call, value_out);
    std::fill(frac_out, frac_out + n_sets, 1.0);
  } else {
    gk_shares_collect(ctx, call, value_out, frac_out);
  }
  return rc;
}
