// Per-position read depth of the filtered, uniquely mapped pairs.
//
// Replaces `samtools depth -aa {name}.no_multi.bam` (samtools_utils.py:9-14, main.py:152-158): the
// reference rewrites the filter-passing pairs with NH == 1 to a BAM and lets samtools count, for
// every backbone position, the reads whose aligned (M) bases cover it; deletions are not counted,
// soft clips are not aligned, mates are counted independently (no overlap removal).
// Here: one thread per mate adds +1 / -1 at the ends of every M run (the walk of gk_materuns.h, shared) into a
// difference array over the concatenated backbones, one exclusive scan turns it into depths.
#include "gk_blocks.h"
#include "gk_materuns.h"

namespace {

constexpr int kThreads = 256;

// one thread per mate; kCompact: the sample in the compact form of gk_mates_compact instead of 128-byte records
template <bool kCompact>
__global__ __launch_bounds__(kThreads) void depth_mark(GkMateSample s, int multiple, const int64_t* __restrict__ gene_off,
                                                       int n_gene, uint32_t* __restrict__ diff) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= 2 * s.n_valid) return;
  const int64_t i = t >> 1;
  const int side = (int)(t & 1);
  if (!multiple && s.pair_nh[i] != 1) return;
  GkMateRuns m;
  if (!gk_mate_find<kCompact>(s, i, side, [&](uint32_t ref) { return (int)ref < n_gene; }, m)) return;
  const int64_t base = gene_off[m.ref], len = gene_off[m.ref + 1] - base;
  gk_mate_walk<kCompact>(s, m, side, len, [&](int64_t a, int64_t e) {
    atomicAdd(&diff[base + a], 1u);
    atomicAdd(&diff[base + e], 0xFFFFFFFFu);   // -1 (mod 2^32); diff has one slot past the end
  });
}

__global__ __launch_bounds__(kThreads) void depth_finish(const uint32_t* excl, const uint32_t* diff, int64_t n,
                                                         uint32_t* depth /* may alias diff */) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) depth[i] = excl[i] + diff[i];
}

}  // namespace

static int depth_of(gk_ctx* ctx, gk_tab* tab, gk_dptr d_mates, gk_dptr d_compact, int32_t multiple, const int64_t* gene_off,
                    int32_t n_gene, uint32_t* depth_out) {
  gk_bind(ctx);
  GK_REQUIRE(ctx && tab && gene_off && depth_out && n_gene > 0, "bad depth arguments");
  GK_REQUIRE(tab->d_pair_src, "depth needs a tabulation made from packed records");
  GK_REQUIRE(tab->n_valid == 0 || d_mates || d_compact, "depth needs the sample's records");
  const int64_t total = gene_off[n_gene];
  hipStream_t st = ctx->stream;
  uint32_t *diff = nullptr, *scan = nullptr;
  int64_t* d_off = nullptr;
  GkBlocks temps(ctx);
  GK_HIP(temps.take(&diff, (size_t)(total + 1) * sizeof(uint32_t)));
  GK_HIP(temps.take(&scan, (size_t)(total + 1) * sizeof(uint32_t)));
  GK_HIP(temps.take(&d_off, (size_t)(n_gene + 1) * sizeof(int64_t)));
  GK_HIP(hipMemsetAsync(diff, 0, (size_t)(total + 1) * sizeof(uint32_t), st));
  GK_HIP(hipMemcpyAsync(d_off, gene_off, (size_t)(n_gene + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
  if (tab->n_valid) {
    const dim3 grid((unsigned)((2 * tab->n_valid + kThreads - 1) / kThreads));
    const GkMateSample s = gk_mate_sample(tab, d_mates, d_compact);
    if (s.c_off)
      GK_KERNEL(depth_mark<true>, grid, dim3(kThreads), 0, st, s, multiple, d_off, n_gene, diff);
    else
      GK_KERNEL(depth_mark<false>, grid, dim3(kThreads), 0, st, s, multiple, d_off, n_gene, diff);
  }
  GK_HIP(hipMemcpyAsync(scan, diff, (size_t)(total + 1) * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  int rc = gk_scan_u32(ctx, scan, total + 1, nullptr);
  if (rc) return rc;
  GK_KERNEL(depth_finish, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, scan, diff,
                     total, diff);
  GK_HIP(hipGetLastError());
  GK_HIP(hipMemcpyAsync(depth_out, diff, (size_t)total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  GK_HIP(hipStreamSynchronize(st));
  return GK_OK;
}

extern "C" int gk_depth(gk_ctx* ctx, gk_tab* tab, gk_dptr d_mates, int32_t multiple, const int64_t* gene_off,
                        int32_t n_gene, uint32_t* depth_out) {
  return depth_of(ctx, tab, d_mates, 0, multiple, gene_off, n_gene, depth_out);
}

/* gk_depth for a sample whose records are in HBM in the compact form (gk_mates_compact / gk_mates_compact_host) --
 * the sample the tabulation was made from, by gk_tabulate_compact or from the expanded records. */
extern "C" int gk_depth_compact(gk_ctx* ctx, gk_tab* tab, gk_dptr d_compact, int32_t multiple, const int64_t* gene_off,
                                int32_t n_gene, uint32_t* depth_out) {
  GK_REQUIRE(d_compact || (tab && tab->n_valid == 0), "null compact records");
  return depth_of(ctx, tab, 0, d_compact, multiple, gene_off, n_gene, depth_out);
}
