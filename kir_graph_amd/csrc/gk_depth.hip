// Per-position read depth of the filtered, uniquely mapped pairs.
//
// Replaces `samtools depth -aa {name}.no_multi.bam` (samtools_utils.py:9-14, main.py:152-158): the
// reference rewrites the filter-passing pairs with NH == 1 to a BAM and lets samtools count, for
// every backbone position, the reads whose aligned (M) bases cover it; deletions are not counted,
// soft clips are not aligned, mates are counted independently (no overlap removal).
// Here: one thread per mate adds +1 / -1 at the ends of every M run into a difference array over
// the concatenated backbones, one exclusive scan turns it into depths.
#include <cstddef>

#include "gk_blocks.h"

namespace {

constexpr int kThreads = 256;
constexpr int kInsWord = offsetof(gk_mate, ins) / 4;      // ins[0] of a record whose pair is in the wide array: its place there
static_assert(offsetof(gk_mate, cig) == 12 && offsetof(gk_mate, pos0) == 0, "gk_mate layout");

// kCompact: the sample in the compact form of gk_mates_compact (c_off word offsets [n_mates + 1], c_words) instead of
// 128-byte records -- a mate's header is words 0 - 2 there, its CIGAR starts at word 3, and a mate whose pair is in the
// wide array carries that pair's place (ins[0] of the record) in word 3.
template <bool kCompact>
__global__ __launch_bounds__(kThreads) void depth_mark(const gk_mate* __restrict__ mates,
                                                       const uint32_t* __restrict__ c_off,
                                                       const uint32_t* __restrict__ c_words,
                                                       const gk_mate_wide* __restrict__ wide,
                                                       const int32_t* __restrict__ pair_src,
                                                       const uint8_t* __restrict__ pair_nh, int64_t n_valid,
                                                       int multiple, const int64_t* __restrict__ gene_off, int n_gene,
                                                       uint32_t* __restrict__ diff) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= 2 * n_valid) return;
  const int64_t i = t >> 1;
  if (!multiple && pair_nh[i] != 1) return;
  const int64_t at = 2 * (int64_t)pair_src[i] + (t & 1);
  // header words 0 - 2 (pos0 | flag, ref, nh | nm, n_cig, n_mm, n_ins), then the words that hold the CIGAR / the wide index
  const uint32_t* w = kCompact ? c_words + c_off[at] : reinterpret_cast<const uint32_t*>(mates + at);
  const uint32_t ref = (w[1] >> 16) & 0xFFu, n_ops = (w[2] >> 8) & 0xFFu;
  if ((int)ref >= n_gene) return;
  const int64_t base = gene_off[ref], len = gene_off[ref + 1] - base;
  int64_t cur = w[0];
  auto run = [&](uint32_t op, uint32_t n) {
    if (op == GK_CIG_M) {
      const int64_t a = cur < 0 ? 0 : cur, b = cur + n > len ? len : cur + n;
      if (b > a) {
        atomicAdd(&diff[base + a], 1u);
        atomicAdd(&diff[base + b], 0xFFFFFFFFu);   // -1 (mod 2^32); diff has one slot past the end
      }
      cur += n;
    } else if (op == GK_CIG_D) {
      cur += n;
    }
  };
  if (n_ops == GK_SPILLED) {   // the pair is in the wide array (gk_mate_wide): its CIGAR is there
    if (!wide) return;
    const uint32_t slot = kCompact ? w[3] : w[kInsWord];
    const gk_mate_wide& x = wide[2 * (int64_t)slot + (t & 1)];
    const int n_cig = x.n_cig < GK_WIDE_CIG ? x.n_cig : GK_WIDE_CIG;
    for (int c = 0; c < n_cig; ++c) run(x.cig[c] & 15u, x.cig[c] >> 4);
    return;
  }
  const int n_cig = n_ops < GK_MAX_CIG ? (int)n_ops : GK_MAX_CIG;
  for (int c = 0; c < n_cig; ++c) {      // uint16 operations, two to a word, from word 3 in either form
    const uint32_t x = w[3 + (c >> 1)];
    const uint32_t cg = (c & 1) ? (x >> 16) : (x & 0xFFFFu);
    run(cg & 15u, cg >> 4);
  }
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
    const uint32_t* c_off = gk_ptr<const uint32_t>(d_compact);
    if (c_off)
      GK_KERNEL(depth_mark<true>, grid, dim3(kThreads), 0, st, (const gk_mate*)nullptr, c_off, c_off + 2 * tab->n_pairs + 1,
                tab->d_wide, tab->d_pair_src, tab->d_pair_nh, tab->n_valid, multiple, d_off, n_gene, diff);
    else
      GK_KERNEL(depth_mark<false>, grid, dim3(kThreads), 0, st, gk_ptr<const gk_mate>(d_mates), c_off, c_off, tab->d_wide,
                tab->d_pair_src, tab->d_pair_nh, tab->n_valid, multiple, d_off, n_gene, diff);
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
