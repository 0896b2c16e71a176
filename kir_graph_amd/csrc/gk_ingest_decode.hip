// The decode step of the ingest on the device: the plain pairs of a BAM file -- nothing but M and D ops,
// everything gk_mate_decode.h restates -- become their two gk_mate records in a kernel, the packer decodes the rest
// (gk_ingest.h: gk_bam_pack_with, gk_packer_decode_subset).  The inflated stream goes up as it is; inflate, record
// index, name sort and pairing stay on the host.  Asked for by name (--ingest-decode device); gk_bam_pack is untouched.
#include <atomic>

#include "gk_blocks.h"
#include "gk_ingest.h"
#include "gk_mate_decode.h"

namespace {

constexpr int kThreads = 256;

// One lane per mate: the mates of pair p in lanes 2p (left) and 2p + 1 (right) of the launch, so a pair never straddles
// a wave.  A lane runs the shared code and nothing else; neighbouring lanes exchange three bits -- after the scan "my
// scan succeeded" and "my mate passes", after the walk "my record is complete".  EVERY lane of the wave takes part in
// all three exchanges, whatever it has found and also past 2 * n_pairs: nothing returns before the last one.  The
// record goes straight to its global slot (a private gk_mate indexed by n_mm / k would live in scratch); a HOST pair
// leaves anything there.  words: the stream as whole aligned words; pairs[t]: record number of lane t's mate, checked
// against n_recs; every record lies inside the stream (the host checks the table before it is sent).
__global__ __launch_bounds__(kThreads) void ingest_decode_pairs(const uint32_t* __restrict__ words,
                                                                const GkBamRec* __restrict__ recs, int64_t n_recs,
                                                                const int64_t* __restrict__ pairs, int64_t n_pairs,
                                                                const int32_t* __restrict__ gene_of_ref, int32_t n_ref,
                                                                gk_mate* __restrict__ out, uint8_t* __restrict__ verdict) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const bool live = t < 2 * n_pairs;
  const GkWordBytes b{words};
  GkMateScan s;
  bool scanned = false;
  if (live) {
    const int64_t i = pairs[t];
    if (i >= 0 && i < n_recs) {
      const GkBamRec rec = recs[i];
      scanned = gk_mate_scan(b, rec.off, rec.size, gene_of_ref, n_ref, s);
    }
  }
  const bool passes = scanned && s.passes;
  const bool mate_scanned = __shfl_xor((int)scanned, 1) != 0;
  const bool mate_passes = __shfl_xor((int)passes, 1) != 0;
  bool complete = false;
  if (scanned && mate_scanned) {
    gk_mate& r = out[t];
    if (passes && mate_passes) {
      complete = gk_mate_walk(b, s, r);
    } else {
      gk_mate_header(s, r);
      complete = true;
    }
  }
  const bool mate_complete = __shfl_xor((int)complete, 1) != 0;
  if (live && !(t & 1)) verdict[t >> 1] = (uint8_t)(complete && mate_complete ? GK_DECODE_DONE : GK_DECODE_HOST);
}

// The pairs the host decoded, patched into the device's record array: which[j] < n_pairs is the pair of the 2 x 128
// bytes at packed[16 j .. 16 j + 16).  16 lanes per pair, 16 bytes each.
__global__ __launch_bounds__(kThreads) void ingest_patch_pairs(const int64_t* __restrict__ which, int64_t n_which,
                                                               int64_t n_pairs, const uint4* __restrict__ packed,
                                                               uint4* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= 16 * n_which) return;
  const int64_t p = which[t >> 4];
  if (p < 0 || p >= n_pairs) return;
  out[16 * p + (t & 15)] = packed[t];
}

// What one call may take from the device for a list of n_pairs pairs, at the most: stream, tables, records and verdicts,
// and the patch step's list and records when every pair is HOST.  Calls run at the same time on other contexts
// (main.mapSamples: `ahead` of them), so the limit -- half the free memory -- is held against this figure PLUS what the
// calls in flight have claimed (Claim: process-wide, whatever the device; memory they hold already is missing from "free"
// as well, which errs towards the host route).
std::atomic<size_t> g_claimed{0};
struct Claim {
  size_t bytes = 0;
  bool take(size_t need, size_t limit) {
    const size_t before = g_claimed.fetch_add(need);
    if (need > limit || before > limit - need) { g_claimed.fetch_sub(need); return false; }
    bytes = need;
    return true;
  }
  ~Claim() { g_claimed.fetch_sub(bytes); }
};
size_t device_bytes(const GkBamRecords& r, int64_t n_pairs) {
  return (r.data_bytes + 3) / 4 * 4 + (size_t)r.n_recs * sizeof(GkBamRec) + (size_t)n_pairs * 2 * sizeof(int64_t) +
         r.gene_of_ref.size() * sizeof(int32_t) + (size_t)n_pairs * (2 * sizeof(gk_mate) + 1) +
         (size_t)n_pairs * (2 * sizeof(gk_mate) + sizeof(int64_t));
}

int pack_device(gk_ctx* ctx, gk_bam* bam, gk_packer* pk, gk_dptr* d_mates_out, int64_t* n_device_pairs, int64_t* n_host_pairs) {
  gk_bind(ctx);
  GK_REQUIRE(ctx && bam && pk && n_device_pairs && n_host_pairs, "gk_bam_pack_device: null argument");
  if (d_mates_out) *d_mates_out = 0;
  *n_device_pairs = *n_host_pairs = 0;
  hipStream_t st = ctx->stream;
  GkPhaseClock clock("pack_device");
  Claim claim;                       // of the device memory this call may take, until it returns
  GkBlocks blocks(ctx);
  gk_mate* d_out = nullptr;         // the records of the list on the device, once the kernel has run
  // An error return while copies from or into host memory may be queued drains the stream first.
  auto drained = [&](hipError_t e, const char* what) {
    (void)hipStreamSynchronize(st);
    gk_set_error("gk_bam_pack_device: %s: %s", what, hipGetErrorString(e));
    return GK_ERR_HIP;
  };
  const GkPlainDecoder decoder = [&](const GkBamRecords& r, const GkPairList& pairs, gk_mate* mates_out, uint8_t* verdict_out) -> int {
    const int64_t n = (int64_t)pairs.size() / 2;
    // what the route cannot take goes wholly through the host decode: 2^27 mates or more, a stream with its tables
    // beyond half the free device memory (GK_TEST_HOOKS=ingest_device_max_bytes=N: beyond N), a damaged record table
    if (2 * n >= (1ll << 27) || !gk_bam_records_inside(r)) return kGkDecoderDeclines;
    size_t free_bytes = 0, total_bytes = 0;
    GK_HIP(hipMemGetInfo(&free_bytes, &total_bytes));
    const long hook = gk_test_hook_value("ingest_device_max_bytes", -1);
    const size_t limit = hook >= 0 ? (size_t)hook : free_bytes / 2;
    if (!claim.take(device_bytes(r, n), limit)) return kGkDecoderDeclines;
    const size_t n_words = (r.data_bytes + 3) / 4;
    const int32_t n_ref = (int32_t)r.gene_of_ref.size();
    uint32_t* d_words = nullptr;
    GkBamRec* d_recs = nullptr;
    int64_t* d_pairs = nullptr;
    int32_t* d_gene = nullptr;
    uint8_t* d_verdict = nullptr;
    gk_mate* d_mates = nullptr;
    GK_HIP(blocks.take(&d_words, n_words * 4));
    GK_HIP(blocks.take(&d_recs, (size_t)r.n_recs * sizeof(GkBamRec)));
    GK_HIP(blocks.take(&d_pairs, (size_t)n * 2 * sizeof(int64_t)));
    GK_HIP(blocks.take(&d_gene, (size_t)n_ref * sizeof(int32_t)));
    GK_HIP(blocks.take(&d_verdict, (size_t)n));
    GK_HIP(blocks.take(&d_mates, (size_t)n * 2 * sizeof(gk_mate)));
    // the stream as a whole number of words, the tail of the last one zero
    hipError_t e = n_words ? hipMemsetAsync(d_words + (n_words - 1), 0, 4, st) : hipSuccess;
    if (e == hipSuccess && r.data_bytes) e = gk_send(ctx, d_words, r.data, r.data_bytes);
    if (e == hipSuccess && r.n_recs) e = gk_send(ctx, d_recs, r.recs, (size_t)r.n_recs * sizeof(GkBamRec));
    if (e == hipSuccess) e = gk_send(ctx, d_pairs, pairs.data(), (size_t)n * 2 * sizeof(int64_t));
    if (e == hipSuccess && n_ref) e = gk_send(ctx, d_gene, r.gene_of_ref.data(), (size_t)n_ref * sizeof(int32_t));
    if (e != hipSuccess) return drained(e, "sending the stream");
    if (clock.on) { (void)hipStreamSynchronize(st); clock.lap("upload"); }
    GK_PROF(ctx, "ingest_decode_pairs",
            GK_KERNEL(ingest_decode_pairs, dim3((unsigned)((2 * n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, d_words,
                      d_recs, r.n_recs, d_pairs, n, d_gene, n_ref, d_mates, d_verdict));
    e = hipGetLastError();
    if (e != hipSuccess) return drained(e, "launching ingest_decode_pairs");
    if (clock.on) { (void)hipStreamSynchronize(st); clock.lap("kernel"); }
    // the verdicts, and all records into the packer's array (the pinned one of gk_packer_set_output when there is one)
    e = hipMemcpyAsync(verdict_out, d_verdict, (size_t)n, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(mates_out, d_mates, (size_t)n * 2 * sizeof(gk_mate), hipMemcpyDeviceToHost, st);
    if (e != hipSuccess) return drained(e, "fetching the records");
    e = hipStreamSynchronize(st);
    if (e != hipSuccess) return drained(e, "ingest_decode_pairs");
    clock.lap("fetch");
    d_out = d_mates;
    return GK_OK;
  };
  GkSplit split;
  const int rc = gk_bam_pack_with(bam, pk, decoder, split);
  clock.lap("host subset");
  *n_device_pairs = split.n_plain;
  *n_host_pairs = split.n_pairs - split.n_plain;
  int32_t err_kind = 0;
  gk_packer_error(pk, &err_kind, nullptr);
  if (rc != GK_OK || err_kind || !d_mates_out) return rc;
  // The caller keeps the final records on the device: the pairs the packer decoded are patched in (their spilled
  // headers and string ids are final by now); a list the kernel never saw goes up whole.
  const int64_t n = split.n_pairs;
  std::vector<gk_mate, GkRawInit<gk_mate>> packed;   // outlives the copies queued from it: the wait below
  if (!d_out) {
    GK_HIP(blocks.take(&d_out, (size_t)n * 2 * sizeof(gk_mate)));
    if (n) {
      const hipError_t e = gk_send(ctx, d_out, split.mates, (size_t)n * 2 * sizeof(gk_mate));
      if (e != hipSuccess) return drained(e, "sending the records");
    }
  } else if (!split.host.empty()) {
    const int64_t n_host = (int64_t)split.host.size();
    packed.resize((size_t)(2 * n_host));
    for (int64_t j = 0; j < n_host; ++j) memcpy(&packed[(size_t)(2 * j)], split.mates + 2 * split.host[(size_t)j], 2 * sizeof(gk_mate));
    int64_t* d_which = nullptr;
    uint4* d_packed = nullptr;
    GK_HIP(blocks.take(&d_which, (size_t)n_host * sizeof(int64_t)));
    GK_HIP(blocks.take(&d_packed, (size_t)n_host * 2 * sizeof(gk_mate)));
    hipError_t e = gk_send(ctx, d_which, split.host.data(), (size_t)n_host * sizeof(int64_t));
    if (e == hipSuccess) e = gk_send(ctx, d_packed, packed.data(), (size_t)n_host * 2 * sizeof(gk_mate));
    if (e != hipSuccess) return drained(e, "sending the host-decoded records");
    GK_PROF(ctx, "ingest_patch_pairs",
            GK_KERNEL(ingest_patch_pairs, dim3((unsigned)((16 * n_host + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                      d_which, n_host, n, d_packed, reinterpret_cast<uint4*>(d_out)));
    e = hipGetLastError();
    if (e != hipSuccess) return drained(e, "launching ingest_patch_pairs");
  }
  const hipError_t e = hipStreamSynchronize(st);   // the records are read on other streams
  if (e != hipSuccess) return drained(e, "ingest_patch_pairs");
  clock.lap("patch");
  blocks.keep(d_out);                // the caller's from here (gk_free)
  *d_mates_out = gk_addr(d_out);
  return GK_OK;
}

}  // namespace

/* gk_bam_pack with the decode of the plain pairs on the device.  The packer afterwards holds what gk_bam_pack leaves of
 * the same file -- records, pair_lines, counts, strings, spill, error kind and line.  *n_device_pairs pairs were decoded
 * by ingest_decode_pairs, *n_host_pairs by the packer; a file the route cannot take (2^27 mates or more, stream and
 * tables beyond half the free device memory) is decoded wholly by the packer: *n_device_pairs == 0, same bytes.  With
 * d_mates_out (may be NULL) and no error in the packer: *d_mates_out is a block of the context's pool (gk_free) with
 * the final 2 x n_pairs records.  Ends synchronised.  A HIP error is returned as such: the host decode is no way round
 * it.  One context is used by one thread at a time. */
extern "C" int gk_bam_pack_device(gk_ctx* ctx, gk_bam* bam, gk_packer* pk, gk_dptr* d_mates_out, int64_t* n_device_pairs,
                                  int64_t* n_host_pairs) {
  return gk_guarded("gk_bam_pack_device", [&] { return pack_device(ctx, bam, pk, d_mates_out, n_device_pairs, n_host_pairs); });
}
