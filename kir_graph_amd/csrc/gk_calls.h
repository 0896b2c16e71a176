// Device calls of a search step in two halves: `enqueue` queues the parameter copy, the kernels and the copy of the
// result on the context's stream and returns at once; `collect`, after ONE stream synchronisation that may cover the
// calls of many genes (gk_fetch_wait), unpacks the result and releases the temporaries.  The blocking entry points of
// the C ABI (gk_bound_step, gk_setsum, gk_fraction, gk_setsum_few) are enqueue + gk_call_wait + collect.
// A blocking entry point that delivers into its caller's arrays (the call reports, the bootstraps, the novel-variant
// step) holds a GkCall on its stack instead: take / send / fetch ... wait(), and every return before the wait is a plain
// return -- the record's drop gives the blocks back and cancels what was queued.  It frees and cancels nothing by hand.
#pragma once
#include <utility>
#include <vector>

#include "gk_blocks.h"

// What a call took from the context, owned: its pool blocks and the pending delivery of its result (GkCallOf<T>::back).
// An enqueue starts with begin(), takes everything through take / send / result and ends with finish(); `collect` ends
// with done().  A record that goes away (or is begun again) before that drops what it holds: an enqueue that fails
// half-way leaves no block out and no entry of ctx->fetches that points into the record.  Move-only; reused from call to
// call.  GkCall itself serves a call that only needs its blocks given back (gk_maxsum, gk_setmax).
// A drop of a PENDING record cancels EVERY queued delivery of the context (gk_fetch_cancel drains the stream and clears
// ctx->fetches), those of other records included: it belongs to error paths.  So a record that is still pending must not
// be begun again or move-assigned to while other calls of the context are in flight (a move FROM it is fine): end it with
// done() once it has been waited for (GeneSearch::discard), as `collect` does.
struct GkCall {
  GkCall() = default;
  explicit GkCall(gk_ctx* ctx) { begin(ctx); }
  GkCall(const GkCall&) = delete;
  GkCall& operator=(const GkCall&) = delete;
  GkCall(GkCall&& o) noexcept { *this = std::move(o); }
  GkCall& operator=(GkCall&& o) noexcept {
    if (this != &o) {
      drop();
      ctx_ = o.ctx_;
      dst_ = o.dst_;
      dst_bytes_ = o.dst_bytes_;
      blocks_ = std::move(o.blocks_);
      due_ = o.due_;
      pending_ = o.pending_;
      o.due_ = nullptr;
      o.pending_ = false;
    }
    return *this;
  }
  ~GkCall() { drop(); }

  void begin(gk_ctx* ctx) {
    drop();
    ctx_ = ctx;
    blocks_.begin(ctx);
  }
  // a pool block of the call
  template <typename T>
  hipError_t take(T** p, size_t bytes) { return blocks_.take(p, bytes); }
  // the block stays out when the call is over (it has another owner now)
  void keep(const void* p) { blocks_.keep(p); }
  // the owner itself, for a helper that takes its scratch through one (gk_compact_enqueue)
  GkBlocks& blocks() { return blocks_; }
  // host -> device; `src` may be reused at once (a transfer too large for the pinned ring goes straight from `src`, so
  // the stream is waited for)
  hipError_t send(void* dst_dev, const void* src, size_t bytes) {
    const hipError_t e = gk_send(ctx_, dst_dev, src, bytes);
    if (e != hipSuccess || bytes <= gk_stage_direct()) return e;
    return hipStreamSynchronize(ctx_->stream);
  }
  // after the last launch: the copy of a result that did not go into the ring
  hipError_t finish() {
    if (!due_) return hipSuccess;
    const void* src = due_;
    due_ = nullptr;
    pending_ = true;               // also when the copy fails: the delivery may be registered by then
    return gk_fetch_queue(ctx_, dst_, src, dst_bytes_);
  }
  // device -> host into memory the record does NOT own, delivered by wait().  THE lifetime rule of a destination: it is the
  // caller's memory, or an object declared BEFORE the record -- that one is destroyed after the record, whose drop has
  // cancelled the delivery by then.  Pending from here on, also when the queue fails (as in finish)
  hipError_t fetch(void* dst, const void* src_dev, size_t bytes) {
    pending_ = true;
    return gk_fetch_queue(ctx_, dst, src_dev, bytes);
  }
  // the entry point queued a copy itself that reads or writes memory under the rule above (a gk_send too large for the
  // ring, a strided copy into the caller's array): a drop drains the stream before that memory may go away
  void expect() { pending_ = true; }
  // the stream is drained and everything queued is delivered; not pending afterwards whatever the result (the context's
  // list is cleared either way).  The blocks stay until the record goes
  hipError_t wait() {
    pending_ = false;
    return gk_fetch_wait(ctx_);
  }
  // the stream has passed the call and its result is delivered (collect), or was never asked for: blocks back to the pool
  void done() {
    pending_ = false;
    due_ = nullptr;
    blocks_.release();
  }
  // the call is given up while its result may still be on the way: the stream is drained and the queued deliveries of
  // the context are dropped (gk_fetch_cancel) before the result's memory may go away.  Nothing to do for a record that
  // holds nothing
  void drop() {
    if (pending_) gk_fetch_cancel(ctx_);
    done();
  }

 protected:
  // `bytes` bytes that the kernels queued after this call store at *dev are delivered to `dst`.  `ring`: one kernel writes
  // them once -- then *dev is a slot of the pinned result ring (no copy) when they fit one; otherwise *dev is a pool block
  // and finish() queues its copy
  hipError_t result_into(void* dst, size_t bytes, void** dev, bool ring) {
    dst_ = dst;
    dst_bytes_ = bytes;
    if (ring && bytes <= gk_stage_direct()) {
      const hipError_t e = gk_fetch_direct(ctx_, dst, bytes, dev);
      if (e == hipSuccess) pending_ = true;
      return e;
    }
    const hipError_t e = take(dev, bytes);
    if (e == hipSuccess) due_ = *dev;
    return e;
  }

 private:
  gk_ctx* ctx_ = nullptr;
  GkBlocks blocks_;
  void* dst_ = nullptr;            // where the result is delivered (the owner's `back`)
  size_t dst_bytes_ = 0;
  const void* due_ = nullptr;      // pool block whose copy to dst_ finish() queues
  bool pending_ = false;           // a delivery to dst_ is registered with the context
};

// a call whose result comes back as elements of T
template <typename T>
struct GkCallOf : GkCall {
  std::vector<T> back;             // the result as fetched; a move takes the buffer along, so a pending delivery finds it
  hipError_t result(size_t bytes, void** dev, bool ring = true) {
    back.resize((bytes + sizeof(T) - 1) / sizeof(T));
    return result_into(back.data(), bytes, dev, ring);
  }
};

// The blocking form of a call: `rc` is what its enqueue returned; waits for the stream.  GK_OK: collect may run.
// Otherwise the record has dropped what it held.  `what` names the call in the message.
static inline int gk_call_wait(gk_ctx* ctx, GkCall& call, int rc, const char* what) {
  if (rc == GK_OK && gk_fetch_wait(ctx) != hipSuccess) {
    gk_set_error("%s: waiting for the stream failed", what);
    rc = GK_ERR_HIP;
  }
  if (rc != GK_OK) call.drop();
  return rc;
}

// GK_HIP with the message of an entry point: `what` ("call fit", "EM bootstrap: queueing the draws") comes first
#define GK_TRY(what, call)                                         \
  do {                                                             \
    const hipError_t e_ = (call);                                  \
    if (e_ != hipSuccess) {                                        \
      gk_set_error("%s: %s", what, hipGetErrorString(e_));         \
      return GK_ERR_HIP;                                           \
    }                                                              \
  } while (0)

// ---- gk_bound.hip: integer bound of a step (gk_bound_step)
struct GkBoundCall : GkCallOf<char> {      // back: [SelState | idx[cap] | m[cap]]
  int32_t cap = 0;
  size_t state_bytes = 0;
};
int gk_bound_enqueue(gk_ctx* ctx, gk_dptr d_miss8, int64_t ldm, int64_t n_rows, gk_dptr d_msum, const int32_t* ids,
                     int32_t n_sets, int32_t c_prev, const int32_t* cols, int32_t n_cols, const uint8_t* first,
                     int32_t top_n, int32_t cap, GkBoundCall& call);
// the same on the pseudo-rows of the table (gk_classrows.h) when `rec` is given: same totals, same cut, same selection
struct GkClassRows;
int gk_bound_enqueue_classes(gk_ctx* ctx, gk_dptr d_miss8, int64_t ldm, int64_t n_rows, gk_dptr d_msum, const int32_t* ids,
                             int32_t n_sets, int32_t c_prev, const int32_t* cols, int32_t n_cols, const uint8_t* first,
                             int32_t top_n, int32_t cap, const GkClassRows* rec, GkBoundCall& call);
// hdr_out[4] = candidates, cut, selected, 0; idx_out / m_out hold min(selected, cap) entries
void gk_bound_collect(gk_ctx* ctx, GkBoundCall& call, uint32_t* hdr_out, int32_t* idx_out, uint32_t* m_out);

// ---- gk_search.hip, gk_setsum_few.hip: exact float64 sums with numpy's tree
// A gene's table of log-likelihoods, column-major [allele][ld]: float64 values (vals == nullptr), or uint16 dense
// indices into the value table's array `vals` (the index form, gk_compat_index).
struct GkTable {
  gk_dptr d = 0;
  int64_t ld = 0;
  const double* vals = nullptr;
  bool indexed() const { return vals != nullptr; }
};
// The kernels that served a call; the values are the kinds of the launch log (gk_search::log, roofmodel.py)
enum GkSumForm : int32_t {
  kSumColumns = 0,                 // colsum_chunks + combine_chunks
  kSumTiles = 2,                   // fraction_chunks + combine_chunks: tiles of 32 sets stage their own columns
  kSumLeaves = 3,                  // setsum_leaves + fold_leaves: every column through LDS once
  kSumFew = 4,                     // setsum_few: a workgroup owns a chunk of one set (or column)
};
struct GkSumCall : GkCallOf<double> {      // back: per set c shares [+ value]; or one sum per column
  int64_t n_rows = 0;
  int32_t n_sets = 0, c = 0;
  bool with_value = false;
  GkSumForm form = kSumTiles;      // set by the enqueue, which picks it
};
// value + shares (value_out != nullptr at collect) or shares only of the given sets (gk_setsum / gk_fraction).  The form:
// few (at most 8 sets of 2 .. 4 alleles, float64 table, with the value), else leaves (a dense selection that fits their
// LDS and set ceilings), else tiles; GK_TEST_HOOKS=setsum=leaves|tiles asks for one of the latter two
int gk_shares_enqueue(gk_ctx* ctx, const GkTable& L, int64_t n_rows, const int32_t* ids, int32_t n_sets, int32_t c,
                      bool with_value, GkSumCall& call);
void gk_shares_collect(gk_ctx* ctx, GkSumCall& call, double* value_out, double* frac_out);
// column sums log_probs[:, cols].sum(axis=0) (gk_maxsum with no previous sets); few for at most 8 columns of a float64
// table (unless the hook above is set), else columns
int gk_colsum_enqueue(gk_ctx* ctx, const GkTable& L, int64_t n_rows, const int32_t* cols, int32_t n_cols,
                      GkSumCall& call);
void gk_colsum_collect(gk_ctx* ctx, GkSumCall& call, double* out);
// the few form whatever the route says (gk_setsum_few.hip): `ids` n_sets <= 4096 sets of c = 2 .. 4 alleles, unpacked by
// gk_shares_collect; c == 1: the sums of n_sets columns, unpacked by gk_colsum_collect
int gk_few_enqueue(gk_ctx* ctx, const GkTable& L, int64_t n_rows, const int32_t* ids, int32_t n_sets, int32_t c,
                   GkSumCall& call);
// the float64 form of an index table (for the exact (max,+) kernel): d_L double [n_allele][ld], queued on the stream
int gk_expand_table(gk_ctx* ctx, const GkTable& L, int64_t n_rows, int32_t n_allele, gk_dptr d_L, int64_t ld);
