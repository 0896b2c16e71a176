// Who gives a pool block back.  THE rule of the library: a host function takes its device scratch through a GkBlocks on
// its stack (or in the record of its call, GkCall) and frees nothing by hand -- every way out of the function, GK_HIP and
// GK_REQUIRE included, gives the blocks back.  A block that outlives the function is taken straight into the field of the
// handle while a std::unique_ptr with the handle's destroy function holds that handle (gk_take_into: gk_tab, gk_index), so
// the destroy function gives it back; a block that joins a handle which exists already (a GenePartition) or goes to the
// caller of the C ABI (gk_mates_compact) is the owner's until the call has succeeded, and keep() hands it over then.
// Giving a block back while work that uses it is still queued is safe (stream-ordered reuse): every kernel and copy of a
// context runs on its one stream, so whoever gets the block next queues behind that work; a large block, which contexts
// share, goes back with an event recorded on the stream (gk_pool_free).
#pragma once
#include <utility>
#include <vector>

#include "gk_common.h"

struct GkBlocks {
  GkBlocks() = default;
  explicit GkBlocks(gk_ctx* ctx) : ctx_(ctx) {}
  GkBlocks(const GkBlocks&) = delete;
  GkBlocks& operator=(const GkBlocks&) = delete;
  GkBlocks(GkBlocks&& o) noexcept : ctx_(o.ctx_), blocks_(std::move(o.blocks_)) { o.blocks_.clear(); }
  GkBlocks& operator=(GkBlocks&& o) noexcept {
    if (this != &o) {
      release();
      ctx_ = o.ctx_;
      blocks_ = std::move(o.blocks_);
      o.blocks_.clear();
    }
    return *this;
  }
  ~GkBlocks() { release(); }

  // gives back what is held; takes from `ctx` from now on
  void begin(gk_ctx* ctx) {
    release();
    ctx_ = ctx;
  }
  gk_ctx* ctx() const { return ctx_; }
  // a pool block of `bytes` bytes (0 is fine: the pool's smallest class is 256 bytes), given back by release()
  template <typename T>
  hipError_t take(T** p, size_t bytes) {
    void* v = nullptr;
    const hipError_t e = gk_pool_malloc(ctx_, &v, bytes);
    if (e == hipSuccess) {
      blocks_.push_back(v);
      *p = static_cast<T*>(v);
    }
    return e;
  }
  // the block has another owner from now on (a handle, or the caller)
  void keep(const void* p) {
    for (size_t i = 0; i < blocks_.size(); ++i)
      if (blocks_[i] == p) { blocks_.erase(blocks_.begin() + (long)i); return; }
  }
  // a pool block of ctx() that another owner let go of (keep) is this one's from now on
  void adopt(void* p) { blocks_.push_back(p); }
  // everything back to the pool, now
  void release() {
    for (void* p : blocks_) gk_pool_free(ctx_, p);
    blocks_.clear();
  }

 private:
  gk_ctx* ctx_ = nullptr;
  std::vector<void*> blocks_;
};

// a block for a field of a handle: the handle's destroy function gives it back
template <typename T>
static inline hipError_t gk_take_into(gk_ctx* ctx, T** field, size_t bytes) {
  void* v = nullptr;
  const hipError_t e = gk_pool_malloc(ctx, &v, bytes);
  if (e == hipSuccess) *field = static_cast<T*>(v);
  return e;
}

// stable compaction (gk_scan.hip), queued: out[k] = values[i] (or i when values == nullptr) for the k-th i with
// flag[i] != 0; *d_total_out is the device word that receives the count.  The scratch is taken through `temps`
int gk_compact_enqueue(gk_ctx* ctx, const uint32_t* d_flag, const int32_t* d_values, int64_t n, int32_t* d_out,
                       uint32_t** d_total_out, GkBlocks& temps);
