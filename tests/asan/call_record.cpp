// Test infrastructure: the ownership rules of a call record (csrc/gk_calls.h: GkCall) and of the owner of pool blocks that it
// holds (csrc/gk_blocks.h: GkBlocks) on the CPU, under AddressSanitizer.
// A stand-alone program: it supplies the pool, the two transfer directions and the result ring that the record uses --
// they count live blocks, cancels and waits, keep the list of pending deliveries, and make the k-th fallible call fail.
// gk_fetch_wait copies into EVERY pending destination, so a delivery left pointing into a dead record, or into a dead
// local of a blocking entry point that holds the record on its stack, is a sanitizer report.  Built by tests/test_call_record.py with `hipcc --cuda-host-only -Xarch_host -fsanitize=address,undefined`.
#include <cstdarg>
#include <cstdio>
#include <set>
#include <utility>

#include "gk_calls.h"

namespace {

constexpr size_t kDirect = 4096;             // the stand-in's gk_stage_direct(): small, so that both sides are cheap
struct Delivery { char* dst; size_t bytes; };
std::set<void*> g_live;                      // blocks out
std::vector<Delivery> g_pending;             // deliveries registered with the "context"
int g_cancels, g_waits, g_stream_waits, g_ring_slots, g_queued, g_calls, g_fail_at;
char g_device[kDirect * 4];                  // where "kernels" would write

bool fails() { return ++g_calls == g_fail_at; }
void reset(int fail_at) {
  g_cancels = g_waits = g_stream_waits = g_ring_slots = g_queued = g_calls = 0;
  g_fail_at = fail_at;
}

int g_failed;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } \
  } while (0)

}  // namespace

void gk_set_error(const char*, ...) {}
size_t gk_stage_direct() { return kDirect; }
hipError_t gk_pool_malloc(gk_ctx*, void** out, size_t bytes) {
  if (fails()) return hipErrorOutOfMemory;
  *out = new char[bytes ? bytes : 1];
  g_live.insert(*out);
  return hipSuccess;
}
void gk_pool_free(gk_ctx*, void* p) {
  if (!p) return;
  if (!g_live.erase(p)) { printf("FAILED: a block freed twice or never taken\n"); ++g_failed; return; }
  delete[] (char*)p;
}
hipError_t gk_send(gk_ctx*, void*, const void*, size_t) { return fails() ? hipErrorUnknown : hipSuccess; }
hipError_t gk_fetch_direct(gk_ctx*, void* dst, size_t bytes, void** dev) {
  *dev = nullptr;
  if (bytes > kDirect || fails()) return hipErrorInvalidValue;
  ++g_ring_slots;
  g_pending.push_back({(char*)dst, bytes});
  *dev = g_device;
  return hipSuccess;
}
hipError_t gk_fetch_queue(gk_ctx*, void* dst, const void*, size_t bytes) {
  ++g_queued;
  g_pending.push_back({(char*)dst, bytes});      // follows the runtime (gk_runtime.hip): registered before the copy is
  if (!fails()) return hipSuccess;               // queued, and taken out again when that fails -- a failed queue leaves
  g_pending.pop_back();                          // nothing behind
  return hipErrorUnknown;
}
hipError_t gk_fetch_wait(gk_ctx*) {
  ++g_waits;
  for (const Delivery& d : g_pending) memset(d.dst, 0x5A, d.bytes);
  g_pending.clear();
  return hipSuccess;
}
void gk_fetch_cancel(gk_ctx*) {
  ++g_cancels;
  g_pending.clear();
}
extern "C" hipError_t hipStreamSynchronize(hipStream_t) {
  ++g_stream_waits;
  return hipSuccess;
}

namespace {

gk_ctx* ctx() {
  static gk_ctx c;
  return &c;
}

// the shape of every enqueue of the library: take, send, take, result, take, "launch" (a fallible call), finish
int enqueue(GkCallOf<char>& call, size_t result_bytes, size_t send_bytes = 64, bool ring = true) {
  std::vector<char> par(send_bytes, 1);
  void *a = nullptr, *b = nullptr, *c = nullptr, *out = nullptr;
  call.begin(ctx());
  GK_HIP(call.take(&a, 100));
  GK_HIP(call.send(a, par.data(), par.size()));
  GK_HIP(call.take(&b, 200));
  GK_HIP(call.result(result_bytes, &out, ring));
  GK_HIP(call.take(&c, 300));
  GK_HIP(fails() ? hipErrorLaunchFailure : hipSuccess);
  GK_HIP(call.finish());
  return GK_OK;
}

bool delivered(const GkCallOf<char>& call) {
  for (char v : call.back)
    if (v != 0x5A) return false;
  return !call.back.empty();
}

// a failure at every step, the record left to go out of scope
void failures(size_t result_bytes, bool ring, int n_steps) {
  for (int k = 1; k <= n_steps; ++k) {
    reset(k);
    {
      GkCallOf<char> call;
      CHECK(enqueue(call, result_bytes, 64, ring) != GK_OK);
    }
    CHECK(g_live.empty());
    CHECK(g_pending.empty());
    CHECK(gk_fetch_wait(ctx()) == hipSuccess);     // a delivery into the dead record would be written here
  }
  reset(n_steps + 1);                              // one step more: nothing fails
  GkCallOf<char> call;
  CHECK(enqueue(call, result_bytes, 64, ring) == GK_OK);
  CHECK(g_calls == n_steps);
}

void good_path(size_t result_bytes) {
  reset(0);
  GkCallOf<char> call;
  for (int round = 0; round < 2; ++round) {        // enqueue, collect, enqueue, collect on one record
    CHECK(gk_call_wait(ctx(), call, enqueue(call, result_bytes), "test") == GK_OK);
    CHECK(delivered(call));
    call.done();
    CHECK(g_live.empty() && g_pending.empty());
  }
  CHECK(g_cancels == 0 && g_waits == 2 && g_stream_waits == 0);
  // the same on a record that was moved while its result was on the way
  CHECK(enqueue(call, result_bytes) == GK_OK);
  GkCallOf<char> moved(std::move(call));
  CHECK(gk_fetch_wait(ctx()) == hipSuccess);
  CHECK(delivered(moved) && call.back.empty());
  moved.done();
  CHECK(enqueue(moved, result_bytes) == GK_OK);
  call = std::move(moved);
  CHECK(gk_fetch_wait(ctx()) == hipSuccess);
  CHECK(delivered(call));
  call.done();
  CHECK(g_live.empty() && g_pending.empty() && g_cancels == 0);
  // given up after the wait without a collect (a table that is written again): no cancel either
  CHECK(gk_call_wait(ctx(), call, enqueue(call, result_bytes), "test") == GK_OK);
  call.done();
  call.drop();
  call.drop();
  CHECK(g_live.empty() && g_cancels == 0);
  // a blocking call whose enqueue failed drops at once
  reset(6);
  CHECK(gk_call_wait(ctx(), call, enqueue(call, result_bytes), "test") != GK_OK);
  CHECK(g_live.empty() && g_pending.empty() && g_waits == 0);
}

void large_result() {
  reset(0);
  GkCallOf<char> call;
  CHECK(enqueue(call, kDirect + 8) == GK_OK);
  CHECK(g_ring_slots == 0 && g_queued == 1 && g_live.size() == 4);     // three temporaries + the result's block
  CHECK(gk_fetch_wait(ctx()) == hipSuccess);
  CHECK(delivered(call) && call.back.size() == kDirect + 8);
  call.done();
  CHECK(g_live.empty() && g_cancels == 0);
  reset(0);
  CHECK(enqueue(call, kDirect) == GK_OK);                              // the ring side of the limit
  CHECK(g_ring_slots == 1 && g_queued == 0 && g_live.size() == 3);
  CHECK(gk_fetch_wait(ctx()) == hipSuccess);
  call.done();
  // state that kernels update in device memory: a block and a queued copy whatever the size
  reset(0);
  CHECK(enqueue(call, 64, 64, false) == GK_OK);
  CHECK(g_ring_slots == 0 && g_queued == 1);
  // ... given up with the copy on the way: one cancel, nothing left
  call.drop();
  CHECK(g_cancels == 1 && g_live.empty() && g_pending.empty());
}

void large_send() {
  reset(0);
  GkCallOf<char> call;
  CHECK(enqueue(call, 64, kDirect) == GK_OK);
  CHECK(g_stream_waits == 0);
  call.drop();
  reset(0);
  CHECK(enqueue(call, 64, kDirect + 1) == GK_OK);
  CHECK(g_stream_waits == 1);                                          // before send returned: the source may go away
  call.drop();
  CHECK(g_live.empty() && g_pending.empty());
}

void kept_block() {
  reset(0);
  void* p = nullptr;
  {
    GkCall call;
    call.begin(ctx());
    CHECK(call.take(&p, 10) == hipSuccess);
    call.keep(p);
  }
  CHECK(g_live.size() == 1);
  gk_pool_free(ctx(), p);
}

// ---- the shape of a blocking entry point: the record on its stack, deliveries into two arrays of the caller and into a
// local declared BEFORE the record (the lifetime rule at GkCall::fetch).  take, send, take, "launch", fetch, fetch, an
// early return between two fetches (a result that has no room), fetch: kBlockingSteps fallible steps, then the wait
constexpr int kBlockingSteps = 8;
struct Caller { char a[40], b[24]; bool local_filled; };

bool filled(const char* p, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (p[i] != 0x5A) return false;
  return true;
}

int blocking(Caller& out) {
  const char par[64] = {1};
  std::vector<char> local(16, 0);
  GkCall call(ctx());
  void *x = nullptr, *y = nullptr;
  GK_HIP(call.take(&x, 100));
  GK_HIP(call.send(x, par, sizeof(par)));
  GK_HIP(call.take(&y, 200));
  GK_HIP(fails() ? hipErrorLaunchFailure : hipSuccess);
  GK_HIP(call.fetch(out.a, g_device, sizeof(out.a)));
  GK_HIP(call.fetch(local.data(), g_device, local.size()));
  if (fails()) return GK_ERR_CAPACITY;
  GK_HIP(call.fetch(out.b, g_device, sizeof(out.b)));
  GK_HIP(call.wait());
  out.local_filled = filled(local.data(), local.size());
  return GK_OK;
}

void blocking_entry_point() {
  for (int k = 1; k <= kBlockingSteps; ++k) {
    reset(k);
    Caller out = {};
    CHECK(blocking(out) != GK_OK);
    CHECK(g_calls == k);
    CHECK(g_live.empty());
    CHECK(g_pending.empty());
    CHECK(g_cancels == (g_queued ? 1 : 0));        // one cancel once a fetch was reached, none before
    CHECK(g_waits == 0);
    CHECK(gk_fetch_wait(ctx()) == hipSuccess);     // a delivery into the dead local would be written here
  }
  reset(0);
  Caller out = {};
  CHECK(blocking(out) == GK_OK);
  CHECK(g_calls == kBlockingSteps && g_queued == 3);
  CHECK(g_waits == 1 && g_cancels == 0 && g_stream_waits == 0);
  CHECK(filled(out.a, sizeof(out.a)) && filled(out.b, sizeof(out.b)) && out.local_filled);
  CHECK(g_live.empty() && g_pending.empty());
  // a queue that failed left nothing registered, before any cancel
  reset(1);
  CHECK(gk_fetch_queue(ctx(), out.a, g_device, sizeof(out.a)) != hipSuccess);
  CHECK(g_pending.empty() && g_cancels == 0);
  // a copy that the entry point queues itself: the record is told, and a drop drains the stream
  reset(0);
  {
    GkCall call(ctx());
    call.expect();
  }
  CHECK(g_cancels == 1);
  // ... while a record that has waited drops nothing
  {
    GkCall call(ctx());
    call.expect();
    CHECK(call.wait() == hipSuccess);
  }
  CHECK(g_cancels == 1 && g_waits == 1);
}

// ---- the bare owner (csrc/gk_blocks.h: GkBlocks), as a host function that takes scratch uses it
int five_takes(void** kept) {
  GkBlocks temps(ctx());
  char *a = nullptr, *c = nullptr;
  uint32_t *b = nullptr, *d = nullptr;
  double* e = nullptr;
  GK_HIP(temps.take(&a, 10));
  GK_HIP(temps.take(&b, 0));        // zero bytes is a block like any other
  GK_HIP(temps.take(&c, 30));
  GK_HIP(temps.take(&d, 40));
  GK_HIP(temps.take(&e, 50));
  if (kept) {
    temps.keep(c);
    *kept = c;
  }
  return GK_OK;
}

void owner_failures() {
  for (int k = 1; k <= 5; ++k) {     // the k-th take fails: the k - 1 before it go back on the way out
    reset(k);
    CHECK(five_takes(nullptr) != GK_OK);
    CHECK(g_calls == k);
    CHECK(g_live.empty());
  }
  reset(0);
  CHECK(five_takes(nullptr) == GK_OK);
  CHECK(g_calls == 5 && g_live.empty());
}

void owner_keep() {
  reset(0);
  void* kept = nullptr;
  CHECK(five_takes(&kept) == GK_OK);
  CHECK(g_live.size() == 1 && g_live.count(kept) == 1);      // exactly that block stays out
  gk_pool_free(ctx(), kept);                                 // its new owner gives it back: accepted
  CHECK(g_live.empty());
  GkBlocks temps(ctx());
  int other = 0;
  temps.keep(&other);                                        // not a block of the owner: nothing happens
}

void owner_moves() {
  reset(0);
  void *p = nullptr, *q = nullptr;
  {
    GkBlocks to;
    {
      GkBlocks from(ctx());
      CHECK(from.take(&p, 10) == hipSuccess);
      to = std::move(from);
    }                                                        // the moved-from owner frees nothing
    CHECK(g_live.size() == 1);
    GkBlocks built(std::move(to));
    CHECK(built.take(&q, 20) == hipSuccess);                 // the context came along
    CHECK(g_live.size() == 2);
  }                                                          // the moved-to owner frees once (twice is a FAILED of the pool)
  CHECK(g_live.empty());
  // a move onto an owner that holds blocks gives those back first
  GkBlocks a(ctx()), b(ctx());
  CHECK(a.take(&p, 10) == hipSuccess && b.take(&q, 20) == hipSuccess);
  a = std::move(b);
  CHECK(g_live.size() == 1 && g_live.count(q) == 1);
}

void owner_release_twice() {
  reset(0);
  void* p = nullptr;
  GkBlocks temps(ctx());
  CHECK(temps.take(&p, 10) == hipSuccess);
  temps.release();
  CHECK(g_live.empty());
  temps.release();                                           // a second free would be a FAILED of the pool
  CHECK(temps.take(&p, 10) == hipSuccess);                   // and the owner serves on
  CHECK(g_live.size() == 1);
  temps.begin(ctx());
  CHECK(g_live.empty());
}

}  // namespace

int main() {
  failures(64, true, 6);             // take, send, take, result (ring slot), take, launch
  failures(kDirect + 8, true, 7);    // take, send, take, result (block), take, launch, finish (copy)
  failures(64, false, 7);
  good_path(64);
  good_path(kDirect + 8);
  large_result();
  large_send();
  kept_block();
  blocking_entry_point();
  CHECK(g_live.empty());
  owner_failures();
  owner_keep();
  owner_moves();
  owner_release_twice();
  CHECK(g_live.empty());
  if (g_failed) return 1;
  printf("call record: ok\n");
  return 0;
}
