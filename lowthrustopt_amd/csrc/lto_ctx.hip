// lto_ctx.hip -- the context: lifetime and its three kinds of owners, page-locked host blocks, last error, device arena and block
// cache, timing.
//
// No C++ exception crosses the ABI (everything in the host units is noexcept by construction: no STL that throws on the hot path,
// allocation failures are turned into LTO_EHIP).  No signal handlers, no global state besides what HIP itself keeps.  A context
// belongs to one device.
#include <chrono>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>

#include "lto_host.hpp"

int set_err(lto_ctx* c, int code, const char* what, hipError_t e) {
  if (c) {
    if (e != hipSuccess) std::snprintf(c->err, sizeof c->err, "%s: %s", what, hipGetErrorString(e));
    else std::snprintf(c->err, sizeof c->err, "%s", what);
  }
  return code;
}

int bind_device(lto_ctx* c) {
  LTO_HIP(c, hipSetDevice(c->device));
  return LTO_OK;
}

// ---- arena: laid out afresh by each host-pointer call, 256-B aligned
int arena_reserve(lto_ctx* c, size_t bytes) {
  if (bytes <= c->arena_bytes) return LTO_OK;
  if (c->arena) { LTO_HIP(c, hipStreamSynchronize(c->stream)); LTO_HIP(c, hipFree(c->arena)); c->arena = nullptr; c->arena_bytes = 0; }
  size_t want = bytes + bytes / 4 + (1u << 20);
  LTO_HIP(c, hipMalloc((void**)&c->arena, want));
  c->arena_bytes = want;
  return LTO_OK;
}

// ---- device block cache (see lto_ctx::pool)
hipError_t pool_alloc(lto_ctx* c, void** out, size_t bytes) {
  int best = -1;
  for (int i = 0; i < 8; ++i)
    if (c->pool[i].ptr && c->pool[i].bytes >= bytes && (best < 0 || c->pool[i].bytes < c->pool[best].bytes)) best = i;
  if (best >= 0 && c->pool[best].bytes <= 4 * bytes + 4096) {
    *out = c->pool[best].ptr;
    c->pool[best].ptr = nullptr;
    return hipSuccess;
  }
  return hipMalloc(out, bytes < 256 ? 256 : bytes);
}
void pool_free(lto_ctx* c, void* ptr, size_t bytes) {
  if (!ptr) return;
  if (bytes < 256) bytes = 256;
  int slot = -1;
  for (int i = 0; i < 8; ++i) if (!c->pool[i].ptr) { slot = i; break; }
  if (slot < 0) {  // evict the smallest cached block
    slot = 0;
    for (int i = 1; i < 8; ++i) if (c->pool[i].bytes < c->pool[slot].bytes) slot = i;
    (void)hipFree(c->pool[slot].ptr);
  }
  c->pool[slot].ptr = ptr;
  c->pool[slot].bytes = bytes;
}

void timing_begin(lto_ctx* c, hipStream_t st) {
  if (c->timing) { (void)hipEventRecord(c->ev0, st); }
}
void timing_end(lto_ctx* c, hipStream_t st) {
  if (c->timing) { (void)hipEventRecord(c->ev1, st); c->ev_valid = true; }
}

// End of a host-pointer call: poll the stream for up to ~1 ms before blocking in the runtime.  A 4 096-segment sweep is
// over in 0.2 ms, and the wake-up of a blocked hipStreamSynchronize is a visible part of that.
hipError_t stream_wait(hipStream_t st) {
  const auto give_up = std::chrono::steady_clock::now() + std::chrono::milliseconds(1);
  do {
    for (int k = 0; k < 16; ++k) {
      const hipError_t q = hipStreamQuery(st);
      if (q != hipErrorNotReady) return q;
    }
  } while (std::chrono::steady_clock::now() < give_up);
  return hipStreamSynchronize(st);
}

// page-locked blocks -> owning context (lto_host_free may come without the handle, from any thread)
static std::mutex g_blocks_mu;
struct HostBlock { void* ptr; lto_ctx* owner; };
static lto::HostList<HostBlock> g_blocks;          // a handful of entries: linear search
static lto_ctx* host_block_take(void* ptr) {       // under g_blocks_mu: the owner of `ptr`, the entry removed; nullptr if unknown
  for (size_t k = 0; k < g_blocks.size(); ++k)
    if (g_blocks[k].ptr == ptr) { lto_ctx* o = g_blocks[k].owner; g_blocks.erase_at(k); return o; }
  return nullptr;
}
static void host_block_forget(void* ptr) { std::lock_guard<std::mutex> lk(g_blocks_mu); (void)host_block_take(ptr); }
static bool ctx_has_blocks(lto_ctx* c) { std::lock_guard<std::mutex> lk(c->pinned_mu); return !c->pinned.empty(); }

// A context has three kinds of owners: its handle (until lto_destroy), its plans, its page-locked blocks; garbage collectors
// release them in any order and from any thread (lto_host_free takes no handle).  Who frees the context is decided under ONE
// lock, and exactly once (advisor finding, round 3: two threads could both see "last owner" and free it twice).
static std::mutex g_life_mu;
void ctx_plan_added(lto_ctx* c) { std::lock_guard<std::mutex> lk(g_life_mu); ++c->live_plans; }
static bool ctx_is_closing(lto_ctx* c) { std::lock_guard<std::mutex> lk(g_life_mu); return c->closing; }
// the caller has given up an owner of kind `what` (a block: already removed from c->pinned); true = the caller frees the context
bool ctx_release(lto_ctx* c, CtxOwner what) {
  std::lock_guard<std::mutex> lk(g_life_mu);
  if (what == OWNER_HANDLE) c->closing = true;
  if (what == OWNER_PLAN) --c->live_plans;
  if (!c->closing || c->live_plans > 0 || c->free_claimed || ctx_has_blocks(c)) return false;
  c->free_claimed = true;
  return true;
}

void ctx_free(lto_ctx* c) {
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();
  for (auto& h : c->host_plans) { if (h.plan) plan_free(h.plan); std::free(h.prm); h.plan = nullptr; h.prm = nullptr; }
  for (const lto_ctx::Pinned& b : c->pinned) { host_block_forget(b.host); (void)hipHostFree(b.host); }   // none left on the deferred path
  c->pinned.clear();
  if (c->arena) (void)hipFree(c->arena);
  for (int k = 0; k < 3; ++k) if (c->order_cache[k]) (void)hipFree(c->order_cache[k]);
  if (c->rep_host) (void)hipHostFree(c->rep_host);
  for (int i = 0; i < 8; ++i) if (c->pool[i].ptr) (void)hipFree(c->pool[i].ptr);
  (void)hipEventDestroy(c->ev0);
  (void)hipEventDestroy(c->ev1);
  (void)hipStreamDestroy(c->stream);
  delete c;
}

// Device view of a caller's buffer that lies wholly inside a block from lto_host_alloc; nullptr for any other memory.
double* pinned_view(lto_ctx* c, const double* host, size_t bytes) {
  const char* h = (const char*)host;
  std::lock_guard<std::mutex> lk(c->pinned_mu);
  for (const lto_ctx::Pinned& b : c->pinned) {
    if (b.dev && h >= b.host && bytes <= b.bytes && (size_t)(h - b.host) <= b.bytes - bytes) return (double*)(b.dev + (h - b.host));
  }
  return nullptr;
}

extern "C" {

int lto_version(void) { return LTO_VERSION; }

int lto_create(lto_ctx** out, int device_id) {
  if (!out) return LTO_ENULL;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return LTO_ENODEVICE;
  if (device_id < 0 || device_id >= n) return LTO_EINVAL;
  lto_ctx* c = new (std::nothrow) lto_ctx();   // value-initialised: every scalar member zero, the vector empty
  if (!c) return LTO_EHIP;
  c->device = device_id;
  c->cu_count = 0;
  std::memcpy(c->round_cost, kRoundCostDefault, sizeof kRoundCostDefault);
  c->lane_round_us = kLaneRoundUs;
  if (hipDeviceGetAttribute(&c->cu_count, hipDeviceAttributeMultiprocessorCount, device_id) != hipSuccess) { c->cu_count = 0; (void)hipGetLastError(); }
  if (hipSetDevice(device_id) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return LTO_EHIP;
  }
  if (hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess) {
    (void)hipStreamDestroy(c->stream);
    delete c;
    return LTO_EHIP;
  }
  *out = c;
  return LTO_OK;
}

void lto_destroy(lto_ctx* c) {
  if (!c) return;
  if (ctx_release(c, OWNER_HANDLE)) ctx_free(c);      // otherwise: freed by the last lto_*_plan_destroy / lto_host_free
}

const char* lto_last_error(const lto_ctx* c) { return c ? c->err : "null context"; }

void* lto_ctx_stream(lto_ctx* c) { return c ? (void*)c->stream : nullptr; }
int lto_ctx_device(const lto_ctx* c) { return c ? c->device : -1; }

int lto_set_timing(lto_ctx* c, int enabled) {
  if (!c) return LTO_ENULL;
  c->timing = enabled != 0;
  c->ev_valid = false;
  return LTO_OK;
}

double lto_last_kernel_ms(lto_ctx* c) {
  if (!c || !c->ev_valid) return -1.0;
  float ms = -1.0f;
  if (hipEventSynchronize(c->ev1) != hipSuccess) return -1.0;
  if (hipEventElapsedTime(&ms, c->ev0, c->ev1) != hipSuccess) return -1.0;
  return (double)ms;
}

double lto_last_call_ms(const lto_ctx* c) { return c ? c->last_call_ms : -1.0; }
int lto_last_call_order(const lto_ctx* c) { return c ? c->last_call_order : LTO_ENULL; }

int lto_host_alloc(lto_ctx* c, size_t bytes, void** out) {
  if (!c || !out) return LTO_ENULL;
  *out = nullptr;
  int rc = bind_device(c);
  if (rc) return rc;
  hipError_t e = hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault);
  if (e != hipSuccess) return set_err(c, LTO_EHIP, "hipHostMalloc", e);
  void* dev = nullptr;
  if (hipHostGetDevicePointer(&dev, *out, 0) != hipSuccess) { dev = nullptr; (void)hipGetLastError(); }   // still page-locked: the copy engine moves it
  bool listed;
  { std::lock_guard<std::mutex> lk(c->pinned_mu); listed = c->pinned.push({(char*)*out, (char*)dev, bytes ? bytes : 1}); }
  if (listed) {
    std::lock_guard<std::mutex> lk(g_blocks_mu);
    listed = g_blocks.push({*out, c});
  }
  if (!listed) {                                   // out of host memory for the bookkeeping: no block
    { std::lock_guard<std::mutex> lk(c->pinned_mu);
      for (size_t k = 0; k < c->pinned.size(); ++k) if (c->pinned[k].host == (char*)*out) { c->pinned.erase_at(k); break; } }
    (void)hipHostFree(*out);
    *out = nullptr;
    return set_err(c, LTO_ENOMEM, "lto_host_alloc: out of host memory");
  }
  return LTO_OK;
}

// ctx may be NULL (a finalizer that no longer has the handle): the owner is looked up.  Freeing the last block of a context
// whose lto_destroy was deferred completes that destroy.
int lto_host_free(lto_ctx* c, void* ptr) {
  if (!ptr) return LTO_OK;
  lto_ctx* owner = nullptr;
  {
    std::lock_guard<std::mutex> lk(g_blocks_mu);
    owner = host_block_take(ptr);
  }
  if (!owner) return c ? set_err(c, LTO_EINVAL, "lto_host_free: not a block from lto_host_alloc (or freed twice)") : LTO_EINVAL;
  // The entry is neutralised FIRST (no device alias, no size: pinned_view skips it), so that no host-pointer call on another thread
  // can be handed the device view of memory about to be freed; it stays in the list -- and keeps its context alive -- as a "dying"
  // entry while the device work drains and the block is freed, and only that dying entry is erased afterwards: a concurrent
  // lto_host_alloc that is given the same address again adds a LIVE entry with the same .host, which must survive (advisor
  // finding, round 4).
  {
    std::lock_guard<std::mutex> lk(owner->pinned_mu);
    for (auto& b : owner->pinned)
      if (b.host == (char*)ptr && b.dev) { b.dev = nullptr; b.bytes = 0; break; }
  }
  (void)hipSetDevice(owner->device);
  if (!ctx_is_closing(owner)) (void)hipStreamSynchronize(owner->stream);   // a sweep may still be writing the block in place
  else (void)hipDeviceSynchronize();
  const hipError_t e = hipHostFree(ptr);
  {
    std::lock_guard<std::mutex> lk(owner->pinned_mu);
    for (size_t k = 0; k < owner->pinned.size(); ++k)
      if (owner->pinned[k].host == (char*)ptr && !owner->pinned[k].dev) { owner->pinned.erase_at(k); break; }
  }
  if (ctx_release(owner, OWNER_BLOCK)) { ctx_free(owner); return e == hipSuccess ? LTO_OK : LTO_EHIP; }
  if (e != hipSuccess) return set_err(owner, LTO_EHIP, "hipHostFree", e);
  return LTO_OK;
}

}  // extern "C"
