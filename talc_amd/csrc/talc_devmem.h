// talc_devmem.h — who owns device and page-locked memory in the C ABI layer (host code; needs the HIP runtime, so it is
// included by talc_capi.hip only).  These are the only places of the library that allocate or free such memory: every
// buffer has one owner whose destructor gives it back, so a call that fails can return where it stands.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <map>
#include <utility>
#include <vector>

namespace talc {

// the runtime's own start-up, as the call that does nothing else
inline hipError_t hip_runtime_start() { return hipFree(nullptr); }

// n elements of hipMalloc memory; move-only.  Which device is current is the caller's business, as with the runtime itself.
template <typename T>
class DevBuf {
  T* p_ = nullptr;

 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(o.release()) {}
  DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { reset(); p_ = o.release(); } return *this; }
  ~DevBuf() { reset(); }
  // (what was held goes first: the old and the new buffer never exist side by side)
  hipError_t alloc(uint64_t n) {
    reset();
    const hipError_t e = hipMalloc((void**)&p_, n * sizeof(T));
    if (e != hipSuccess) p_ = nullptr;
    return e;
  }
  T* get() const { return p_; }
  explicit operator bool() const { return p_ != nullptr; }
  void reset() { if (p_) { (void)hipFree(p_); p_ = nullptr; } }   // free now
  T* release() { T* p = p_; p_ = nullptr; return p; }            // hand over to a longer-lived owner
};

// the same for page-locked host memory, in bytes; also takes over a pointer that had left through the C ABI
class PinnedBuf {
  char* p_ = nullptr;

 public:
  PinnedBuf() = default;
  explicit PinnedBuf(void* p) : p_((char*)p) {}
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  ~PinnedBuf() { reset(); }
  hipError_t alloc(uint64_t bytes) {
    reset();
    const hipError_t e = hipHostMalloc((void**)&p_, bytes, hipHostMallocDefault);
    if (e != hipSuccess) p_ = nullptr;
    return e;
  }
  char* get() const { return p_; }
  void reset() { if (p_) { (void)hipHostFree(p_); p_ = nullptr; } }
  char* release() { char* p = p_; p_ = nullptr; return p; }
};

// device buffers of finished batches, kept for the next batch of their context (a streaming run creates and destroys
// a batch per chunk of reads: ~20 hipMalloc / hipFree pairs each time otherwise)
struct DevCache {
  std::vector<std::pair<uint64_t, void*>> pool;   // (bytes, pointer), free
  std::map<void*, uint64_t> live;                 // pointer -> bytes, handed out
  uint64_t pool_bytes = 0;        // bytes cached (free)
  uint64_t live_bytes = 0;        // bytes handed out
  uint64_t peak_live_bytes = 0;   // the largest footprint the batches of this context have had together

  DevCache() = default;
  DevCache(const DevCache&) = delete;
  DevCache& operator=(const DevCache&) = delete;
  // (what is still handed out goes too: batches that outlived their context lose their memory with it)
  ~DevCache() { trim(0); for (auto& e : live) (void)hipFree(e.first); }

  // drop cached buffers, oldest first, until the cache holds at most `keep_bytes`
  void trim(uint64_t keep_bytes) {
    while (!pool.empty() && pool_bytes > keep_bytes) {
      pool_bytes -= pool.front().first;
      (void)hipFree(pool.front().second);
      pool.erase(pool.begin());
    }
  }

  // a device buffer of at least `bytes` from the cache (smallest cached one that fits and is not more than twice as
  // large), or a fresh one
  hipError_t alloc(void** out, uint64_t bytes) {
    bytes = std::max<uint64_t>(bytes, 256);
    int best = -1;
    for (int i = 0; i < (int)pool.size(); ++i)
      if (pool[i].first >= bytes && pool[i].first <= 2 * bytes + 4096 && (best < 0 || pool[i].first < pool[best].first)) best = i;
    if (best >= 0) {
      *out = pool[best].second;
      live[*out] = pool[best].first;
      live_bytes += pool[best].first;
      peak_live_bytes = std::max(peak_live_bytes, live_bytes);
      pool_bytes -= pool[best].first;
      pool.erase(pool.begin() + best);
      return hipSuccess;
    }
    if (hipMalloc(out, bytes) != hipSuccess) {
      // out of memory: drop the cache and try once more
      (void)hipGetLastError();
      trim(0);
      const hipError_t e = hipMalloc(out, bytes);
      if (e != hipSuccess) { *out = nullptr; return e; }   // (nothing is handed out)
    }
    live[*out] = bytes;
    live_bytes += bytes;
    peak_live_bytes = std::max(peak_live_bytes, live_bytes);
    return hipSuccess;
  }

  void release(void* p) {
    if (!p) return;
    auto it = live.find(p);
    if (it == live.end()) { (void)hipFree(p); return; }
    const uint64_t bytes = it->second;
    live.erase(it);
    live_bytes -= bytes;
    pool.push_back({bytes, p});
    pool_bytes += bytes;
    // a bounded cache, by count and by bytes: what one batch hands back is what the next one of the same shape asks for, so
    // cache + live buffers never need to exceed the largest footprint the batches of this context have had (everybody
    // else who sizes something from hipMemGetInfo — the search scratch, the retry stage, another context on the same GPU,
    // the walk-table decision of an upload — sees cached bytes as used)
    while (pool.size() > 64) {
      pool_bytes -= pool.front().first;
      (void)hipFree(pool.front().second);
      pool.erase(pool.begin());
    }
    if (pool_bytes + live_bytes > peak_live_bytes)
      trim(peak_live_bytes > live_bytes ? peak_live_bytes - live_bytes : 0);
  }
};

// n elements from a DevCache; they go back to that cache, not to the runtime
template <typename T>
class CachedBuf {
  T* p_ = nullptr;
  DevCache* cache_ = nullptr;

 public:
  CachedBuf() = default;
  CachedBuf(const CachedBuf&) = delete;
  CachedBuf& operator=(const CachedBuf&) = delete;
  ~CachedBuf() { reset(); }
  hipError_t alloc(DevCache& cache, uint64_t n) {
    reset();
    cache_ = &cache;
    return cache.alloc((void**)&p_, n * sizeof(T));
  }
  T* get() const { return p_; }
  explicit operator bool() const { return p_ != nullptr; }
  void reset() { if (p_) { cache_->release(p_); p_ = nullptr; } }
};

}  // namespace talc
