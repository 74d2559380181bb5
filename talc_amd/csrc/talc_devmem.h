// talc_devmem.h — who owns device and page-locked memory in the C ABI layer (host code; needs the HIP runtime, so it is
// included by talc_capi.hip only).  These are the only places of the library that allocate or free such memory: every
// buffer has one owner whose destructor gives it back, so a call that fails can return where it stands.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

namespace talc {

// the runtime's own start-up, as the call that does nothing else
inline hipError_t hip_runtime_start() { return hipFree(nullptr); }

// Test hook (talc_test_fail_alloc, include/talc_hip.h; docs/out_of_memory.md): allocations that fail on request.  While it is
// armed, the device requests (everything that goes through memcheck::alloc; a request a DevCache serves from its pool is
// none) and the page-locked ones (PinnedBuf::alloc, host_block_alloc) of the selected kinds are numbered from 0 in the order
// they are made, process-wide, and requests skip .. skip + count - 1 fail: with hipErrorOutOfMemory made here (real 0), or
// with whatever the runtime answers when it is asked for 2^60 bytes (real 1: its own error state is then that of a true
// failure).  It also keeps the number of device buffers the owners of this file hold.  Off, a request costs one relaxed load.
namespace failhook {

enum Kind : uint32_t { kDevice = 1, kPinned = 2 };
enum Owner : uint32_t { kDevBuf = 1, kDevCache = 2, kPinnedBuf = 3, kHostBlock = 4 };
constexpr uint64_t kHuge = 1ull << 60;

struct State {
  std::atomic<uint32_t> kinds{0};        // 0: off
  std::atomic<int64_t> skip{0};
  std::atomic<uint32_t> count{0}, real{0};
  std::atomic<uint64_t> seen[2];         // requests since the arming call: device, pinned
  std::atomic<uint64_t> next{0};         // ... of the selected kinds: the number of the next one
  std::atomic<uint64_t> injected{0}, lastOwner{0}, lastBytes{0}, lastRuntimeCode{0};
  std::atomic<int64_t> live{0};          // device buffers held (never reset)
  State() { seen[0] = 0; seen[1] = 0; }
};
inline State& state() { static State s; return s; }

inline void arm(uint32_t kinds, int64_t skip, uint32_t count, uint32_t real) {
  State& s = state();
  s.kinds.store(0);
  if (!kinds) return;   // (off: the numbers stay for the report)
  s.skip.store(skip); s.count.store(count); s.real.store(real);
  s.seen[0].store(0); s.seen[1].store(0); s.next.store(0);
  s.injected.store(0); s.lastOwner.store(0); s.lastBytes.store(0); s.lastRuntimeCode.store(0);
  s.kinds.store(kinds);
}
// Is this request to fail?  0: no.  1: yes, with hipErrorOutOfMemory made by the owner.  2: yes, by asking the runtime for kHuge.
inline int decide(Kind kind, Owner owner, uint64_t bytes) {
  State& s = state();
  const uint32_t kinds = s.kinds.load(std::memory_order_relaxed);
  if (!kinds) return 0;
  s.seen[kind == kDevice ? 0 : 1].fetch_add(1);
  if (!(kinds & kind)) return 0;
  const int64_t i = (int64_t)s.next.fetch_add(1), skip = s.skip.load();
  if (i < skip || i - skip >= (int64_t)s.count.load()) return 0;
  s.injected.fetch_add(1); s.lastOwner.store(owner); s.lastBytes.store(bytes);
  return s.real.load() ? 2 : 1;
}
// what the runtime answered to the request for kHuge bytes (a runtime that grants it: the memory goes back, out of memory it is)
inline hipError_t runtime_said(hipError_t e) {
  state().lastRuntimeCode.store((uint64_t)(uint32_t)e);
  return e == hipSuccess ? hipErrorOutOfMemory : e;
}
inline void born() { state().live.fetch_add(1, std::memory_order_relaxed); }
inline void gone() { state().live.fetch_sub(1, std::memory_order_relaxed); }

}  // namespace failhook

// The runtime's device allocation as every owner below sees it: the request hook first; a success counts one live buffer; a
// failure leaves no error behind in the runtime (the caller has the code: nothing is left for a later hipGetLastError()).
inline hipError_t device_malloc(void** out, uint64_t bytes, failhook::Owner owner) {
  hipError_t e;
  switch (failhook::decide(failhook::kDevice, owner, bytes)) {
    case 0: e = hipMalloc(out, bytes); break;
    case 1: e = hipErrorOutOfMemory; break;
    default: {
      e = hipMalloc(out, failhook::kHuge);
      if (e == hipSuccess) (void)hipFree(*out);
      e = failhook::runtime_said(e);
    }
  }
  if (e == hipSuccess) failhook::born();
  else { *out = nullptr; (void)hipGetLastError(); }
  return e;
}
inline void device_free(void* p) { failhook::gone(); (void)hipFree(p); }
// ... and its page-locked allocation
inline hipError_t pinned_malloc(void** out, uint64_t bytes, failhook::Owner owner) {
  hipError_t e;
  switch (failhook::decide(failhook::kPinned, owner, bytes)) {
    case 0: e = hipHostMalloc(out, bytes, hipHostMallocDefault); break;
    case 1: e = hipErrorOutOfMemory; break;
    default: {
      e = hipHostMalloc(out, failhook::kHuge, hipHostMallocDefault);
      if (e == hipSuccess) (void)hipHostFree(*out);
      e = failhook::runtime_said(e);
    }
  }
  if (e != hipSuccess) { *out = nullptr; (void)hipGetLastError(); }
  return e;
}

// Test hook (talc_test_set_poison, include/talc_hip.h): poisoned allocations and red zones.  While the setting is on, every
// buffer the two owners below hand out is filled with `byte` over its whole capacity (a pooled buffer's slack included)
// before its pointer is returned, and sits between two red zones of `guard` bytes of ~byte that are read back and compared
// when the buffer is given back.  A buffer remembers the guard and the fill it was made with, so one made under one setting
// can be released under another.  With the setting off an allocation costs one relaxed load more than without the hook.
// What this cannot see: a read past a red zone, and a stray write that lands inside the same buffer (one wave's scratch
// slot spilling into its neighbour's).
namespace memcheck {

struct Setting { bool on; uint8_t byte; uint32_t guard; };
inline std::atomic<uint64_t>& setting_word() { static std::atomic<uint64_t> w{0}; return w; }   // 0: off; 1 << 40 | byte << 32 | guard
inline Setting setting() {
  const uint64_t w = setting_word().load(std::memory_order_relaxed);
  return Setting{w != 0, (uint8_t)(w >> 32), (uint32_t)w};
}
inline void set(int byte, uint32_t guard) { setting_word().store(byte < 0 ? 0 : (1ull << 40 | (uint64_t)(byte & 0xFF) << 32 | guard)); }

// what the checks have seen: process-wide, or the self test's own while it runs (tally_override)
struct Tally {
  uint64_t checked = 0, violations = 0;
  uint64_t firstBytes = 0, firstWhere = 0;   // the first offender: bytes asked for; side << 32 | offset of the first changed byte (side 0: before the buffer, 1: behind it)
  uint64_t reused = 0;                       // DevCache::alloc calls served from the pool
};
inline std::mutex& lock() { static std::mutex m; return m; }
inline Tally& global_tally() { static Tally t; return t; }
inline Tally*& tally_override() { static thread_local Tally* t = nullptr; return t; }
inline void count_reuse() {
  std::lock_guard<std::mutex> g(lock());
  ++(tally_override() ? *tally_override() : global_tally()).reused;
}

// one guarded buffer: the caller's pointer is base + guard
struct Guard { uint32_t guard = 0; uint8_t fill = 0; uint64_t asked = 0; };

// `bytes` of device memory, poisoned and between red zones when the setting is on (g says what was made)
inline hipError_t alloc(void** out, uint64_t bytes, Guard& g, failhook::Owner owner) {
  const Setting s = setting();
  g = Guard();
  if (!s.on) return device_malloc(out, bytes, owner);
  char* base = nullptr;
  hipError_t e = device_malloc((void**)&base, bytes + 2ull * s.guard, owner);
  if (e != hipSuccess) return e;
  g.guard = s.guard; g.fill = (uint8_t)~s.byte; g.asked = bytes;
  if (s.guard) {
    if (e == hipSuccess) e = hipMemset(base, g.fill, s.guard);
    if (e == hipSuccess) e = hipMemset(base + s.guard + bytes, g.fill, s.guard);
  }
  if (e == hipSuccess) e = hipMemset(base + s.guard, s.byte, bytes);
  if (e == hipSuccess) e = hipDeviceSynchronize();   // (the null stream is not ordered with the contexts' non-blocking streams)
  if (e != hipSuccess) { device_free(base); (void)hipGetLastError(); return e; }
  *out = base + s.guard;
  return hipSuccess;
}
// a buffer that is handed out again (DevCache's pool): poisoned over its whole capacity when the setting is on
inline hipError_t repoison(void* p, uint64_t capacity) {
  const Setting s = setting();
  if (!s.on) return hipSuccess;
  hipError_t e = hipMemset(p, s.byte, capacity);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  return e;
}
// both red zones of a buffer of `capacity` bytes against their fill; a mismatch is counted, the first one kept
inline void check(const void* p, uint64_t capacity, const Guard& g) {
  if (!g.guard) return;
  std::vector<uint8_t> h(2ull * g.guard);
  const char* base = (const char*)p - g.guard;
  bool read = hipDeviceSynchronize() == hipSuccess && hipMemcpy(h.data(), base, g.guard, hipMemcpyDeviceToHost) == hipSuccess &&
              hipMemcpy(h.data() + g.guard, (const char*)p + capacity, g.guard, hipMemcpyDeviceToHost) == hipSuccess;
  if (!read) (void)hipGetLastError();
  std::lock_guard<std::mutex> lk(lock());
  Tally& t = tally_override() ? *tally_override() : global_tally();
  ++t.checked;
  for (uint64_t side = 0; side < 2; ++side)
    for (uint32_t i = 0; i < g.guard; ++i)
      if (!read || h[side * g.guard + i] != g.fill) {
        if (!t.violations) { t.firstBytes = g.asked; t.firstWhere = side << 32 | i; }
        ++t.violations;
        break;
      }
}
inline void free_checked(void* p, uint64_t capacity, const Guard& g) {
  check(p, capacity, g);
  device_free((char*)p - g.guard);
}

// the guarded buffers that DevBuf owns, by the caller's pointer (DevBuf::release() hands a pointer to another DevBuf: the
// record stays with the pointer); n_registered spares the lock while nothing is guarded
struct Registered { uint64_t bytes; Guard g; };
inline std::map<void*, Registered>& registry() { static std::map<void*, Registered> r; return r; }
inline std::atomic<uint64_t>& n_registered() { static std::atomic<uint64_t> n{0}; return n; }
inline hipError_t alloc_registered(void** out, uint64_t bytes) {
  Guard g;
  const hipError_t e = alloc(out, bytes, g, failhook::kDevBuf);
  if (e == hipSuccess && g.guard) {
    std::lock_guard<std::mutex> lk(lock());
    registry()[*out] = Registered{bytes, g};
    n_registered().fetch_add(1);
  }
  return e;
}
inline void free_registered(void* p) {
  if (n_registered().load(std::memory_order_relaxed)) {
    Registered r{0, Guard()};
    {
      std::lock_guard<std::mutex> lk(lock());
      auto it = registry().find(p);
      if (it != registry().end()) { r = it->second; registry().erase(it); n_registered().fetch_sub(1); }
    }
    if (r.g.guard) { free_checked(p, r.bytes, r.g); return; }
  }
  device_free(p);
}

}  // namespace memcheck

// n elements of hipMalloc memory; move-only.  Which device is current is the caller's business, as with the runtime itself.
template <typename T>
class DevBuf {
  T* p_ = nullptr;
  uint64_t n_ = 0;   // the elements it was allocated with; 0 while empty

 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept { *this = std::move(o); }
  DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { reset(); n_ = o.n_; p_ = o.release(); } return *this; }
  ~DevBuf() { reset(); }
  // (what was held goes first: the old and the new buffer never exist side by side)
  [[nodiscard]] hipError_t alloc(uint64_t n) {
    reset();
    const hipError_t e = memcheck::alloc_registered((void**)&p_, n * sizeof(T));
    if (e != hipSuccess) p_ = nullptr; else n_ = n;
    return e;
  }
  T* get() const { return p_; }
  uint64_t size() const { return n_; }
  explicit operator bool() const { return p_ != nullptr; }
  void reset() { if (p_) { memcheck::free_registered(p_); p_ = nullptr; n_ = 0; } }   // free now
  T* release() { T* p = p_; p_ = nullptr; n_ = 0; return p; }    // hand over to a longer-lived owner
};

// the same for page-locked host memory, in bytes; also takes over a pointer that had left through the C ABI
class PinnedBuf {
  char* p_ = nullptr;
  uint64_t n_ = 0;   // the bytes it was allocated with; 0 while empty, and for a pointer that was taken over

 public:
  PinnedBuf() = default;
  explicit PinnedBuf(void* p) : p_((char*)p) {}
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  ~PinnedBuf() { reset(); }
  [[nodiscard]] hipError_t alloc(uint64_t bytes) {
    reset();
    const hipError_t e = pinned_malloc((void**)&p_, bytes, failhook::kPinnedBuf);
    if (e != hipSuccess) p_ = nullptr; else n_ = bytes;
    return e;
  }
  char* get() const { return p_; }
  uint64_t size() const { return n_; }
  void reset() { if (p_) { (void)hipHostFree(p_); p_ = nullptr; n_ = 0; } }
  char* release() { char* p = p_; p_ = nullptr; n_ = 0; return p; }
};

// Host arrays that device-to-host copies land in (a batch's states and offsets).  Page-locked, so that the copy is one DMA
// transfer the stream does not stage; where page-locked memory cannot be had the block is pageable and everything still
// works (as talc_cli_io.h's growable buffer does).  Page-locking is slow and a streaming run makes a batch per chunk of
// reads: a batch's blocks go back to its context's HostPool, the next batch takes them, the context frees them.
struct HostBlock { void* p = nullptr; uint64_t bytes = 0; bool pinned = false; };
inline HostBlock host_block_alloc(uint64_t bytes) {
  HostBlock b;
  bytes = std::max<uint64_t>(bytes, 64);
  if (pinned_malloc(&b.p, bytes, failhook::kHostBlock) == hipSuccess) { b.bytes = bytes; b.pinned = true; return b; }
  b.p = malloc(bytes);
  b.bytes = b.p ? bytes : 0;
  return b;
}
inline void host_block_free(HostBlock& b) {
  if (b.p) { if (b.pinned) (void)hipHostFree(b.p); else free(b.p); }
  b = HostBlock();
}
struct HostPool {
  std::vector<HostBlock> free_;   // oldest first
  HostPool() = default;
  HostPool(const HostPool&) = delete;
  HostPool& operator=(const HostPool&) = delete;
  ~HostPool() { for (auto& b : free_) host_block_free(b); }
  // the smallest kept block that holds `bytes` and is not more than twice as large, or a fresh one (p == nullptr: no memory)
  HostBlock take(uint64_t bytes) {
    int best = -1;
    for (int i = 0; i < (int)free_.size(); ++i)
      if (free_[i].bytes >= bytes && free_[i].bytes <= 2 * bytes + 4096 && (best < 0 || free_[i].bytes < free_[best].bytes)) best = i;
    if (best < 0) return host_block_alloc(bytes);
    const HostBlock b = free_[best];
    free_.erase(free_.begin() + best);
    return b;
  }
  void give(HostBlock b) {
    if (!b.p) return;
    free_.push_back(b);
    while (free_.size() > 16) { host_block_free(free_.front()); free_.erase(free_.begin()); }
  }
};
// n elements of a trivially copyable T in one HostBlock: the few operations of std::vector that the library uses.
// resize() keeps what the array held and leaves new elements as they are: every user fills them.
template <typename T>
class HostArr {
  HostBlock blk_;
  uint64_t n_ = 0;
  HostPool* pool_ = nullptr;

 public:
  HostArr() = default;
  HostArr(const HostArr&) = delete;
  HostArr& operator=(const HostArr&) = delete;
  ~HostArr() { drop(); }
  void use_pool(HostPool* pool) { pool_ = pool; }
  void drop() { if (pool_) pool_->give(blk_); else host_block_free(blk_); blk_ = HostBlock(); n_ = 0; }
  bool resize(uint64_t n) {   // false: no memory (the array is as it was)
    if (n * sizeof(T) > blk_.bytes) {
      HostBlock nb = pool_ ? pool_->take(n * sizeof(T)) : host_block_alloc(n * sizeof(T));
      if (!nb.p) return false;
      if (n_) memcpy(nb.p, blk_.p, n_ * sizeof(T));
      const uint64_t keep = n_;
      drop();
      blk_ = nb; n_ = keep;
    }
    n_ = n;
    return true;
  }
  bool pinned() const { return blk_.pinned; }
  T* data() { return (T*)blk_.p; }
  const T* data() const { return (const T*)blk_.p; }
  uint64_t size() const { return n_; }
  bool empty() const { return n_ == 0; }
  T& operator[](uint64_t i) { return data()[i]; }
  const T& operator[](uint64_t i) const { return data()[i]; }
  T* begin() { return data(); }
  T* end() { return data() + n_; }
  const T* begin() const { return data(); }
  const T* end() const { return data() + n_; }
};

// device buffers of finished batches, kept for the next batch of their context (a streaming run creates and destroys
// a batch per chunk of reads: ~20 hipMalloc / hipFree pairs each time otherwise)
struct DevCache {
  struct Buf { uint64_t bytes; void* p; memcheck::Guard g; };
  std::vector<Buf> pool;          // free
  std::map<void*, Buf> live;      // by pointer, handed out
  uint64_t pool_bytes = 0;        // bytes cached (free)
  uint64_t live_bytes = 0;        // bytes handed out
  uint64_t peak_live_bytes = 0;   // the largest footprint the batches of this context have had together

  DevCache() = default;
  DevCache(const DevCache&) = delete;
  DevCache& operator=(const DevCache&) = delete;
  // (what is still handed out goes too: batches that outlived their context lose their memory with it)
  ~DevCache() { trim(0); for (auto& e : live) memcheck::free_checked(e.first, e.second.bytes, e.second.g); }

  void drop_oldest() {
    pool_bytes -= pool.front().bytes;
    memcheck::free_checked(pool.front().p, pool.front().bytes, pool.front().g);
    pool.erase(pool.begin());
  }
  // drop cached buffers, oldest first, until the cache holds at most `keep_bytes`
  void trim(uint64_t keep_bytes) {
    while (!pool.empty() && pool_bytes > keep_bytes) drop_oldest();
  }
  void hand_out(void** out, const Buf& b) {
    *out = b.p;
    live[b.p] = b;
    live_bytes += b.bytes;
    peak_live_bytes = std::max(peak_live_bytes, live_bytes);
  }

  // a device buffer of at least `bytes` from the cache (smallest cached one that fits and is not more than twice as
  // large), or a fresh one.  (Test hook: only a cached buffer with the red zones of the current setting fits, and it is
  // poisoned again, slack included.)
  [[nodiscard]] hipError_t alloc(void** out, uint64_t bytes) {
    bytes = std::max<uint64_t>(bytes, 256);
    const memcheck::Setting ms = memcheck::setting();
    const uint32_t guard = ms.on ? ms.guard : 0;
    int best = -1;
    for (int i = 0; i < (int)pool.size(); ++i)
      if (pool[i].bytes >= bytes && pool[i].bytes <= 2 * bytes + 4096 && pool[i].g.guard == guard && (best < 0 || pool[i].bytes < pool[best].bytes)) best = i;
    if (best >= 0) {
      Buf b = pool[best];
      if (ms.on) {
        const hipError_t e = memcheck::repoison(b.p, b.bytes);
        if (e != hipSuccess) { *out = nullptr; return e; }
        b.g.asked = bytes;
        memcheck::count_reuse();
      }
      pool_bytes -= b.bytes;
      pool.erase(pool.begin() + best);
      hand_out(out, b);
      return hipSuccess;
    }
    memcheck::Guard g;
    if (memcheck::alloc(out, bytes, g, failhook::kDevCache) != hipSuccess) {
      // out of memory: drop the cache and try once more
      trim(0);
      const hipError_t e = memcheck::alloc(out, bytes, g, failhook::kDevCache);
      if (e != hipSuccess) { *out = nullptr; return e; }   // (nothing is handed out)
    }
    hand_out(out, Buf{bytes, *out, g});
    return hipSuccess;
  }

  void release(void* p) {
    if (!p) return;
    auto it = live.find(p);
    if (it == live.end()) { device_free(p); return; }
    const Buf b = it->second;
    live.erase(it);
    live_bytes -= b.bytes;
    memcheck::check(b.p, b.bytes, b.g);
    pool.push_back(b);
    pool_bytes += b.bytes;
    // a bounded cache, by count and by bytes: what one batch hands back is what the next one of the same shape asks for, so
    // cache + live buffers never need to exceed the largest footprint the batches of this context have had (everybody
    // else who sizes something from hipMemGetInfo — the search scratch, the retry stage, another context on the same GPU,
    // the walk-table decision of an upload — sees cached bytes as used)
    while (pool.size() > 64) drop_oldest();
    if (pool_bytes + live_bytes > peak_live_bytes)
      trim(peak_live_bytes > live_bytes ? peak_live_bytes - live_bytes : 0);
  }
};

// n elements from a DevCache; they go back to that cache, not to the runtime
template <typename T>
class CachedBuf {
  T* p_ = nullptr;
  uint64_t n_ = 0;   // the elements the buffer was asked for (the cache rounds up and may have served a larger one); 0 while empty
  DevCache* cache_ = nullptr;

 public:
  CachedBuf() = default;
  CachedBuf(const CachedBuf&) = delete;
  CachedBuf& operator=(const CachedBuf&) = delete;
  ~CachedBuf() { reset(); }
  // (what was held goes back first: the cache may serve the request from it; a failure leaves the buffer empty)
  [[nodiscard]] hipError_t alloc(DevCache& cache, uint64_t n) {
    reset();
    cache_ = &cache;
    const hipError_t e = cache.alloc((void**)&p_, n * sizeof(T));
    if (e == hipSuccess) n_ = n;
    return e;
  }
  // the buffer as it is when it was asked for at least n elements, else a new one of exactly max(n, 1)
  [[nodiscard]] hipError_t ensure(DevCache& cache, uint64_t n) { return p_ && n_ >= n ? hipSuccess : alloc(cache, std::max<uint64_t>(n, 1)); }
  T* get() const { return p_; }
  explicit operator bool() const { return p_ != nullptr; }
  void reset() { if (p_) { cache_->release(p_); p_ = nullptr; n_ = 0; } }
};

}  // namespace talc
