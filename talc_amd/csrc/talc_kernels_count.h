// talc_kernels_count.h — short-read k-mer counting on the device (replaces `jellyfish count -m K` + `dump -c`, the first
// two steps of the reference README's pipeline; docs/kmer_counting.md).
//
// Contract: in every record every window of K consecutive bytes that are all one of ACGTacgt counts once; any other byte
// ends the window (N, IUPAC letters, '\r', the separator between records).  k-mers are directional and packed 2 bits per
// base, first base most significant (include/talc_hip.h).  A both-strands counter (docs/both_strands.md) keys every
// observation by canon(x) = min(x, rc(x)) instead, so that the hash holds the folded counts C(y) of the canonical k-mers.
//
// Layout: an open-addressed hash of 16-byte slots {u64 key, u32 count, u32 spare} with a power-of-two capacity, home
// slot = mix64(key) & (capacity - 1), linear probing.  kEmptyKey (~0) marks an empty slot: a real key takes 2 K <= 62
// bits.  A slot is claimed with a 64-bit CAS on its key and counted with a 32-bit add on its count.
//   k_count_init     every slot empty, every count 0
//   k_count_batch    one batch of raw bytes (records separated by one byte that is not a base): a workgroup stages its
//                    tile of bytes plus the K - 1 before it in LDS, each lane rolls a k-mer over kCountPerLane window ends
//                    and inserts runs of equal consecutive k-mers (homopolymers) with one add of the run's length; the
//                    new distinct k-mers and the windows are summed per wave and added once per wave; the canonical
//                    instance rolls the reverse complement alongside and keys every window by the smaller of the two
//   k_count_add_counts  counted k-mers (kmers[], counts[]) into the hash, one entry per lane: a count file's lines
//   k_count_rehash   the slots of a full table into a larger one (growth)
//   k_count_compact  the slots with count >= a threshold to (kmers[], counts[]), output positions one add per wave (per
//                    64 x 64 slots); with no output arrays it only counts them; the expanding instance writes (y, C)
//                    and, unless y is its own reverse complement, (rc(y), C): what the table of both strands stores
// Counts cannot pass the number of windows counted so far: while the host's running bound of those stays below 2^32 the
// adds need no return value; past it the checked form tests every add and raises *overflow instead of wrapping.  Counted
// k-mers (k_count_add_counts) bring counts of any size: they always take the checked add, and so does every batch after them.
#pragma once
#include "talc_common.h"
#include "talc_kernels_build.h"   // dev_revcomp

namespace talc {

struct __attribute__((aligned(16))) CountSlot {
  uint64_t key;     // packed k-mer, kEmptyKey if unused
  uint32_t count;
  uint32_t spare;
};
static_assert(sizeof(CountSlot) == 16, "count slot must be 16 bytes");

static constexpr int kCountThreads = 256;
static constexpr int kCountPerLane = 32;                                  // window ends per lane
static constexpr uint64_t kCountTile = (uint64_t)kCountThreads * kCountPerLane;   // window ends per workgroup

TALC_D uint64_t count_home(uint64_t key, uint64_t mask) { return mix64(key) & mask; }

__global__ void k_count_init(CountSlot* __restrict__ tab, uint64_t cap) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < cap) { tab[i].key = kEmptyKey; tab[i].count = 0; tab[i].spare = 0; }
}

// find or claim the slot of `key` and add n; returns 1 when this call claimed a new slot
template <bool kChecked>
TALC_D uint32_t count_insert(CountSlot* tab, uint64_t mask, uint64_t key, uint32_t n, uint32_t* overflow) {
  uint64_t i = count_home(key, mask);
  uint32_t fresh = 0;
  while (true) {
    unsigned long long* kp = (unsigned long long*)&tab[i].key;
    unsigned long long cur = __hip_atomic_load(kp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == kEmptyKey) {
      cur = atomicCAS(kp, (unsigned long long)kEmptyKey, (unsigned long long)key);
      if (cur == kEmptyKey) { cur = key; fresh = 1; }
    }
    if (cur == key) break;
    i = (i + 1) & mask;
  }
  if (kChecked) {
    const uint32_t old = atomicAdd(&tab[i].count, n);
    if (old > 0xFFFFFFFFu - n) atomicOr(overflow, 1u);
  } else {
    __hip_atomic_fetch_add(&tab[i].count, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  return fresh;
}

// stats[0] += windows counted, stats[1] += new distinct k-mers.  kCanon: the key of a window is min(km, rc), rc the reverse
// complement rolled from the other end: rc = (rc >> 2) | ((3 - c) << 2 (K - 1)); after K bases nothing older is left in it.
template <bool kChecked, bool kCanon>
__global__ void __launch_bounds__(kCountThreads)
k_count_batch(const uint8_t* __restrict__ text, uint64_t n, uint32_t K, CountSlot* tab, uint64_t mask,
              unsigned long long* __restrict__ stats, uint32_t* __restrict__ overflow) {
  __shared__ uint8_t s[kCountTile + 32];
  const uint64_t tile0 = (uint64_t)blockIdx.x * kCountTile;   // first window end of the workgroup
  const uint64_t lo = tile0 >= K - 1 ? tile0 - (K - 1) : 0;  // first byte staged
  const uint32_t pre = (uint32_t)(tile0 - lo);               // bytes staged ahead of the tile (< K)
  const uint64_t hi = tile0 + kCountTile < n ? tile0 + kCountTile : n;
  const uint32_t len = (uint32_t)(hi - lo);
  for (uint32_t j = threadIdx.x; j < len; j += kCountThreads) s[j] = text[lo + j];
  __syncthreads();
  const uint64_t kmask = (1ULL << (2 * K)) - 1;
  const uint32_t e0 = pre + threadIdx.x * kCountPerLane;     // this lane's first window end, as an LDS index
  const uint32_t e1 = e0 + kCountPerLane < len ? e0 + kCountPerLane : len;
  uint32_t nWin = 0, nNew = 0;
  if (e0 < len) {
    // roll over the K - 1 bytes before the first end (fewer at the start of the batch)
    const uint32_t b0 = e0 >= K - 1 ? e0 - (K - 1) : 0;
    uint64_t km = 0, rc = 0;
    const uint32_t top = 2 * (K - 1);
    uint32_t run = 0;   // consecutive bases ending at the current byte
    for (uint32_t j = b0; j < e0; ++j) {
      const uint8_t c = ascii_to_code(s[j]);
      if (c < 4) {
        km = ((km << 2) | c) & kmask; ++run;
        if (kCanon) rc = (rc >> 2) | ((uint64_t)(3u - c) << top);
      } else { run = 0; }
    }
    uint64_t pend = kEmptyKey;
    uint32_t pendN = 0;
    for (uint32_t j = e0; j < e1; ++j) {
      const uint8_t c = ascii_to_code(s[j]);
      if (c < 4) {
        km = ((km << 2) | c) & kmask; ++run;
        if (kCanon) rc = (rc >> 2) | ((uint64_t)(3u - c) << top);
      } else { run = 0; }
      if (run >= K) {
        ++nWin;
        if (kCanon) {   // (the two cases spelled out: the directional instance then compiles to the instructions it had before)
          const uint64_t key = km < rc ? km : rc;
          if (key == pend) { ++pendN; continue; }
          if (pendN) nNew += count_insert<kChecked>(tab, mask, pend, pendN, overflow);
          pend = key; pendN = 1;
        } else {
          if (km == pend) { ++pendN; continue; }
          if (pendN) nNew += count_insert<kChecked>(tab, mask, pend, pendN, overflow);
          pend = km; pendN = 1;
        }
      }
    }
    if (pendN) nNew += count_insert<kChecked>(tab, mask, pend, pendN, overflow);
  }
  // one add per wave for each sum
  unsigned long long w = nWin, f = nNew;
  for (int off = 32; off > 0; off >>= 1) {
    w += (unsigned long long)__shfl_down((long long)w, off, 64);
    f += (unsigned long long)__shfl_down((long long)f, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (w) atomicAdd(&stats[0], w);
    if (f) atomicAdd(&stats[1], f);
  }
}

// counted k-mers into the hash, one entry per lane: counts[i] to kmers[i], or to canon(kmers[i]) (kCanon).  An entry with
// count 0 adds nothing and claims no slot.  Always the checked add: a file's counts are arbitrary.  stats[0] += entries
// added, stats[1] += new distinct keys, one add per wave each.
template <bool kCanon>
__global__ void __launch_bounds__(kCountThreads)
k_count_add_counts(const uint64_t* __restrict__ kmers, const uint32_t* __restrict__ counts, uint64_t n, uint32_t K, CountSlot* tab,
                   uint64_t mask, unsigned long long* __restrict__ stats, uint32_t* __restrict__ overflow) {
  const uint64_t i = (uint64_t)blockIdx.x * kCountThreads + threadIdx.x;
  uint32_t nEnt = 0, nNew = 0;
  if (i < n) {
    const uint32_t cnt = counts[i];
    if (cnt) {
      uint64_t key = kmers[i];
      if (kCanon) { const uint64_t rc = dev_revcomp(key, K); key = rc < key ? rc : key; }
      nNew = count_insert<true>(tab, mask, key, cnt, overflow);
      nEnt = 1;
    }
  }
  unsigned long long w = nEnt, f = nNew;
  for (int off = 32; off > 0; off >>= 1) {
    w += (unsigned long long)__shfl_down((long long)w, off, 64);
    f += (unsigned long long)__shfl_down((long long)f, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (w) atomicAdd(&stats[0], w);
    if (f) atomicAdd(&stats[1], f);
  }
}

// every used slot of `src` into `dst` (keys are distinct: a claimed empty slot is this thread's alone)
__global__ void k_count_rehash(const CountSlot* __restrict__ src, uint64_t srcCap, CountSlot* dst, uint64_t dstMask) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= srcCap) return;
  const uint64_t key = src[i].key;
  if (key == kEmptyKey) return;
  uint64_t j = count_home(key, dstMask);
  while (atomicCAS((unsigned long long*)&dst[j].key, (unsigned long long)kEmptyKey, (unsigned long long)key) != kEmptyKey)
    j = (j + 1) & dstMask;
  dst[j].count = src[i].count;
}

// slots with count >= thr: a wave takes kCompactRows x 64 consecutive slots, counts its kept ones, takes their output
// positions with ONE add on *nOut and writes them on a second pass over the same (cached) slots.  (One add per 64 slots
// put 4 M adds on one address for a hash of 2^28 slots: 0.19 s per pass.)  outK == nullptr: count only.  Never writes at
// or beyond outCap.  kExpand (the slots hold canonical k-mers): a kept slot gives (y, C) and, unless y == rc(y), next to
// it (rc(y), C); the sizes of both passes come from the same two ballots, so the counting pass gives what the writing
// pass fills: 2 * kept - palindromes.
static constexpr int kCompactRows = 64;
template <bool kExpand>
__global__ void k_count_compact(const CountSlot* __restrict__ tab, uint64_t cap, uint32_t thr, uint32_t K, uint64_t* __restrict__ outK,
                                uint32_t* __restrict__ outC, uint64_t outCap, unsigned long long* __restrict__ nOut) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint64_t s0 = wave * kCompactRows * 64;
  if (s0 >= cap) return;
  uint32_t total = 0;
  for (int r = 0; r < kCompactRows; ++r) {
    const uint64_t i = s0 + (uint64_t)r * 64 + lane;
    const bool keep = i < cap && tab[i].key != kEmptyKey && tab[i].count >= thr;
    total += (uint32_t)__popcll(__ballot(keep));
    if (kExpand) {
      const bool twin = keep && dev_revcomp(tab[i].key, K) != tab[i].key;
      total += (uint32_t)__popcll(__ballot(twin));
    }
  }
  if (!total) return;
  unsigned long long base = 0;
  if (lane == 0) base = atomicAdd(nOut, (unsigned long long)total);
  base = (unsigned long long)__shfl((long long)base, 0, 64);
  if (!outK) return;
  for (int r = 0; r < kCompactRows; ++r) {
    const uint64_t i = s0 + (uint64_t)r * 64 + lane;
    uint64_t key = kEmptyKey;
    uint32_t cnt = 0;
    if (i < cap) { key = tab[i].key; cnt = tab[i].count; }
    const bool keep = key != kEmptyKey && cnt >= thr;
    const uint64_t ballot = __ballot(keep);
    const uint64_t below = (1ULL << lane) - 1;
    if (kExpand) {
      const uint64_t rc = dev_revcomp(key, K);
      const bool twin = keep && rc != key;
      const uint64_t twins = __ballot(twin);
      const uint64_t pos = base + (uint64_t)__popcll(ballot & below) + (uint64_t)__popcll(twins & below);
      if (keep && pos < outCap) { outK[pos] = key; outC[pos] = cnt; }
      if (twin && pos + 1 < outCap) { outK[pos + 1] = rc; outC[pos + 1] = cnt; }
      base += (uint64_t)__popcll(ballot) + (uint64_t)__popcll(twins);
    } else {
      const uint64_t pos = base + (uint64_t)__popcll(ballot & below);
      if (keep && pos < outCap) { outK[pos] = key; outC[pos] = cnt; }
      base += (uint64_t)__popcll(ballot);
    }
  }
}

}  // namespace talc
