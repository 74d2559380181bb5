// talc_kernels_spectrum.h — the count spectrum of the counted k-mers (replaces `jellyfish histo`, the third command of the
// reference README's short-read workflow; docs/kmer_spectrum.md).
//
// Contract: with bins = high + 2, over every count the slots hold,
//   hist[c], 1 <= c <= high   the counts equal to c
//   hist[high + 1]            the counts above high
//   hist[0]                   the used slots of the counter's hash with count 0 (none in practice: a slot is claimed together
//                             with an add of at least 1; the bin stays so that index equals count)
// and four totals behind the bins: distinct (the counts seen), unique (those equal to 1), total (their sum) and max_count.
// out[] is bins + 4 words of 64 bits, zeroed by the caller before the launch.
//
// One body, two kernels:
//   k_count_histo   over the counter's hash (talc_kernels_count.h): a used CountSlot holds one count
//   k_table_histo   over a table's RIGHT buckets (talc_common.h): a used bucket holds up to four, every non-zero cnt[b] is
//                   one stored k-mer
// Shape: the kernel streams its slots once (16 or 32 bytes each) and is bound by that.  In a raw short-read spectrum three
// quarters of the k-mers have count 1 and most of the rest 2 or 3: an LDS add per lane would put nearly every lane of a wave
// on one or two LDS words.  So
//   * a fixed grid (a small multiple of the CU count) walks the slots with a grid stride, a wave taking a few rows of 64
//     consecutive slots per step (kRows: 4 KiB per wave either way), all loaded before the first is looked at;
//   * the counts 1 .. kSpectrumLow are tallied without atomics: one ballot per low bin and count, its popcount added to an
//     accumulator that is uniform across the wave (the code is right for any kSpectrumLow >= 0, also one above `high`);
//   * every other count <= high goes to the workgroup's own histogram in LDS (bins words of 32 bits, dynamic) with an LDS add;
//   * the catch-all bin and the totals are ballots / per-lane sums reduced across the wave in registers;
//   * at the end the four waves add their register bins into the LDS histogram, and the workgroup flushes once: one 64-bit
//     global add per non-zero bin, one per total, one max.
// A 32-bit LDS bin (and a wave's register bin) cannot overflow while a workgroup sees fewer than 2^32 counts.  A workgroup
// takes S = kRows x 64 x 4 slots per trip (1024 hash slots, 512 buckets) and makes at most ceil(n / (S x gridDim.x)) trips,
// so it sees fewer than n / gridDim.x + S slots of kCounts counts each; the host launches min(ceil(n / S), 4 x CUs)
// workgroups.  On a device of 8 CUs or more (32 workgroups) that stays below 2^32 for every hash of up to 2^36 slots (1 TiB)
// and for every table (below 2^32 buckets of four counts: fewer than 2^29 + 2^11 counts per workgroup); with 256 CUs the
// hash may have 2^41 slots.
#pragma once
#include "talc_common.h"
#include "talc_kernels_count.h"   // CountSlot

namespace talc {

static constexpr int kSpectrumThreads = 256;
static constexpr int kSpectrumWaves = kSpectrumThreads / 64;
static constexpr int kSpectrumLow = 8;        // counts 1 .. kSpectrumLow are tallied in registers
static constexpr int kSpectrumGridPerCu = 4;  // workgroups per CU of the fixed grid
// the totals behind the bins of out[]
enum { SPECTRUM_DISTINCT = 0, SPECTRUM_UNIQUE = 1, SPECTRUM_TOTAL = 2, SPECTRUM_MAX = 3, SPECTRUM_TOTALS = 4 };
// LDS words of a launch: the bins, and not fewer than the words the waves' totals take when the histogram is done with
static constexpr uint32_t kSpectrumTotalWords = kSpectrumWaves * 5;   // per wave: distinct lo/hi, total lo/hi, max
TALC_HD uint32_t spectrum_lds_words(uint32_t bins) { return bins > kSpectrumTotalWords ? bins : kSpectrumTotalWords; }

// How a "slot" yields its 0 .. kCounts counts, and how many rows of 64 slots a wave loads per step.  load() is only
// called for i < n.
struct CounterSlots {   // the counter's hash
  const CountSlot* tab;
  static constexpr int kCounts = 1, kRows = 4;
  struct Raw { uint64_t key; uint32_t cnt[1]; };
  TALC_D Raw load(uint64_t i) const { Raw r; r.key = tab[i].key; r.cnt[0] = tab[i].count; return r; }
  static TALC_D bool holds(const Raw& r, int) { return r.key != kEmptyKey; }
};
struct TableSlots {     // a table's RIGHT buckets, staged or uploaded: the in-degree bits an upload writes into the top of a
  const Bucket* right;  // used key never make it the all-ones word (a key takes 60 bits), so empty is tested as the probers do
  static constexpr int kCounts = 4, kRows = 2;
  struct Raw { uint64_t key; uint32_t cnt[4]; };
  TALC_D Raw load(uint64_t i) const {
    Raw r;
    r.key = right[i].key;
#pragma unroll
    for (int b = 0; b < 4; ++b) r.cnt[b] = right[i].cnt[b];
    return r;
  }
  static TALC_D bool holds(const Raw& r, int b) { return r.key != kEmptyKey && r.cnt[b] != 0; }
};

// the slots a workgroup takes per trip of its grid-stride loop: what the host sizes the grid by
template <class Slots>
constexpr uint64_t spectrum_group_slots() { return (uint64_t)Slots::kRows * 64 * kSpectrumWaves; }

template <class Slots>
TALC_D void spectrum_body(const Slots& slots, uint64_t n, uint32_t high, unsigned long long* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s_hist[];
  const uint32_t bins = high + 2;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (uint32_t b = threadIdx.x; b < spectrum_lds_words(bins); b += kSpectrumThreads) s_hist[b] = 0;
  __syncthreads();

  uint32_t low[kSpectrumLow > 0 ? kSpectrumLow : 1];   // uniform across the wave: bin j + 1
#pragma unroll
  for (int j = 0; j < kSpectrumLow; ++j) low[j] = 0;
  uint32_t over = 0;                    // uniform: counts above high
  unsigned long long nUsed = 0;         // uniform: counts seen
  unsigned long long sum = 0;           // per lane
  uint32_t mx = 0;                      // per lane

  // (step0 and stride are uniform across the wave: every lane makes the same trips, so the ballots see all 64)
  const uint64_t step = (uint64_t)Slots::kRows * 64;
  const uint64_t stride = (uint64_t)gridDim.x * kSpectrumWaves * step;
  for (uint64_t s0 = ((uint64_t)blockIdx.x * kSpectrumWaves + wave) * step; s0 < n; s0 += stride) {
    typename Slots::Raw raw[Slots::kRows];
    bool in[Slots::kRows];
#pragma unroll
    for (int r = 0; r < Slots::kRows; ++r) {
      const uint64_t i = s0 + (uint64_t)r * 64 + lane;
      in[r] = i < n;
      if (in[r]) raw[r] = slots.load(i);
    }
#pragma unroll
    for (int r = 0; r < Slots::kRows; ++r) {
#pragma unroll
      for (int c = 0; c < Slots::kCounts; ++c) {
        const bool used = in[r] && Slots::holds(raw[r], c);
        const uint32_t cnt = used ? raw[r].cnt[c] : 0u;
        const bool binned = used && cnt <= high;
        nUsed += (unsigned long long)__popcll(__ballot(used));
        over += (uint32_t)__popcll(__ballot(used && cnt > high));
#pragma unroll
        for (int j = 0; j < kSpectrumLow; ++j) low[j] += (uint32_t)__popcll(__ballot(binned && cnt == (uint32_t)(j + 1)));
        if (binned && (cnt == 0 || cnt > (uint32_t)kSpectrumLow)) atomicAdd(&s_hist[cnt], 1u);
        sum += cnt;
        mx = cnt > mx ? cnt : mx;
      }
    }
  }

  // the waves' register bins into the LDS histogram (a register bin above `high` is zero: those counts went to `over`)
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < kSpectrumLow; ++j)
      if (low[j]) atomicAdd(&s_hist[j + 1], low[j]);
    if (over) atomicAdd(&s_hist[high + 1], over);
  }
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < bins; b += kSpectrumThreads) {
    const uint32_t v = s_hist[b];
    if (v) {
      atomicAdd(&out[b], (unsigned long long)v);
      if (b == 1) atomicAdd(&out[bins + SPECTRUM_UNIQUE], (unsigned long long)v);
    }
  }
  // the totals: reduced across the wave in registers, across the waves through the LDS words the histogram no longer needs
  for (int off = 32; off > 0; off >>= 1) {
    sum += (unsigned long long)__shfl_down((long long)sum, off, 64);
    const uint32_t o = (uint32_t)__shfl_down((int)mx, off, 64);
    mx = o > mx ? o : mx;
  }
  __syncthreads();   // (every bin has been read)
  if (lane == 0) {
    uint32_t* w = s_hist + wave * 5;
    w[0] = (uint32_t)nUsed; w[1] = (uint32_t)(nUsed >> 32);
    w[2] = (uint32_t)sum; w[3] = (uint32_t)(sum >> 32);
    w[4] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long d = 0, t = 0;
    uint32_t m = 0;
    for (int v = 0; v < kSpectrumWaves; ++v) {
      const uint32_t* w = s_hist + v * 5;
      d += (unsigned long long)w[0] | (unsigned long long)w[1] << 32;
      t += (unsigned long long)w[2] | (unsigned long long)w[3] << 32;
      m = w[4] > m ? w[4] : m;
    }
    if (d) atomicAdd(&out[bins + SPECTRUM_DISTINCT], d);
    if (t) atomicAdd(&out[bins + SPECTRUM_TOTAL], t);
    if (m) atomicMax(&out[bins + SPECTRUM_MAX], (unsigned long long)m);
  }
}

// dynamic LDS: spectrum_lds_words(high + 2) * 4 bytes; 2 <= high <= kSpectrumMaxHigh (talc_pure.h), checked by the host
__global__ void __launch_bounds__(kSpectrumThreads)
k_count_histo(const CountSlot* __restrict__ tab, uint64_t cap, uint32_t high, unsigned long long* __restrict__ out) {
  spectrum_body(CounterSlots{tab}, cap, high, out);
}
__global__ void __launch_bounds__(kSpectrumThreads)
k_table_histo(const Bucket* __restrict__ right, uint64_t cap, uint32_t high, unsigned long long* __restrict__ out) {
  spectrum_body(TableSlots{right}, cap, high, out);
}

}  // namespace talc
