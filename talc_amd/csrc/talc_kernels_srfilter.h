// talc_kernels_srfilter.h — short-read clean-up ahead of the k-mer counter (docs/sr_filter.md): a 3' adapter clip and a
// quality floor, applied in place to the counter's staged batch before k_count_batch runs.  The count kernel's contract
// does the rest: any byte that is not one of ACGTacgt ends a window, so a masked byte ('N') removes exactly the windows
// that hold it.
//
// Contract, per record S of L bytes with optional qualities q[0 .. L):
//   adapter clip   for a start p in [0, L) and an adapter A of m letters: o = min(m, L - p), mm = the number of i < o with
//                  S[p + i] != A[i] after upper-casing (a byte of S outside ACGTacgt always differs).  p is accepted when
//                  o >= min_overlap and 100 mm <= max_error_pct o (integers).  clip = the smallest accepted p over all
//                  adapters, L when there is none.  No indels; the bases are matched as given, before the floor.
//   quality floor  j < clip is masked when q[j] < 33 + min_qual (min_qual 0 or no qualities: no floor).
//   masked copy    bytes [clip, L) and the quality-masked bytes become 'N'; every other byte, and the separator behind the
//                  record, stays as it is.
//   stats          [0] records, [1] records with clip < L, [2] sum of L - clip, [3] bytes below the floor among [0, clip);
//                  summed per wave, one add per wave and word.
//
//   k_sr_mask   one wave per record (grid-stride over the batch).  The record goes through LDS in tiles of kSrTile starts
//               as base codes (0-3, 4 for anything else); every lane takes the starts p, p + 64, ... of the tile and
//               compares eight codes at a time with each adapter: XOR of two 8-byte words, one bit per differing byte,
//               the bytes past the overlap masked off, popcount.  The tiles go front to back, so the first tile with an
//               accepted start holds the clip: the wave-minimum of the lanes' smallest accepted p.  Then the lanes write
//               'N' over [clip, L) and apply the floor to [0, clip).
#pragma once
#include "talc_common.h"
#include "talc_wave.h"

namespace talc {

static constexpr int kSrMaxAdapters = 4;
static constexpr int kSrMaxAdapterLen = 64;
static constexpr int kSrThreads = 256;                       // four records in flight per workgroup
static constexpr int kSrWaves = kSrThreads / 64;
static constexpr uint32_t kSrTile = 512;                     // candidate starts per tile
static constexpr uint32_t kSrTileBytes = kSrTile + kSrMaxAdapterLen + 8;   // codes staged per tile (whole 8-byte words behind the last start)
static constexpr uint32_t kSrMaxBlocks = 4096;

// the adapters as the kernel reads them (packed once by talc_counter_set_filter): base codes, zero-padded
struct SrAdapters {
  uint32_t n;
  uint32_t len[kSrMaxAdapters];
  uint32_t pad_[3];
  uint8_t code[kSrMaxAdapters][kSrMaxAdapterLen + 8];
};
static_assert(sizeof(SrAdapters) % 8 == 0, "the adapters are copied to LDS in 8-byte words");

struct SrFilter {
  uint32_t minQual;       // 0: no floor
  uint32_t minOverlap;
  uint32_t maxErrPct;
};

// one bit (0x80) per byte of x that is not zero
TALC_D unsigned long long sr_nonzero_bytes(unsigned long long x) {
  const unsigned long long low7 = 0x7F7F7F7F7F7F7F7Full;
  return (((x & low7) + low7) | x) & 0x8080808080808080ull;
}

// text: the batch as the count kernel reads it (record r at offsets[r] - offsets[0] + r, one separator behind each);
// quals: the same layout or nullptr; clipOut (test hook) and stats may be nullptr
__global__ void __launch_bounds__(kSrThreads)
k_sr_mask(uint8_t* __restrict__ text, const uint8_t* __restrict__ quals, const uint64_t* __restrict__ offsets, uint32_t nReads,
          const SrAdapters* __restrict__ adapters, SrFilter f, unsigned long long* __restrict__ stats, uint32_t* __restrict__ clipOut) {
  __shared__ __attribute__((aligned(8))) SrAdapters sA;
  __shared__ __attribute__((aligned(8))) uint8_t sCodes[kSrWaves][kSrTileBytes];
  const uint32_t nAd = adapters ? adapters->n : 0;
  if (nAd) {
    const unsigned long long* src = (const unsigned long long*)adapters;
    unsigned long long* dst = (unsigned long long*)&sA;
    for (uint32_t i = threadIdx.x; i < sizeof(SrAdapters) / 8; i += kSrThreads) dst[i] = src[i];
  }
  __syncthreads();   // (the only workgroup barrier: from here on every wave is on its own records and its own LDS row)
  const int l = lane_id();
  const uint32_t wave = (uint32_t)uni((int)(threadIdx.x >> 6));
  const uint8_t TALC_AS3* codes = (const uint8_t TALC_AS3*)sCodes[wave];
  uint8_t* codesW = sCodes[wave];
  const uint64_t o0 = offsets[0];
  const uint32_t qfloor = quals && f.minQual ? 33u + f.minQual : 0u;
  unsigned long long nRec = 0, nClipped = 0, nClipBytes = 0, nLow = 0;   // nLow per lane, the others wave-uniform
  for (uint32_t r = blockIdx.x * kSrWaves + wave; r < nReads; r += gridDim.x * kSrWaves) {
    const uint64_t at = offsets[r] - o0 + r;
    const uint32_t L = (uint32_t)(offsets[r + 1] - offsets[r]);   // (the host refuses a record of 2^32 bytes)
    uint32_t clip = L;
    if (nAd && L >= f.minOverlap) {
      const uint32_t lastStart = L - f.minOverlap;   // no start behind it has o >= min_overlap
      for (uint64_t t0 = 0; t0 <= lastStart; t0 += kSrTile) {
        const uint32_t staged = (uint32_t)(L - t0 < kSrTileBytes ? L - t0 : kSrTileBytes);
        LSYNC();   // (the previous tile's reads are done)
        // (four loads in flight per lane; what lies behind `staged` in the row is never inside an overlap: it is masked off)
        for (uint32_t j0 = 0; j0 < staged; j0 += 4 * 64) {
          uint8_t c[4];
#pragma unroll
          for (uint32_t u = 0; u < 4; ++u) { const uint32_t j = j0 + 64 * u + (uint32_t)l; c[u] = j < staged ? text[at + t0 + j] : (uint8_t)0; }
#pragma unroll
          for (uint32_t u = 0; u < 4; ++u) { const uint32_t j = j0 + 64 * u + (uint32_t)l; if (j < staged) codesW[j] = (uint8_t)ascii_to_code_select(c[u]); }
        }
        LSYNC();
        uint32_t best = 0xFFFFFFFFu;
        for (uint32_t s = (uint32_t)l; s < kSrTile && t0 + s <= lastStart; s += 64) {
          const uint32_t p = (uint32_t)t0 + s;
          const uint32_t room = L - p;
          bool ok = false;
          for (uint32_t a = 0; a < nAd && !ok; ++a) {
            const uint32_t m = sA.len[a];
            const uint32_t o = m < room ? m : room;
            if (o < f.minOverlap) continue;
            const uint8_t TALC_AS3* ad = (const uint8_t TALC_AS3*)sA.code[a];
            const uint32_t allowed = f.maxErrPct * o;   // 100 mm may reach it
            uint32_t mm = 0;
            for (uint32_t w = 0; w < o && 100u * mm <= allowed; w += 8) {   // (mm only grows: a start that has failed stops)
              const unsigned long long diff = sr_nonzero_bytes(lds_load_u64(codes + s + w) ^ lds_load_u64(ad + w));
              const uint32_t left = o - w;   // bytes of this word inside the overlap
              const unsigned long long in = left >= 8 ? ~0ull : (1ull << (8 * left)) - 1;
              mm += (uint32_t)__builtin_popcountll(diff & in);
            }
            ok |= 100u * mm <= allowed;
          }
          if (ok) { best = p; break; }   // (the lane's starts ascend: its first accepted one is its smallest)
        }
        const uint32_t found = (uint32_t)wave_min_i32((int)(best ^ 0x80000000u)) ^ 0x80000000u;
        if (found != 0xFFFFFFFFu) { clip = found; break; }
      }
    }
    // the masked copy
    for (uint64_t j0 = 0; j0 < L; j0 += 4 * 64) {   // (the qualities of four rounds asked for together)
      uint8_t q[4];
#pragma unroll
      for (uint32_t u = 0; u < 4; ++u) { const uint64_t j = j0 + 64 * u + (uint64_t)l; q[u] = qfloor && j < clip ? quals[at + j] : (uint8_t)255; }
#pragma unroll
      for (uint32_t u = 0; u < 4; ++u) {
        const uint64_t j = j0 + 64 * u + (uint64_t)l;
        if (j >= L) continue;
        if (j >= clip) text[at + j] = 'N';
        else if (q[u] < qfloor) { text[at + j] = 'N'; ++nLow; }
      }
    }
    if (clipOut && l == 0) clipOut[r] = clip;
    ++nRec;
    nClipped += clip < L ? 1 : 0;
    nClipBytes += L - clip;
  }
  if (stats) {
    nLow = wave_sum_u64(nLow);
    if (l == 0) {
      if (nRec) atomicAdd(&stats[0], nRec);
      if (nClipped) atomicAdd(&stats[1], nClipped);
      if (nClipBytes) atomicAdd(&stats[2], nClipBytes);
      if (nLow) atomicAdd(&stats[3], nLow);
    }
  }
}

}  // namespace talc
