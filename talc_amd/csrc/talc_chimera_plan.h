// talc_chimera_plan.h — the host's part of the chimera split (docs/chimeras.md): the records, how k_read_chimera deals a
// read's columns over the lanes of its wave, and the rule that turns the hits of a read into its kept pieces.  Host and
// device; no HIP type, so the CPU test-suite builds it too (pure_capi.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "talc_sellers.h"

namespace talc {

struct ChimeraHit {   // talc_chimera_hit
  uint32_t read, start, end;
  uint8_t adapter, strand, err, pad;
};
struct SplitPiece {   // talc_split_piece
  uint32_t read, start, len, ordinal;
};
TALC_HD GatherInterval gather_interval(const SplitPiece& pc, uint32_t) { return GatherInterval{pc.read, pc.start, pc.len}; }

// ------------------------------------------------------------------ how a wave is dealt over a read
// A wave has 64 lanes and the setting 2 .. 8 patterns (two per adapter): every pattern gets 64 / patterns lanes, each
// lane one chunk of columns, and the read is walked in tiles of chunks-per-pattern * chunk columns.  A chunk is the read's
// length dealt evenly, within [kChimeraChunkMin, kChimeraChunkMax], rounded up to 4 mod 8 bytes: the lanes of a pattern then
// read LDS at an odd stride in words, which spreads them over the banks.
constexpr uint32_t kChimeraMaxPatterns = 8;
constexpr uint32_t kChimeraChunkMin = 36, kChimeraChunkMax = 252;
constexpr uint32_t kChimeraMaxHalf = 32;                                          // w = ceil(m / 2), m <= 64
constexpr uint32_t kChimeraMaxPre = kChimeraMaxHalf + 64u + 19u;                  // w + m + k_a, k_a <= 0.3 * 64
constexpr uint32_t kChimeraStage = 32u * kChimeraChunkMax + kChimeraMaxPre + kChimeraMaxHalf + 13u;   // 8224 codes in LDS

struct ChimeraGeometry { uint32_t lanesPerPattern, chunk, tile; };
TALC_HD ChimeraGeometry chimera_geometry(uint32_t L, uint32_t nPatterns) {
  ChimeraGeometry g;
  g.lanesPerPattern = 64u / nPatterns;
  uint32_t chunk = (L + g.lanesPerPattern - 1u) / g.lanesPerPattern;
  chunk = chunk < kChimeraChunkMin ? kChimeraChunkMin : chunk > kChimeraChunkMax ? kChimeraChunkMax : chunk;
  g.chunk = chunk + ((4u - (chunk & 7u)) & 7u);   // the next 4 mod 8 (both bounds are 4 mod 8)
  g.tile = g.lanesPerPattern * g.chunk;
  return g;
}

// The setting as the kernel takes it, by value.  Pattern 2 a + s is adapter a on strand s (0: the adapter, 1: its reverse
// complement).  peq[p][c]: bit i set when letter i of pattern p has code c; peqRev: the same of the pattern back to front,
// for the search of a hit's start.
struct ChimeraParams {
  uint64_t peq[kChimeraMaxPatterns][4], peqRev[kChimeraMaxPatterns][4];
  uint32_t m[kChimeraMaxPatterns], k[kChimeraMaxPatterns];
  uint32_t nPatterns, pad_;
};
// both patterns of an adapter of m letters that pattern_fault has passed under set_of, k_a = floor(pct m / 100)
template <class Letter, class SetOf>
inline void chimera_params_add(ChimeraParams& P, const Letter* adapter, uint32_t m, SetOf set_of, uint32_t pct) {
  for (uint32_t s = 0; s < 2; ++s) {
    const uint32_t p = P.nPatterns++;
    for (uint32_t c = 0; c < 4; ++c) P.peq[p][c] = P.peqRev[p][c] = 0;
    pattern_masks(adapter, m, set_of, s == 1u, false, P.peq[p]);
    pattern_masks(adapter, m, set_of, s == 1u, true, P.peqRev[p]);
    P.m[p] = m;
    P.k[p] = pct * m / 100u;
  }
}

// the order of a batch's hits: (read, end, adapter, strand); whatever order the waves appended them in is gone after it
inline void chimera_sort(std::vector<ChimeraHit>& hits) {
  std::sort(hits.begin(), hits.end(), [](const ChimeraHit& a, const ChimeraHit& b) {
    if (a.read != b.read) return a.read < b.read;
    if (a.end != b.end) return a.end < b.end;
    if (a.adapter != b.adapter) return a.adapter < b.adapter;
    return a.strand < b.strand;
  });
}
// readHitOff[r]: the first hit of read r among sorted hits whose reads are all below n_reads
inline void chimera_read_offsets(const std::vector<ChimeraHit>& hits, uint32_t n_reads, std::vector<uint64_t>& readHitOff) {
  readHitOff.assign((size_t)n_reads + 1, 0);
  for (const ChimeraHit& h : hits) ++readHitOff[(size_t)h.read + 1];
  for (uint32_t r = 0; r < n_reads; ++r) readHitOff[r + 1] += readHitOff[r];
}

// ------------------------------------------------------------------ the piece rule
// The kept pieces of every read, reads in order, from the batch's hits in the order (read, end, adapter, strand) with
// readHitOff[r] the first hit of read r.  A read without a hit is one piece [0, L) with ordinal 0, whatever L.  Otherwise its
// pieces are the maximal non-empty intervals of [0, L) that no hit's [start, end) covers, in order; those shorter than
// minPiece are dropped (counted in *dropped, their bytes in *droppedBases) and the kept ones numbered from 1.
inline void split_pieces(const ChimeraHit* hits, const uint64_t* readHitOff, const uint64_t* offsets, uint32_t n_reads, uint32_t minPiece,
                         std::vector<SplitPiece>& pieces, std::vector<uint64_t>& readPieceOff, uint64_t* dropped, uint64_t* droppedBases) {
  pieces.clear();
  readPieceOff.assign((size_t)n_reads + 1, 0);
  uint64_t nDropped = 0, nDroppedBases = 0;
  std::vector<std::pair<uint32_t, uint32_t>> cover;
  for (uint32_t r = 0; r < n_reads; ++r) {
    readPieceOff[r] = pieces.size();
    const uint32_t L = (uint32_t)(offsets[r + 1] - offsets[r]);
    const uint64_t h0 = readHitOff[r], h1 = readHitOff[r + 1];
    if (h0 == h1) { pieces.push_back(SplitPiece{r, 0u, L, 0u}); continue; }
    cover.clear();
    for (uint64_t h = h0; h < h1; ++h) cover.emplace_back(std::min(hits[h].start, L), std::min(hits[h].end, L));
    std::sort(cover.begin(), cover.end());
    uint32_t at = 0, ordinal = 0;   // everything below `at` is covered or already a piece
    auto piece = [&](uint32_t from, uint32_t to) {
      if (to <= from) return;
      if (to - from < minPiece) { ++nDropped; nDroppedBases += to - from; return; }
      pieces.push_back(SplitPiece{r, from, to - from, ++ordinal});
    };
    for (const auto& iv : cover) {
      if (iv.first > at) piece(at, iv.first);
      at = std::max(at, iv.second);
    }
    piece(at, L);
  }
  readPieceOff[n_reads] = pieces.size();
  if (dropped) *dropped = nDropped;
  if (droppedBases) *droppedBases = nDroppedBases;
}

}  // namespace talc
