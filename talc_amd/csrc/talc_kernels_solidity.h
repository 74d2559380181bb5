// talc_kernels_solidity.h — the solidity report (docs/solidity.md): how much of a sequence the short reads support.
// For a sequence S of L bases, n = max(0, L - K + 1) k-mer positions, c[i] = the table count of S[i, i + K) (0 when the
// k-mer is absent or holds an N), position i solid when c[i] >= MIN_COUNT, k_solidity leaves six integers per sequence
// (talc_solidity, include/talc_hip.h) and nothing per position.  What lordec-stat reports, and what the last column of
// the reference's stats header (nbInKmers2, Read.cpp:392,413) was meant to hold.
#pragma once
#include "talc_kmer_window.h"
#include "talc_kernels_search.h"   // ReadState

namespace talc {

struct SolidityRow { uint32_t nKmers, nSolid, nIn, nRegions, solidBases, longestWeak; };

// One wave per sequence; the wave walks it in order, SOL_TILE positions per pass.  The sequence view (the batch's codes
// as they are, or a dense ASCII record, from its far end when k_pack reverse complemented it, never copied in another
// form), the pass's window in LDS and the round of SOL_UNROLL count lookups per lane are talc_kmer_window.h's.  This
// kernel's own: __ballot turns each group of 64 positions into a word of solid bits and a word of IN bits; the rest is
// wave-uniform integer work on those words, with what crosses a 64-position word carried in registers: the last solid
// bit, the base coverage the word still owes the next (K - 1 <= 30 bits) and the open weak run.
#define SOL_UNROLL 4
#define SOL_TILE (64 * SOL_UNROLL)
static_assert(SOL_TILE == KWIN_TILE, "a pass is one window");

// the longest run of ones in x
TALC_D uint32_t longest_run(uint64_t x) {
  uint32_t best = 0;
  while (x) {
    const uint32_t s = (uint32_t)__builtin_ctzll(x);
    const uint64_t y = x >> s;                                           // (bit 0 set)
    const uint32_t r = (~y == 0ull) ? 64u : (uint32_t)__builtin_ctzll(~y);
    best = max(best, r);
    if (s + r >= 64u) break;
    x = (y >> r) << (s + r);
  }
  return best;
}

__global__ void __launch_bounds__(64)
k_solidity(TableView T, const uint8_t* __restrict__ seqs, const uint64_t* __restrict__ offsets, const ReadState* __restrict__ state,
           int ascii, int reverse, const uint8_t* __restrict__ rev_flags, uint32_t min_count, uint32_t n_reads, SolidityRow* __restrict__ rows) {
  __shared__ uint64_t s_pack[KWIN_PACK_WORDS];
  __shared__ uint64_t s_nmask[KWIN_N_WORDS];
  const KmerWindow win = {s_pack, s_nmask};
  const uint32_t r = blockIdx.x;
  if (r >= n_reads) return;
  const uint32_t lane = threadIdx.x;
  const uint32_t K = T.k;
  const uint64_t rb = offsets[r];
  const uint32_t L = (uint32_t)(offsets[r + 1] - rb);
  const uint32_t n = L >= K ? L - K + 1 : 0;
  // a record k_pack reverse complemented (a corrected read under -rev) is read back to front: the sequence the kernels
  // worked on, the orientation the table's directional counts belong to
  // (rev_flags: one byte per read, auto strand: a read whose byte is set is taken as under -rev)
  const bool flip = state != nullptr && (reverse || (rev_flags && rev_flags[r])) && state[r].status == TALC_READ_CORRECTED && state[r].overflow == 0;
  const SeqView seq = {(const uint8_t TALC_AS1*)(seqs + rb), L, ascii != 0, flip};
  const uint32_t kshift = 64 - 2 * K;
  const uint64_t nkmask = (1ULL << K) - 1;          // K <= 31
  const uint64_t cap = T.capacity;                  // >= 64: HostTable::capacity_for never gives less

  SolidityRow row = {n, 0u, 0u, 0u, 0u, 0u};
  uint64_t prevBit = 0;    // the solid bit of the position before the word
  uint64_t owed = 0;       // bases from the word's first on that solid k-mers of earlier words cover
  uint32_t openWeak = 0;   // weak positions that end at the position before the word

  for (uint32_t p0 = 0; p0 < n; p0 += SOL_TILE) {
    const uint32_t cnt = min((uint32_t)SOL_TILE, n - p0);
    const uint32_t wlen = cnt + K - 1;              // p0 + wlen <= L
    win.stage(seq, p0, wlen, lane);
    __syncthreads();
    uint64_t kmer[SOL_UNROLL];
    bool ask[SOL_UNROLL];
#pragma unroll
    for (int u = 0; u < SOL_UNROLL; ++u) {
      const uint32_t q = (uint32_t)u * 64u + lane;
      ask[u] = q < cnt && (win.nbits(q) & nkmask) == 0;               // no N among bases [q, q + K)
      kmer[u] = win.window(q) >> kshift;
    }
    probe_round<SOL_UNROLL>(T.right, cap, kmer, ask, cnt, [&](int u, uint32_t c) {   // one word of 64 positions
      const uint64_t solid = __ballot(c >= min_count);
      const uint64_t in = __ballot(c > min_count);
      const uint32_t nv = min(64u, cnt - (uint32_t)u * 64u);          // positions of this word
      const uint64_t valid = nv == 64u ? ~0ull : ((1ull << nv) - 1);
      row.nSolid += (uint32_t)__popcll(solid);
      row.nIn += (uint32_t)__popcll(in);
      row.nRegions += (uint32_t)__popcll(solid & ~((solid << 1) | prevBit));
      prevBit = solid >> 63;
      // bases: the word's solid bits dilated by K towards higher positions, as 128 bits
      uint64_t lo = solid, hi = 0;
      uint32_t have = 1;
      while (have < K) {
        const uint32_t s = min(have, K - have);     // 1 <= s <= 16
        hi |= (hi << s) | (lo >> (64 - s));
        lo |= lo << s;
        have += s;
      }
      row.solidBases += (uint32_t)__popcll(lo | owed);
      owed = hi;
      // weak runs
      const uint64_t weak = ~solid & valid;
      if (weak == valid) {
        openWeak += nv;
      } else {
        const uint32_t lead = (uint32_t)__builtin_ctzll(~weak);       // < nv
        row.longestWeak = max(row.longestWeak, max(openWeak + lead, longest_run(weak >> lead)));
        openWeak = (uint32_t)__builtin_clzll(~(weak << (64 - nv)));   // the run at the word's upper end, < nv
      }
    });
    __syncthreads();                                // (the next pass stages into the same words)
  }
  row.solidBases += (uint32_t)__popcll(owed);       // beyond the last word: bases n .. L - 1
  row.longestWeak = max(row.longestWeak, openWeak);
  if (lane == 0) rows[r] = row;
}

}  // namespace talc
