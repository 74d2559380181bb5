// talc_kernels_solidity.h — the solidity report (docs/solidity.md): how much of a sequence the short reads support.
// For a sequence S of L bases, n = max(0, L - K + 1) k-mer positions, c[i] = the table count of S[i, i + K) (0 when the
// k-mer is absent or holds an N), position i solid when c[i] >= MIN_COUNT, k_solidity leaves six integers per sequence
// (talc_solidity, include/talc_hip.h) and nothing per position.  What lordec-stat reports, and what the last column of
// the reference's stats header (nbInKmers2, Read.cpp:392,413) was meant to hold.
#pragma once
#include "talc_kernels_probe.h"
#include "talc_kernels_search.h"   // ReadState

namespace talc {

struct SolidityRow { uint32_t nKmers, nSolid, nIn, nRegions, solidBases, longestWeak; };

// One wave per sequence; the wave walks it in order, SOL_TILE positions per pass, and carries in registers what crosses a
// 64-position word: the last solid bit, the base coverage the word still owes the next (K - 1 <= 30 bits) and the open
// weak run.  A pass:
//   * the window's SOL_TILE + K - 1 bases go to LDS as 2-bit words and an N bitmap (the layout of k_coverage's window:
//     a k-mer is one funnel shift away), 8 bases per lane, all 8 bytes asked for before the first is used: the batch's
//     codes as they are, or a dense ASCII record through what ascii_to_code does — from its far end with what
//     complement_code does when the record was reverse complemented on its way out (k_pack) —, so the records are never
//     copied in another form;
//   * every lane takes SOL_UNROLL positions 64 apart and asks for the home buckets of all of them on one branch-free path
//     before it looks at the first: SOL_UNROLL random bucket reads in flight per lane; the home bucket decides nearly
//     every position, probe_bucket finishes the chains that go on;
//   * __ballot turns each group of 64 positions into a word of solid bits and a word of IN bits; the rest is wave-uniform
//     integer work on those words.
#define SOL_UNROLL 4
#define SOL_TILE (64 * SOL_UNROLL)

// what a count lookup reads of a bucket: the key and the four counts, 24 of its 32 bytes, so that no loaded register is
// left over for the compiler to reuse (it then has to wait for the load before the next one is asked for)
struct HomeBucket {
  uint64_t key;
  uint32_t cnt[4];
  TALC_D uint32_t count_of(int b) const { const uint32_t lo = (b & 1) ? cnt[1] : cnt[0], hi = (b & 1) ? cnt[3] : cnt[2]; return (b & 2) ? hi : lo; }
};
TALC_D HomeBucket load_home_bucket(const Bucket* p) {
  const v4u32 a = *(const v4u32 TALC_AS1*)p;
  const v2u32 c = *(const v2u32 TALC_AS1*)((const uint8_t TALC_AS1*)p + 16);
  HomeBucket r;
  r.key = ((uint64_t)a.y << 32) | a.x;
  r.cnt[0] = a.z; r.cnt[1] = a.w; r.cnt[2] = c.x; r.cnt[3] = c.y;
  return r;
}

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
  __shared__ uint64_t s_pack[SOL_TILE / 32 + 8];    // base i of the window at bits [63 - 2 (i % 32) - 1, 63 - 2 (i % 32)] of word i / 32
  __shared__ uint64_t s_nmask[SOL_TILE / 64 + 4];   // bit (i % 64) of word i / 64: base i is N
  static_assert(sizeof(s_pack) == 64 * 2 && sizeof(s_nmask) == 64, "one 8-base group per lane fills both arrays");
  static_assert(SOL_TILE + 32 + 64 <= 8 * 64, "a window of SOL_TILE + K - 1 bases, and window() / nbits() read one word beyond a k-mer's first");
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
  const uint8_t TALC_AS1* src = (const uint8_t TALC_AS1*)(seqs + rb);
  // base i (< L) of the sequence sits at byte at_byte(i); code_of turns the byte into a Dna5 code: ascii_to_code and
  // complement_code as selects (the staging below asks for a lane's 8 bytes at once and must not branch between them)
  auto at_byte = [&](uint32_t i) -> uint32_t { return flip ? L - 1 - i : i; };
  const uint32_t flipMask = flip ? 3u : 0u;         // complement_code of A, C, G, T is code ^ 3
  auto code_of = [&](uint32_t c) -> uint32_t {
    const uint32_t up = c & 0xDFu;                  // 'a' -> 'A': no other byte becomes a letter
    const uint32_t two = (up >> 1) & 3u;            // A, C, G, T -> 0, 1, 3, 2
    const bool letter = (up == 'A') | (up == 'C') | (up == 'G') | (up == 'T');
    const uint32_t a = letter ? (two ^ (two >> 1)) : 4u;
    const uint32_t code = ascii ? a : c;
    return code ^ (code < 4u ? flipMask : 0u);
  };
  auto window = [&](uint32_t q) -> uint64_t {
    const uint32_t w = q >> 5, sh = 2 * (q & 31);
    const uint64_t hi = s_pack[w], lo = s_pack[w + 1];
    return (sh == 0) ? hi : ((hi << sh) | (lo >> (64 - sh)));
  };
  auto nbits = [&](uint32_t q) -> uint64_t {
    const uint32_t nw = q >> 6, nsh = q & 63;
    const uint64_t nlo = s_nmask[nw], nhi = s_nmask[nw + 1];
    return (nsh == 0) ? nlo : ((nlo >> nsh) | (nhi << (64 - nsh)));
  };
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
    {   // stage the window: lane g packs bases 8 g .. 8 g + 7 (zeros beyond the window).  The 8 byte loads are asked for
        // together, at addresses clamped into the window, and masked afterwards: one round trip per pass
      uint32_t raw8[8];
#pragma unroll
      for (uint32_t j = 0; j < 8; ++j) raw8[j] = src[at_byte(p0 + min(8 * lane + j, wlen - 1))];
      uint32_t w = 0, nm = 0;
#pragma unroll
      for (uint32_t j = 0; j < 8; ++j) {
        const uint32_t c = (8 * lane + j < wlen) ? code_of(raw8[j]) : 0u;
        nm |= (c > 3u ? 1u : 0u) << j;
        w |= (c & 3u) << (14 - 2 * j);
      }
      reinterpret_cast<uint16_t*>(s_pack)[lane ^ 3u] = (uint16_t)w;   // group 0 of four = the top 16 bits of its word
      reinterpret_cast<uint8_t*>(s_nmask)[lane] = (uint8_t)nm;
    }
    __syncthreads();
    // the home buckets of all of the lane's positions are asked for on one branch-free path (a position that has
    // nothing to ask — beyond the sequence, an N in its k-mer — reads bucket 0 and ignores it), then the chains
    uint64_t kmer[SOL_UNROLL];
    uint32_t slot[SOL_UNROLL];                      // (capacity < 2^32)
    HomeBucket bk[SOL_UNROLL];
    bool ask[SOL_UNROLL];
#pragma unroll
    for (int u = 0; u < SOL_UNROLL; ++u) {
      const uint32_t q = (uint32_t)u * 64u + lane;
      ask[u] = q < cnt && (nbits(q) & nkmask) == 0;                   // no N among bases [q, q + K)
      kmer[u] = window(q) >> kshift;
      slot[u] = ask[u] ? (uint32_t)dev_home(kmer[u] >> 2, cap) : 0u;
    }
#pragma unroll
    for (int u = 0; u < SOL_UNROLL; ++u) bk[u] = load_home_bucket(T.right + slot[u]);
#pragma unroll
    for (int u = 0; u < SOL_UNROLL; ++u) {
      if ((uint32_t)u * 64u >= cnt) break;          // (wave-uniform)
      // the home bucket decides nearly every position, by selects; a chain that goes on is the prober's
      const uint64_t key = kmer[u] >> 2;
      const int b = (int)(kmer[u] & 3);
      const bool match = (bk[u].key & kKeyMask) == key;
      uint32_t c = (ask[u] && match) ? bk[u].count_of(b) : 0u;
      if (ask[u] && !match && bk[u].key != kEmptyKey) {
        BucketRegs r;
        if (probe_bucket(T.right, cap, key, r)) c = r.count_of(b);
      }
      const uint64_t solid = __ballot(c >= min_count);   // (MIN_COUNT >= 1: an absent k-mer is never solid)
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
    }
    __syncthreads();                                // (the next pass stages into the same words)
  }
  row.solidBases += (uint32_t)__popcll(owed);       // beyond the last word: bases n .. L - 1
  row.longestWeak = max(row.longestWeak, openWeak);
  if (lane == 0) rows[r] = row;
}

}  // namespace talc
