// talc_kmer_window.h — what the "one wave per sequence, KWIN_TILE k-mer positions per pass" kernels share (k_solidity,
// k_base_support, k_strand_vote): where a base of the sequence lies and what code it has, the pass's window of bases in
// LDS, and one round of count lookups.  This header owns the layout rules; the kernels keep the ballots and what follows.
// k_coverage (talc_kernels_probe.h) reads a window of the same layout with accessors of its own; its staging differs.
#pragma once
#include "talc_kernels_probe.h"

namespace talc {

// ------------------------------------------------------------------ the sequence
// Base i (< L) of the sequence sits at byte at_byte(i) of src; code_of turns that byte into a Dna5 code.  ascii: the bytes
// are letters (a dense record, a raw read), else codes already.  flip: the sequence is the reverse complement of the
// bytes (a record k_pack reverse complemented on its way out): read from the far end, A, C, G, T complemented.  All
// selects: the staging asks for a lane's 8 bytes at once and must not branch between them.
struct SeqView {
  const uint8_t TALC_AS1* src;
  uint32_t L;
  bool ascii, flip;
  TALC_D uint32_t at_byte(uint32_t i) const { return flip ? L - 1 - i : i; }
  TALC_D uint32_t code_of(uint32_t c) const {
    const uint32_t code = ascii ? ascii_to_code_select(c) : c;
    return code ^ (code < 4u ? (flip ? 3u : 0u) : 0u);   // complement_code of A, C, G, T is code ^ 3
  }
};

// ------------------------------------------------------------------ the window
// A pass covers up to KWIN_TILE positions, so its window holds up to KWIN_TILE + K - 1 <= KWIN_TILE + 30 bases.  Every
// lane stages one group of 8 bases, 512 in all, zeros beyond the window: both arrays are written whole on every pass, and
// the words behind the window's last base are the guard words that window() and nbits() read one beyond a k-mer's first.
#define KWIN_TILE 256
#define KWIN_PACK_WORDS (KWIN_TILE / 32 + 8)   /* s_pack: base i at bits [63 - 2 (i % 32) - 1, 63 - 2 (i % 32)] of word i / 32 */
#define KWIN_N_WORDS (KWIN_TILE / 64 + 4)      /* s_nmask: bit (i % 64) of word i / 64: base i is N */
static_assert(KWIN_PACK_WORDS * 8 == 64 * 2 && KWIN_N_WORDS * 8 == 64, "one 8-base group per lane fills both arrays");
static_assert(KWIN_TILE + 32 + 64 <= 8 * 64, "a window of KWIN_TILE + K - 1 bases, and window() / nbits() read one word beyond a k-mer's first");

struct KmerWindow {
  uint64_t* pack;    // __shared__ uint64_t [KWIN_PACK_WORDS], declared by the kernel
  uint64_t* nmask;   // __shared__ uint64_t [KWIN_N_WORDS]
  // bases [p0, p0 + wlen) of the sequence, wlen >= 1 and p0 + wlen <= L: lane g packs bases 8 g .. 8 g + 7.  The 8 byte
  // loads are asked for together, at addresses clamped into the window, and masked afterwards: one round trip per pass.
  // The caller puts a barrier between stage() and the accessors, and between the accessors and the next stage().
  TALC_D void stage(const SeqView& v, uint32_t p0, uint32_t wlen, uint32_t lane) const {
    uint32_t raw8[8];
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) raw8[j] = v.src[v.at_byte(p0 + min(8 * lane + j, wlen - 1))];
    uint32_t w = 0, nm = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
      const uint32_t c = (8 * lane + j < wlen) ? v.code_of(raw8[j]) : 0u;
      nm |= (c > 3u ? 1u : 0u) << j;
      w |= (c & 3u) << (14 - 2 * j);
    }
    reinterpret_cast<uint16_t*>(pack)[lane ^ 3u] = (uint16_t)w;   // group 0 of four = the top 16 bits of its word
    reinterpret_cast<uint8_t*>(nmask)[lane] = (uint8_t)nm;
  }
  // the 64 window bits that start with base q (first base most significant: a k-mer is `>> (64 - 2 K)` away), and the N
  // bits of bases [q, q + 64)
  TALC_D uint64_t window(uint32_t q) const {
    const uint32_t w = q >> 5, sh = 2 * (q & 31);
    const uint64_t hi = pack[w], lo = pack[w + 1];
    return (sh == 0) ? hi : ((hi << sh) | (lo >> (64 - sh)));
  }
  TALC_D uint64_t nbits(uint32_t q) const {
    const uint32_t nw = q >> 6, nsh = q & 63;
    const uint64_t nlo = nmask[nw], nhi = nmask[nw + 1];
    return (nsh == 0) ? nlo : ((nlo >> nsh) | (nhi << (64 - nsh)));
  }
};

// ------------------------------------------------------------------ the probe round
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

// The table counts of a lane's U k-mers, position u * 64 + lane of a pass of cnt positions: use(u, c) is called by the whole
// wave, in order, for every group u that has a position (u * 64 < cnt), with c = the count of kmer[u] where go[u], 0 where
// nothing was asked or found — and the table holds no count 0, MIN_COUNT >= 1: such a position is never solid.  The home
// buckets of all U are asked for on one branch-free path before the first is looked at (a position with nothing to ask
// reads bucket 0 and ignores it): U random bucket reads in flight per lane.  The home bucket decides nearly every position,
// by selects; a chain that goes on is the prober's.  A count is handed over as soon as it is known (the ballots of group u
// come before the chains of group u + 1: no count is held in a register across them).  `right` has `cap` >= 1 buckets.
template <int U, class Use>
TALC_D void probe_round(const Bucket* right, uint64_t cap, const uint64_t (&kmer)[U], const bool (&go)[U], uint32_t cnt, Use&& use) {
  uint32_t slot[U];                                 // (capacity < 2^32)
  HomeBucket bk[U];
#pragma unroll
  for (int u = 0; u < U; ++u) slot[u] = go[u] ? (uint32_t)dev_home(kmer[u] >> 2, cap) : 0u;
#pragma unroll
  for (int u = 0; u < U; ++u) bk[u] = load_home_bucket(right + slot[u]);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if ((uint32_t)u * 64u >= cnt) break;            // (wave-uniform: no lane has a position in this group or a later one)
    const uint64_t key = kmer[u] >> 2;
    const int b = (int)(kmer[u] & 3);
    const bool match = (bk[u].key & kKeyMask) == key;
    uint32_t c = (go[u] && match) ? bk[u].count_of(b) : 0u;
    if (go[u] && !match && bk[u].key != kEmptyKey) {
      BucketRegs r;
      if (probe_bucket(right, cap, key, r)) c = r.count_of(b);
    }
    use(u, c);
  }
}

}  // namespace talc
