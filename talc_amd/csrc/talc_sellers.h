// talc_sellers.h — what the scans of the long-read preparation share (docs/read_preparation.md): the end clean-up, the
// chimera split, the barcode demultiplexing and the UMI read-out all run the Sellers recurrence of a pattern of m <= 64
// letters over a text of codes, as Myers' bit vectors in Hyyrö's form.  Here are the column step, the lane that runs it over
// a chunk of a staged text, the text of a read's end, the interval record of the gather, and how a setting's patterns are
// walked, checked and made into match masks.  Host and device; no HIP type and no kernel, so the CPU test-suite builds it too (pure_capi.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "talc_common.h"

namespace talc {

// The match mask of a text code.  peq[c]: bit i set when letter i of the pattern matches code c; a code of 4 (a byte
// outside ACGTacgt) matches nothing and has no mask.
TALC_HD uint64_t sellers_eq(const uint64_t (&peq)[4], uint32_t c) {
  return c == 0u ? peq[0] : c == 1u ? peq[1] : c == 2u ? peq[2] : c == 3u ? peq[3] : 0ull;
}

// One column of the matrix: its vertical deltas (Pv, Mv: bit i set when row i + 1 is one more, one less than row i) and
// its bottom cell, D[m][j].
struct SellersColumn {
  uint64_t Pv, Mv;
  uint32_t score;
  // the first column, D[i][0] = i
  TALC_HD void start(uint32_t m) { Pv = ~0ull; Mv = 0ull; score = m; }
  // The next column, under the match mask Eq of its text code.  Free: the top row is 0 in every column, a match may start
  // anywhere.  Anchored (!Free): the top row is j, the positive horizontal delta is carried in.
  template <bool Free = true>
  TALC_HD void step(uint64_t Eq, uint32_t m) {
    const uint64_t top = 1ull << (m - 1u);
    const uint64_t Xv = Eq | Mv;
    const uint64_t Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
    uint64_t Ph = Mv | ~(Xh | Pv);
    uint64_t Mh = Pv & Xh;
    score += (Ph & top) ? 1u : 0u;
    score -= (Mh & top) ? 1u : 0u;
    Ph = Free ? Ph << 1 : Ph << 1 | 1ull;
    Mh <<= 1;
    Pv = Mh | ~(Xv | Ph);
    Mv = Ph & Xv;
  }
};

// the columns [*c0, *c1) of chunk q when a text of n columns is dealt evenly over `chunks` chunks
TALC_HD void sellers_chunk(uint32_t n, uint32_t chunks, uint32_t q, uint32_t* c0, uint32_t* c1) {
  const uint32_t chunk = (n + chunks - 1u) / chunks;
  *c0 = q * chunk < n ? q * chunk : n;
  *c1 = *c0 + chunk < n ? *c0 + chunk : n;
}

// One lane: the pattern `peq` (m letters, bound k) over the staged codes s[0, n), of which it owns the columns [c0, c1).
// Its key is the accepted column (D <= k) with the smallest D, the largest among ties, as D << 32 | (0xFFFFFFFF - e), e the
// number of letters the match ends behind; `noKey` without one.  Keys of lanes and of patterns reduce by their minimum.
//
// The warm-up.  A lane whose chunk does not start the text starts m + k columns before it from the free-start state
// (start(): Pv all ones, score m).  That is what column 0 holds, and an upper bound of any later column, so every score of
// the lane is >= the true D.  An alignment of cost d <= k spans at most m + d <= m + k letters of the text: for every
// column of the chunk whose true D is <= k, the best alignment begins inside the warm-up, where the lane's state allows
// everything the true one does, and the lane's score is exact.  Everywhere else it is >= D > k, which stays rejected.
// A lane that starts at column 0 holds the true state throughout.  (The chimera lane, which needs C = min(D, k + 1) exactly
// on a neighbourhood of its chunk, and the UMI recompute, which restarts m + k columns before an accepted column, rest on
// the same argument.)
// (the device's own min keeps the 64-bit minimum one compare and one pair of selects under a single condition; written as a
//  ternary the column loop of k_read_ends gets a third select, or a branch)
#if defined(__HIP_DEVICE_COMPILE__)
TALC_D uint64_t sellers_min(uint64_t a, uint64_t b) { return min(a, b); }
#else
inline uint64_t sellers_min(uint64_t a, uint64_t b) { return b < a ? b : a; }
#endif
TALC_HD uint64_t sellers_no_key(uint32_t k) { return (uint64_t)(k + 1u) << 32 | 0xFFFFFFFFull; }   // D clamped to k + 1, no end
TALC_HD uint64_t sellers_lane(const uint8_t* s, const uint64_t (&peq)[4], uint32_t m, uint32_t k, uint32_t c0, uint32_t c1, uint64_t noKey) {
  uint64_t best = noKey;
  if (c0 >= c1) return best;
  const uint32_t warm = m + k;
  SellersColumn col;
  col.start(m);
  for (uint32_t j = c0 > warm ? c0 - warm : 0u; j < c1; ++j) {
    col.step(sellers_eq(peq, s[j]), m);
    const uint64_t key = (uint64_t)col.score << 32 | (0xFFFFFFFFu - (j + 1u));
    if (j >= c0 && col.score <= k) best = sellers_min(best, key);
  }
  return best;
}

// ------------------------------------------------------------------ the text of a read's end
// code i of the end's text: the read's bytes as they lie (head), or back to front and complemented (tail); the reverse
// complement is never written anywhere
TALC_HD uint32_t end_code(const uint8_t* __restrict__ rd, uint32_t L, uint32_t i, bool tail) {
  const uint32_t c = ascii_to_code_select(rd[tail ? L - 1u - i : i]);
  return tail && c < 4u ? 3u - c : c;
}
// codes [from, from + n) of the end's text into s[0, n) (from + n <= L): every `step`-th from `first` on.  A wave stages
// with (lane, 64), the host with (0, 1).
TALC_HD void stage_end(uint8_t* s, const uint8_t* __restrict__ rd, uint32_t L, uint32_t from, uint32_t n, bool tail, uint32_t first, uint32_t step) {
  for (uint32_t i = first; i < n; i += step) s[i] = (uint8_t)end_code(rd, L, from + i, tail);
}

// ------------------------------------------------------------------ what k_gather copies
// Record i of a table of rows stands for bytes [start, start + len) of source read `read`.  Every row type that is gathered
// from states that next to its definition, as gather_interval(row, i): the end rows, the UMI rows, the split pieces.
struct GatherInterval { uint32_t read, start, len; };

// ------------------------------------------------------------------ a setting's patterns
// the set of a plain letter as a mask over the codes A C G T (bit c); 0: not a letter of ACGTacgt
inline uint32_t acgt_set(uint8_t ch) { const uint8_t c = ascii_to_code(ch); return c < 4 ? 1u << c : 0u; }
// ... of a letter that is kept as its code already (0 .. 3)
inline uint32_t code_set(uint8_t code) { return 1u << code; }

// What refuses a pattern of m letters: its length (12 .. 64), or its first letter without a set (*bad: its index).  The
// callers word the refusal: the messages are theirs.
enum PatternFault { PATTERN_OK = 0, PATTERN_LENGTH, PATTERN_LETTER };
template <class Letter, class SetOf>
inline PatternFault pattern_fault(const Letter* p, size_t m, SetOf set_of, size_t* bad) {
  if (m < 12 || m > 64) return PATTERN_LENGTH;
  for (size_t i = 0; i < m; ++i)
    if (!set_of((uint8_t)p[i])) { *bad = i; return PATTERN_LETTER; }
  return PATTERN_OK;
}

// The items of a comma-separated list, in order, each checked by pattern_fault:
//   for (PatternList it(text); it.next(acgt_set);) { it.p[0, it.m), it.fault ... }
// An empty or null text has no item.
struct PatternList {
  const char* rest;    // the next item; null behind the last
  const char* p;
  size_t m, bad;
  PatternFault fault;
  explicit PatternList(const char* text) : rest(text && *text ? text : nullptr), p(nullptr), m(0), bad(0), fault(PATTERN_OK) {}
  template <class SetOf>
  bool next(SetOf set_of) {
    if (!rest) return false;
    const char* const e = strchr(rest, ',');
    p = rest; m = e ? (size_t)(e - rest) : strlen(rest);
    rest = e ? e + 1 : nullptr;
    fault = pattern_fault(p, m, set_of, &bad);
    return true;
  }
};

// The match masks of a pattern that pattern_fault has passed, ored into peq[0 .. 4).  revcomp: of its reverse complement
// (letter i is the complement of p[m - 1 - i]); mirrored: of the pattern back to front (bit m - 1 - i for letter i), which
// is what a search from a match's end towards its start runs.
template <class Letter, class SetOf>
inline void pattern_masks(const Letter* p, size_t m, SetOf set_of, bool revcomp, bool mirrored, uint64_t* peq) {
  for (size_t i = 0; i < m; ++i) {
    const uint32_t set = set_of((uint8_t)p[revcomp ? m - 1 - i : i]);
    for (uint32_t c = 0; c < 4u; ++c)
      if (set >> c & 1u) peq[revcomp ? 3u - c : c] |= 1ull << (mirrored ? m - 1 - i : i);
  }
}

}  // namespace talc
