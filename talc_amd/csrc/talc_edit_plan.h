// talc_edit_plan.h — how the edit scripts (talc_kernels_edits.h, docs/correction_edits.md) size and place their alignments:
// which part a CORRECTED segment gets, whether a pair's delta words live in LDS, how many global words it takes
// otherwise, and the rounds the host cuts the DPs into so that the words of one round stay under a budget.  Host and
// device; no HIP type, so the CPU test-suite builds it too (pure_capi.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "talc_common.h"

namespace talc {

// one DP: a CORRECTED segment of a read, and where its delta words live (kEditInLds: in the wave's LDS)
struct EditTask { uint32_t seg, read; uint64_t scratchWord; };
constexpr uint64_t kEditInLds = ~0ull;

// The pattern (bits across the lanes) is the longer sequence, so that the words of a column hold few unused bits: the
// delta words of a pair take at most n m + min(n, m) / 4 + 136 bytes.  nw = words per column.
constexpr uint32_t kEditLdsWords = 1024;    // LDS delta words per wave (8 KiB)
constexpr uint32_t kEditLdsSeq = 1280;      // and bytes of the two sequences
constexpr uint32_t kEditLdsMaxNw = 16;      // an LDS pair has a pattern of at most 1024 positions (one block) ...
constexpr uint32_t kEditBlock = 4096;       // pattern positions per block of 64 lanes
TALC_HD uint32_t edit_nw(uint32_t n, uint32_t m) { return ((n > m ? n : m) + 63u) / 64u; }
// ... and nw * (text length) <= 256, so its text has at most 256 bytes: 1024 + 256 = kEditLdsSeq
TALC_HD bool edit_in_lds(uint32_t n, uint32_t m) { const uint64_t nw = edit_nw(n, m); return nw <= kEditLdsMaxNw && 4ull * nw * (n < m ? n : m) <= kEditLdsWords; }
// global words of a pair: 4 per column word, then the block carries (2 bit arrays over the text), rounded to 128 bytes so
// that no two pairs share a cache line
TALC_HD uint64_t edit_scratch_words(uint32_t n, uint32_t m) {
  const uint64_t nt = n < m ? n : m, w = 4ull * edit_nw(n, m) * nt + 2ull * ((nt + 63u) / 64u);
  return (w + 15ull) & ~15ull;
}
// how a CORRECTED segment's part is made
enum : int { EDIT_PART_EMPTY = 0, EDIT_PART_INS, EDIT_PART_DEL, EDIT_PART_UNALIGNED, EDIT_PART_DP };
TALC_HD int edit_part_kind(uint32_t n, uint32_t m, uint64_t max_cells) {
  if (n == 0) return m == 0 ? EDIT_PART_EMPTY : EDIT_PART_INS;
  if (m == 0) return EDIT_PART_DEL;
  return (uint64_t)n * m > max_cells ? EDIT_PART_UNALIGNED : EDIT_PART_DP;
}

// The DPs of a batch in the order they are added, cut into rounds: the tasks of round i are tasks[roundEnd[i - 1] ..
// roundEnd[i]); the global words of a round's tasks lie side by side from word 0 and together take at most budgetWords;
// mostWords is the largest round's sum — what the host allocates.  LDS pairs take no words and never end a round.
struct EditPlan {
  uint64_t budgetWords;
  std::vector<EditTask> tasks;
  std::vector<size_t> roundEnd;
  uint64_t used = 0, mostWords = 0;
  explicit EditPlan(uint64_t budget) : budgetWords(budget) {}
  // false: the pair alone is beyond the budget (nothing is added)
  bool add(uint32_t seg, uint32_t read, uint32_t n, uint32_t m) {
    if (edit_in_lds(n, m)) { tasks.push_back(EditTask{seg, read, kEditInLds}); return true; }
    const uint64_t w = edit_scratch_words(n, m);
    if (w > budgetWords) return false;
    if (used + w > budgetWords) { roundEnd.push_back(tasks.size()); used = 0; }
    tasks.push_back(EditTask{seg, read, used});
    used += w;
    if (used > mostWords) mostWords = used;
    return true;
  }
  void finish() { if (roundEnd.empty() || roundEnd.back() != tasks.size()) roundEnd.push_back(tasks.size()); }
};

}  // namespace talc
