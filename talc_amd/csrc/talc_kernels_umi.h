// talc_kernels_umi.h — UMI read-out of long reads (docs/umi.md): one degenerate pattern (IUPAC letters, m = 12 .. 64, of
// which u = 1 .. 32 stand for more than one base) found at either end of every read, aligned, and the read's bases under
// the degenerate positions reported.  Bound k = floor(max_error_pct m / 100).  For a read S of L bytes the end rule U(S) is
//   T = S[0, min(L, window)); D[i][j] = the Sellers matrix of the pattern against T (top row 0, first column i, substitution
//   0 when T[j-1] is in the set of pattern letter i, else 1, indel 1); d = min over j >= 1 of D[m][j] (m for an empty T);
//   accepted when d <= k: err = d, stop = the largest j with D[m][j] = d; the canonical alignment is the traceback from
//   (m, stop) that at (i, j), i > 0, takes the first that holds of: the diagonal (j > 0, D[i-1][j-1] + cost = D[i][j]), up
//   (D[i-1][j] + 1 = D[i][j]: letter i faces a gap), left (T[j-1] is inserted); start = the j it reaches row 0 at; the UMI
//   is, per degenerate position in pattern order, the text base the diagonal put under it (N when it is not of ACGT), '-'
//   when the position faces a gap;
// the head is U(S), the tail U(revcomp(S)): the codes are read back to front and complemented, the reverse complement is
// never written anywhere.  The read's UMI is that of the accepted end with the smaller err, the head on equal err.
// k_read_umi leaves one 56-byte talc_umi_row per read.
//
// The lane code is TALC_HD: k_read_umi runs 64 lanes of the search per end and one lane of the recompute and the traceback,
// umi_scan_host (pure_capi.cpp, the CPU test-suite) runs the same lanes one after another.
#pragma once
#include <cstdio>
#include <cstring>

#include "talc_sellers.h"
#if defined(__HIPCC__)
#include "talc_kernels_ends.h"    // EndRow
#include "talc_wave.h"
#endif

namespace talc {

constexpr uint32_t kUmiMaxWindow = 4096, kUmiDefaultWindow = 256, kUmiMaxDegenerate = 32;
constexpr uint32_t kUmiMaxColumns = 84;   // m + k + 1 at m = 64, k = 19: the columns j0 .. stop of the recompute
constexpr uint32_t kUmiRowWords = 14;     // a row as 32-bit words

struct UmiRow {   // talc_umi_row
  uint8_t end, err, otherErr, umiLen;
  uint32_t start, stop;
  uint32_t keptStart, keptLen;
  char umi[32];
  uint32_t pad_;
};
TALC_HD GatherInterval gather_interval(const UmiRow& row, uint32_t i) { return GatherInterval{i, row.keptStart, row.keptLen}; }

// The setting as the kernel takes it, by value: everything in it is wave-uniform.  peq[c]: bit i set when the set of
// pattern letter i holds code c (a degenerate letter sets its bit in several of the four); degen: bit i set when letter i
// is degenerate.
struct UmiParams {
  uint64_t peq[4];
  uint64_t degen;
  uint32_t m, k, window, u;
};

// the set of an IUPAC letter as a mask over the codes A C G T (bit c); 0: not a letter of ACGTRYSWKMBDHVN
TALC_HD uint32_t iupac_set(uint8_t ch) {
  switch (ch & 0xDFu) {
    case 'A': return 1u;  case 'C': return 2u;  case 'G': return 4u;  case 'T': return 8u;
    case 'R': return 5u;  case 'Y': return 10u; case 'S': return 6u;  case 'W': return 9u;
    case 'K': return 12u; case 'M': return 3u;  case 'B': return 14u; case 'D': return 13u;
    case 'H': return 11u; case 'V': return 7u;  case 'N': return 15u;
    default: return 0u;
  }
}

// The setting from its text (the library and the CPU suite).  False and a message in `why` when a value is refused; P is
// written only when every value has passed.  An empty or null pattern is the setting switched off: P.m = 0.
inline bool umi_make_setting(const char* pattern, uint32_t max_error_pct, uint32_t window, UmiParams& P, char* why, size_t whyLen) {
  UmiParams Q;
  memset(&Q, 0, sizeof Q);
  if (!pattern || !*pattern) { P = Q; return true; }
  if (max_error_pct > 30) { snprintf(why, whyLen, "max_error_pct=%u: at most 30", max_error_pct); return false; }
  if (!window) window = kUmiDefaultWindow;
  if (window < 32 || window > kUmiMaxWindow) { snprintf(why, whyLen, "window=%u: 32 .. %u (0: %u)", window, kUmiMaxWindow, kUmiDefaultWindow); return false; }
  const size_t m = strlen(pattern);
  size_t bad = 0;
  const PatternFault fault = pattern_fault(pattern, m, iupac_set, &bad);
  if (fault == PATTERN_LENGTH) { snprintf(why, whyLen, "pattern: %llu letters: 12 .. 64", (unsigned long long)m); return false; }
  if (fault) { snprintf(why, whyLen, "pattern: letter %llu is not one of ACGTRYSWKMBDHVN", (unsigned long long)(bad + 1)); return false; }
  pattern_masks(pattern, m, iupac_set, false, false, Q.peq);
  for (size_t i = 0; i < m; ++i) {
    const uint32_t set = iupac_set((uint8_t)pattern[i]);
    if (set & (set - 1u)) { Q.degen |= 1ull << i; ++Q.u; }
  }
  if (Q.u < 1 || Q.u > kUmiMaxDegenerate) { snprintf(why, whyLen, "pattern: %u degenerate letters: 1 .. %u", Q.u, kUmiMaxDegenerate); return false; }
  Q.m = (uint32_t)m; Q.k = max_error_pct * Q.m / 100u; Q.window = window;
  P = Q;
  return true;
}

// the kernel's LDS: the recompute's columns (Pv, Mv), the row as it is put together, then the codes of the two end
// windows, each rounded up to 16 bytes
TALC_HD uint32_t umi_code_stride(const UmiParams& P) {
  const uint32_t w = P.window < kUmiMaxWindow ? P.window : kUmiMaxWindow;
  return (w + 15u) & ~15u;
}
TALC_HD uint32_t umi_lds_bytes(const UmiParams& P) { return kUmiMaxColumns * 16u + kUmiRowWords * 4u + 2u * umi_code_stride(P); }

// ------------------------------------------------------------------ 1. the search
// lane `lane` of 64 over the staged codes s[0, n): its chunk of the columns behind a warm-up of m + k (sellers_lane); the
// key is score << 32 | (0xFFFFFFFF - j), sellers_no_key(k) without a column of D <= k
TALC_HD uint64_t umi_search_lane(const uint8_t* s, uint32_t n, const UmiParams& P, uint32_t lane) {
  uint32_t c0, c1;
  sellers_chunk(n, 64u, lane, &c0, &c1);
  return sellers_lane(s, P.peq, P.m, P.k, c0, c1, sellers_no_key(P.k));
}

// the read's end from the two ends' keys: end 1 head, 2 tail, 0 none
struct UmiPick { uint32_t end, err, otherErr, stop; };
TALC_HD UmiPick umi_pick(uint64_t keyHead, uint64_t keyTail, uint32_t k) {
  const uint32_t eh = (uint32_t)(keyHead >> 32), et = (uint32_t)(keyTail >> 32);
  UmiPick p = {0u, 0u, 255u, 0u};
  if (eh > k && et > k) return p;
  const bool head = eh <= k && (et > k || eh <= et);
  p.end = head ? 1u : 2u;
  p.err = head ? eh : et;
  p.stop = 0xFFFFFFFFu - (uint32_t)(head ? keyHead : keyTail);
  const uint32_t other = head ? et : eh;
  p.otherErr = other <= k ? other : 255u;
  return p;
}

// ------------------------------------------------------------------ 2. the recompute
// The recurrence again from the free-start state at column j0 = max(0, stop - (m + k)), Pv and Mv of every column
// j0 .. stop kept in cols[2 (j - j0)], cols[2 (j - j0) + 1].  The alignment that ends at (m, stop) with d <= k edits spans
// at most m + k letters of the text, and so does every alignment a step's equality can hold for: all of them begin at or
// after j0, where the restarted columns are exact.  Returns j0.
TALC_HD uint32_t umi_recompute(const uint8_t* s, const UmiParams& P, uint32_t stop, uint64_t* cols) {
  const uint32_t span = P.m + P.k;
  const uint32_t j0 = stop > span ? stop - span : 0u;
  SellersColumn col;                                   // (its score is not read: the traceback sums the deltas)
  col.start(P.m);
  cols[0] = col.Pv; cols[1] = col.Mv;
  for (uint32_t j = j0; j < stop; ++j) {
    col.step(sellers_eq(P.peq, s[j]), P.m);
    cols[2u * (j + 1u - j0)] = col.Pv; cols[2u * (j + 1u - j0) + 1u] = col.Mv;
  }
  return j0;
}

// D[i][j0 + at] of the recomputed columns: the vertical deltas of rows 1 .. i summed
TALC_HD int32_t umi_cell(const uint64_t* cols, uint32_t at, uint32_t i) {
  const uint64_t low = i >= 64u ? ~0ull : (1ull << i) - 1ull;
  return (int32_t)__builtin_popcountll(cols[2u * at] & low) - (int32_t)__builtin_popcountll(cols[2u * at + 1u] & low);
}

// ------------------------------------------------------------------ 3. the traceback
// One lane walks back from (m, stop) over the recomputed columns; umi[0, 32): '-' at the u degenerate positions until a
// diagonal step puts a base under one, zero behind them.  Returns start.  At column j0 only `up` is left (see above), and
// at most 2 m + k steps are taken.
TALC_HD uint32_t umi_traceback(const uint8_t* s, const UmiParams& P, uint32_t stop, uint32_t j0, const uint64_t* cols, char* umi) {
  for (uint32_t x = 0; x < kUmiMaxDegenerate; ++x) umi[x] = x < P.u ? '-' : (char)0;
  uint32_t i = P.m, j = stop;
  for (uint32_t step = 0; i > 0u && step < 2u * P.m + P.k; ++step) {
    const int32_t here = umi_cell(cols, j - j0, i);
    const uint64_t bit = 1ull << (i - 1u);
    if (j > j0) {
      const uint32_t c = s[j - 1u];
      if (umi_cell(cols, j - 1u - j0, i - 1u) + ((sellers_eq(P.peq, c) & bit) ? 0 : 1) == here) {
        if (P.degen & bit) umi[__builtin_popcountll(P.degen & (bit - 1ull))] = c == 0u ? 'A' : c == 1u ? 'C' : c == 2u ? 'G' : c == 3u ? 'T' : 'N';
        --i; --j;
        continue;
      }
    }
    if (umi_cell(cols, j - j0, i - 1u) + 1 == here || j == j0) { --i; continue; }
    --j;
  }
  return j;
}

// the row of a read of L bytes from its pick; head, tail: what the end clean-up claims of the read (0, 0 without it)
TALC_HD void umi_row_fill(UmiRow& row, const UmiPick& pk, uint32_t start, uint32_t u, uint32_t L, uint32_t head, uint32_t tail) {
  row.end = (uint8_t)pk.end; row.err = (uint8_t)pk.err; row.otherErr = (uint8_t)pk.otherErr; row.umiLen = (uint8_t)(pk.end ? u : 0u);
  row.start = pk.end ? start : 0u; row.stop = pk.end ? pk.stop : 0u;
  const uint32_t cutHead = pk.end == 1u ? pk.stop : 0u, cutTail = pk.end == 2u ? pk.stop : 0u;
  const uint32_t h = head > cutHead ? head : cutHead, t = tail > cutTail ? tail : cutTail;   // h <= L: each is
  row.keptStart = h;
  row.keptLen = L - h - (t < L - h ? t : L - h);
  row.pad_ = 0u;
}

// ------------------------------------------------------------------ the kernel's walk on the host, lanes one after another
inline UmiRow umi_scan_host(const uint8_t* rd, uint32_t L, const UmiParams& P) {
  const uint32_t window = P.window < kUmiMaxWindow ? P.window : kUmiMaxWindow;
  const uint32_t n = L < window ? L : window;
  static thread_local uint8_t code[2][kUmiMaxWindow];
  for (uint32_t end = 0; end < 2u; ++end) stage_end(code[end], rd, L, 0u, n, end == 1u, 0u, 1u);
  uint64_t key[2];
  for (uint32_t end = 0; end < 2u; ++end) {
    key[end] = sellers_no_key(P.k);
    for (uint32_t lane = 0; lane < 64u; ++lane) { const uint64_t x = umi_search_lane(code[end], n, P, lane); key[end] = x < key[end] ? x : key[end]; }
  }
  const UmiPick pk = umi_pick(key[0], key[1], P.k);
  UmiRow row;
  memset(&row, 0, sizeof row);
  uint32_t start = 0;
  if (pk.end) {
    uint64_t cols[2 * kUmiMaxColumns];
    const uint8_t* const s = code[pk.end - 1u];
    const uint32_t j0 = umi_recompute(s, P, pk.stop, cols);
    start = umi_traceback(s, P, pk.stop, j0, cols, row.umi);
  }
  umi_row_fill(row, pk, start, P.u, L, 0u, 0u);
  return row;
}

#if defined(__HIPCC__)
// One wave per read.  Both end windows are staged once as codes; the ends are searched one after the other, 64 chunks
// each; lane 0 recomputes the columns behind the winning stop, walks back and puts the row together in LDS; the wave
// writes it out, a word a lane.  ends: the rows of k_read_ends over the same reads, whose claims the kept interval
// combines with, or null.
__global__ void __launch_bounds__(64)
k_read_umi(const uint8_t* __restrict__ raw, const uint64_t* __restrict__ offsets, uint32_t n_reads, UmiParams P, const EndRow* __restrict__ ends,
           UmiRow* __restrict__ rows) {
  extern __shared__ uint64_t s_umi[];                  // umi_lds_bytes(P)
  const uint32_t r = blockIdx.x;
  if (r >= n_reads || P.m < 12u || P.m > 64u || P.m + P.k + 1u > kUmiMaxColumns || P.u > kUmiMaxDegenerate) return;
  const uint32_t lane = threadIdx.x;
  const uint64_t rb = offsets[r];
  const uint32_t L = (uint32_t)(offsets[r + 1] - rb);
  const uint8_t* const rd = raw + rb;
  const uint32_t stride = umi_code_stride(P);
  uint64_t* const s_cols = s_umi;
  UmiRow* const s_row = (UmiRow*)(s_umi + 2u * kUmiMaxColumns);
  uint8_t* const s_head = (uint8_t*)(s_umi + 2u * kUmiMaxColumns) + kUmiRowWords * 4u;
  uint8_t* const s_tail = s_head + stride;
  const uint32_t n = min(L, min(P.window, stride));
  stage_end(s_head, rd, L, 0u, n, false, lane, 64u);
  stage_end(s_tail, rd, L, 0u, n, true, lane, 64u);
  __syncthreads();
  const uint64_t keyHead = wave_min_u64(umi_search_lane(s_head, n, P, lane));
  const uint64_t keyTail = wave_min_u64(umi_search_lane(s_tail, n, P, lane));
  const UmiPick pk = umi_pick(keyHead, keyTail, P.k);
  if (lane == 0) {
    uint32_t start = 0u;
    if (pk.end) {
      const uint8_t* const s = pk.end == 1u ? s_head : s_tail;
      const uint32_t j0 = umi_recompute(s, P, pk.stop, s_cols);
      start = umi_traceback(s, P, pk.stop, j0, s_cols, s_row->umi);
    } else {
      for (uint32_t x = 0; x < kUmiMaxDegenerate; ++x) s_row->umi[x] = (char)0;
    }
    uint32_t head = 0u, tail = 0u;
    if (ends) {
      const EndRow e = ends[r];
      head = min(e.headAdapterLen + e.headPolyLen, L); tail = e.tailAdapterLen + e.tailPolyLen;
    }
    umi_row_fill(*s_row, pk, start, P.u, L, head, tail);
  }
  __syncthreads();
  if (lane < kUmiRowWords) ((uint32_t*)(rows + r))[lane] = ((const uint32_t*)s_row)[lane];
}
#endif

}  // namespace talc
