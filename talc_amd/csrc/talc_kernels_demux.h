// talc_kernels_demux.h — barcode demultiplexing of long reads (docs/demux.md): every read's sample barcode called from the
// raw bytes of a batch.  B barcodes of one length m, bound k = floor(max_error_pct m / 100).  For a read S of L bytes the end
// rule E(S) is
//   T = S[0, min(L, window)); D_b[e] (e = 1 .. |T|) = the Sellers distance of barcode b against the substrings of T that end
//   at e; d_b = min_e D_b[e] (m when T is empty), c_b = min(d_b, k + 1); best = the b with the smallest c_b, the lowest index
//   among ties, accepted when c_best <= k: err = c_best, end = the largest e with D_best[e] = d_best, margin = (min over
//   b != best of c_b, k + 1 when B = 1) - err; the end calls best when it is accepted and margin >= min_margin;
// the head is E(S), the tail E(revcomp(S)): the codes are read back to front and complemented, the reverse complement is never
// written anywhere, and one table of match masks serves both ends.  k_read_demux leaves one 16-byte talc_demux_row per read.
//
// The lane code (one pattern — an end and a barcode — over one chunk of columns) is TALC_HD: k_read_demux runs 64 lanes of
// it per pass, demux_scan_host (pure_capi.cpp, the CPU test-suite) runs the same lanes one after another.
#pragma once
#include <cstdio>
#include <cstring>

#include "talc_sellers.h"
#if defined(__HIPCC__)
#include "talc_wave.h"
#endif

namespace talc {

constexpr uint32_t kDemuxMaxBarcodes = 96, kDemuxMaxWindow = 4096, kDemuxDefaultWindow = 256;
constexpr uint32_t kDemuxMaxSlots = 192;   // 2 * kDemuxMaxBarcodes, three passes of a wave
static_assert(kDemuxMaxBarcodes <= 128, "k_read_demux reduces two barcodes per lane");

struct DemuxRow {   // talc_demux_row
  uint8_t barcode, status, headBest, headErr, headMargin, tailBest, tailErr, tailMargin;
  uint32_t headEnd, tailEnd;
};
enum : uint32_t { DEMUX_NONE = 0, DEMUX_BOTH = 1, DEMUX_HEAD_ONLY = 2, DEMUX_TAIL_ONLY = 3, DEMUX_CONFLICT = 4 };

// The setting as the kernel takes it, by value: everything in it is wave-uniform.  The match masks are not in it: they are
// a table of nBarcodes x 4 words in device memory (peq[4 b + c]: bit i set when letter i of barcode b has code c).
struct DemuxParams { uint32_t nBarcodes, m, k, minMargin, window, bothEnds; };

// ------------------------------------------------------------------ how a wave is dealt over the patterns
// There are 2 B patterns (end, barcode) and 64 lanes.  A slot is a lane of a pass: slot = 64 pass + lane.
//   B <= 16 (2 B <= 32): one pass; every pattern gets chunks = floor(64 / 2 B) lanes, each one chunk of the window behind a
//     warm-up of m + k columns (sellers_lane's argument); slot = (end B + b) chunks + q.
//   B >= 17: a lane takes a whole window, no warm-up.  The heads' patterns are slots 0 .. B - 1, the tails' start at
//     tailSlot = B rounded up to 32, so no 32-lane half of a pass holds patterns of both ends: the LDS serves byte reads by
//     halves of the wave and broadcasts equal addresses, and every half reads one byte per column.  The rounding never costs
//     a pass: with B = 32 q + r, 0 < r < 32, both 2 B and tailSlot + B need q + 1 passes.
struct DemuxGeometry { uint32_t chunks, passes, tailSlot; };
TALC_HD DemuxGeometry demux_geometry(uint32_t B) {
  DemuxGeometry g;
  if (2u * B <= 32u) { g.chunks = 64u / (2u * B); g.passes = 1u; g.tailSlot = B * g.chunks; return g; }
  g.chunks = 1u;
  g.tailSlot = (B + 31u) / 32u * 32u;
  g.passes = (g.tailSlot + B + 63u) / 64u;
  return g;
}
// the pattern and the chunk of a slot; *b >= B: the slot is idle
TALC_HD void demux_slot_place(const DemuxGeometry& g, uint32_t B, uint32_t slot, uint32_t* end, uint32_t* b, uint32_t* q) {
  *end = slot >= g.tailSlot ? 1u : 0u;
  const uint32_t at = slot - (*end ? g.tailSlot : 0u);
  *b = at / g.chunks; *q = at % g.chunks;
  if (!*end && slot >= B * g.chunks) *b = B;     // (between the heads' last slot and tailSlot)
}
// the first slot of pattern (end, b): its chunks are the g.chunks slots from there
TALC_HD uint32_t demux_pattern_slot(const DemuxGeometry& g, uint32_t end, uint32_t b) { return (end ? g.tailSlot : 0u) + b * g.chunks; }

// The kernel's LDS: one 8-byte key per slot, then the codes of the two end windows, each window rounded up to 16 bytes
// (at most 4096).  2048 bytes at the default window with 96 barcodes, 9728 at the largest window.
TALC_HD uint32_t demux_code_stride(const DemuxParams& P) {
  const uint32_t w = P.window < kDemuxMaxWindow ? P.window : kDemuxMaxWindow;
  return (w + 15u) & ~15u;
}
TALC_HD uint32_t demux_lds_bytes(const DemuxParams& P) { return demux_geometry(P.nBarcodes).passes * 64u * 8u + 2u * demux_code_stride(P); }

// a pattern's key (sellers_lane) from its slots' keys (`key`: one per slot, in LDS or on the host): the smallest over its
// chunks, sellers_no_key(k) without a column of D <= k
TALC_HD uint64_t demux_pattern_key(const uint64_t* key, const DemuxGeometry& g, uint32_t end, uint32_t b, uint32_t k) {
  uint64_t pk = sellers_no_key(k);
  const uint32_t first = demux_pattern_slot(g, end, b);
  for (uint32_t q = 0; q < g.chunks; ++q) { const uint64_t x = key[first + q]; pk = x < pk ? x : pk; }
  return pk;
}
// ... as the candidate the barcodes of an end are reduced by: c << 40 | b << 32 | (0xFFFFFFFF - e)
TALC_HD uint64_t demux_candidate(uint64_t pk, uint32_t b) { return (pk >> 32) << 40 | (uint64_t)b << 32 | (uint32_t)pk; }

// What the barcodes of one end reduce to, and the end rule on it
struct DemuxEnd { uint32_t best, err, margin, end, call; };
// bestC, bestB (0-based), bestE: the smallest c_b, its lowest b and that barcode's end; second: the smallest c_b of the others
TALC_HD DemuxEnd demux_end_rule(uint32_t bestC, uint32_t bestB, uint32_t bestE, uint32_t second, const DemuxParams& P) {
  DemuxEnd r = {0u, 0u, 0u, 0u, 0u};
  if (bestC > P.k) return r;
  r.best = bestB + 1u; r.err = bestC; r.end = bestE;
  r.margin = second - bestC;                           // (second >= bestC: bestC is the smallest)
  r.call = r.margin >= P.minMargin ? r.best : 0u;
  return r;
}
// the read call from its two ends
TALC_HD DemuxRow demux_row(const DemuxEnd& h, const DemuxEnd& t, const DemuxParams& P) {
  DemuxRow row;
  row.headBest = (uint8_t)h.best; row.headErr = (uint8_t)h.err; row.headMargin = (uint8_t)h.margin; row.headEnd = h.end;
  row.tailBest = (uint8_t)t.best; row.tailErr = (uint8_t)t.err; row.tailMargin = (uint8_t)t.margin; row.tailEnd = t.end;
  uint32_t barcode = 0u, status = DEMUX_NONE;
  if (h.call && h.call == t.call) { barcode = h.call; status = DEMUX_BOTH; }
  else if (h.call && t.call) status = DEMUX_CONFLICT;
  else if (h.call) { barcode = P.bothEnds ? 0u : h.call; status = DEMUX_HEAD_ONLY; }
  else if (t.call) { barcode = P.bothEnds ? 0u : t.call; status = DEMUX_TAIL_ONLY; }
  row.barcode = (uint8_t)barcode; row.status = (uint8_t)status;
  return row;
}

// ------------------------------------------------------------------ the setting from its text (the library and the CPU suite)
// barcodes: comma-separated.  False and a message in `why` when a value is refused; nothing is written then: the masks are
// built apart and copied into `peq` only once every value has passed, so a refused setting leaves the caller's table as it
// was.  Of several bad values the one named is the first in this order: max_error_pct, window, both_ends, the barcodes in
// the order given, min_margin (it depends on their length).  An empty or null text is the setting switched off:
// P.nBarcodes = 0.  peq: kDemuxMaxBarcodes x 4 words.
inline bool demux_make_setting(const char* barcodes, uint32_t max_error_pct, uint32_t min_margin, uint32_t window, int both_ends, DemuxParams& P,
                               uint64_t* peq, char* why, size_t whyLen) {
  DemuxParams Q = {0u, 0u, 0u, 0u, 0u, 0u};
  if (!barcodes || !*barcodes) { P = Q; return true; }
  if (max_error_pct > 30) { snprintf(why, whyLen, "max_error_pct=%u: at most 30", max_error_pct); return false; }
  if (!window) window = kDemuxDefaultWindow;
  if (window < 32 || window > kDemuxMaxWindow) { snprintf(why, whyLen, "window=%u: 32 .. %u (0: %u)", window, kDemuxMaxWindow, kDemuxDefaultWindow); return false; }
  if (both_ends != 0 && both_ends != 1) { snprintf(why, whyLen, "both_ends=%d: 0 or 1", both_ends); return false; }
  uint64_t masks[kDemuxMaxBarcodes * 4];
  memset(masks, 0, sizeof masks);
  for (PatternList it(barcodes); it.next(acgt_set);) {
    const unsigned long long m = it.m;
    if (Q.nBarcodes == kDemuxMaxBarcodes) { snprintf(why, whyLen, "barcodes: more than %u", kDemuxMaxBarcodes); return false; }
    if (it.fault == PATTERN_LENGTH) { snprintf(why, whyLen, "barcodes: barcode %u has %llu letters: 12 .. 64", Q.nBarcodes + 1, m); return false; }
    if (Q.nBarcodes && m != Q.m) {
      snprintf(why, whyLen, "barcodes: barcode %u has %llu letters, barcode 1 has %u: one length for all", Q.nBarcodes + 1, m, Q.m);
      return false;
    }
    if (it.fault) { snprintf(why, whyLen, "barcodes: barcode %u has a letter that is not one of ACGTacgt", Q.nBarcodes + 1); return false; }
    pattern_masks(it.p, it.m, acgt_set, false, false, masks + 4u * Q.nBarcodes);
    Q.m = (uint32_t)m;
    ++Q.nBarcodes;
  }
  Q.k = max_error_pct * Q.m / 100u;
  if (min_margin > Q.k + 1u) { snprintf(why, whyLen, "min_margin=%u: 0 .. k + 1 (%u)", min_margin, Q.k + 1u); return false; }
  Q.minMargin = min_margin; Q.window = window; Q.bothEnds = (uint32_t)both_ends;
  P = Q;
  memcpy(peq, masks, sizeof masks);
  return true;
}

// ------------------------------------------------------------------ the kernel's walk on the host, lanes one after another
inline DemuxRow demux_scan_host(const uint8_t* rd, uint32_t L, const DemuxParams& P, const uint64_t* peqTable) {
  const uint32_t B = P.nBarcodes, window = P.window < kDemuxMaxWindow ? P.window : kDemuxMaxWindow;
  const uint32_t n = L < window ? L : window;
  const DemuxGeometry g = demux_geometry(B);
  static thread_local uint8_t code[2][kDemuxMaxWindow];
  for (uint32_t end = 0; end < 2u; ++end) stage_end(code[end], rd, L, 0u, n, end == 1u, 0u, 1u);
  uint64_t key[kDemuxMaxSlots];
  for (uint32_t slot = 0; slot < g.passes * 64u; ++slot) {
    uint32_t end, b, q, c0, c1;
    demux_slot_place(g, B, slot, &end, &b, &q);
    key[slot] = ~0ull;
    if (b >= B) continue;
    sellers_chunk(n, g.chunks, q, &c0, &c1);
    const uint64_t peq[4] = {peqTable[4u * b], peqTable[4u * b + 1u], peqTable[4u * b + 2u], peqTable[4u * b + 3u]};
    key[slot] = sellers_lane(code[end], peq, P.m, P.k, c0, c1, sellers_no_key(P.k));
  }
  DemuxEnd ends[2];
  for (uint32_t end = 0; end < 2u; ++end) {
    uint64_t best = ~0ull;                             // c << 40 | b << 32 | (0xFFFFFFFF - e)
    uint32_t cOf[kDemuxMaxBarcodes];
    for (uint32_t b = 0; b < B; ++b) {
      const uint64_t pk = demux_pattern_key(key, g, end, b, P.k);
      cOf[b] = (uint32_t)(pk >> 32);
      const uint64_t cand = demux_candidate(pk, b);
      best = cand < best ? cand : best;
    }
    const uint32_t bestB = (uint32_t)(best >> 32) & 0xFFu;
    uint32_t second = P.k + 1u;
    for (uint32_t b = 0; b < B; ++b) if (b != bestB && cOf[b] < second) second = cOf[b];
    ends[end] = demux_end_rule((uint32_t)(best >> 40), bestB, 0xFFFFFFFFu - (uint32_t)best, second, P);
  }
  return demux_row(ends[0], ends[1], P);
}

#if defined(__HIPCC__)
// One wave per read.  Both end windows are staged once as codes; every pass gives each lane one pattern (and chunk), whose
// key goes to LDS; then, per end, the lanes reduce the chunks of their barcodes and the wave the barcodes; lane 0 applies the
// call rule and writes the row.  peqTable: P.nBarcodes x 4 words.
__global__ void __launch_bounds__(64)
k_read_demux(const uint8_t* __restrict__ raw, const uint64_t* __restrict__ offsets, uint32_t n_reads, const uint64_t* __restrict__ peqTable, DemuxParams P,
             DemuxRow* __restrict__ rows) {
  extern __shared__ uint64_t s_demux[];                // demux_lds_bytes(P): the slots' keys, then the two windows' codes
  const uint32_t r = blockIdx.x, B = P.nBarcodes;
  if (r >= n_reads || B == 0u || B > kDemuxMaxBarcodes || P.m < 1u || P.m > 64u) return;
  const uint32_t lane = threadIdx.x;
  const uint64_t rb = offsets[r];
  const uint32_t L = (uint32_t)(offsets[r + 1] - rb);
  const uint8_t* const rd = raw + rb;
  const DemuxGeometry g = demux_geometry(B);
  const uint32_t stride = demux_code_stride(P);
  uint64_t* const s_key = s_demux;
  uint8_t* const s_head = (uint8_t*)(s_demux + g.passes * 64u);
  uint8_t* const s_tail = s_head + stride;
  const uint32_t n = min(L, min(P.window, stride));
  stage_end(s_head, rd, L, 0u, n, false, lane, 64u);
  stage_end(s_tail, rd, L, 0u, n, true, lane, 64u);
  __syncthreads();
  for (uint32_t pass = 0; pass < g.passes; ++pass) {
    const uint32_t slot = pass * 64u + lane;           // < kDemuxMaxSlots: passes <= 3
    uint32_t end, b, q, c0, c1;
    demux_slot_place(g, B, slot, &end, &b, &q);
    uint64_t key = ~0ull;
    if (b < B) {
      sellers_chunk(n, g.chunks, q, &c0, &c1);
      const uint64_t peq[4] = {peqTable[4u * b], peqTable[4u * b + 1u], peqTable[4u * b + 2u], peqTable[4u * b + 3u]};
      key = sellers_lane(end ? s_tail : s_head, peq, P.m, P.k, c0, c1, sellers_no_key(P.k));
    }
    s_key[slot] = key;
  }
  __syncthreads();
  DemuxEnd ends[2];
#pragma unroll
  for (uint32_t end = 0; end < 2u; ++end) {
    uint64_t best = ~0ull;                             // demux_candidate
    uint32_t cOf[2] = {P.k + 1u, P.k + 1u};            // c of the lane's barcodes lane, lane + 64 (B <= 96: two at most)
#pragma unroll
    for (uint32_t i = 0; i < 2u; ++i) {
      const uint32_t b = lane + 64u * i;
      if (b >= B) continue;
      const uint64_t pk = demux_pattern_key(s_key, g, end, b, P.k);
      cOf[i] = (uint32_t)(pk >> 32);
      best = min(best, demux_candidate(pk, b));
    }
    best = wave_min_u64(best);
    const uint32_t bestB = (uint32_t)(best >> 32) & 0xFFu;
    uint64_t second = P.k + 1u;
#pragma unroll
    for (uint32_t i = 0; i < 2u; ++i)
      if (lane + 64u * i < B && lane + 64u * i != bestB) second = min(second, (uint64_t)cOf[i]);
    second = wave_min_u64(second);
    ends[end] = demux_end_rule((uint32_t)(best >> 40), bestB, 0xFFFFFFFFu - (uint32_t)best, (uint32_t)second, P);
  }
  if (lane == 0) rows[r] = demux_row(ends[0], ends[1], P);
}
#endif

}  // namespace talc
