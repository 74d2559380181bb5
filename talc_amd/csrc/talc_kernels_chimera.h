// talc_kernels_chimera.h — internal primers of chimeric long reads (docs/chimeras.md): every adapter of the end clean-up,
// on both strands, searched over the whole read.  For pattern P of m letters and a read S of L bytes, D[e] (e = 1 .. L) is
// the Sellers distance of P against the substrings of S that end at e, C[e] = min(D[e], k_a + 1), w = ceil(m / 2), and e is
// a hit end when C[e] <= k_a, C[e] < C[e'] for e < e' <= min(L, e + w), and C[e] <= C[e'] for max(1, e - w) <= e' < e.  The
// hit starts at e - j*, j* the smallest j for which the global edit distance of P and S[e - j, e) is D[e].
//
// The lane code (one pattern over one chunk of columns) is TALC_HD: k_read_chimera runs 64 lanes of it per read, and
// chimera_scan_host (pure_capi.cpp, the CPU test-suite) runs the same lanes one after another over the same tiles.
#pragma once
#include "talc_chimera_plan.h"
#include "talc_sellers.h"
#if defined(__HIPCC__)
#include "talc_wave.h"
#endif

namespace talc {

// One lane: pattern `peq` (m letters, bound k) over the columns (js, jend] of a read, of which it owns (c0, c1].  It starts
// w + m + k columns before its chunk from the free-start state (sellers_lane's proof: from m + k columns on its clamped
// scores are exact) and runs w columns beyond it, so that it knows C exactly on [c0 + 1 - w, c1 + w]: all the hit rule reads
// for the columns it owns.  C moves by at most 1 per column, so the last 64 columns are two bit masks (up, dn: bit i is the
// step into column t - i); `delayed` is C[tick - w], the column whose window has just been completed.
struct ChimeraLane {
  SellersColumn col;   // column tick - 1
  uint64_t up, dn;
  uint32_t m, k, w, clamped, delayed;
  uint32_t js, jend, c0, c1;
  uint32_t tick;       // the next tick: column `tick` is computed (while tick <= jend), column tick - w is tested
  uint32_t ticks;      // how many this lane runs
};

TALC_HD void chimera_lane_init(ChimeraLane& s, uint32_t m, uint32_t k, uint32_t L, uint32_t c0, uint32_t c1) {
  s.m = m; s.k = k; s.w = (m + 1u) / 2u;
  const uint32_t pre = s.w + m + k;
  s.c0 = c0; s.c1 = c1;
  s.js = c0 > pre ? c0 - pre : 0u;
  s.jend = c1 + s.w < L ? c1 + s.w : L;
  s.col.start(m);
  s.up = s.dn = 0ull;
  s.clamped = s.delayed = k + 1u;     // column js (and everything outside the read) counts as k + 1: it forbids nothing
  s.tick = s.js + 1u;
  s.ticks = c0 < c1 ? c1 + s.w - s.js : 0u;
}

// the hit rule for column e with C[e] = ce, the masks standing at column t = min(e + w, jend)
TALC_HD bool chimera_hit_test(uint64_t up, uint64_t dn, uint32_t t, uint32_t e, uint32_t ce, uint32_t w) {
  int32_t cur = (int32_t)ce;
  for (uint32_t i = 0; i < w; ++i) {                     // e' = e - 1 - i, down to max(1, e - w)
    const uint32_t col = e - i;
    if (col <= 1u) break;
    const uint32_t idx = t - col;                        // <= 2 w - 1 <= 63
    cur -= (int32_t)((up >> idx) & 1u) - (int32_t)((dn >> idx) & 1u);
    if (cur < (int32_t)ce) return false;
  }
  cur = (int32_t)ce;
  for (uint32_t col = e + 1u; col <= t; ++col) {         // e' up to min(L, e + w)
    const uint32_t idx = t - col;
    cur += (int32_t)((up >> idx) & 1u) - (int32_t)((dn >> idx) & 1u);
    if (cur <= (int32_t)ce) return false;
  }
  return true;
}

// One tick.  `code` is the code of byte tick - 1 of the read (read only while tick <= jend).  True when column tick - w is
// a hit end that this lane owns: *end and *err are then that column and its D.
TALC_HD bool chimera_lane_tick(ChimeraLane& s, const uint64_t (&peq)[4], uint32_t code, uint32_t* end, uint32_t* err) {
  const uint32_t tau = s.tick++;
  if (tau <= s.jend) {
    s.col.step(sellers_eq(peq, code), s.m);
    const uint32_t nc = s.col.score < s.k + 1u ? s.col.score : s.k + 1u;
    s.up = s.up << 1 | (nc > s.clamped ? 1ull : 0ull);
    s.dn = s.dn << 1 | (nc < s.clamped ? 1ull : 0ull);
    s.clamped = nc;
  }
  if (tau <= s.js + s.w) return false;                   // column tau - w is not one of this lane's
  const uint32_t t = tau < s.jend ? tau : s.jend, e = tau - s.w, idx = t - e;   // (e <= c1 <= jend; idx <= w)
  s.delayed += (uint32_t)((s.up >> idx) & 1u) - (uint32_t)((s.dn >> idx) & 1u);
  if (e <= s.c0 || s.delayed > s.k) return false;
  if (!chimera_hit_test(s.up, s.dn, t, e, s.delayed, s.w)) return false;
  *end = e; *err = s.delayed;
  return true;
}

// The start of the hit that ends at column e with distance d: the same recurrence anchored at e (the top row is j), the
// pattern back to front over the read's bytes e - 1, e - 2, ...; the first column whose score is d.
// code_at(i) is the code of byte i of the read; at most m + k bytes are read, none below 0.
template <class CodeAt>
TALC_HD uint32_t chimera_start(CodeAt code_at, uint32_t e, const uint64_t (&peqRev)[4], uint32_t m, uint32_t k, uint32_t d) {
  SellersColumn col;
  col.start(m);
  const uint32_t far = e < m + k ? e : m + k;
  for (uint32_t j = 1; j <= far; ++j) {
    col.step<false>(sellers_eq(peqRev, code_at(e - j)), m);
    if (col.score == d) return e - j;
  }
  return e - far;   // (never: some j <= m + d has that distance, by the definition of D)
}

// where lane `lane` of the wave works in the tile that starts at column tb: its pattern (>= nPatterns: none) and its chunk
TALC_HD void chimera_lane_place(const ChimeraGeometry& g, uint32_t lane, uint32_t tb, uint32_t L, uint32_t* pattern, uint32_t* c0, uint32_t* c1) {
  *pattern = lane / g.lanesPerPattern;
  const uint64_t at = (uint64_t)tb + (uint64_t)(lane % g.lanesPerPattern) * g.chunk;
  *c0 = at < L ? (uint32_t)at : L;
  *c1 = at + g.chunk < L ? (uint32_t)(at + g.chunk) : L;
}
// the bytes of the read a tile stages: [*sb, *se), at most kChimeraStage
TALC_HD void chimera_tile_stage(const ChimeraGeometry& g, uint32_t tb, uint32_t L, uint32_t preMax, uint32_t wMax, uint32_t* sb, uint32_t* se) {
  *sb = tb > preMax ? tb - preMax : 0u;
  const uint64_t end = (uint64_t)tb + g.tile + wMax;
  *se = end < L ? (uint32_t)end : L;
}
TALC_HD void chimera_halos(const ChimeraParams& P, uint32_t* preMax, uint32_t* wMax) {
  uint32_t pre = 0, wm = 0;
  for (uint32_t p = 0; p < P.nPatterns && p < kChimeraMaxPatterns; ++p) {
    const uint32_t w = (P.m[p] + 1u) / 2u, x = w + P.m[p] + P.k[p];
    pre = x > pre ? x : pre; wm = w > wm ? w : wm;
  }
  *preMax = pre; *wMax = wm;
}

// The kernel's walk on the host, lanes one after another: the hits of one read (`read` goes into the records), appended in
// the lanes' order.  The tile is staged as codes exactly as the kernel stages it.
inline void chimera_scan_host(const uint8_t* rd, uint32_t L, uint32_t read, const ChimeraParams& P, std::vector<ChimeraHit>& out) {
  if (!P.nPatterns || !L) return;
  const ChimeraGeometry g = chimera_geometry(L, P.nPatterns);
  uint32_t preMax, wMax;
  chimera_halos(P, &preMax, &wMax);
  std::vector<uint8_t> stage(kChimeraStage);
  for (uint64_t tb64 = 0; tb64 < L; tb64 += g.tile) {
    const uint32_t tb = (uint32_t)tb64;
    uint32_t sb, se;
    chimera_tile_stage(g, tb, L, preMax, wMax, &sb, &se);
    for (uint32_t i = 0; i < se - sb; ++i) stage.at(i) = (uint8_t)ascii_to_code_select(rd[sb + i]);
    for (uint32_t lane = 0; lane < 64u; ++lane) {
      uint32_t p, c0, c1;
      chimera_lane_place(g, lane, tb, L, &p, &c0, &c1);
      if (p >= P.nPatterns) continue;
      ChimeraLane s;
      chimera_lane_init(s, P.m[p], P.k[p], L, c0, c1);
      for (uint32_t n = 0; n < s.ticks; ++n) {
        const uint32_t code = s.tick <= s.jend ? stage.at(s.tick - 1u - sb) : 4u;
        uint32_t e, d;
        if (!chimera_lane_tick(s, P.peq[p], code, &e, &d)) continue;
        const uint32_t start = chimera_start([&](uint32_t i) { return (uint32_t)stage.at(i - sb); }, e, P.peqRev[p], P.m[p], P.k[p], d);
        out.push_back(ChimeraHit{read, start, e, (uint8_t)(p / 2u + 1u), (uint8_t)(p & 1u), (uint8_t)d, 0});
      }
    }
  }
}

#if defined(__HIPCC__)
// One wave per read.  The lanes tick together (a lane reads LDS at its chunk's place plus the common tick); a tick on which
// some lane found a hit end is rare: those lanes then find their starts, and the wave appends its hits behind one atomic add.
// *count counts every hit; those below `capacity` are written.
__global__ void __launch_bounds__(64)
k_read_chimera(const uint8_t* __restrict__ raw, const uint64_t* __restrict__ offsets, uint32_t n_reads, ChimeraParams P,
               ChimeraHit* __restrict__ hits, uint32_t capacity, uint32_t* __restrict__ count) {
  __shared__ uint8_t s_code[kChimeraStage];
  const uint32_t r = blockIdx.x;
  if (r >= n_reads || P.nPatterns == 0u || P.nPatterns > kChimeraMaxPatterns) return;
  const uint32_t lane = threadIdx.x;
  const uint64_t rb = offsets[r];
  const uint32_t L = (uint32_t)(offsets[r + 1] - rb);
  const uint8_t* const rd = raw + rb;
  const ChimeraGeometry g = chimera_geometry(L, P.nPatterns);
  uint32_t preMax, wMax;
  chimera_halos(P, &preMax, &wMax);
  const uint32_t pat = lane / g.lanesPerPattern;
  uint64_t peq[4] = {0, 0, 0, 0}, peqRev[4] = {0, 0, 0, 0};
  uint32_t m = 12u, k = 0u;
#pragma unroll
  for (uint32_t p = 0; p < kChimeraMaxPatterns; ++p)     // (the setting is indexed by constants only: it stays in scalar registers)
    if (p == pat && p < P.nPatterns) {
#pragma unroll
      for (int c = 0; c < 4; ++c) { peq[c] = P.peq[p][c]; peqRev[c] = P.peqRev[p][c]; }
      m = P.m[p]; k = P.k[p];
    }
  for (uint64_t tb64 = 0; tb64 < L; tb64 += g.tile) {
    const uint32_t tb = (uint32_t)tb64;
    uint32_t sb, se;
    chimera_tile_stage(g, tb, L, preMax, wMax, &sb, &se);
    const uint32_t staged = min(se - sb, (uint32_t)kChimeraStage);
    for (uint32_t i = lane; i < staged; i += 64u) s_code[i] = (uint8_t)ascii_to_code_select(rd[sb + i]);
    __syncthreads();
    uint32_t p_, c0, c1;
    chimera_lane_place(g, lane, tb, L, &p_, &c0, &c1);
    if (pat >= P.nPatterns) c1 = c0;
    ChimeraLane s;
    chimera_lane_init(s, m, k, L, c0, c1);
    const uint32_t most = wave_max_u32(s.ticks);
    for (uint32_t n = 0; n < most; ++n) {
      bool hit = false;
      uint32_t e = 0, d = 0;
      if (n < s.ticks) {
        const uint32_t at = s.tick - 1u - sb;
        const uint32_t code = s.tick <= s.jend && at < staged ? s_code[at] : 4u;
        hit = chimera_lane_tick(s, peq, code, &e, &d);
      }
      const uint64_t found = __ballot(hit);
      if (found) {                                       // (wave-uniform)
        uint32_t start = 0;
        if (hit) start = chimera_start([&](uint32_t i) { const uint32_t a = i - sb; return a < staged ? (uint32_t)s_code[a] : 4u; }, e, peqRev, m, k, d);
        const uint32_t leader = (uint32_t)__ffsll((unsigned long long)found) - 1u;
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(count, (uint32_t)__popcll(found));
        base = (uint32_t)__shfl((int)base, (int)leader, 64);
        const uint32_t slot = base + (uint32_t)__popcll(found & ((1ull << lane) - 1ull));
        if (hit && slot < capacity && slot >= base) hits[slot] = ChimeraHit{r, start, e, (uint8_t)(pat / 2u + 1u), (uint8_t)(pat & 1u), (uint8_t)d, 0};
      }
    }
    __syncthreads();                                     // (the next tile is staged into the same bytes)
  }
}
#endif

}  // namespace talc
