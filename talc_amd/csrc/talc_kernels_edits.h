// talc_kernels_edits.h — the edit scripts of a correction (docs/correction_edits.md): for every read of a corrected batch
// the run-length list of =, X, I, D operations that turns the read as the caller gave it into its record, from the
// correction map (k_pack_map's talc_segment array).  A SOLID or RAW segment is out_len matches and nothing is compared; a
// CORRECTED segment is aligned, raw stretch against record stretch, under unit costs, and its part of the script is the
// canonical traceback: from the far corner, the diagonal when it is optimal, else a deletion (a raw base is consumed)
// when that is optimal, else an insertion.  A pair of more than max_cells cells is not aligned: raw_len D, then out_len I.
//   k_edit_align  one wave per CORRECTED segment that needs a DP: Myers / Hyyro bit vectors with every column's delta
//                 words kept (4 bits per cell), then the traceback over those words.  Run twice: the first run leaves the
//                 part's summary (EditPart), the second writes the part's runs where k_edit_count said they go.
//   k_edit_count  one wave per read over its segments, 64 per pass: the read's six totals (talc_edit_row), and for every
//                 segment the index of the op that holds its first run (parts merge where the last op of one equals the
//                 first op of the next non-empty one).
//   k_edit_pack   the same walk again: writes the runs of the parts that needed no DP.
// Runs are added into a zeroed op array (len << 4 | code): the part that opens an op adds its code with its length, a part
// whose first run merges into the op before it adds the length alone.  Integer adds commute, so the result does not
// depend on the order in which the waves arrive.
#pragma once
#include "talc_edit_plan.h"
#include "talc_kernels_search.h"   // MapSeg, SEG_*
#include "talc_wave.h"

namespace talc {

enum : uint32_t { EDIT_I = 1, EDIT_D = 2, EDIT_EQ = 7, EDIT_X = 8 };   // BAM's CIGAR codes
struct EditRow { uint32_t nMatch, nMismatch, nIns, nDel, nOps, nUnaligned; };   // talc_edit_row
// what a DP leaves of a segment's part, and where k_edit_count puts it
struct EditPart {
  uint32_t nRuns;        // runs of the part on its own (>= 1: a DP part is never empty)
  uint32_t ends;         // first op code | last op code << 8 | (k_edit_count) "the first run merges into the op before" << 16
  uint32_t cnt[4];       // bases in =, X, I, D runs
  uint32_t opBase;       // (k_edit_count) run r of the part belongs to op opBase + r of its read
  int32_t distance;      // the DP's edit distance (equals cnt[1] + cnt[2] + cnt[3]: held against it by the tests)
};
// One wave aligns a = raw[0, n) with b = rec[0, m) (ASCII, compared as Dna5 codes: N equals N), n, m > 0, and walks the
// canonical path back.  `store` holds the delta words (LDS or global, edit_scratch_words(n, m) of them).  emit(code, len,
// k) is called, wave-uniformly, once per run, last run first: k counts the runs from the end.  Returns the part's summary.
//
// Forward (wave_edit_bitpar's recurrences): pattern P = the longer of a and b, np positions, bit i of word w = position
// 64 w + i, lane l of block blk holds word 64 blk + l; text T = the other, consumed base by base.  After column t the
// words Pv, Mv hold the vertical deltas D[p][t] - D[p - 1][t] of every pattern position p (bit p - 1), and Ph, Mh — as
// they are before the shift — the horizontal deltas D[p][t] - D[p][t - 1]; row 0 has the horizontal delta +1.  All four
// are kept: store[(t nw + w) 4 + {0, 1, 2, 3}] = Pv, Mv, Ph, Mh.
//
// Back from (np, nt): with dv the vertical delta of (p, t) and dh' the horizontal delta of (p - 1, t),
// D[p][t] - D[p - 1][t - 1] = dv + dh', so the diagonal is optimal exactly when dv + dh' == (P[p - 1] != T[t - 1]).  A
// deletion consumes a base of a: it is optimal when the delta along a is +1 — dv when a is the pattern, the horizontal
// delta of (p, t) when a is the text.  No distance is carried: the rule needs deltas only.
template <typename Emit>
TALC_D EditPart wave_edit_trace(const uint8_t* a, uint32_t n, const uint8_t* b, uint32_t m, uint64_t* store, Emit emit) {
  const bool aIsPat = n >= m;
  const uint8_t* const pat = aIsPat ? a : b;
  const uint8_t* const txt = aIsPat ? b : a;
  const uint32_t np = aIsPat ? n : m, nt = aIsPat ? m : n;
  const uint32_t nw = (np + 63u) / 64u, ntw = (nt + 63u) / 64u;
  const uint32_t nblk = (np + kEditBlock - 1u) / kEditBlock;
  uint64_t* const work = store + 4ull * nw * nt;     // the carries between blocks: ntw words of +1, ntw words of -1
  const uint32_t l = threadIdx.x;
  const uint64_t laneBit = 1ull << l;
  int32_t score = (int32_t)np;
  for (uint32_t blk = 0; blk < nblk; ++blk) {
    const uint32_t w = 64u * blk + l, p0 = 64u * w;
    const bool lastBlk = blk + 1u == nblk;
    uint64_t pm[5] = {0ull, 0ull, 0ull, 0ull, 0ull};
    if (p0 < np) {
      const uint32_t cnt = min(64u, np - p0);
      for (uint32_t i = 0; i < cnt; ++i) {
        const uint32_t c = ascii_to_code(pat[p0 + i]);
#pragma unroll
        for (uint32_t k = 0; k < 5; ++k) pm[k] |= (c == k ? 1ull : 0ull) << i;
      }
    }
    const uint32_t topPos = lastBlk ? np - 1u - kEditBlock * blk : kEditBlock - 1u, topLane = topPos >> 6, topBit = topPos & 63u;
    uint64_t Pv = ~0ull, Mv = 0ull;
    for (uint32_t t0 = 0; t0 < nt; t0 += 64u) {
      const uint32_t tn = min(64u, nt - t0);
      const int tvec = l < tn ? (int)ascii_to_code(txt[t0 + l]) : 0;
      const uint64_t hinP = blk > 0 ? work[t0 >> 6] : ~0ull, hinM = blk > 0 ? work[ntw + (t0 >> 6)] : 0ull;
      uint64_t outP = 0, outM = 0;
      for (uint32_t tt = 0; tt < tn; ++tt) {
        const int c = lane_get(tvec, (int)tt);
        const uint64_t Eq = c == 0 ? pm[0] : c == 1 ? pm[1] : c == 2 ? pm[2] : c == 3 ? pm[3] : pm[4];
        const uint32_t hp = (uint32_t)((hinP >> tt) & 1ull), hm = (uint32_t)((hinM >> tt) & 1ull);
        const uint64_t Xv = Eq | Mv;
        const uint64_t Eqx = Eq | ((l == 0u && hm) ? 1ull : 0ull);   // a -1 entering the block's first row acts like a match there
        const uint64_t Xa = Eqx & Pv;
        uint64_t S = Xa + Pv;
        const uint64_t G = ballot64(S < Pv), P = ballot64(S == ~0ull);
        const uint64_t Y = G << 1;
        const uint64_t C = ((Y + P) ^ P) | Y;
        S += (C & laneBit) ? 1ull : 0ull;
        const uint64_t Xh = (S ^ Pv) | Eqx;
        const uint64_t Ph = Mv | ~(Xh | Pv);
        const uint64_t Mh = Pv & Xh;
        const uint64_t up = ballot64(l == topLane && ((Ph >> topBit) & 1ull)), dn = ballot64(l == topLane && ((Mh >> topBit) & 1ull));
        if (lastBlk) { score += up != 0ull ? 1 : 0; score -= dn != 0ull ? 1 : 0; }
        else { outP |= (up != 0ull ? 1ull : 0ull) << tt; outM |= (dn != 0ull ? 1ull : 0ull) << tt; }
        int pTop = (int)(Ph >> 63), mTop = (int)(Mh >> 63);
        pTop = lane_shr1(pTop); mTop = lane_shr1(mTop);
        if (l == 0u) { pTop = (int)hp; mTop = (int)hm; }
        const uint64_t Phs = (Ph << 1) | (uint64_t)(uint32_t)pTop;
        const uint64_t Mhs = (Mh << 1) | (uint64_t)(uint32_t)mTop;
        Pv = Mhs | ~(Xv | Phs);
        Mv = Phs & Xv;
        if (w < nw) {
          uint64_t* const o = store + ((uint64_t)(t0 + tt) * nw + w) * 4ull;
          o[0] = Pv; o[1] = Mv; o[2] = Ph; o[3] = Mh;
        }
      }
      if (!lastBlk && l == 0u) { work[t0 >> 6] = outP; work[ntw + (t0 >> 6)] = outM; }
      if (!lastBlk) WSYNC();   // (a later pass of this loop, in the next block, reads what lane 0 wrote)
    }
  }
  WSYNC();   // every lane reads every lane's words below

  // ---- back.  All lanes walk the same path (the values are wave-uniform).
  EditPart part = {0u, 0u, {0u, 0u, 0u, 0u}, 0u, score};
  uint32_t p = np, t = nt, cur = 0, len = 0, lastCode = 0;
  auto step = [&](uint32_t code) {
    if (code != cur) {
      if (len) { emit(cur, len, part.nRuns); part.nRuns += 1u; }
      else lastCode = code;
      cur = code; len = 0;
    }
    len += 1u;
    part.cnt[0] += code == EDIT_EQ ? 1u : 0u; part.cnt[1] += code == EDIT_X ? 1u : 0u;
    part.cnt[2] += code == EDIT_I ? 1u : 0u; part.cnt[3] += code == EDIT_D ? 1u : 0u;
  };
  while (p > 0u && t > 0u) {
    const uint64_t* const o = store + ((uint64_t)(t - 1u) * nw + ((p - 1u) >> 6)) * 4ull;
    const uint32_t bit = (p - 1u) & 63u;
    const uint64_t pv = o[0], mv = o[1], ph = o[2];
    int dhAbove = 1;                                  // the border row
    if (p >= 2u) {
      const uint32_t q = p - 2u;
      const uint64_t* const oq = store + ((uint64_t)(t - 1u) * nw + (q >> 6)) * 4ull;
      dhAbove = (int)((oq[2] >> (q & 63u)) & 1ull) - (int)((oq[3] >> (q & 63u)) & 1ull);
    }
    const int dv = (int)((pv >> bit) & 1ull) - (int)((mv >> bit) & 1ull);
    const uint32_t cp = ascii_to_code(pat[p - 1u]), ct = ascii_to_code(txt[t - 1u]);
    const int neq = cp != ct ? 1 : 0;
    if (dv + dhAbove == neq) { step(neq ? EDIT_X : EDIT_EQ); p -= 1u; t -= 1u; continue; }
    const bool del = aIsPat ? ((pv >> bit) & 1ull) != 0ull : ((ph >> bit) & 1ull) != 0ull;
    step(del ? EDIT_D : EDIT_I);
    // a deletion consumes a base of a, an insertion one of b
    if (del == aIsPat) p -= 1u; else t -= 1u;
  }
  // the border: what is left of a is deleted, what is left of b inserted
  { const uint32_t ra = aIsPat ? p : t, rb = aIsPat ? t : p;
    for (uint32_t i = 0; i < ra; ++i) step(EDIT_D);
    for (uint32_t i = 0; i < rb; ++i) step(EDIT_I); }
  if (len) { emit(cur, len, part.nRuns); part.nRuns += 1u; }
  part.ends = cur | (lastCode << 8);                  // the walk ends at the part's first op
  return part;
}

// adds one run into the op array (see the head of the file)
TALC_D void edit_add_run(uint32_t* ops, uint64_t at, uint64_t end, uint32_t code, uint32_t len, bool opens) {
  if (at < end) atomicAdd(ops + at, (len << 4) | (opens ? code : 0u));
}

// one wave per task.  write == 0: parts[seg] = the part's summary (nRuns, ends, cnt, distance; opBase and the merge bit
// are k_edit_count's).  write != 0: the part's runs into ops, at parts[seg].opBase of the read's ops.
__global__ void __launch_bounds__(64)
k_edit_align(const EditTask* __restrict__ tasks, uint32_t n_tasks, const MapSeg* __restrict__ segs, const uint8_t* __restrict__ raw,
             const uint64_t* __restrict__ raw_off, const uint8_t* __restrict__ records, const uint64_t* __restrict__ dense_off,
             uint64_t* scratch, EditPart* parts, int write, const uint64_t* __restrict__ op_off, uint32_t* ops) {
  __shared__ uint64_t s_words[kEditLdsWords];
  __shared__ uint8_t s_seq[kEditLdsSeq];
  if (blockIdx.x >= n_tasks) return;
  const EditTask task = tasks[blockIdx.x];
  const MapSeg s = segs[task.seg];
  const uint8_t* a = raw + raw_off[task.read] + s.rawStart;
  const uint8_t* b = records + dense_off[task.read] + s.outStart;
  const uint32_t n = s.rawLen, m = s.outLen;
  uint64_t* store = scratch + task.scratchWord;
  if (task.scratchWord == kEditInLds) {     // (wave-uniform) n + m <= kEditLdsSeq: edit_in_lds
    for (uint32_t i = threadIdx.x; i < n; i += 64u) s_seq[i] = a[i];
    for (uint32_t i = threadIdx.x; i < m; i += 64u) s_seq[n + i] = b[i];
    a = s_seq; b = s_seq + n; store = s_words;
    WSYNC();
  }
  if (!write) {
    EditPart part = wave_edit_trace(a, n, b, m, store, [](uint32_t, uint32_t, uint32_t) {});
    if (threadIdx.x == 0) {
      EditPart* const o = parts + task.seg;
      o->nRuns = part.nRuns; o->ends = part.ends; o->distance = part.distance;
      o->cnt[0] = part.cnt[0]; o->cnt[1] = part.cnt[1]; o->cnt[2] = part.cnt[2]; o->cnt[3] = part.cnt[3];
    }
    return;
  }
  const EditPart mine = parts[task.seg];
  const uint64_t o0 = op_off[task.read], o1 = op_off[task.read + 1];
  const bool merges = ((mine.ends >> 16) & 1u) != 0u;
  (void)wave_edit_trace(a, n, b, m, store, [&](uint32_t code, uint32_t len, uint32_t k) {
    if (threadIdx.x == 0u && k < mine.nRuns) {
      const uint32_t r = mine.nRuns - 1u - k;
      edit_add_run(ops, o0 + mine.opBase + r, o1, code, len, !(r == 0u && merges));
    }
  });
}

// One wave walks the segments of one read in order, 64 per pass.  A lane holds one part: its run count, its first and
// last op, its bases by op.  A part merges into the one before when that one's last op — of the nearest non-empty part
// below, in this pass or carried from an earlier one — equals its first.  emit(seg index, segment, kind of part, opBase,
// merges) is called on every lane that holds a segment.  Returns the read's row.
template <typename Emit>
TALC_D EditRow walk_edit_parts(const MapSeg* __restrict__ segs, const EditPart* parts, uint32_t nseg, uint64_t max_cells,
                               uint32_t lane, Emit emit) {
  const uint64_t below = (1ull << lane) - 1ull;
  EditRow row = {0u, 0u, 0u, 0u, 0u, 0u};
  uint32_t openLast = 0;                   // the last op of the last non-empty part so far (0: none)
  for (uint32_t base = 0; base < nseg; base += 64u) {
    const uint32_t j = base + lane;
    MapSeg s = {SEG_RAW, 0u, 0u, 0u, 0u};
    if (j < nseg) s = segs[j];
    uint32_t nRuns = 0, first = 0, last = 0, cnt[4] = {0u, 0u, 0u, 0u}, unal = 0;
    int kind = EDIT_PART_EMPTY;
    if (s.kind != SEG_CORRECTED) {
      if (s.outLen) { nRuns = 1u; first = last = EDIT_EQ; cnt[0] = s.outLen; }
    } else {
      kind = edit_part_kind(s.rawLen, s.outLen, max_cells);
      if (kind == EDIT_PART_INS) { nRuns = 1u; first = last = EDIT_I; cnt[2] = s.outLen; }
      else if (kind == EDIT_PART_DEL) { nRuns = 1u; first = last = EDIT_D; cnt[3] = s.rawLen; }
      else if (kind == EDIT_PART_UNALIGNED) { nRuns = 2u; first = EDIT_D; last = EDIT_I; cnt[3] = s.rawLen; cnt[2] = s.outLen; unal = 1u; }
      else if (kind == EDIT_PART_DP) {
        const EditPart p = parts[j];
        nRuns = p.nRuns; first = p.ends & 0xFFu; last = (p.ends >> 8) & 0xFFu;
        cnt[0] = p.cnt[0]; cnt[1] = p.cnt[1]; cnt[2] = p.cnt[2]; cnt[3] = p.cnt[3];
      }
    }
    const uint64_t ne = __ballot(nRuns > 0u);
    const uint64_t lower = ne & below;
    const uint32_t prevLane = lower ? 63u - (uint32_t)__builtin_clzll(lower) : 0u;
    const uint32_t prevLastIn = (uint32_t)__shfl((int)last, (int)prevLane, 64);
    const uint32_t prevLast = lower ? prevLastIn : openLast;
    const bool merges = nRuns > 0u && prevLast == first;
    const uint32_t v = nRuns - (merges ? 1u : 0u);
    uint32_t incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)incl, off, 64); if (lane >= (uint32_t)off) incl += t; }
    // run r of the part goes to op opBase + r: a part that merges starts in the op before its own first
    const uint32_t opBase = row.nOps + incl - v - (merges ? 1u : 0u);
    if (j < nseg) emit(j, s, kind, opBase, merges);
    row.nOps += (uint32_t)__shfl((int)incl, 63, 64);
    if (ne) openLast = (uint32_t)__shfl((int)last, 63 - __builtin_clzll(ne), 64);
    uint32_t sum[5] = {cnt[0], cnt[1], cnt[2], cnt[3], unal};
#pragma unroll
    for (int k = 0; k < 5; ++k)
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) sum[k] += (uint32_t)__shfl_xor((int)sum[k], off, 64);
    row.nMatch += sum[0]; row.nMismatch += sum[1]; row.nIns += sum[2]; row.nDel += sum[3]; row.nUnaligned += sum[4];
  }
  return row;
}

// one wave per read: its row, and where the DP parts go
__global__ void __launch_bounds__(64)
k_edit_count(const MapSeg* __restrict__ segs, const uint64_t* __restrict__ segOff, EditPart* parts, uint32_t n_reads, uint64_t max_cells,
             EditRow* __restrict__ rows) {
  const uint32_t r = blockIdx.x;
  if (r >= n_reads) return;
  const uint32_t lane = threadIdx.x;
  EditPart* const mine = parts + segOff[r];
  const EditRow row = walk_edit_parts(segs + segOff[r], mine, (uint32_t)(segOff[r + 1] - segOff[r]), max_cells, lane,
                                      [&](uint32_t j, const MapSeg&, int kind, uint32_t opBase, bool merges) {
                                        if (kind == EDIT_PART_DP) { mine[j].opBase = opBase; mine[j].ends = (mine[j].ends & 0xFFFFu) | (merges ? 1u << 16 : 0u); }
                                      });
  if (lane == 0) rows[r] = row;
}

// one wave per read: the runs of every part that k_edit_align does not write
__global__ void __launch_bounds__(64)
k_edit_pack(const MapSeg* __restrict__ segs, const uint64_t* __restrict__ segOff, const EditPart* __restrict__ parts, uint32_t n_reads,
            uint64_t max_cells, const uint64_t* __restrict__ op_off, uint32_t* ops) {
  const uint32_t r = blockIdx.x;
  if (r >= n_reads) return;
  const uint64_t o0 = op_off[r], o1 = op_off[r + 1];
  (void)walk_edit_parts(segs + segOff[r], parts + segOff[r], (uint32_t)(segOff[r + 1] - segOff[r]), max_cells, threadIdx.x,
                        [&](uint32_t, const MapSeg& s, int kind, uint32_t opBase, bool merges) {
                          if (s.kind != SEG_CORRECTED) { if (s.outLen) edit_add_run(ops, o0 + opBase, o1, EDIT_EQ, s.outLen, !merges); }
                          else if (kind == EDIT_PART_INS) edit_add_run(ops, o0 + opBase, o1, EDIT_I, s.outLen, !merges);
                          else if (kind == EDIT_PART_DEL) edit_add_run(ops, o0 + opBase, o1, EDIT_D, s.rawLen, !merges);
                          else if (kind == EDIT_PART_UNALIGNED) {
                            edit_add_run(ops, o0 + opBase, o1, EDIT_D, s.rawLen, !merges);
                            edit_add_run(ops, o0 + opBase + 1u, o1, EDIT_I, s.outLen, true);
                          }
                        });
}

}  // namespace talc
