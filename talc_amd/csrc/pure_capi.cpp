// pure_capi.cpp — host build (g++) of the host/device-pure pieces of the product
// (talc_pure.h) plus the host table builder, exported with C linkage so the CPU test-suite can
// check them without a GPU: libtalc_pure.so.  This is product code compiled for the host, not a
// CPU fallback of the correction path (nothing in libtalc_hip.so calls it).
#include <algorithm>
#include <cstdint>
#include <vector>

#include "talc_edit_plan.h"
#include "talc_kernels_chimera.h"
#include "talc_kernels_demux.h"
#include "talc_kernels_search.h"
#include "talc_kernels_umi.h"
#include "talc_pure.h"
#include "talc_wfa.h"

using namespace talc;

extern "C" {

// the work-queue bucket of a searched read (talc_pure.h: order_key_bucket), 1024 buckets as the kernels use it
uint32_t talc_pure_order_bucket(uint32_t cost_est, uint32_t cost_gap, uint32_t gap_scale) { return order_key_bucket(cost_est, cost_gap, gap_scale, 1024u); }

// the byte -> Dna5 code select of the k-mer window kernels (talc_common.h), next to the switch it restates
uint32_t talc_pure_ascii_to_code_select(uint32_t c) { return ascii_to_code_select(c); }
uint32_t talc_pure_ascii_to_code(uint32_t c) { return ascii_to_code((uint8_t)c); }
uint32_t talc_pure_complement_code(uint32_t c) { return complement_code((uint8_t)c); }

// the per-wave scratch of a search stage (talc_kernels_search.h: make_caps) as 36 words: the ten capacities in SearchLimits'
// order, slotBytes, the 23 offsets in layout order (o_setA .. o_trace), what follows the last region (o_trace + 64), and caps_hold_read
void talc_pure_make_caps(uint32_t max_len, uint32_t k, uint32_t scale, uint32_t arena_limit, int tiny, uint64_t* out36) {
  const SearchCaps c = make_caps(max_len, k, scale, arena_limit, tiny != 0);
  const uint64_t w[36] = {c.seqCap, c.seqArena, c.refCap, c.edgeCap, c.anchCap, c.fullCap, c.fullPool, c.dpCap, c.regCap, c.weakPool, c.slotBytes,
                          c.o_setA, c.o_setB, c.o_seqPool, c.o_ref, c.o_ancL, c.o_ancR, c.o_ancPos, c.o_fullMeta, c.o_fullPoolB, c.o_edgeLong,
                          c.o_edgeShort, c.o_edgeTmp, c.o_dp, c.o_gard, c.o_regS, c.o_regE, c.o_wOff, c.o_wLen, c.o_weak, c.o_wideBloom, c.o_rowPool,
                          c.o_regH, c.o_trace, c.o_trace + 64, caps_hold_read(c, max_len) ? 1u : 0u};
  for (int i = 0; i < 36; ++i) out36[i] = w[i];
}

int pure_is_expected_by_model(double alpha, uint32_t nextc, uint32_t cc, int classe_unexpected) {
  return is_expected_by_model(alpha, nextc, cc, classe_unexpected != 0) ? 1 : 0;
}
int pure_is_expected_by_last_node(double alpha, uint32_t nextc, uint32_t cc) {
  return is_expected_by_last_node(alpha, nextc, cc) ? 1 : 0;
}
int pure_tag_next_nodes(double alpha, double err, uint32_t minc, const uint32_t* cnt4, const uint32_t* jc4, uint32_t count,
                        int complex, int32_t* tags4, double* dist4) {
  int t[4];
  double d[4];
  int n = tag_next_nodes(alpha, err, minc, cnt4, jc4, count, complex != 0, t, d);
  for (int i = 0; i < 4; ++i) { tags4[i] = t[i]; dist4[i] = d[i]; }
  return n;
}

// gnu_sort (the product's restatement of libstdc++ std::sort) vs the real std::sort on
// (key, payload) pairs ordered by key only: both must produce the same permutation.
struct KP { int32_t key; int32_t payload; };
struct KPLess { bool operator()(const KP& a, const KP& b) const { return a.key < b.key; } };
void pure_gnu_sort_pairs(int32_t* keys, int32_t* payloads, int n) {
  std::vector<KP> v(n);
  for (int i = 0; i < n; ++i) v[i] = KP{keys[i], payloads[i]};
  gnu_sort(v.data(), n, KPLess());
  for (int i = 0; i < n; ++i) { keys[i] = v[i].key; payloads[i] = v[i].payload; }
}
void pure_std_sort_pairs(int32_t* keys, int32_t* payloads, int n) {
  std::vector<KP> v(n);
  for (int i = 0; i < n; ++i) v[i] = KP{keys[i], payloads[i]};
  std::sort(v.begin(), v.end(), KPLess());
  for (int i = 0; i < n; ++i) { keys[i] = v[i].key; payloads[i] = v[i].payload; }
}

// the depth-limit fallback of introsort: std::__partial_sort(first, last, last) == heapsort
void pure_gnu_heapsort_pairs(int32_t* keys, int32_t* payloads, int n) {
  std::vector<KP> v(n);
  for (int i = 0; i < n; ++i) v[i] = KP{keys[i], payloads[i]};
  gs_heapsort(v.data(), 0, n, KPLess());
  for (int i = 0; i < n; ++i) { keys[i] = v[i].key; payloads[i] = v[i].payload; }
}
void pure_std_heapsort_pairs(int32_t* keys, int32_t* payloads, int n) {
  std::vector<KP> v(n);
  for (int i = 0; i < n; ++i) v[i] = KP{keys[i], payloads[i]};
  std::partial_sort(v.begin(), v.end(), v.end(), KPLess());
  for (int i = 0; i < n; ++i) { keys[i] = v[i].key; payloads[i] = v[i].payload; }
}

int pure_gardening(uint32_t maxb, int n, const double* scores, const double* dists, uint32_t* kept, int32_t* isComplex) {
  std::vector<ValIdx> wv(n + 1);
  std::vector<Rank4> r1(n + 1), r2(n + 1);
  bool cx = false;
  int nk = gardening(maxb, n, scores, dists, wv.data(), r1.data(), r2.data(), kept, &cx);
  *isComplex = cx ? 1 : 0;
  return nk;
}

// anchors ordering (sortAnchorsByNearest, Explorer.cpp:402-411) on (pos,count) records
void pure_sort_anchors(double cc, uint32_t* pos, uint32_t* count, int n) {
  std::vector<AnchorRec> a(n);
  for (int i = 0; i < n; ++i) a[i] = AnchorRec{0, 0, pos[i], count[i]};
  gnu_sort(a.data(), n, LessAnchor{cc});
  for (int i = 0; i < n; ++i) { pos[i] = a[i].pos; count[i] = a[i].count; }
}

// wavefront statement of the unit-cost x-drop extension (talc_wfa.h); out4 = moved, extCols, extRows, score
void pure_wfa_xdrop(const uint8_t* q, int qlen, const uint8_t* d, int dlen, int x, int32_t* out4) {
  const WfaResult r = wfa_xdrop_scalar(q, qlen, d, dlen, x);
  out4[0] = r.moved; out4[1] = r.extCols; out4[2] = r.extRows; out4[3] = r.score;
}

// ... as one run of a series over the same pair (talc_wfa.h: WfaKept).  keep130 = level, qlenAt, F[64], E[64]: zeroed
// before a pair's first run, handed back unchanged to the next; returns 1 if this run resumed from the kept level
int pure_wfa_xdrop_resume(const uint8_t* q, int qlen, const uint8_t* d, int dlen, int x, int32_t* keep130, int32_t* out4) {
  static_assert(sizeof(WfaKept) == 130 * sizeof(int32_t), "WfaKept is 130 ints");
  bool resumed = false;
  const WfaResult r = wfa_xdrop_scalar_run(q, qlen, d, dlen, x, reinterpret_cast<WfaKept*>(keep130), &resumed);
  out4[0] = r.moved; out4[1] = r.extCols; out4[2] = r.extRows; out4[3] = r.score;
  return resumed ? 1 : 0;
}

// the edit scripts' planner (talc_edit_plan.h) on `count` pairs n[i] x m[i], in order: kind[i] = edit_part_kind; for a DP
// word[i] = where its delta words start (all ones: LDS) and round[i] = its round; *most = the largest round's words.
// Returns the number of rounds, -1 when a pair alone is beyond budget_words.
int pure_edit_plan(const uint32_t* n, const uint32_t* m, uint32_t count, uint64_t max_cells, uint64_t budget_words, int32_t* kind,
                   uint64_t* word, int32_t* round, uint64_t* most) {
  EditPlan plan(budget_words);
  for (uint32_t i = 0; i < count; ++i) {
    kind[i] = edit_part_kind(n[i], m[i], max_cells); word[i] = 0; round[i] = -1;
    if (kind[i] == EDIT_PART_DP && !plan.add(i, 0, n[i], m[i])) return -1;
  }
  plan.finish();
  size_t t = 0;
  for (size_t r = 0; r < plan.roundEnd.size(); ++r)
    for (; t < plan.roundEnd[r]; ++t) { word[plan.tasks[t].seg] = plan.tasks[t].scratchWord; round[plan.tasks[t].seg] = (int32_t)r; }
  *most = plan.mostWords;
  return (int)plan.roundEnd.size();
}
// walk_repeat_possible (talc_pure.h) beside the comparison it stands for, on n cases of K + TALC_WALK_LEVELS bases each
// (codes 0..3, growth order: the tip oldest base first, then the bases of levels 0, 1, ...).  pair[c]: bit p is set when
// two of the record's k-mers p levels apart are equal, compared base by base on the array; pred[c]: bit p is the
// predicate for period p on the tip packed as a walk in that direction holds it.
void pure_walk_repeat_check(const uint8_t* g, uint64_t n, uint32_t K, int dir_right, uint32_t* pair, uint32_t* pred) {
  const int L = TALC_WALK_LEVELS;
  for (uint64_t c = 0; c < n; ++c) {
    const uint8_t* G = g + c * (K + L);
    uint32_t pm = 0;
    for (int i = 0; i < L; ++i)            // level i's k-mer is G[i+1 .. i+K]
      for (int j = i + 1; j < L; ++j)
        if (std::equal(G + i + 1, G + i + 1 + K, G + j + 1)) pm |= 1u << (j - i);
    uint64_t kmer = 0;                     // RIGHT: the oldest base on top; LEFT: the newest
    for (uint32_t t = 0; t < K; ++t) kmer |= (uint64_t)G[t] << (dir_right ? 2 * (K - 1 - t) : 2 * t);
    uint32_t qm = 0;
    for (int p = 1; p < L; ++p)
      if (walk_repeat_possible(kmer, K, (uint32_t)p, dir_right != 0)) qm |= 1u << p;
    pair[c] = pm; pred[c] = qm;
  }
}

uint64_t pure_edit_scratch_words(uint32_t n, uint32_t m) { return edit_scratch_words(n, m); }
int pure_edit_in_lds(uint32_t n, uint32_t m) { return edit_in_lds(n, m) ? 1 : 0; }

// ---- chimeras (docs/chimeras.md): k_read_chimera's lanes one after another, and the piece rule
// out3: lanes per pattern, chunk, tile of a read of L bytes under nPatterns patterns
void pure_chimera_geometry(uint32_t L, uint32_t nPatterns, uint32_t* out3) {
  const ChimeraGeometry g = chimera_geometry(L, nPatterns);
  out3[0] = g.lanesPerPattern; out3[1] = g.chunk; out3[2] = g.tile;
}
// adapters: comma-separated ACGTacgt, as talc_ctx_set_ends takes them (not validated again: at most 4 of 12 .. 64 letters).
// The sorted hits of the batch; returns their number and writes those that fit.
int64_t pure_chimera_scan(const char* adapters, uint32_t max_error_pct, const uint8_t* bases, const uint64_t* offsets, uint32_t n_reads,
                          ChimeraHit* out, uint64_t capacity) {
  ChimeraParams P;
  P.nPatterns = 0; P.pad_ = 0;
  for (PatternList it(adapters); it.next(acgt_set);) {
    if (it.fault || P.nPatterns + 2 > kChimeraMaxPatterns) return -1;
    chimera_params_add(P, it.p, (uint32_t)it.m, acgt_set, max_error_pct);
  }
  std::vector<ChimeraHit> hits;
  for (uint32_t r = 0; r < n_reads; ++r) chimera_scan_host(bases + offsets[r], (uint32_t)(offsets[r + 1] - offsets[r]), r, P, hits);
  chimera_sort(hits);
  for (size_t i = 0; i < hits.size() && i < capacity; ++i) out[i] = hits[i];
  return (int64_t)hits.size();
}
// the pieces of a batch from its sorted hits; returns their number and writes those that fit; read_piece_off: n_reads + 1;
// dropped2: pieces dropped, their bytes
int64_t pure_split_pieces(const ChimeraHit* hits, uint64_t n_hits, const uint64_t* offsets, uint32_t n_reads, uint32_t min_piece, SplitPiece* out,
                          uint64_t capacity, uint64_t* read_piece_off, uint64_t* dropped2) {
  std::vector<ChimeraHit> h(hits, hits + n_hits);
  for (const ChimeraHit& x : h) if (x.read >= n_reads) return -1;
  std::vector<uint64_t> hitOff, pieceOff;
  chimera_read_offsets(h, n_reads, hitOff);
  std::vector<SplitPiece> pieces;
  split_pieces(h.data(), hitOff.data(), offsets, n_reads, min_piece, pieces, pieceOff, dropped2, dropped2 + 1);
  for (size_t i = 0; i < pieces.size() && i < capacity; ++i) out[i] = pieces[i];
  for (uint32_t r = 0; r <= n_reads; ++r) read_piece_off[r] = pieceOff[r];
  return (int64_t)pieces.size();
}

// ---- barcode demultiplexing (docs/demux.md): k_read_demux's lanes one after another
// out3: chunks per pattern, passes, the tails' first slot under n_barcodes barcodes
void pure_demux_geometry(uint32_t n_barcodes, uint32_t* out3) {
  const DemuxGeometry g = demux_geometry(n_barcodes);
  out3[0] = g.chunks; out3[1] = g.passes; out3[2] = g.tailSlot;
}
// the slot of pattern (end, b) and the columns [c0, c1) of its chunk q in a text of n columns: out3 = slot, c0, c1
void pure_demux_place(uint32_t n_barcodes, uint32_t end, uint32_t b, uint32_t q, uint32_t n, uint32_t* out3) {
  const DemuxGeometry g = demux_geometry(n_barcodes);
  out3[0] = demux_pattern_slot(g, end, b) + q;
  sellers_chunk(n, g.chunks, q, &out3[1], &out3[2]);
}
// The setting as talc_ctx_set_demux takes it, validated the same way: -1 and the message in `why` when it is refused or off.
// One row per read.
int pure_demux_scan(const char* barcodes, uint32_t max_error_pct, uint32_t min_margin, uint32_t window, int both_ends, const uint8_t* bases,
                    const uint64_t* offsets, uint32_t n_reads, DemuxRow* rows, char* why, uint64_t why_len) {
  DemuxParams P;
  std::vector<uint64_t> peq((size_t)kDemuxMaxBarcodes * 4, 0);
  if (why && why_len) why[0] = 0;
  char msg[256] = "the setting is off";
  if (!demux_make_setting(barcodes, max_error_pct, min_margin, window, both_ends, P, peq.data(), msg, sizeof msg) || !P.nBarcodes) {
    if (why && why_len) snprintf(why, (size_t)why_len, "%s", msg);
    return -1;
  }
  for (uint32_t r = 0; r < n_reads; ++r) rows[r] = demux_scan_host(bases + offsets[r], (uint32_t)(offsets[r + 1] - offsets[r]), P, peq.data());
  return 0;
}

// ---- UMI read-out (docs/umi.md): k_read_umi's lanes one after another
// The setting as talc_ctx_set_umi takes it, validated the same way: -1 and the message in `why` when it is refused or off.
// One row per read, as on a plain batch.
int pure_umi_scan(const char* pattern, uint32_t max_error_pct, uint32_t window, const uint8_t* bases, const uint64_t* offsets, uint32_t n_reads,
                  UmiRow* rows, char* why, uint64_t why_len) {
  UmiParams P;
  if (why && why_len) why[0] = 0;
  char msg[256] = "the setting is off";
  if (!umi_make_setting(pattern, max_error_pct, window, P, msg, sizeof msg) || !P.m) {
    if (why && why_len) snprintf(why, (size_t)why_len, "%s", msg);
    return -1;
  }
  for (uint32_t r = 0; r < n_reads; ++r) rows[r] = umi_scan_host(bases + offsets[r], (uint32_t)(offsets[r + 1] - offsets[r]), P);
  return 0;
}
// the kept interval of a read of L bytes: out2 = kept_start, kept_len (umi_row_fill); end 0, 1, 2
void pure_umi_kept(uint32_t L, uint32_t end, uint32_t stop, uint32_t head, uint32_t tail, uint32_t* out2) {
  UmiRow row;
  const UmiPick pk = {end, 0u, 255u, stop};
  umi_row_fill(row, pk, 0u, 0u, L, head, tail);
  out2[0] = row.keptStart; out2[1] = row.keptLen;
}
}  // extern "C"
