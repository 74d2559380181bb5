// talc_capi.hip — the C ABI of libtalc_hip.so (include/talc_hip.h): host orchestration of the
// GPU k-mer table and of the per-read correction kernels.  gfx950 only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <mutex>
#include <sstream>
#include <string>
#include <vector>

#include "talc_common.h"
#include "talc_devmem.h"
#include "talc_hip.h"
#include "talc_kernels_build.h"
#include "talc_kernels_count.h"
#include "talc_kernels_edits.h"
#include "talc_kernels_ends.h"
#include "talc_kernels_pieces.h"
#include "talc_kernels_probe.h"
#include "talc_kernels_search.h"
#include "talc_kernels_solidity.h"
#include "talc_kernels_spectrum.h"
#include "talc_kernels_srfilter.h"
#include "talc_kernels_strand.h"
#include "talc_kernels_support.h"
#include "talc_kernels_chimera.h"   // (last: the code object lays kernels out in this order; the correction's kernels keep the places they had: docs/chimeras.md)
#include "talc_kernels_demux.h"     // (behind it, for the same reason: docs/demux.md)
#include "talc_kernels_umi.h"       // (and last of all, for the same reason: docs/umi.md)
#include "talc_switches.h"
#include "talc_table_host.h"

using namespace talc;

// ------------------------------------------------------------------ error plumbing
static thread_local std::string g_err;
static int fail(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
// (what does not fit is TALC_ERR_NOMEM, every other failure a device error: docs/out_of_memory.md)
#define HIPCHK(x)                                                                          \
  do {                                                                                     \
    hipError_t _e = (x);                                                                   \
    if (_e != hipSuccess)                                                                  \
      return fail(_e == hipErrorOutOfMemory ? TALC_ERR_NOMEM : TALC_ERR_DEVICE, "%s failed: %s (%s:%d)", #x, hipGetErrorString(_e), __FILE__, __LINE__); \
  } while (0)

// seconds on the steady clock, since the start or since the last lap (where a build's wall time goes, TALC_TIMING)
struct Stopwatch {
  using Clock = std::chrono::steady_clock;
  Clock::time_point t0 = Clock::now();
  double seconds() const { return std::chrono::duration<double>(Clock::now() - t0).count(); }
  double lap() { const auto t1 = Clock::now(); const double s = std::chrono::duration<double>(t1 - t0).count(); t0 = t1; return s; }
};

// The device time of the last X: an event pair of its own (made on first use), recorded around the launch on the owner's
// stream.  Nobody waits for it: the pair is pending until whoever waits for that stream next reads it (read(); a context's
// spans all at once, read_spans), so a span launched by one entry point and waited for by another is still reported.
struct Span {
  hipEvent_t ev[2] = {nullptr, nullptr};
  float ms = 0;
  bool pending = false;   // recorded and not yet read
  ~Span() { for (auto& e : ev) if (e) (void)hipEventDestroy(e); }   // (the owner has made its device current)
  // launch() on `stream` between the two events; a launch that fails leaves the span without a pair to read
  template <class Launch>
  int around(hipStream_t stream, Launch launch) {
    pending = false;
    for (auto& e : ev) if (!e) HIPCHK(hipEventCreate(&e));
    HIPCHK(hipEventRecord(ev[0], stream));
    launch();
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev[1], stream));
    pending = true;
    return TALC_OK;
  }
  // once the stream has been waited for
  int read() {
    if (pending) HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[1]));
    pending = false;
    return TALC_OK;
  }
  void skip() { ms = 0; pending = false; }   // X did not run in this call: its time is exactly 0
};

// The table lives where it was built.  A host-built table has a host image (h.right / h.left) that uploads copy; a
// table built (or imported) on a GPU has a *staged* device image there — colouring and de-colouring run on it as
// kernels, talc_table_upload to that same GPU adopts it without any copy, and the host image is only materialised
// when something asks for it (host lookups, an upload to another GPU).
struct DeviceImage {   // everything the table owns on one GPU
  DevBuf<Bucket> right, left;
  DevBuf<uint64_t> filter;                 // presence filter of filterWords words
  uint64_t filterWords = 0;
  DevBuf<WalkEntry> walkRight, walkLeft;   // optional (talc_table_upload decides)
  // staged (buckets only: built or imported, still editable) until an upload derives the filter, the in-degree bits in
  // the RIGHT keys and perhaps the walk tables
  bool uploaded() const { return (bool)filter; }
  void drop_derived() { filter.reset(); filterWords = 0; walkRight.reset(); walkLeft.reset(); }   // staged again
  uint64_t bytes(uint64_t capacity) const { return 2 * capacity * sizeof(Bucket) + filterWords * 8 + (walkRight ? 2 * capacity * sizeof(WalkEntry) : 0); }
  TableView view(uint64_t capacity, uint32_t k) const { return TableView{right.get(), left.get(), capacity, k, filter.get(), filterWords, walkRight.get(), walkLeft.get()}; }
};
struct talc_table {
  HostTable h;
  bool hostValid = true;       // h.right / h.left hold the current table
  // device -> its image.  A device build or an import leaves one staged image, uploads leave uploaded ones; every image
  // holds the current table (a staged one is the only place edits go, and nothing is edited once an upload has happened)
  using Images = std::map<int, DeviceImage>;
  Images images;
  ~talc_table() { for (auto& kv : images) { (void)hipSetDevice(kv.first); kv.second = DeviceImage(); } }
  // (device, image) on `device`, or on whichever GPU has one; nullptr when there is none
  Images::value_type* image(int device) { auto it = images.find(device); return it == images.end() ? nullptr : &*it; }
  Images::value_type* any_image() { return images.empty() ? nullptr : &*images.begin(); }
  const DeviceImage* first_uploaded() const {
    for (auto& kv : images) if (kv.second.uploaded()) return &kv.second;
    return nullptr;
  }
  bool frozen() const { return first_uploaded() != nullptr; }   // some upload has happened: the table is immutable
};

// make the host image current (device-built tables: copy it back from a GPU that holds it)
static int ensure_host(talc_table* t) {
  if (t->hostValid) return TALC_OK;
  auto* at = t->any_image();
  if (!at) return fail(TALC_ERR_STATE, "the table has neither a host image nor a device image");
  const uint64_t bytes = t->h.capacity * sizeof(Bucket);
  if (!t->h.right) t->h.right = (Bucket*)malloc(bytes);
  if (!t->h.left) t->h.left = (Bucket*)malloc(bytes);
  if (!t->h.right || !t->h.left) return fail(TALC_ERR_NOMEM, "cannot allocate the host image (%llu bytes)", (unsigned long long)(2 * bytes));
  HIPCHK(hipSetDevice(at->first));
  HIPCHK(hipMemcpy(t->h.right, at->second.right.get(), bytes, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(t->h.left, at->second.left.get(), bytes, hipMemcpyDeviceToHost));
  t->hostValid = true;
  return TALC_OK;
}

struct Stage {
  // per-wave scratch for the search kernel
  DevBuf<uint8_t> scratch;
  uint64_t scratch_bytes = 0;
  uint32_t n_slots = 0;
  SearchCaps caps;
  // edge tasks (first pass only): one box per slot + the slots' claim counters (talc_kernels_search.h, "edge tasks")
  DevBuf<uint8_t> boxes;
  uint64_t boxes_bytes = 0;
  uint32_t box_seq_cap = 0;
};

// the marks of the correction's stages, a chain of events on the context's stream (read_stage_times), in order: before
// k_encode, after it, after k_coverage, after k_structure, after the first k_search, around the retry passes, after k_pack,
// after k_pack_map
enum CtxEvent { kEvBegin, kEvEncoded, kEvCovered, kEvStructured, kEvSearched, kEvRetry0, kEvRetry1, kEvEmitted, kEvPackMap, kEvCount };

// the kernels of the reports, each timed by a Span of the context (read_spans)
enum CtxSpan {
  kSpanVote,                             // k_strand_vote
  kSpanPackMap,                          // k_pack_map: its time comes from the chain's marks (read_stage_times), its own pair is never made
  kSpanMaskCase,                         // k_mask_case
  kSpanSolidityRaw, kSpanSolidityRecords,   // the two k_solidity of talc_batch_solidity: over the reads, over the records
  kSpanPieceCount, kSpanPiecePack,       // talc_batch_pieces: k_piece_count, k_piece_pack
  // the edit scripts (run_edits): the first k_edit_align rounds, k_edit_count, the second rounds, k_edit_pack
  kSpanEditAlignA, kSpanEditCount, kSpanEditAlignB, kSpanEditPack,
  kSpanSupport,                          // k_base_support
  kSpanEndsScan, kSpanEndsGather,        // the end clean-up: k_read_ends, k_gather of a clipped batch
  kSpanChimeraScan, kSpanChimeraGather,  // the chimera split: k_read_chimera, k_gather of the pieces
  kSpanDemuxScan,                        // barcode demultiplexing: k_read_demux
  kSpanUmiScan,                          // the UMI read-out: k_read_umi
  kSpanCount
};

struct talc_ctx {
  talc_table* table = nullptr;
  talc_params p;
  DevParams dp;
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev[kEvCount] = {};
  Span span[kSpanCount];   // the last run of each report kernel on this context
  TableView view;
  talc_timing timing;
  uint32_t retryReport[4] = {};   // talc_test_retry_report: the last correction's retry passes (search_retry_passes)
  Switches sw;          // the environment's switches when the context was created (talc_switches.h)
  bool map = false;     // talc_ctx_set_map: corrections keep the correction map
  bool autoStrand = false;   // talc_ctx_set_auto_strand: every read in the orientation k_strand_vote chooses
  bool endsOn = false;       // talc_ctx_set_ends (docs/read_ends.md): nothing of it exists while it is off
  uint32_t endsGen = 0;      // ... counts the settings: a plain batch's rows are those of the setting they were made under
  EndsParams ends;           // ... as k_read_ends takes it
  uint8_t endsCodes[ENDS_MAX_ADAPTERS][64] = {};   // ... and its adapters' letters as codes (the chimera scan makes its patterns from them)
  bool chimeraOn = false;    // talc_ctx_set_chimera (docs/chimeras.md): nothing of it exists while it is off
  uint32_t chimeraGen = 0;   // ... counts the settings, as endsGen does
  uint32_t chimeraPct = 0, chimeraMinPiece = 0;
  bool demuxOn = false;      // talc_ctx_set_demux (docs/demux.md): nothing of it exists while it is off
  uint32_t demuxGen = 0;     // ... counts the settings, as endsGen does
  DemuxParams demux;         // ... as k_read_demux takes it
  DevBuf<uint64_t> d_demux_peq;   // ... and the barcodes' match masks (kDemuxMaxBarcodes x 4 words), written when a setting is accepted
  bool umiOn = false;        // talc_ctx_set_umi (docs/umi.md): nothing of it exists while it is off
  uint32_t umiGen = 0;       // ... counts the settings, as endsGen does
  UmiParams umi;             // ... as k_read_umi takes it
  Stage stage;          // default scratch
  DevBuf<uint32_t> d_queue;      // work-queue counters
  DevBuf<uint32_t> d_hist;       // kHistWords: the buckets of the work-queue ordering, then the batch statistics
  DevBuf<uint64_t> d_counters;   // kCounterWords: trail steps, dp cells, the profile build's counters and wave log
  DevBuf<uint32_t> d_thr;        // the count model's thresholds by count (DevParams.thr)
  DevCache cache;       // the device buffers of this context's batches
  HostPool host_pool;   // the page-locked host arrays of its finished batches, for the next batch (talc_devmem.h)
  HostArr<uint64_t> h_land;   // page-locked: kTotWords of the offset kernels' totals, then the counters below the wave log
  ~talc_ctx() {
    (void)hipSetDevice(device);
    for (auto& e : ev) if (e) hipEventDestroy(e);
    if (stream) hipStreamDestroy(stream);
  }
};

// the edit scripts of a batch (talc_batch_edits; talc_capi_edits.inc)
struct EditOut {
  std::vector<uint64_t> h_op_off;    // n_reads + 1: the reads' first op
  std::vector<EditRow> h_rows;       // n_reads
  CachedBuf<uint32_t> d_ops;         // the ops of all reads, dense, sized exactly
};

// What a batch holds and what drops it.  A result is valid while its flag is set; "->" reads "is made from", and
// what drops a result drops everything made from it:
//   voted                                  from the raw bytes; never dropped
//   ended                                  from the raw bytes (of a clipped batch: from those it was made from); never dropped
//   chimera                                from the raw bytes (of a split batch: from those it was made from); never dropped
//   demuxed                                from the raw bytes (of a clipped or split batch: from those it was made from); never dropped
//   umi                                    from the raw bytes (of a clipped batch: from those it was made from); never dropped
//   encoded(encodedAuto) -> covered
//   encoded -> solidity (raw rows), supported (RAW)
//   encoded -> structured            (test hook; k_search consumes the region lists)
//   encoded -> corrected(mapped) -> masked, pieced, edited, solidityCorrected, supported (RECORD)
// A call that makes one result clears that result's flag first and sets it when everything has succeeded.
struct BatchHolds {
  bool voted = false;         // d_strand, d_strand_flag: k_strand_vote runs once per batch
  bool ended = false;         // d_ends: k_read_ends under the context's setting number endsGen
  bool clipped = false;       // ... and the batch was made from those rows (talc_batch_create_clipped): they are never made again
  bool chimera = false;       // h_hits: k_read_chimera under the settings chimeraGen and chimeraEndsGen; never dropped
  bool split = false;         // ... and the batch was made from those hits (talc_batch_create_split): they are never made again
  bool demuxed = false;       // d_demux: k_read_demux under the setting demuxGen; of a clipped or split batch the rows of the reads it was made from
  bool umi = false;           // d_umi: k_read_umi under the setting umiGen; of a clipped or split batch the rows of the scan that made it
  bool encoded = false;       // d_codes
  bool encodedAuto = false;   // ... made with the vote's flags: k_pack, k_pack_map, k_solidity and k_base_support then take them too
  bool covered = false;       // d_cov, d_covw, d_nin
  bool structured = false;    // the region lists are as k_structure left them: no search has touched them since
  bool corrected = false;     // the records of the last correction: h_state, h_dense_off, d_dense
  bool mapped = false;        // ... which kept its map: h_seg_off, d_segs
  bool masked = false;        // d_masked: those records, RAW stretches in lower case
  bool pieced = false, edited = false;                // their pieces, their edit scripts
  bool solidity = false, solidityCorrected = false;   // d_sol_raw, the rows of the reads; d_sol_corr, those of the records
  bool supported = false, supportRecords = false;     // d_support: of the reads, or of the records
  // before a correction or talc_batch_structure launches anything: k_search edits the region lists in place, and a run that
  // fails leaves no records (h_state, h_dense_off and d_dense would be a mixture of this run's and the last one's)
  void drop_results() { structured = corrected = mapped = masked = solidity = solidityCorrected = pieced = edited = supported = false; }
  // the codes were made under the other auto-strand setting: the batch is as if it were new, but for the vote
  void drop_codes() { encoded = covered = false; drop_results(); }
  bool has_records() const { return corrected; }
  bool has_map() const { return corrected && mapped; }
  bool has_mask() const { return has_map() && masked; }
  bool has_pieces() const { return has_map() && pieced; }
  bool has_edits() const { return has_map() && edited; }
  bool has_support() const { return supported; }   // (of the reads: needs no records; of the records: dropped with them)
  bool has_solidity(bool ofRecords) const { return solidity && (!ofRecords || (corrected && solidityCorrected)); }
};

struct talc_batch {
  talc_ctx* ctx = nullptr;
  uint32_t n_reads = 0;
  uint64_t n_bases = 0, n_kmers = 0;
  uint32_t max_len = 0;
  std::vector<uint64_t> h_offsets, h_koff;
  std::vector<uint32_t> h_tile_read, h_tile_start, h_chunk_read, h_chunk_start;
  std::vector<uint64_t> h_regoff;
  std::vector<uint64_t> h_outoff;
  BatchHolds holds;
  // what comes back from the device with every correction: page-locked, from the context's pool and back to it
  HostArr<ReadState> h_state;
  HostArr<uint64_t> h_dense_off;
  HostArr<uint64_t> h_seg_off;   // with the correction map
  std::vector<uint64_t> h_read_piece_off, h_read_byte_off;   // n_reads + 1 each: the reads' first piece, first kept byte (talc_batch_pieces)
  // device buffers, from the context's cache.  Members go last to first, so the cache (which drops its oldest entries
  // first) gets them back from d_raw to d_headcov
  // the chimera scan: the hits of the scanned reads in the contract's order and each read's first hit; of a split batch the
  // source reads' hits, its pieces and each source read's first piece
  std::vector<ChimeraHit> h_hits;
  std::vector<uint64_t> h_read_hit_off;
  std::vector<SplitPiece> h_split;
  std::vector<uint64_t> h_read_split_off;
  uint32_t chimeraGen = 0, chimeraEndsGen = 0;
  CachedBuf<DemuxRow> d_demux;        // one row per source read (k_read_demux): n_demux of them
  uint32_t n_demux = 0, demuxGen = 0; // ... and the setting they were made under
  CachedBuf<UmiRow> d_umi;            // one row per read (k_read_umi)
  uint32_t umiGen = 0;                // the setting those rows were made under
  CachedBuf<EndRow> d_ends;           // one row per read (k_read_ends)
  uint32_t endsGen = 0;               // the setting those rows were made under
  CachedBuf<StrandRow> d_strand;      // one row per read (k_strand_vote)
  CachedBuf<uint8_t> d_strand_flag;   // ... and its choice as one byte per read: what the four kernels that orient a read take
  const uint8_t* rev_flags() const { return holds.encodedAuto ? d_strand_flag.get() : nullptr; }
  CachedBuf<uint8_t> d_support;       // one byte per base (k_base_support), sized exactly
  EditOut edits;
  CachedBuf<uint8_t> d_piece_bytes;  // the kept pieces' bytes, dense (k_piece_pack), sized exactly
  CachedBuf<uint64_t> d_piece_off;   // one per piece: where its bytes start in d_piece_bytes
  CachedBuf<OutPiece> d_pieces;         // the talc_piece entries, reads in input order
  CachedBuf<uint64_t> d_read_byte_off, d_read_piece_off;   // h_read_byte_off / h_read_piece_off on the device
  CachedBuf<PieceCount> d_piece_count;   // per read: kept pieces and their bytes (k_piece_count)
  CachedBuf<SolidityRow> d_sol_corr, d_sol_raw;   // one row per read (k_solidity): of its record, of the read itself
  CachedBuf<uint8_t> d_masked;       // the dense records again, RAW stretches in lower case (k_mask_case; made on first use)
  CachedBuf<MapSeg> d_segs;          // the dense correction map (k_pack_map) and the reads' offsets into it
  CachedBuf<uint64_t> d_seg_off;
  CachedBuf<uint32_t> d_mapedge;     // 2 x u32 per read: what k_search made of its head and its tail (leave_outcome)
  CachedBuf<uint32_t> d_headcov;     // 16 x u32 per read: dense counts of its first positions (k_structure -> k_search)
  CachedBuf<EmitSum> d_emit;         // the offset kernels' block sums, then their totals record (k_emit_sums, k_emit_offsets)
  CachedBuf<uint64_t> d_dense_off;
  CachedBuf<uint8_t> d_dense;
  CachedBuf<uint64_t> d_outoff;      // per-read offset into d_out
  CachedBuf<uint8_t> d_out;          // corrected codes, per-read capacity slots
  CachedBuf<uint64_t> d_regoff;      // per-read offset (in regions) into d_regions
  CachedBuf<uint32_t> d_regions;     // 3 x u32 per region slot (start, end, hit index of the start)
  CachedBuf<ReadState> d_state;      // structure + results
  CachedBuf<int32_t> d_nin;
  CachedBuf<CovWord> d_covw;         // one word per 64 k-mer positions
  CachedBuf<uint2> d_cov;            // hit pairs, packed per tile inside each read's dense slot (talc_common.h: CovWord)
  CachedBuf<uint32_t> d_order;       // the work queue: read numbers, heaviest first (k_order_scatter)
  CachedBuf<uint32_t> d_chunk_start, d_chunk_read, d_tile_start, d_tile_read;
  CachedBuf<uint64_t> d_koff;
  CachedBuf<uint64_t> d_offsets;
  CachedBuf<uint8_t> d_codes;
  CachedBuf<uint8_t> d_raw;
  ~talc_batch() { if (ctx) (void)hipSetDevice(ctx->device); }
};

static_assert(sizeof(MapSeg) == sizeof(talc_segment) && TALC_SEG_SOLID == SEG_SOLID && TALC_SEG_CORRECTED == SEG_CORRECTED && TALC_SEG_RAW == SEG_RAW,
              "k_pack_map writes talc_segment records");
static_assert(sizeof(OutPiece) == sizeof(talc_piece) && sizeof(talc_piece) == 12 && sizeof(PieceCount) == 8 && TALC_PIECES_TRIM == PIECES_TRIM &&
              TALC_PIECES_SPLIT == PIECES_SPLIT, "k_piece_pack writes talc_piece records");
static_assert(sizeof(EditRow) == sizeof(talc_edit_row) && sizeof(talc_edit_row) == 24 && sizeof(EditPart) == 32 && sizeof(EditTask) == 16, "k_edit_count writes talc_edit_row records");
static_assert(sizeof(SolidityRow) == sizeof(talc_solidity) && sizeof(talc_solidity) == 24, "k_solidity writes talc_solidity records");
static_assert(sizeof(StrandRow) == sizeof(talc_strand) && sizeof(talc_strand) == 24, "k_strand_vote writes talc_strand records");
static_assert(sizeof(EndRow) == sizeof(talc_end_row) && sizeof(talc_end_row) == 32, "k_read_ends writes talc_end_row records");
static_assert(sizeof(DemuxRow) == sizeof(talc_demux_row) && sizeof(talc_demux_row) == 16 && TALC_DEMUX_CONFLICT == DEMUX_CONFLICT, "k_read_demux writes talc_demux_row records");
static_assert(sizeof(UmiRow) == sizeof(talc_umi_row) && sizeof(talc_umi_row) == 56 && sizeof(UmiRow) == kUmiRowWords * 4, "k_read_umi writes talc_umi_row records");
static_assert(sizeof(ChimeraHit) == sizeof(talc_chimera_hit) && sizeof(talc_chimera_hit) == 16 && sizeof(SplitPiece) == sizeof(talc_split_piece) &&
              sizeof(talc_split_piece) == 16, "k_read_chimera writes talc_chimera_hit records, k_gather reads talc_split_piece records");

// What an entry point that takes a context and a batch checks first: they belong together and the `rest` of its arguments is there
// (`msg`: the call's own wording).  enter() makes the context's device current as well; belong() where a state check comes before that.
static int belong(const talc_ctx* c, const talc_batch* b, const char* msg, bool rest = true) {
  if (!c || !b || b->ctx != c || !rest) return fail(TALC_ERR_INVALID, "%s", msg);
  return TALC_OK;
}
static int enter(talc_ctx* c, talc_batch* b, const char* msg, bool rest = true) {
  if (int rc = belong(c, b, msg, rest)) return rc;
  HIPCHK(hipSetDevice(c->device));
  return TALC_OK;
}

template <typename T>
static int up(talc_ctx* c, CachedBuf<T>& d, const std::vector<T>& h, hipStream_t s) {
  HIPCHK(d.alloc(c->cache, std::max<size_t>(h.size(), 1)));
  if (!h.empty()) HIPCHK(hipMemcpyAsync(d.get(), h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, s));
  return TALC_OK;
}

// what an entry point does once it has waited for the context's stream: every span launched since the last wait gets its time
static int read_spans(talc_ctx* c) {
  for (auto& sp : c->span)
    if (int rc = sp.read()) return rc;
  return TALC_OK;
}

// What a kernel that takes the reads or their records reads (talc_kmer_window.h): the batch's codes at the input offsets, or
// the dense records of its last correction at theirs, with the reads' states and the flag that says so
struct BatchSource { const uint8_t* bytes; const uint64_t* d_off; const uint64_t* h_off; const ReadState* states; int records; };
static BatchSource batch_source(const talc_batch* b, bool records) {
  if (records) return {b->d_dense.get(), b->d_dense_off.get(), b->h_dense_off.data(), b->d_state.get(), 1};
  return {b->d_codes.get(), b->d_offsets.get(), b->h_offsets.data(), nullptr, 0};
}

// A sized result into the caller's `out` (a host buffer, or a device one: `kind`) of `capacity` units; null: nothing is
// asked for.  `total` units of `unit` bytes from `src`, on the context's stream: a DMA transfer when a host `out` is pinned
// (talc_pinned_alloc).  `what`, `units`: the nouns of "<what> too small: need <n> <units>".
static int copy_out(talc_ctx* c, void* out, uint64_t capacity, const void* src, uint64_t total, size_t unit, hipMemcpyKind kind,
                    const char* what, const char* units) {
  if (!out) return TALC_OK;
  if (capacity < total) return fail(TALC_ERR_CAPACITY, "%s too small: need %llu %s", what, (unsigned long long)total, units);
  if (!total) return TALC_OK;
  HIPCHK(hipMemcpyAsync(out, src, total * unit, kind, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return TALC_OK;
}

extern "C" {

int talc_abi_version(void) { return TALC_ABI_VERSION; }
const char* talc_last_error(void) { return g_err.c_str(); }

int talc_params_default(talc_params* p) {
  if (!p) return fail(TALC_ERR_INVALID, "null params");
  p->k = 21; p->min_count = 2; p->alpha = 2.57; p->window_size = 9; p->sr_error_rate = 0.025;
  p->min_inner_score = 0.7; p->min_border_score = 0.7; p->max_nb_competing_paths = 7; p->use_junctions = 0;
  p->reverse = 0; p->min_start_anchors = 3; p->max_start_anchors = 5; p->max_in_count = 100000;
  p->max_nb_border_paths = 75; p->max_nb_inner_paths = 50; p->check_interval = 6; p->allowed_failure_rate = 0.3;
  p->max_nb_border_failures = 3; p->coloured_count_thr = 10000; p->max_border_length = 500;
  return TALC_OK;
}

int talc_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return n;
}

// page-locked host memory for read / record buffers: copies to and from it are DMA transfers that run beside kernels
void* talc_pinned_alloc(uint64_t bytes) {
  PinnedBuf p;
  if (p.alloc(std::max<uint64_t>(bytes, 1)) != hipSuccess) { fail(TALC_ERR_NOMEM, "cannot allocate %llu bytes of pinned host memory", (unsigned long long)bytes); return nullptr; }
  return p.release();
}
void talc_pinned_free(void* p) { PinnedBuf gone(p); }

// ---- Test hooks: poisoned allocations and red zones (talc_devmem.h: memcheck)
int talc_test_set_poison(int byte, uint32_t guard_bytes) {
  if (byte < -1 || byte > 255) return fail(TALC_ERR_INVALID, "the poison byte is -1 (off) or 0 .. 255, %d given", byte);
  if (guard_bytes % 256 || guard_bytes > (1u << 20)) return fail(TALC_ERR_INVALID, "red zones are a multiple of 256 bytes, at most 1 MiB: %u given", guard_bytes);
  memcheck::set(byte, byte < 0 ? 0 : guard_bytes);
  return TALC_OK;
}
int talc_test_get_poison(int* byte, uint32_t* guard_bytes) {
  const memcheck::Setting s = memcheck::setting();
  if (byte) *byte = s.on ? (int)s.byte : -1;
  if (guard_bytes) *guard_bytes = s.on ? s.guard : 0;
  return TALC_OK;
}
int talc_test_guard_report(uint64_t out[4]) {
  if (!out) return fail(TALC_ERR_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(memcheck::lock());
  const memcheck::Tally& t = memcheck::global_tally();
  out[0] = t.checked; out[1] = t.violations; out[2] = t.firstBytes; out[3] = t.firstWhere;
  return TALC_OK;
}
uint64_t talc_test_cache_reuses(void) {
  std::lock_guard<std::mutex> lk(memcheck::lock());
  return memcheck::global_tally().reused;
}
// ---- Test hooks: allocations that fail on request (talc_devmem.h: failhook; docs/out_of_memory.md)
int talc_test_fail_alloc(uint32_t kinds, int64_t skip, uint32_t count, int real) {
  if (kinds > 3) return fail(TALC_ERR_INVALID, "kinds is a mask of 1 (device) and 2 (pinned host), 0 switches the hook off: %u given", kinds);
  if (skip < 0 || (real != 0 && real != 1)) return fail(TALC_ERR_INVALID, "skip is >= 0 and real is 0 or 1: %lld, %d given", (long long)skip, real);
  failhook::arm(kinds, skip, count, (uint32_t)real);
  return TALC_OK;
}
int talc_test_alloc_report(uint64_t out[8]) {
  if (!out) return fail(TALC_ERR_INVALID, "null argument");
  const failhook::State& s = failhook::state();
  out[0] = s.seen[0].load(); out[1] = s.seen[1].load(); out[2] = s.injected.load(); out[3] = s.lastOwner.load();
  out[4] = s.lastBytes.load(); out[5] = s.lastRuntimeCode.load(); out[6] = (uint64_t)s.live.load(); out[7] = s.kinds.load();
  return TALC_OK;
}
// ---- Test hook: which retry stages the last correction of a context ran (search_retry_passes)
int talc_test_retry_report(const talc_ctx* c, uint32_t out[4]) {
  if (!c || !out) return fail(TALC_ERR_INVALID, "null argument");
  for (int i = 0; i < 4; ++i) out[i] = c->retryReport[i];
  return TALC_OK;
}
// the checks of a scope go to a tally of its own
struct TallyScope {
  memcheck::Tally* before;
  explicit TallyScope(memcheck::Tally* t) : before(memcheck::tally_override()) { memcheck::tally_override() = t; }
  ~TallyScope() { memcheck::tally_override() = before; }
};
int talc_test_guard_selftest(uint64_t out[4]) {
  if (!out) return fail(TALC_ERR_INVALID, "null argument");
  const memcheck::Setting s = memcheck::setting();
  if (!s.on || !s.guard) return fail(TALC_ERR_STATE, "the self test needs a poison byte and red zones (talc_test_set_poison)");
  const uint8_t poison = s.byte, red = (uint8_t)~s.byte;
  const uint64_t n = 1000, G = s.guard;
  auto all = [](const uint8_t* p, uint64_t len, uint8_t v) { for (uint64_t i = 0; i < len; ++i) if (p[i] != v) return false; return true; };
  uint64_t fills = 0;
  memcheck::Tally ofBuf, ofCached, rest;
  std::vector<uint8_t> h(2 * n + 2 * G);
  {   // a DevBuf of n bytes; one byte just past its end
    TallyScope scope(&ofBuf);
    DevBuf<uint8_t> d;
    HIPCHK(d.alloc(n));
    HIPCHK(hipMemcpy(h.data(), d.get() - G, n + 2 * G, hipMemcpyDeviceToHost));
    fills |= all(h.data() + G, n, poison) ? 1 : 0;
    fills |= all(h.data(), G, red) && all(h.data() + G + n, G, red) ? 2 : 0;
    HIPCHK(hipMemcpy(d.get() + n, &poison, 1, hipMemcpyHostToDevice));
    HIPCHK(hipDeviceSynchronize());
  }
  {   // a cached buffer of n bytes, taken from the pool (2 n bytes, overwritten before it went there); one byte just before its start
    TallyScope scope(&rest);
    DevCache cache;
    void *big = nullptr, *p = nullptr;
    HIPCHK(cache.alloc(&big, 2 * n));
    HIPCHK(hipMemset(big, red, 2 * n));
    HIPCHK(hipDeviceSynchronize());
    cache.release(big);
    HIPCHK(cache.alloc(&p, n));
    if (p == big && rest.reused == 1) {
      HIPCHK(hipMemcpy(h.data(), (uint8_t*)p - G, 2 * n + 2 * G, hipMemcpyDeviceToHost));
      fills |= all(h.data() + G, 2 * n, poison) ? 4 : 0;   // (the slack behind the n bytes too)
      fills |= all(h.data(), G, red) && all(h.data() + G + 2 * n, G, red) ? 8 : 0;
    }
    HIPCHK(hipMemcpy((uint8_t*)p - 1, &poison, 1, hipMemcpyHostToDevice));
    HIPCHK(hipDeviceSynchronize());
    TallyScope mine(&ofCached);
    cache.release(p);
  }
  out[0] = fills; out[1] = ofBuf.violations + ofCached.violations; out[2] = ofBuf.firstWhere; out[3] = ofCached.firstWhere;
  return TALC_OK;
}

static int check_params(const talc_params* p) {
  if (!p) return fail(TALC_ERR_INVALID, "null params");
  if (p->k < 18 || p->k > 31) return fail(TALC_ERR_INVALID, "k=%u outside the supported range 18..31", p->k);
  if (p->min_count < 1) return fail(TALC_ERR_INVALID, "min_count must be >= 1 (reference CLI: >= 2)");
  if (p->coloured_count_thr > 65535) return fail(TALC_ERR_INVALID, "coloured_count_thr must be <= 65535");
  if (p->max_nb_competing_paths < 1 || p->max_nb_competing_paths > 64) return fail(TALC_ERR_INVALID, "max_nb_competing_paths must be in 1..64");
  if (p->max_nb_inner_paths < 1 || p->max_nb_inner_paths > 60) return fail(TALC_ERR_INVALID, "max_nb_inner_paths must be in 1..60");
  if (p->max_start_anchors < 1 || p->max_start_anchors > 64) return fail(TALC_ERR_INVALID, "max_start_anchors must be in 1..64");
  if (p->check_interval < 1) return fail(TALC_ERR_INVALID, "check_interval must be >= 1");
  if (!(p->sr_error_rate > 0)) return fail(TALC_ERR_INVALID, "sr_error_rate must be > 0");
  return TALC_OK;
}

// ------------------------------------------------------------------ table
// Tables travel between the builders as unique_ptr; a raw talc_table* exists only where one crosses the ABI.
using TablePtr = std::unique_ptr<talc_table>;

// the dump lines at or above MIN_COUNT: what a table of these lines stores, duplicates aside (sizes the tables)
static uint64_t count_kept(const uint32_t* counts, uint64_t n, uint32_t min_count) {
  uint64_t kept = 0;
#pragma omp parallel for reduction(+ : kept)
  for (long i = 0; i < (long)n; ++i) kept += counts[i] >= min_count ? 1 : 0;
  return kept;
}

int talc_table_from_arrays(const uint64_t* kmers, const uint32_t* counts, uint64_t n, const talc_params* p,
                           talc_table** out) {
  int rc = check_params(p);
  if (rc) return rc;
  if (!out || (n && (!kmers || !counts))) return fail(TALC_ERR_INVALID, "null argument");
  const uint64_t kept = count_kept(counts, n, p->min_count);
  auto t = std::make_unique<talc_table>();
  t->h.p = *p;
  if (!t->h.allocate(kept, read_switches().tableSlotsX10)) return fail(TALC_ERR_NOMEM, "cannot allocate host table for %llu k-mers", (unsigned long long)kept);
  t->h.insertAll(kmers, counts, n);
  *out = t.release();
  return TALC_OK;
}

// The device builder's core (talc_kernels_build.h): n dump lines as device arrays dK / dC (line i of the dump at index i;
// the kernels drop the lines below MIN_COUNT themselves), `kept` = how many reach MIN_COUNT (sizes the tables).  Takes
// ownership of dK / dC.  The image stays on `device`, staged, until talc_table_upload adopts it.
static int build_table_from_device_arrays(DevBuf<uint64_t> dK, DevBuf<uint32_t> dC, uint64_t n, uint64_t kept, const talc_params* p, int device,
                                          TablePtr& out, double h2d_seconds, double h2d_megabytes, const Switches& sw) {
  if (n >= 0xFFFFFFFEull) return fail(TALC_ERR_INVALID, "the device builder takes fewer than 2^32-2 entries");   // (a bid is index + 1 < 0xFFFFFFFF)
  auto t = std::make_unique<talc_table>();
  t->h.p = *p;
  hipDeviceProp_t prop;   // (sparser than load 0.5 when the device has the room: HostTable::capacity_for)
  const uint64_t devBytes = hipGetDeviceProperties(&prop, device) == hipSuccess ? (uint64_t)prop.totalGlobalMem : 0;
  t->h.capacity = HostTable::capacity_for(kept, devBytes, sw.tableSlotsX10);
  if (t->h.capacity >= (1ULL << 32)) return fail(TALC_ERR_NOMEM, "table of %llu k-mers exceeds 2^32 buckets", (unsigned long long)kept);
  t->hostValid = false;
  const uint64_t cap = t->h.capacity, bytes = cap * sizeof(Bucket);
  DevBuf<uint32_t> dSR, dSL; DevBuf<unsigned long long> dStats; DevBuf<Bucket> dR, dL;
  Stopwatch watch;
  HIPCHK(hipSetDevice(device));
  HIPCHK(dR.alloc(cap)); HIPCHK(dL.alloc(cap));
  HIPCHK(dSR.alloc(std::max<uint64_t>(n, 1))); HIPCHK(dSL.alloc(std::max<uint64_t>(n, 1)));
  HIPCHK(dStats.alloc(3));
  HIPCHK(hipMemset(dR.get(), 0xFF, bytes)); HIPCHK(hipMemset(dL.get(), 0xFF, bytes)); HIPCHK(hipMemset(dStats.get(), 0, 3 * 8));
  HIPCHK(hipDeviceSynchronize());
  const double tClear = watch.lap();
  // claim, resolve, finalize, write.  Finalize comes before the counts are written: a stored count may be any value from
  // MIN_COUNT to 0xFFFFFFFF, a bid may not be 0xFFFFFFFF.  Without lines there is only the finalize pass.
  const unsigned nb = (unsigned)((n + 255) / 256), nbCap = (unsigned)((cap + 255) / 256);
  if (n) {
    hipLaunchKernelGGL(k_build_claim, dim3(nb), dim3(256), 0, 0, dR.get(), dL.get(), cap, p->k, dK.get(), dC.get(), n, p->min_count, dSR.get(), dSL.get());
    hipLaunchKernelGGL(k_build_resolve, dim3(nb), dim3(256), 0, 0, dR.get(), dL.get(), p->k, dK.get(), n, dSR.get(), dSL.get());
    hipLaunchKernelGGL(k_build_finalize, dim3(nbCap), dim3(256), 0, 0, dR.get(), dL.get(), cap, dStats.get());
    hipLaunchKernelGGL(k_build_write, dim3(nb), dim3(256), 0, 0, dR.get(), dL.get(), p->k, dK.get(), dC.get(), n, dSR.get(), dSL.get());
  } else {
    hipLaunchKernelGGL(k_build_finalize, dim3(nbCap), dim3(256), 0, 0, dR.get(), dL.get(), cap, dStats.get());
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  unsigned long long st[3];
  HIPCHK(hipMemcpy(st, dStats.get(), 3 * 8, hipMemcpyDeviceToHost));
  const double tKernels = watch.lap();
  dK.reset(); dC.reset(); dSR.reset(); dSL.reset(); dStats.reset();   // (before the caller colours: only the image stays)
  if (sw.timing) fprintf(stderr, "[talc-lib] device build: %.0f MB to the device %.3f s, table allocations + clears %.3f s, kernels %.3f s, frees %.3f s\n",
                      h2d_megabytes, h2d_seconds, tClear, tKernels, watch.lap());
  DeviceImage& staged = t->images[device];
  staged.right = std::move(dR); staged.left = std::move(dL);
  t->h.nkmers = st[0]; t->h.nbuckets_right = st[1]; t->h.nbuckets_left = st[2];
  out = std::move(t);
  return TALC_OK;
}

int talc_table_from_arrays_device(const uint64_t* kmers, const uint32_t* counts, uint64_t n, const talc_params* p, int device,
                                  talc_table** out) {
  int rc = check_params(p);
  if (rc) return rc;
  if (!out || (n && (!kmers || !counts))) return fail(TALC_ERR_INVALID, "null argument");
  const uint64_t kept = count_kept(counts, n, p->min_count);
  DevBuf<uint64_t> dK; DevBuf<uint32_t> dC;
  Stopwatch watch;
  HIPCHK(hipSetDevice(device));
  HIPCHK(hip_runtime_start());
  HIPCHK(dK.alloc(std::max<uint64_t>(n, 1))); HIPCHK(dC.alloc(std::max<uint64_t>(n, 1)));
  if (n) { HIPCHK(hipMemcpy(dK.get(), kmers, n * 8, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(dC.get(), counts, n * 4, hipMemcpyHostToDevice)); }
  const double h2d = watch.seconds();
  TablePtr t;
  if ((rc = build_table_from_device_arrays(std::move(dK), std::move(dC), n, kept, p, device, t, h2d, (double)n * 12 / 1e6, read_switches()))) return rc;
  *out = t.release();
  return TALC_OK;
}

// The text dump parsed ON the device (talc_kernels_build.h): the file's bytes are read by a few host threads into
// page-locked buffers and copied as they are; two kernels make the builder's arrays.  Returns TALC_OK with *out set, or
// a positive value when the file is not for this route (too small to matter, a line that is not canonical, no memory: 2):
// the caller then parses on the host, as before.
static int parse_on_host_instead() { (void)hipGetLastError(); return 1; }   // (a copy or a launch failed: no error is left behind)
static int parse_on_host_no_memory() { return 2; }                          // (an allocation failed: its owner has left none behind)

// Step 1, the file's bytes to the device as they are: reader threads (one per chunk of chunkBytes, at most maxReaders),
// each with its own descriptor, page-locked buffer and stream, claim the chunks in turn; chunk i lands at byte
// i * chunkBytes of dText (size + 64 bytes).  0, or a positive value when memory or a read failed.
static int text_to_device(const char* path, uint64_t size, uint64_t chunkBytes, int maxReaders, int device, DevBuf<uint8_t>& dText, int* readers) {
  if (dText.alloc(size + 64) != hipSuccess) return parse_on_host_no_memory();
  const uint64_t CH = chunkBytes;
  const uint64_t nch = (size + CH - 1) / CH;
  const int T = (int)std::min<uint64_t>(nch, (uint64_t)maxReaders);
  std::atomic<uint64_t> next{0};
  std::atomic<int> err{0};
#pragma omp parallel num_threads(T)
  {
    int fd = open(path, O_RDONLY);
    PinnedBuf pin;
    hipStream_t st = nullptr;
    bool ok = fd >= 0 && hipSetDevice(device) == hipSuccess;
    if (ok && pin.alloc(CH) != hipSuccess) { ok = false; err.store(2); }   // (2: no memory)
    ok = ok && hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess;
    while (ok && !err.load()) {
      const uint64_t i = next.fetch_add(1);
      if (i >= nch) break;
      const uint64_t off = i * CH, len = std::min<uint64_t>(CH, size - off);
      uint64_t got = 0;
      while (got < len) { const ssize_t r = pread(fd, pin.get() + got, len - got, (off_t)(off + got)); if (r <= 0) { ok = false; break; } got += (uint64_t)r; }
      if (!ok) break;
      if (hipMemcpyAsync(dText.get() + off, pin.get(), len, hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) ok = false;
    }
    if (!ok) { int none = 0; err.compare_exchange_strong(none, 1); }
    if (st) hipStreamDestroy(st);
    if (fd >= 0) close(fd);
  }
  if (err.load()) return err.load() == 2 ? parse_on_host_no_memory() : parse_on_host_instead();
  *readers = T;
  return 0;
}

// Step 2, the device text to the builder's arrays (talc_kernels_build.h): lines per tile, the tiles' first line numbers,
// the lines themselves; line i of the text at index i of out.kmers / out.counts, lines below minc included (out.stats.kept
// counts the others).  The one place the parse kernels are launched from.  0, or a positive value when the text has no
// line, too many, or memory failed; out.stats.flags != 0 when a line is not canonical (the arrays then mean nothing).
struct ParsedText { DevBuf<uint64_t> kmers; DevBuf<uint32_t> counts; uint64_t nlines = 0; ParseStats stats = {0, 0}; };
static int parse_device_text(const uint8_t* dText, uint64_t size, uint32_t K, uint32_t minc, ParsedText& out) {
  const uint64_t ntiles = (size + kParseTile - 1) / kParseTile;
  DevBuf<uint32_t> dCount; DevBuf<uint64_t> dFirst; DevBuf<ParseStats> dPS;
  if (ntiles == 0 || ntiles >= (1ull << 31)) return parse_on_host_instead();
  if (dCount.alloc(ntiles) != hipSuccess || dFirst.alloc(ntiles) != hipSuccess || dPS.alloc(1) != hipSuccess) return parse_on_host_no_memory();
  if (hipMemset(dPS.get(), 0, sizeof(ParseStats)) != hipSuccess) return parse_on_host_instead();
  hipLaunchKernelGGL(k_parse_count, dim3((unsigned)ntiles), dim3(kParseThreads), 0, 0, dText, size, dCount.get());
  std::vector<uint32_t> hCount(ntiles);
  if (hipMemcpy(hCount.data(), dCount.get(), ntiles * 4, hipMemcpyDeviceToHost) != hipSuccess) return parse_on_host_instead();
  std::vector<uint64_t> hFirst(ntiles);
  uint64_t nlines = 0;
  for (uint64_t i = 0; i < ntiles; ++i) { hFirst[i] = nlines; nlines += hCount[i]; }
  if (nlines == 0 || nlines >= 0xFFFFFFFEull) return parse_on_host_instead();
  if (hipMemcpy(dFirst.get(), hFirst.data(), ntiles * 8, hipMemcpyHostToDevice) != hipSuccess) return parse_on_host_instead();
  if (out.kmers.alloc(nlines) != hipSuccess || out.counts.alloc(nlines) != hipSuccess) return parse_on_host_no_memory();
  hipLaunchKernelGGL(k_parse_lines, dim3((unsigned)ntiles), dim3(kParseThreads), 0, 0, dText, size, dFirst.get(), K, minc, out.kmers.get(), out.counts.get(), dPS.get());
  if (hipGetLastError() != hipSuccess || hipMemcpy(&out.stats, dPS.get(), sizeof out.stats, hipMemcpyDeviceToHost) != hipSuccess) return parse_on_host_instead();
  out.nlines = nlines;
  return 0;
}

constexpr uint64_t kDumpChunkBytes = 32ull << 20;   // of the production upload
constexpr int kDumpReaders = 8;

static int table_from_text_on_device(const char* path, const talc_params* p, int device, TablePtr& out, DumpStats& ds, const Switches& sw) {
  struct stat sb;
  if (stat(path, &sb) != 0) return fail(TALC_ERR_IO, "cannot open %s", path);
  const uint64_t size = (uint64_t)sb.st_size;
  if (size < (8u << 20) || sw.hostParse) return 1;
  {   // a Jellyfish 2 count file goes the host's way (talc_jf.h)
    char head[64] = {0};
    FILE* f = fopen(path, "rb");
    if (!f) return fail(TALC_ERR_IO, "cannot open %s", path);
    const size_t got = fread(head, 1, sizeof head, f);
    fclose(f);
    if (jfLooksLike(head, got)) return 1;
  }
  Stopwatch watch;
  if (hipSetDevice(device) != hipSuccess || hip_runtime_start() != hipSuccess) return fail(TALC_ERR_DEVICE, "device %d cannot be used", device);
  DevBuf<uint8_t> dText;
  int T = 0;
  if (text_to_device(path, size, kDumpChunkBytes, kDumpReaders, device, dText, &T)) return 1;
  const double tUp = watch.lap();
  ParsedText parsed;
  if (parse_device_text(dText.get(), size, p->k, p->min_count, parsed)) return 1;
  dText.reset();   // (the text goes before the builder allocates its buckets)
  const ParseStats ps = parsed.stats;
  const uint64_t nlines = parsed.nlines;
  if (ps.flags != 0) {   // a line the device parser does not take: the host's tokeniser decides what every line means
    if (sw.timing) fprintf(stderr, "[talc-lib] the dump has lines that are not 'KMER count': parsing on the host\n");
    return 1;
  }
  if (sw.timing) fprintf(stderr, "[talc-lib] dump parsed on the device: %.0f MB of text to the device in %.3f s (%d reader threads), %llu lines parsed in %.3f s\n",
                      (double)size / 1e6, tUp, T, (unsigned long long)nlines, watch.seconds());
  ds.nread += (int64_t)nlines; ds.nkept += (int64_t)ps.kept;
  return build_table_from_device_arrays(std::move(parsed.kmers), std::move(parsed.counts), nlines, ps.kept, p, device, out, 0.0, 0.0, sw);
}

// Test hook (include/talc_hip.h): the two steps above on a file of any size with the caller's chunk size and reader count
// (where = 1), or parseDumpFile unfiltered (where = 0).
int talc_test_parse_text(const char* path, uint32_t k, uint32_t min_count, int where, int device, uint64_t chunk_bytes, int reader_threads,
                         uint64_t* kmers_out, uint32_t* counts_out, uint64_t capacity, uint64_t* n_lines_out, uint64_t* kept_out,
                         uint64_t* flags_out) {
  if (!path || k < 18 || k > 31 || (where != 0 && where != 1)) return fail(TALC_ERR_INVALID, "bad argument");
  uint64_t n = 0, kept = 0, flags = 0;
  auto report = [&] { if (n_lines_out) *n_lines_out = n; if (kept_out) *kept_out = kept; if (flags_out) *flags_out = flags; };   // (before a capacity error too)
  if (where == 0) {
    std::vector<uint64_t> kmers;
    std::vector<uint32_t> counts;
    DumpStats ds;
    std::string why;
    if (!parseDumpFile(path, k, min_count, false, kmers, &counts, nullptr, ds, &why))
      return why.empty() ? fail(TALC_ERR_IO, "cannot open %s", path) : fail(TALC_ERR_INVALID, "%s", why.c_str());
    n = kmers.size();
    for (uint64_t i = 0; i < n; ++i) kept += counts[i] >= min_count ? 1 : 0;
    flags = ((uint64_t)ds.nread - n) << 32 | (uint64_t)ds.nbad;   // lines read that gave no entry | lines without two tokens
    report();
    if (kmers_out || counts_out) {
      if (capacity < n) return fail(TALC_ERR_CAPACITY, "line buffers too small: need %llu entries", (unsigned long long)n);
      if (kmers_out && n) memcpy(kmers_out, kmers.data(), n * 8);
      if (counts_out && n) memcpy(counts_out, counts.data(), n * 4);
    }
  } else {
    if (device < 0 || chunk_bytes == 0 || chunk_bytes > (1ull << 30) || reader_threads < 1 || reader_threads > 64) return fail(TALC_ERR_INVALID, "bad argument");
    struct stat sb;
    if (stat(path, &sb) != 0) return fail(TALC_ERR_IO, "cannot open %s", path);
    const uint64_t size = (uint64_t)sb.st_size;
    if (size == 0) return fail(TALC_ERR_INVALID, "%s is empty", path);
    if (hipSetDevice(device) != hipSuccess || hip_runtime_start() != hipSuccess) return fail(TALC_ERR_DEVICE, "device %d cannot be used", device);
    DevBuf<uint8_t> dText;
    int T = 0;
    // (the hook has no host route to fall back to: what the production route answers by parsing on the host is an error here)
    if (const int why = text_to_device(path, size, chunk_bytes, reader_threads, device, dText, &T))
      return fail(why == 2 ? TALC_ERR_NOMEM : TALC_ERR_DEVICE, "the text of %s did not reach the device", path);
    ParsedText parsed;
    if (const int why = parse_device_text(dText.get(), size, k, min_count, parsed))
      return fail(why == 2 ? TALC_ERR_NOMEM : TALC_ERR_DEVICE, "the text of %s was not parsed on the device", path);
    n = parsed.nlines; kept = parsed.stats.kept; flags = parsed.stats.flags;
    report();
    if (kmers_out || counts_out) {
      if (capacity < n) return fail(TALC_ERR_CAPACITY, "line buffers too small: need %llu entries", (unsigned long long)n);
      if (kmers_out) HIPCHK(hipMemcpy(kmers_out, parsed.kmers.get(), n * 8, hipMemcpyDeviceToHost));
      if (counts_out) HIPCHK(hipMemcpy(counts_out, parsed.counts.get(), n * 4, hipMemcpyDeviceToHost));
    }
  }
  return TALC_OK;
}

// Junction colouring (Jellyfish.cpp:273-290) on the staged device image: last line wins, both strands.
static int colour_on_device(talc_table* t, talc_table::Images::value_type& staged, const uint64_t* jkmers, const int64_t* jcounts, uint64_t n) {
  if (n == 0) return TALC_OK;
  if (n >= (1ull << 31)) return fail(TALC_ERR_INVALID, "the device colouring takes fewer than 2^31 junction lines");
  HIPCHK(hipSetDevice(staged.first));
  Bucket *right = staged.second.right.get(), *left = staged.second.left.get();
  uint64_t hsize = 1024;
  while (hsize < 4 * n) hsize *= 2;   // two bids per line at most: load <= 0.5
  DevBuf<uint64_t> dJ, dIds; DevBuf<int64_t> dC; DevBuf<unsigned long long> dHK; DevBuf<uint32_t> dHS;
  HIPCHK(dJ.alloc(n)); HIPCHK(dC.alloc(n)); HIPCHK(dIds.alloc(2 * n));
  HIPCHK(dHK.alloc(hsize)); HIPCHK(dHS.alloc(hsize));
  HIPCHK(hipMemcpy(dJ.get(), jkmers, n * 8, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(dC.get(), jcounts, n * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemset(dHK.get(), 0xFF, hsize * 8)); HIPCHK(hipMemset(dHS.get(), 0, hsize * 4));
  const unsigned nb = (unsigned)((2 * n + 255) / 256);
  hipLaunchKernelGGL(k_colour_claim, dim3(nb), dim3(256), 0, 0, right, t->h.capacity, t->h.p.k, dJ.get(), dC.get(), n, t->h.p.coloured_count_thr,
                     dIds.get(), dHK.get(), dHS.get(), hsize - 1);
  hipLaunchKernelGGL(k_colour_write, dim3(nb), dim3(256), 0, 0, right, left, t->h.capacity, t->h.p.k, dJ.get(), dC.get(), n, dIds.get(), dHK.get(), dHS.get(),
                     hsize - 1);
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  t->hostValid = false;
  return TALC_OK;
}
static int decolour_on_device(talc_table* t, talc_table::Images::value_type& staged) {
  HIPCHK(hipSetDevice(staged.first));
  hipLaunchKernelGGL(k_decolour_repeats, dim3(1), dim3(64), 0, 0, staged.second.right.get(), staged.second.left.get(), t->h.capacity, t->h.p.k);
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  t->hostValid = false;
  return TALC_OK;
}

// The tail every table build shares: junction colouring (Jellyfish.cpp:273-290), then the homopolymer de-colouring
// (main.cpp:232); stats = {lines read, lines kept, malformed lines}.  Sets *out on success.
static int table_finish(TablePtr t, const char* junction_path, const talc_params* p, DumpStats& ds, talc_table** out,
                        int64_t stats[3]) {
  int rc;
  if (junction_path && junction_path[0]) {  // Jellyfish.cpp:273-290
    std::vector<uint64_t> jk;
    std::vector<int64_t> jc;
    DumpStats js;
    std::string why;
    if (!parseDumpFile(junction_path, p->k, 0, false, jk, nullptr, &jc, js, &why))
      return why.empty() ? fail(TALC_ERR_IO, "cannot open %s", junction_path) : fail(TALC_ERR_INVALID, "%s", why.c_str());
    ds.nbad += js.nbad;
    if ((rc = talc_table_colour(t.get(), jk.data(), jc.data(), jk.size()))) return rc;
  }
  if ((rc = talc_table_decolour_repeats(t.get()))) return rc;  // main.cpp:232
  if (stats) { stats[0] = ds.nread; stats[1] = ds.nkept; stats[2] = ds.nbad; }
  *out = t.release();
  return TALC_OK;
}

static int table_build_impl(const char* dump_path, const char* junction_path, const talc_params* p, int device, talc_table** out,
                            int64_t stats[3]) {
  int rc = check_params(p);
  if (rc) return rc;
  if (!dump_path || !out) return fail(TALC_ERR_INVALID, "null argument");
  // Jellyfish.cpp:251-269: whitespace-separated "kmer count" per line
  std::vector<uint64_t> kmers;
  std::vector<uint32_t> counts;
  DumpStats ds;
  std::string why;
  const Switches sw = read_switches();   // (TALC_TIMING: where a table build's wall time goes, on stderr)
  Stopwatch watch;
  TablePtr t;
  int viaDevice = 1;   // > 0: not taken
  if (device >= 0) {
    viaDevice = table_from_text_on_device(dump_path, p, device, t, ds, sw);
    if (viaDevice < 0) return viaDevice;
    if (viaDevice == 0 && sw.timing)
      fprintf(stderr, "[talc-lib] dump to table on the device %.3f s (%llu lines)\n", watch.seconds(), (unsigned long long)ds.nread);
  }
  if (viaDevice > 0) {
    if (!parseDumpFile(dump_path, p->k, p->min_count, true, kmers, &counts, nullptr, ds, &why))
      return why.empty() ? fail(TALC_ERR_IO, "cannot open %s", dump_path) : fail(TALC_ERR_INVALID, "%s", why.c_str());
    const double tParse = watch.lap();
    talc_table* built = nullptr;   // (through the ABI's own two builders)
    rc = (device >= 0) ? talc_table_from_arrays_device(kmers.data(), counts.data(), kmers.size(), p, device, &built)
                       : talc_table_from_arrays(kmers.data(), counts.data(), kmers.size(), p, &built);
    t.reset(built);
    if (sw.timing)
      fprintf(stderr, "[talc-lib] dump parse %.3f s (%llu lines), table build on %s %.3f s\n", tParse,
              (unsigned long long)ds.nread, device >= 0 ? "the device (incl. its first HIP call)" : "the host", watch.seconds());
    if (rc) return rc;
  }
  std::vector<uint64_t>().swap(kmers);
  std::vector<uint32_t>().swap(counts);
  return table_finish(std::move(t), junction_path, p, ds, out, stats);
}

int talc_table_build(const char* dump_path, const char* junction_path, const talc_params* p, talc_table** out,
                     int64_t stats[3]) {
  return table_build_impl(dump_path, junction_path, p, -1, out, stats);
}
int talc_table_build_device(const char* dump_path, const char* junction_path, const talc_params* p, int device,
                            talc_table** out, int64_t stats[3]) {
  if (device < 0) return fail(TALC_ERR_INVALID, "device must be >= 0");
  return table_build_impl(dump_path, junction_path, p, device, out, stats);
}

int talc_table_colour(talc_table* t, const uint64_t* jkmers, const int64_t* jcounts, uint64_t n) {
  if (!t || (n && (!jkmers || !jcounts))) return fail(TALC_ERR_INVALID, "null argument");
  if (t->frozen()) return fail(TALC_ERR_STATE, "table already uploaded (immutable)");
  if (auto* staged = t->any_image()) return colour_on_device(t, *staged, jkmers, jcounts, n);   // (not frozen: an image is a staged one)
  t->h.colour(jkmers, jcounts, n);
  return TALC_OK;
}
int talc_table_decolour_repeats(talc_table* t) {
  if (!t) return fail(TALC_ERR_INVALID, "null argument");
  if (t->frozen()) return fail(TALC_ERR_STATE, "table already uploaded (immutable)");
  if (auto* staged = t->any_image()) return decolour_on_device(t, *staged);
  t->h.decolourRepeats();
  return TALC_OK;
}
uint64_t talc_table_size(const talc_table* t) { return t ? t->h.nkmers : 0; }
// presence-filter words for `bitsPerKmer` bits per k-mer (default 20; config 2's k_coverage: 10 bits 2.64 ms, 14 2.49, 20 2.39, 28 2.34)
static uint64_t filter_words_for(uint64_t nkmers, uint64_t bitsPerKmer) {
  return (std::max<uint64_t>(64, (nkmers * bitsPerKmer + 63) / 64) + 7) & ~7ull;   // whole 64-byte blocks
}
// device bytes of one uploaded copy (what talc_table_upload allocated), or — before any upload — of the copy an upload
// would make without the walk tables (whether those are built is decided then, from the free memory)
uint64_t talc_table_device_bytes(const talc_table* t) {
  if (!t) return 0;
  if (const DeviceImage* img = t->first_uploaded()) return img->bytes(t->h.capacity);
  return 2 * t->h.capacity * sizeof(Bucket) + filter_words_for(t->h.nkmers, read_switches().filterBits) * 8;
}

// What an upload adds to the buckets of an image on the current device: the presence filter, the in-degree bits, and the
// walk tables when they fit.  On failure the caller drops what was made (DeviceImage::drop_derived).
static int derive_tables(DeviceImage& img, const HostTable& h, const Switches& sw) {
  Bucket *right = img.right.get(), *left = img.left.get();
  const unsigned nbCap = (unsigned)((h.capacity + 255) / 256);
  // presence filter, from the RIGHT table
  img.filterWords = filter_words_for(h.nkmers, sw.filterBits);
  HIPCHK(img.filter.alloc(img.filterWords));
  HIPCHK(hipMemset(img.filter.get(), 0, img.filterWords * 8));
  if (h.capacity)
    hipLaunchKernelGGL(k_build_filter, dim3(nbCap), dim3(256), 0, 0, right, h.capacity, h.p.k, (unsigned long long*)img.filter.get(), img.filterWords);
  HIPCHK(hipGetLastError());
  // ... and every RIGHT bucket's in-degree into its key word (talc_common.h: the coverage kernel's left degrees)
  if (h.capacity) hipLaunchKernelGGL(k_build_indegree, dim3(nbCap), dim3(256), 0, 0, right, left, h.capacity, (uint32_t)h.p.min_count);
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  // walk tables (WalkEntry, talc_common.h).  Built when they leave the correction batches and their scratch a reserve
  // (64 GB, or a quarter of the device if that is less).  TALC_WALK=0 turns them off, TALC_WALK=1 insists.
  const uint64_t wbytes = h.capacity * sizeof(WalkEntry);
  size_t freeB = 0, totalB = 0;
  HIPCHK(hipMemGetInfo(&freeB, &totalB));
  const uint64_t reserve = std::min<uint64_t>(64ull << 30, (uint64_t)totalB / 4);
  const bool want = sw.walk >= 0 ? sw.walk != 0 : ((uint64_t)freeB >= 2 * wbytes + reserve);
  if (!want || !h.capacity) return TALC_OK;
  if (img.walkRight.alloc(h.capacity) != hipSuccess || img.walkLeft.alloc(h.capacity) != hipSuccess) {
    img.walkRight.reset(); img.walkLeft.reset();
    if (sw.walk == 1) return fail(TALC_ERR_NOMEM, "TALC_WALK=1 but the walk tables (%llu bytes) do not fit the device", (unsigned long long)(2 * wbytes));
    return TALC_OK;
  }
  const uint64_t nthr = 2 * h.capacity;
  hipLaunchKernelGGL(k_build_walk, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, 0, right, left, h.capacity, h.p.k, (uint32_t)h.p.min_count,
                     img.walkRight.get(), img.walkLeft.get());
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  return TALC_OK;
}

// The staged image of `device` is completed where it is (adopted: no copy); any other GPU gets a copy of the host image,
// completed in a record of its own that joins the table only when it is whole.  A failed upload leaves the table as it
// was: a staged image staged, without filter or walk tables.
int talc_table_upload(talc_table* t, int device) {
  if (!t) return fail(TALC_ERR_INVALID, "null table");
  auto* held = t->image(device);
  if (held && held->second.uploaded()) return TALC_OK;
  const Switches sw = read_switches();
  DeviceImage copy;
  DeviceImage& img = held ? held->second : copy;
  int rc;
  if (held) {
    HIPCHK(hipSetDevice(device));
  } else {
    const uint64_t bytes = t->h.capacity * sizeof(Bucket);
    if ((rc = ensure_host(t))) return rc;
    HIPCHK(hipSetDevice(device));
    HIPCHK(copy.right.alloc(t->h.capacity));
    HIPCHK(copy.left.alloc(t->h.capacity));
    HIPCHK(hipMemcpy(copy.right.get(), t->h.right, bytes, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(copy.left.get(), t->h.left, bytes, hipMemcpyHostToDevice));
  }
  if ((rc = derive_tables(img, t->h, sw))) { img.drop_derived(); return rc; }
  if (!held) t->images.emplace(device, std::move(copy));
  return TALC_OK;
}

// ---- the device image as plain bytes (replication across the GPUs of a node: rank 0 builds, the image travels over
// RCCL / xGMI in caller-owned device buffers, every other rank imports it)
uint64_t talc_table_capacity(const talc_table* t) { return t ? t->h.capacity : 0; }
uint64_t talc_table_image_bytes(const talc_table* t) { return t ? t->h.capacity * sizeof(Bucket) : 0; }

int talc_table_export_device(talc_table* t, int device, void* dst_right, void* dst_left) {
  if (!t || !dst_right || !dst_left) return fail(TALC_ERR_INVALID, "null argument");
  auto* at = t->image(device);
  if (!at) return fail(TALC_ERR_STATE, "the table has no image on device %d", device);
  HIPCHK(hipSetDevice(device));
  const uint64_t bytes = t->h.capacity * sizeof(Bucket);
  HIPCHK(hipMemcpy(dst_right, at->second.right.get(), bytes, hipMemcpyDeviceToDevice));
  HIPCHK(hipMemcpy(dst_left, at->second.left.get(), bytes, hipMemcpyDeviceToDevice));
  HIPCHK(hipDeviceSynchronize());
  return TALC_OK;
}

int talc_table_import_device(const talc_params* p, uint64_t capacity, uint64_t n_kmers, const void* src_right, const void* src_left,
                             int device, talc_table** out) {
  int rc = check_params(p);
  if (rc) return rc;
  if (!out || !src_right || !src_left || capacity == 0 || capacity >= (1ULL << 32)) return fail(TALC_ERR_INVALID, "bad argument");
  auto t = std::make_unique<talc_table>();
  t->h.p = *p; t->h.capacity = capacity; t->h.nkmers = n_kmers; t->hostValid = false;
  const uint64_t bytes = capacity * sizeof(Bucket);
  HIPCHK(hipSetDevice(device));
  DeviceImage& staged = t->images[device];
  HIPCHK(staged.right.alloc(capacity)); HIPCHK(staged.left.alloc(capacity));
  HIPCHK(hipMemcpy(staged.right.get(), src_right, bytes, hipMemcpyDeviceToDevice));
  HIPCHK(hipMemcpy(staged.left.get(), src_left, bytes, hipMemcpyDeviceToDevice));
  HIPCHK(hipDeviceSynchronize());
  // an image carries no parameters of its own: what the kernels rely on — every stored count >= MIN_COUNT, keys of K - 1
  // bases — is checked against the parameters given (an image filtered with a lower MIN_COUNT would give wrong regions)
  unsigned long long chk[2] = {~0ull, 0ull};
  DevBuf<unsigned long long> dChk;
  HIPCHK(dChk.alloc(2));
  HIPCHK(hipMemcpy(dChk.get(), chk, sizeof chk, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_image_check, dim3((unsigned)((capacity + 255) / 256)), dim3(256), 0, 0, staged.right.get(), capacity, dChk.get());
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(chk, dChk.get(), sizeof chk, hipMemcpyDeviceToHost));
  const unsigned long long keyBits = 2ull * (p->k - 1);
  if ((chk[0] != ~0ull && chk[0] < p->min_count) || (keyBits < 64 && (chk[1] >> keyBits) != 0ull))
    return fail(TALC_ERR_INVALID, "the image does not belong to these parameters: smallest stored count %llu (MIN_COUNT %u), keys wider than %llu bits: %s",
                chk[0] == ~0ull ? 0ull : chk[0], p->min_count, keyBits, (keyBits < 64 && (chk[1] >> keyBits) != 0ull) ? "yes" : "no");
  *out = t.release();
  return TALC_OK;
}

// what the kernels read of the uploaded image on `device`
static int table_view(talc_table* t, int device, TableView& v) {
  auto* at = t->image(device);
  if (!at || !at->second.uploaded()) return fail(TALC_ERR_STATE, "table not uploaded to device %d", device);
  v = at->second.view(t->h.capacity, t->h.p.k);
  return TALC_OK;
}

// the body of the two device lookup calls.  direction < 0: k_lookup, one (count, colour) per k-mer; 0 / 1: k_next_counts, four
static int lookup_on_device(talc_table* t, int device, const uint64_t* kmers, uint64_t n, int direction, uint32_t* counts, uint32_t* jcounts) {
  if (!t || !kmers || !counts || !jcounts) return fail(TALC_ERR_INVALID, "null argument");
  TableView v;
  int rc = table_view(t, device, v);
  if (rc) return rc;
  if (n == 0) return TALC_OK;
  HIPCHK(hipSetDevice(device));
  const uint64_t width = direction < 0 ? 1 : 4;
  const dim3 grid((unsigned)((n + 255) / 256));
  DevBuf<uint64_t> dk; DevBuf<uint32_t> dc, dj;
  HIPCHK(dk.alloc(n)); HIPCHK(dc.alloc(width * n)); HIPCHK(dj.alloc(width * n));
  HIPCHK(hipMemcpy(dk.get(), kmers, n * 8, hipMemcpyHostToDevice));
  if (direction < 0) hipLaunchKernelGGL(k_lookup, grid, dim3(256), 0, 0, v, dk.get(), n, dc.get(), dj.get());
  else hipLaunchKernelGGL(k_next_counts, grid, dim3(256), 0, 0, v, dk.get(), n, direction, dc.get(), dj.get());
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(counts, dc.get(), n * width * 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(jcounts, dj.get(), n * width * 4, hipMemcpyDeviceToHost));
  return TALC_OK;
}
int talc_table_lookup_batch(talc_table* t, int device, const uint64_t* kmers, uint64_t n, uint32_t* counts,
                            uint32_t* jcounts) {
  return lookup_on_device(t, device, kmers, n, -1, counts, jcounts);
}
int talc_table_next_counts_batch(talc_table* t, int device, const uint64_t* kmers, uint64_t n, int direction,
                                 uint32_t* counts4, uint32_t* jcounts4) {
  return lookup_on_device(t, device, kmers, n, direction ? 1 : 0, counts4, jcounts4);
}

int talc_table_lookup_host_batch(const talc_table* t, const uint64_t* kmers, uint64_t n, uint32_t* counts,
                                 uint32_t* jcounts) {
  if (!t || (n && (!kmers || !counts || !jcounts))) return fail(TALC_ERR_INVALID, "null argument");
  int rc = ensure_host(const_cast<talc_table*>(t));   // (a device-built table: the image is copied back on first use)
  if (rc) return rc;
#pragma omp parallel for schedule(static) if (n > 100000)
  for (long i = 0; i < (long)n; ++i) t->h.lookup(kmers[i], counts[i], jcounts[i]);
  return TALC_OK;
}

// Test hook (not part of the reference surface): the walk table of one direction of the copy on `device`, as it is
int talc_table_fetch_walk(talc_table* t, int device, int direction, void* dst, uint64_t bytes) {
  if (!t || !dst) return fail(TALC_ERR_INVALID, "null argument");
  TableView v;
  int rc = table_view(t, device, v);
  if (rc) return rc;
  const WalkEntry* src = direction ? v.walkRight : v.walkLeft;
  if (!src) return fail(TALC_ERR_STATE, "the copy on device %d has no walk tables", device);
  const uint64_t need = t->h.capacity * sizeof(WalkEntry);
  if (bytes != need) return fail(TALC_ERR_CAPACITY, "a walk table is %llu bytes, %llu given", (unsigned long long)need, (unsigned long long)bytes);
  HIPCHK(hipSetDevice(device));
  HIPCHK(hipMemcpy(dst, src, need, hipMemcpyDeviceToHost));
  return TALC_OK;
}

void talc_table_destroy(talc_table* t) { delete t; }

// ------------------------------------------------------------------ context
int talc_ctx_create(talc_table* t, const talc_params* p, int device, talc_ctx** out) {
  int rc = check_params(p);
  if (rc) return rc;
  if (!t || !out) return fail(TALC_ERR_INVALID, "null argument");
  if (p->k != t->h.p.k) return fail(TALC_ERR_INVALID, "k mismatch between params (%u) and table (%u)", p->k, t->h.p.k);
  if (p->min_count != t->h.p.min_count)
    return fail(TALC_ERR_INVALID, "min_count mismatch between params (%u) and the table it was filtered with (%u)", p->min_count, t->h.p.min_count);
  TableView v;
  rc = table_view(t, device, v);
  if (rc) return rc;
  HIPCHK(hipSetDevice(device));
  auto c = std::make_unique<talc_ctx>();
  c->table = t; c->p = *p; c->device = device; c->view = v;
  c->sw = read_switches();
  memset(&c->timing, 0, sizeof c->timing);
  DevParams& d = c->dp;
  d.K = p->k; d.MIN_COUNT = p->min_count; d.ALPHA = p->alpha; d.WINDOW = p->window_size; d.ERR = p->sr_error_rate;
  d.MIN_INNER = p->min_inner_score; d.MIN_BORDER = p->min_border_score; d.MAXB = p->max_nb_competing_paths;
  d.reverse = p->reverse; d.MIN_START_ANCHORS = p->min_start_anchors; d.MAX_START_ANCHORS = p->max_start_anchors;
  d.MAX_IN_COUNT = p->max_in_count; d.MAX_BORDER_PATHS = p->max_nb_border_paths; d.MAX_INNER_PATHS = p->max_nb_inner_paths;
  d.CHECK_INTERVAL = p->check_interval; d.FAILURE_RATE = p->allowed_failure_rate;
  d.MAX_BORDER_FAILURES = p->max_nb_border_failures; d.MAX_BORDER_LEN = p->max_border_length;
  d.costEdgeLin = 2800; d.costEdgeQuad = 135;
  d.costGapQuad = 10; d.costGapFork = 200; d.costGapCap = 900; d.pad_ = 0;   // (profiles/r03/cost_sweep.txt)
  HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  for (auto& e : c->ev) HIPCHK(hipEventCreate(&e));
  HIPCHK(c->d_queue.alloc(kQueueWords));
  HIPCHK(c->d_hist.alloc(kHistWords));
  HIPCHK(c->d_counters.alloc(kCounterWords));
  if (!c->h_land.resize(kTotWords + kCntWaveLog)) return fail(TALC_ERR_NOMEM, "cannot allocate the context's host landing area");
  {   // isExpectedbyMyModel as two thresholds per count (Explorer.cpp:1185-1201), from the formula itself, for this ALPHA
    const uint32_t n = 4096;
    HIPCHK(c->d_thr.alloc(2ull * n));
    hipLaunchKernelGGL(k_build_thresholds, dim3((n + 255) / 256), dim3(256), 0, c->stream, d.ALPHA, n, c->d_thr.get());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    d.thr = c->d_thr.get(); d.thrN = n; d.pad2_ = 0;
  }
  *out = c.release();
  return TALC_OK;
}

void talc_ctx_destroy(talc_ctx* c) { delete c; }

int talc_ctx_set_map(talc_ctx* c, int on) {
  if (!c) return fail(TALC_ERR_INVALID, "null context");
  c->map = on != 0;
  return TALC_OK;
}

int talc_ctx_set_auto_strand(talc_ctx* c, int on) {
  if (!c) return fail(TALC_ERR_INVALID, "null context");
  if (c->p.reverse) return fail(TALC_ERR_INVALID, "auto strand chooses every read's orientation: it does not go with reverse set in the context's params");
  c->autoStrand = on != 0;
  return TALC_OK;
}

int talc_ctx_get_strand_timing(const talc_ctx* c, float* vote_ms) {
  if (!c) return fail(TALC_ERR_INVALID, "null context");
  if (vote_ms) *vote_ms = c->span[kSpanVote].ms;
  return TALC_OK;
}

int talc_ctx_get_map_timing(const talc_ctx* c, float* pack_map_ms, float* mask_case_ms) {
  if (!c) return fail(TALC_ERR_INVALID, "null context");
  if (pack_map_ms) *pack_map_ms = c->span[kSpanPackMap].ms;
  if (mask_case_ms) *mask_case_ms = c->span[kSpanMaskCase].ms;
  return TALC_OK;
}

int talc_ctx_get_pieces_timing(const talc_ctx* c, float* count_ms, float* pack_ms) {
  if (!c) return fail(TALC_ERR_INVALID, "null context");
  if (count_ms) *count_ms = c->span[kSpanPieceCount].ms;
  if (pack_ms) *pack_ms = c->span[kSpanPiecePack].ms;
  return TALC_OK;
}

int talc_ctx_get_solidity_timing(const talc_ctx* c, float* raw_ms, float* corrected_ms) {
  if (!c) return fail(TALC_ERR_INVALID, "null context");
  if (raw_ms) *raw_ms = c->span[kSpanSolidityRaw].ms;
  if (corrected_ms) *corrected_ms = c->span[kSpanSolidityRecords].ms;
  return TALC_OK;
}

int talc_ctx_get_timing(const talc_ctx* c, talc_timing* out) {
  if (!c || !out) return fail(TALC_ERR_INVALID, "null argument");
  *out = c->timing;
  return TALC_OK;
}

// ------------------------------------------------------------------ batch
void talc_batch_destroy(talc_batch* b) { delete b; }

// The batch laid out on the host from its reads' offsets, its device buffers made and the layout sent; fill(stream) puts the
// n_bases raw bytes into b->d_raw, ordered on that stream behind the upload of the offsets.  Returns once the stream is idle.
extern "C++" {   // (a template has no C linkage)
template <class Fill>
static int batch_build(talc_ctx* c, talc_batch* b, const uint64_t* offsets, uint32_t n_reads, Fill fill) {
  b->ctx = c; b->n_reads = n_reads;
  b->h_state.use_pool(&c->host_pool); b->h_dense_off.use_pool(&c->host_pool); b->h_seg_off.use_pool(&c->host_pool);
  b->h_offsets.assign(offsets, offsets + n_reads + 1);
  if (b->h_offsets[0] != 0) return fail(TALC_ERR_INVALID, "offsets[0] must be 0");
  b->n_bases = b->h_offsets[n_reads];
  const uint32_t K = c->p.k;
  b->h_koff.resize(n_reads + 1);
  b->h_regoff.resize(n_reads + 1);
  b->h_outoff.resize(n_reads + 1);
  uint64_t ko = 0, ro = 0, oo = 0;
  for (uint32_t r = 0; r < n_reads; ++r) {
    if (offsets[r + 1] < offsets[r]) return fail(TALC_ERR_INVALID, "offsets must be non-decreasing");
    const uint64_t L = offsets[r + 1] - offsets[r];
    if (L > 0x7fffff00ull) return fail(TALC_ERR_INVALID, "read %u too long", r);
    b->max_len = std::max<uint32_t>(b->max_len, (uint32_t)L);
    const uint64_t nk = L >= K ? L - K + 1 : 0;
    b->h_koff[r] = ko; ko += nk;
    b->h_regoff[r] = ro; ro += nk / 2 + 2;
    b->h_outoff[r] = oo; oo += out_capacity_for(L);
    for (uint64_t p = 0; p < nk; p += COV_TILE) { b->h_tile_read.push_back(r); b->h_tile_start.push_back((uint32_t)p); }
    for (uint64_t p = 0; p < L; p += 4096) { b->h_chunk_read.push_back(r); b->h_chunk_start.push_back((uint32_t)p); }
  }
  b->h_koff[n_reads] = ko; b->h_regoff[n_reads] = ro; b->h_outoff[n_reads] = oo;
  b->n_kmers = ko;
  hipStream_t s = c->stream;
  int rc;
  HIPCHK(b->d_raw.alloc(c->cache, std::max<uint64_t>(b->n_bases, 1)));
  // (+ 64: a search may read a stretch of a read in place, and the wave routines fetch whole 8- and 16-byte words)
  HIPCHK(b->d_codes.alloc(c->cache, std::max<uint64_t>(b->n_bases, 1) + 64));
  if ((rc = up(c, b->d_offsets, b->h_offsets, s))) return rc;
  if ((rc = fill(s))) return rc;
  if ((rc = up(c, b->d_koff, b->h_koff, s))) return rc;
  if ((rc = up(c, b->d_regoff, b->h_regoff, s))) return rc;
  if ((rc = up(c, b->d_outoff, b->h_outoff, s))) return rc;
  if ((rc = up(c, b->d_tile_read, b->h_tile_read, s))) return rc;
  if ((rc = up(c, b->d_tile_start, b->h_tile_start, s))) return rc;
  if ((rc = up(c, b->d_chunk_read, b->h_chunk_read, s))) return rc;
  if ((rc = up(c, b->d_chunk_start, b->h_chunk_start, s))) return rc;
  HIPCHK(b->d_order.alloc(c->cache, std::max<uint32_t>(n_reads, 1)));   // (run_pipeline orders the queue)
  HIPCHK(b->d_cov.alloc(c->cache, std::max<uint64_t>(b->n_kmers, 1)));
  HIPCHK(b->d_covw.alloc(c->cache, cov_words_total(b->n_kmers, n_reads)));
  HIPCHK(b->d_nin.alloc(c->cache, std::max<uint32_t>(n_reads, 1)));
  HIPCHK(b->d_state.alloc(c->cache, std::max<uint32_t>(n_reads, 1)));
  HIPCHK(b->d_headcov.alloc(c->cache, std::max<uint32_t>(n_reads, 1) * (uint64_t)kHeadCov));
  HIPCHK(b->d_regions.alloc(c->cache, std::max<uint64_t>(ro, 1) * 3));
  HIPCHK(b->d_out.alloc(c->cache, std::max<uint64_t>(oo, 1)));
  HIPCHK(hipStreamSynchronize(s));
  return TALC_OK;
}
}  // extern "C++"

int talc_batch_create(talc_ctx* c, const char* bases, const uint64_t* offsets, uint32_t n_reads, talc_batch** out) {
  if (!c || !offsets || !out || (!bases && n_reads && offsets[n_reads] > 0)) return fail(TALC_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(c->device));
  auto b = std::make_unique<talc_batch>();
  talc_batch* const bp = b.get();
  const int rc = batch_build(c, bp, offsets, n_reads, [&](hipStream_t s) {
    if (bp->n_bases) HIPCHK(hipMemcpyAsync(bp->d_raw.get(), bases, bp->n_bases, hipMemcpyHostToDevice, s));
    return (int)TALC_OK;
  });
  if (rc) return rc;
  *out = b.release();
  return TALC_OK;
}

uint64_t talc_batch_num_kmers(const talc_batch* b) { return b ? b->n_kmers : 0; }
uint64_t talc_batch_num_bases(const talc_batch* b) { return b ? b->n_bases : 0; }

// ---- auto strand (docs/auto_strand.md).  k_strand_vote over the batch's raw bytes (kSpanVote)
static int launch_vote(talc_ctx* c, talc_batch* b) {
  HIPCHK(b->d_strand.ensure(c->cache, b->n_reads));
  HIPCHK(b->d_strand_flag.ensure(c->cache, b->n_reads));
  const int rc = c->span[kSpanVote].around(c->stream, [&] {
    if (b->n_reads)
      hipLaunchKernelGGL(k_strand_vote, dim3(b->n_reads), dim3(64), 0, c->stream, c->view, b->d_raw.get(), b->d_offsets.get(), c->p.min_count, b->n_reads,
                         b->d_strand.get(), b->d_strand_flag.get());
  });
  if (rc) return rc;
  b->holds.voted = true;
  return TALC_OK;
}
// What every entry point that needs the batch's codes does first: codes made under the other setting are dropped with
// everything that came of them, and with auto strand on the vote runs before k_encode
static int prepare_strand(talc_ctx* c, talc_batch* b) {
  if (b->holds.encoded && b->holds.encodedAuto != c->autoStrand) b->holds.drop_codes();
  if (c->autoStrand && !b->holds.voted) return launch_vote(c, b);
  return TALC_OK;
}

static int launch_encode(talc_ctx* c, talc_batch* b) {
  b->holds.encodedAuto = c->autoStrand;
  if (!b->h_chunk_read.empty())
    hipLaunchKernelGGL(k_encode, dim3((unsigned)b->h_chunk_read.size()), dim3(256), 0, c->stream, b->d_raw.get(), b->d_codes.get(),
                       b->d_offsets.get(), b->d_chunk_read.get(), b->d_chunk_start.get(), c->p.reverse ? 1 : 0, b->rev_flags());
  HIPCHK(hipGetLastError());
  b->holds.encoded = true;
  return TALC_OK;
}

int talc_batch_strand(talc_ctx* c, talc_batch* b) {
  int rc;
  if ((rc = enter(c, b, "bad context/batch"))) return rc;
  if (!b->holds.voted && (rc = launch_vote(c, b))) return rc;
  HIPCHK(hipStreamSynchronize(c->stream));
  return read_spans(c);
}

int talc_batch_fetch_strand(talc_ctx* c, talc_batch* b, talc_strand* rows) {
  if (int rc = belong(c, b, "bad context/batch")) return rc;
  if (!b->holds.voted) return fail(TALC_ERR_STATE, "no strand vote has run on this batch (talc_batch_strand, or auto strand and a call that needs the batch's codes)");
  HIPCHK(hipSetDevice(c->device));
  if (rows && b->n_reads) HIPCHK(hipMemcpyAsync(rows, b->d_strand.get(), (size_t)b->n_reads * sizeof(talc_strand), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return read_spans(c);
}
static int launch_coverage(talc_ctx* c, talc_batch* b) {
  HIPCHK(hipMemsetAsync(b->d_nin.get(), 0, std::max<uint32_t>(b->n_reads, 1) * sizeof(int32_t), c->stream));
  if (!b->h_tile_read.empty())
    hipLaunchKernelGGL(k_coverage, dim3((unsigned)b->h_tile_read.size()), dim3(COV_THREADS), 0, c->stream, c->view,
                       b->d_codes.get(), b->d_offsets.get(), b->d_koff.get(), b->d_tile_read.get(), b->d_tile_start.get(), b->d_cov.get(), b->d_covw.get(), b->d_nin.get(),
                       c->p.min_count);
  HIPCHK(hipGetLastError());
  b->holds.covered = true;
  return TALC_OK;
}

// the status a caller sees: a read whose scratch ran out is passed through unchanged
static int32_t read_status(const ReadState& st) { return st.overflow ? TALC_READ_ERROR : st.status; }

// the stage times into c->timing, from the events around the stages.  `last`: the last event recorded and waited for —
// kEvCovered, kEvStructured or kEvEmitted (the whole correction).  search_ms ends with the first k_search; retry_ms spans
// the retry passes (next to nothing when no read overflowed); emit_ms spans the offset kernels, the host's wait for their
// totals and k_pack; a correction that keeps its map has kEvPackMap behind kEvEmitted, and k_pack_map's time goes to its span
static int read_stage_times(talc_ctx* c, CtxEvent last) {
  talc_timing& t = c->timing;
  HIPCHK(hipEventElapsedTime(&t.encode_ms, c->ev[kEvBegin], c->ev[kEvEncoded]));
  HIPCHK(hipEventElapsedTime(&t.coverage_ms, c->ev[kEvEncoded], c->ev[kEvCovered]));
  if (last >= kEvStructured) HIPCHK(hipEventElapsedTime(&t.structure_ms, c->ev[kEvCovered], c->ev[kEvStructured]));
  if (last >= kEvEmitted) {
    HIPCHK(hipEventElapsedTime(&t.search_ms, c->ev[kEvStructured], c->ev[kEvSearched]));
    HIPCHK(hipEventElapsedTime(&t.retry_ms, c->ev[kEvRetry0], c->ev[kEvRetry1]));
    HIPCHK(hipEventElapsedTime(&t.emit_ms, c->ev[kEvRetry1], c->ev[kEvEmitted]));
    if (c->map) HIPCHK(hipEventElapsedTime(&c->span[kSpanPackMap].ms, c->ev[kEvEmitted], c->ev[kEvPackMap]));
  }
  return TALC_OK;
}

// the orientation settled (prepare_strand), k_encode where the batch has no codes yet, k_coverage: kEvBegin, kEvEncoded and
// kEvCovered around the two.  What talc_batch_coverage and the correction (launch_structure) start with
static int launch_encode_coverage(talc_ctx* c, talc_batch* b) {
  int rc;
  if ((rc = prepare_strand(c, b))) return rc;
  HIPCHK(hipEventRecord(c->ev[kEvBegin], c->stream));
  if (!b->holds.encoded && (rc = launch_encode(c, b))) return rc;
  HIPCHK(hipEventRecord(c->ev[kEvEncoded], c->stream));
  if ((rc = launch_coverage(c, b))) return rc;
  HIPCHK(hipEventRecord(c->ev[kEvCovered], c->stream));
  return TALC_OK;
}

int talc_batch_coverage(talc_ctx* c, talc_batch* b) {
  int rc;
  if ((rc = enter(c, b, "bad context/batch"))) return rc;
  if ((rc = launch_encode_coverage(c, b))) return rc;
  HIPCHK(hipStreamSynchronize(c->stream));
  if ((rc = read_stage_times(c, kEvCovered)) || (rc = read_spans(c))) return rc;
  c->timing.n_kmers = b->n_kmers; c->timing.n_bases = b->n_bases;
  return TALC_OK;
}

// the dense vector<colouredCount> of Read.cpp:174-195 exists only here: the device keeps the hits and a bitmap
// (talc_common.h: CovWord).  counts / jcounts / degrees: one entry per k-mer position, any of them may be null
static int expand_coverage(talc_ctx* c, talc_batch* b, uint32_t* counts, uint32_t* jcounts, uint8_t* degrees) {
  if (!b->n_kmers || !(counts || jcounts || degrees)) return TALC_OK;
  // hipMemcpy on the null stream would not be ordered with the context's stream
  HIPCHK(hipStreamSynchronize(c->stream));
  const uint64_t nw = cov_words_total(b->n_kmers, b->n_reads);
  std::vector<uint2> h(b->n_kmers);
  std::vector<CovWord> w(nw);
  HIPCHK(hipMemcpy(h.data(), b->d_cov.get(), b->n_kmers * sizeof(uint2), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(w.data(), b->d_covw.get(), nw * sizeof(CovWord), hipMemcpyDeviceToHost));
  for (uint32_t r = 0; r < b->n_reads; ++r) {
    const uint64_t k0 = b->h_koff[r], nk = b->h_koff[r + 1] - k0;
    const CovWord* rw = w.data() + cov_word_base(k0, r);
    for (uint64_t p = 0; p < nk; ++p) {
      const CovWord& cw = rw[p >> 6];
      uint32_t cx = 0, cy = 0;
      if ((cw.bits >> (p & 63)) & 1ull) {
        const uint64_t idx = (p & ~(uint64_t)(TALC_COV_TILE - 1)) + cw.rank + (uint64_t)__builtin_popcountll(cw.bits & ((1ull << (p & 63)) - 1ull));
        cx = h[k0 + idx].x; cy = h[k0 + idx].y;
      }
      if (counts) counts[k0 + p] = cx;
      if (jcounts) jcounts[k0 + p] = cy & kCovColourMask;
      if (degrees) degrees[k0 + p] = (uint8_t)((cy >> kCovDegRShift) & 0x7Fu);   // right degree, left degree, known flag
    }
  }
  return TALC_OK;
}

int talc_batch_fetch_coverage(talc_ctx* c, talc_batch* b, uint32_t* counts, uint32_t* jcounts, uint64_t* kmer_offsets,
                              int32_t* n_in_kmers) {
  if (int rc = belong(c, b, "bad context/batch")) return rc;
  if (!b->holds.covered) return fail(TALC_ERR_STATE, "coverage has not been computed for this batch");
  HIPCHK(hipSetDevice(c->device));
  int rc;
  if ((rc = expand_coverage(c, b, counts, jcounts, nullptr))) return rc;
  if (kmer_offsets) memcpy(kmer_offsets, b->h_koff.data(), (b->n_reads + 1) * 8);
  if (n_in_kmers && b->n_reads) HIPCHK(hipMemcpy(n_in_kmers, b->d_nin.get(), b->n_reads * 4, hipMemcpyDeviceToHost));
  return TALC_OK;
}

// Test hook (not part of the reference surface): the degree bits k_coverage leaves beside every hit's colour
static_assert(kCovDegLShift == kCovDegRShift + 3 && kCovDegKnown == (1u << (kCovDegRShift + 6)), "the degree byte of talc_batch_fetch_coverage_degrees");
int talc_batch_fetch_coverage_degrees(talc_ctx* c, talc_batch* b, uint8_t* degrees) {
  if (int rc = belong(c, b, "bad context/batch/buffer", degrees)) return rc;
  if (!b->holds.covered) return fail(TALC_ERR_STATE, "coverage has not been computed for this batch");
  HIPCHK(hipSetDevice(c->device));
  return expand_coverage(c, b, nullptr, nullptr, degrees);
}

}  // extern "C"

#include "talc_capi_counter.inc"   // (at file scope: it puts its own entry points inside extern "C")

extern "C" {

#include "talc_capi_correct.inc"
#include "talc_capi_edits.inc"
#include "talc_capi_support.inc"
#include "talc_capi_demux.inc"
#include "talc_capi_umi.inc"
#include "talc_capi_ends.inc"
#include "talc_capi_chimera.inc"

}  // extern "C"
