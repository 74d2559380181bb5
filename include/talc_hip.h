/* talc_hip.h — C ABI of libtalc_hip.so, the MI355X-native replacement of TALC's per-long-read
 * correction hot path (reference: lbroseus/TALC 1.01, paths below are under /root/reference/src).
 *
 * TALC has no plugin/FFI API; the seam this library sits behind is made of two C++ call
 * surfaces of the reference:
 *   (1) the k-mer table surface   Jellyfish.hpp:42-71  + utils.hpp:145
 *   (2) the per-read surface      Read.hpp:43-77, driven by main.cpp:247-308
 * Each entry point below cites the reference interface it replaces.  Plain pointers and sizes
 * only; no C++ or torch types cross the boundary; no exceptions cross the boundary.
 *
 * Error convention (replaces the reference's bool returns / throw std::string,
 * Read.cpp:194,275, main.cpp:298-303): every function returns 0 on success or a negative
 * talc_error; talc_last_error() returns a human-readable message for the calling thread.
 * Per-read outcomes are reported in a status array so the caller can emit the reference's log
 * lines verbatim (main.cpp:290,294).
 *
 * Threading (reference: any number of OpenMP threads on one shared read-only map,
 * main.cpp:247): a talc_table is immutable after talc_table_upload and may be shared by any
 * number of contexts; a talc_ctx is bound to one device + one HIP stream and must be used by
 * one host thread at a time.  The calls that only read an uploaded table (talc_table_lookup_batch,
 * talc_table_next_counts_batch, talc_table_histo) may run from any number of threads beside the
 * contexts that use it; nothing that changes a table, and not talc_table_lookup_host_batch, which
 * may make the host image on first use, runs beside another call on that table (docs/threading.md).
 */
#ifndef TALC_HIP_H
#define TALC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TALC_ABI_VERSION 1

typedef enum talc_error {
  TALC_OK = 0,
  TALC_ERR_INVALID = -1,     /* bad argument / parameter out of the supported range */
  TALC_ERR_IO = -2,          /* cannot open / parse an input file */
  TALC_ERR_NOMEM = -3,       /* host or device allocation failed (the contract: docs/out_of_memory.md) */
  TALC_ERR_DEVICE = -4,      /* HIP runtime error (no GPU, launch failure, ...) */
  TALC_ERR_CAPACITY = -5,    /* caller-provided output buffer too small (needed size reported) */
  TALC_ERR_STATE = -6,       /* call sequence error (e.g. table not uploaded) */
  /* not an error (positive): the batch is complete and valid, but some reads carry TALC_READ_ERROR — they
   * exhausted the device scratch even in the retry pass and are returned unchanged, like any read the
   * reference fails on (main.cpp:298-303 logs and goes on); talc_ctx_get_timing().n_failed says how many */
  TALC_WARN_READ_ERRORS = 1
} talc_error;

/* Per-read status after the main.cpp:247-308 loop body. */
typedef enum talc_read_status {
  TALC_READ_CORRECTED = 0,      /* main.cpp:277-286: corrected sequence returned */
  TALC_READ_SKIPPED_SHORT = 1,  /* main.cpp:262: length <= K; passed through, no log line */
  TALC_READ_NO_SOLID_KMER = 2,  /* main.cpp:294: log "No solid kmer could be found." */
  TALC_READ_NO_STRUCTURE = 3,   /* main.cpp:290: log "Unable to define convenient structure." */
  TALC_READ_ERROR = 4           /* device scratch exhausted even after the retry pass; the read is
                                   passed through unchanged and talc_batch_correct returns
                                   TALC_WARN_READ_ERRORS (> 0: the other records are valid) */
} talc_read_status;

/* The reference's process globals (Settings.cpp:33-63) plus its hard-coded tunables
 * (Explorer.cpp:85-102, Jellyfish.cpp:64, Read.cpp:361,368) as one POD.  Field meaning and
 * defaults are the reference's; talc_params_default() fills them. */
typedef struct talc_params {
  uint32_t k;                       /* K, -k; 18..31 (reference CLI stops at 30, main.cpp:115) */
  uint32_t min_count;               /* gp_MIN_COUNT, --MIN_COUNT (2) */
  double alpha;                     /* gp_ALPHA, --ALPHA_FOR_PRED (2.57) */
  uint32_t window_size;             /* gp_WINDOW_SIZE, --WINDOW_SIZE (9) */
  double sr_error_rate;             /* gp_SR_ERROR_RATE, --SR_ERROR_RATE (0.025) */
  double min_inner_score;           /* gp_MIN_INNER_SCORE (0.7) */
  double min_border_score;          /* gp_MIN_BORDER_SCORE (0.7) */
  uint32_t max_nb_competing_paths;  /* gp_MAX_NB_COMPETING_PATHS, --MAX_NB_BRANCHES (7) */
  int32_t use_junctions;            /* gp_useJunctions: informational; colouring is explicit */
  int32_t reverse;                  /* gp_reverse, -rev */
  uint32_t min_start_anchors;       /* p_MIN_START_ANCHORS (3)        Explorer.cpp:85 */
  uint32_t max_start_anchors;       /* p_MAX_START_ANCHORS (5)        Explorer.cpp:86 */
  uint32_t max_in_count;            /* p_MAX_IN_COUNT (100000)        Explorer.cpp:88 */
  uint32_t max_nb_border_paths;     /* p_MAX_NB_OF_BORDER_PATHS (75)  Explorer.cpp:90 */
  uint32_t max_nb_inner_paths;      /* p_MAX_NB_OF_INNER_PATHS (50)   Explorer.cpp:91 */
  uint32_t check_interval;          /* p_CHECK_INTERVAL (6)           Explorer.cpp:93 */
  double allowed_failure_rate;      /* p_ALLOWED_FAILURE_RATE (0.3)   Explorer.cpp:94 */
  int32_t max_nb_border_failures;   /* p_MAX_NB_BORDER_FAILURES (3)   Explorer.cpp:97 */
  uint32_t coloured_count_thr;      /* colouredCountThr (10000)       Jellyfish.cpp:64; <= 65535 */
  uint32_t max_border_length;       /* head/tail limit (500)          Read.cpp:361,368 */
} talc_params;

typedef struct talc_table talc_table;   /* the SR k-mer table ("SR-dBG", Settings.cpp:50) */
typedef struct talc_ctx talc_ctx;       /* one device + stream + scratch */
typedef struct talc_batch talc_batch;   /* a batch of reads resident in HBM */

int talc_abi_version(void);
const char* talc_last_error(void);
int talc_params_default(talc_params* p);
/* number of visible HIP devices (0 when there is no GPU); never initialises a device */
int talc_device_count(void);
/* Page-locked host memory for the buffers handed to talc_batch_create / talc_batch_fetch_corrected (replaces the
 * StringSets of loadSeqData / outputSeqData, io.cpp:26-75): copies to and from it are DMA transfers that overlap the
 * kernels of another context's batch.  Ordinary (pageable) buffers work everywhere too, only slower.  NULL on failure. */
void* talc_pinned_alloc(uint64_t bytes);
void talc_pinned_free(void* p);

/* ---------------------------------------------------------------- (1) table surface ------
 * Replaces  colouredDBG buildCDBG(int, string& dump, string& junctionDump)   Jellyfish.cpp:236-295
 *           void decolourRepeatsFromDBG(colouredDBG&, K)                     utils.cpp:658-669
 * k-mers are directional (non-canonical, main.cpp:89) unless a table is built on both strands, (1c).  Packed k-mers are 2 bits per base
 * (A=0,C=1,G=2,T=3), first base in the most significant position of the 2K-bit value. */

/* Parse a `jellyfish dump -c` text file ("KMER count" per line, whitespace separated,
 * Jellyfish.cpp:251-269): keeps lines with count >= min_count, first duplicate wins; then,
 * if junction_path is not NULL, colours k-mers from the junction dump (both strands,
 * jcount < coloured_count_thr, Jellyfish.cpp:273-290); then un-colours the 4 homopolymer
 * k-mers (utils.cpp:658-669).  Lines whose k-mer is not K letters of ACGT can never match a
 * query and are counted in stats but not stored.  A count token that does not start with a number
 * (std::stoi throws in the reference, Jellyfish.cpp:259) reads as 0 here.  stats (may be NULL) receives
 * {lines read, lines kept, malformed lines}.
 * Either path may also name a Jellyfish 2 count file (the `.jf` of `jellyfish count`, format "binary/sorted": the file
 * the reference's jellyfish2 query mode would have asked `jellyfish query` about once per look-up,
 * Jellyfish.cpp:323-379,415-467,498-552).  It is recognised by its header and read under the same contract (every
 * record is a "line"; csrc/talc_jf.h); a file that carries that header but does not verify — another format, k-mers
 * of another length than p->k, a body that is not whole records, padding bits set, a zero count — fails with
 * TALC_ERR_INVALID and a message, it is never guessed at. */
int talc_table_build(const char* dump_path, const char* junction_path, const talc_params* p,
                     talc_table** out, int64_t stats[3]);

/* Same build from arrays (dump order = array order; the count >= min_count filter and the
 * first-duplicate-wins rule are applied here).  No colouring, no de-colouring. */
int talc_table_from_arrays(const uint64_t* kmers, const uint32_t* counts, uint64_t n,
                           const talc_params* p, talc_table** out);
/* The same two builders with the insert loop of buildCDBG (Jellyfish.cpp:251-269) run on GPU `device`
 * (parallel text parse on the host, CAS insertion with the first-duplicate-wins rule on the device); the
 * result is an ordinary talc_table, identical in content: every lookup returns what it returns on a
 * host-built table.  The image stays on that GPU: talc_table_colour / talc_table_decolour_repeats run there as
 * kernels (Jellyfish.cpp:273-290: last line wins, both strands; utils.cpp:658-669), talc_table_upload to the
 * same GPU adopts it without a copy, and a host image is only made when something needs one (host lookups, an
 * upload to another GPU).  Fails with TALC_ERR_DEVICE when the GPU cannot be used. */
int talc_table_build_device(const char* dump_path, const char* junction_path, const talc_params* p,
                            int device, talc_table** out, int64_t stats[3]);
int talc_table_from_arrays_device(const uint64_t* kmers, const uint32_t* counts, uint64_t n,
                                  const talc_params* p, int device, talc_table** out);
/* Junction colouring on arrays, in order, both strands (Jellyfish.cpp:278-289). */
int talc_table_colour(talc_table* t, const uint64_t* jkmers, const int64_t* jcounts, uint64_t n);
/* decolourRepeatsFromDBG (utils.cpp:658-669). */
int talc_table_decolour_repeats(talc_table* t);

uint64_t talc_table_size(const talc_table* t);        /* SR_DBG.size() (main.cpp:237) */
/* Device memory of one uploaded copy: the two bucket tables and the presence filter, plus the walk tables
 * (2 * capacity * 32 bytes, as much as the bucket tables: the fast-forward's lookahead records) once an upload has
 * built them; before any upload, the size an upload without walk tables would have.  An upload builds them when they
 * leave a reserve (64 GB, or a quarter of the device if that is less) to the correction batches
 * (547 M k-mers: 70 GB of buckets + 70 GB of walk records + 1.4 GB of filter on a 288 GB device);
 * the environment variable TALC_WALK=0 turns them off, TALC_WALK=1 makes their allocation mandatory. */
uint64_t talc_table_device_bytes(const talc_table* t);

/* Copy the table to `device` (HBM resident, replicated per GPU).  The table becomes
 * immutable.  May be called once per device. */
int talc_table_upload(talc_table* t, int device);

/* The table image of one GPU as plain bytes, for replication across the GPUs of a node (built once,
 * sent to the peers over xGMI): two arrays of talc_table_image_bytes() bytes each (the RIGHT and the LEFT bucket
 * table, talc_table_capacity() buckets of 32 bytes).  export copies them device-to-device into caller-owned DEVICE
 * buffers on `device` (e.g. tensors that a RCCL broadcast then sends); import builds a table on `device` from such
 * buffers (it copies them; the buffers stay the caller's) with the given parameters — the exporter's — and
 * size(); the imported table is then uploaded / used like any other. */
uint64_t talc_table_capacity(const talc_table* t);
uint64_t talc_table_image_bytes(const talc_table* t);
int talc_table_export_device(talc_table* t, int device, void* dst_right, void* dst_left);
int talc_table_import_device(const talc_params* p, uint64_t capacity, uint64_t n_kmers, const void* src_right,
                             const void* src_left, int device, talc_table** out);

/* Test hooks on the uploaded table — the reference's point queries:
 *   getCount(kmer)               Jellyfish.cpp:397-413  -> (count, junction colour) or (0,0)
 *   getNextCounts(kmer, dir)     Jellyfish.cpp:299-321  -> 4 x (count, colour), order A,C,G,T
 * direction: 0 = LEFT, 1 = RIGHT (utils.hpp:56).  Host pointers. */
int talc_table_lookup_batch(talc_table* t, int device, const uint64_t* kmers, uint64_t n,
                            uint32_t* counts, uint32_t* jcounts);
int talc_table_next_counts_batch(talc_table* t, int device, const uint64_t* kmers, uint64_t n,
                                 int direction, uint32_t* counts4, uint32_t* jcounts4);
/* Host-side point query on the host image of the table (verification hook for the table
 * builder; works without a GPU, before talc_table_upload or after it). */
int talc_table_lookup_host_batch(const talc_table* t, const uint64_t* kmers, uint64_t n, uint32_t* counts,
                                 uint32_t* jcounts);
/* Test hook, not part of the reference surface: the walk table of one direction (0 = LEFT, 1 = RIGHT) of the copy on
 * `device`, copied to the host as it stands: talc_table_capacity() records of 32 bytes in bucket order — a 64-bit key
 * (all ones: unused slot) and twelve 16-bit levels, bits 0-12 the largest successor count (0x1FFF: does not fit), bit
 * 13 "exactly one successor >= MIN_COUNT", bits 14-15 that successor's base.  `bytes` must be the table's size;
 * TALC_ERR_STATE when the copy was uploaded without walk tables.  (The in-degree bits an upload writes into the top
 * three bits of every RIGHT key need no hook: talc_table_export_device after the upload copies them.) */
int talc_table_fetch_walk(talc_table* t, int device, int direction, void* dst, uint64_t bytes);
void talc_table_destroy(talc_table* t);

/* ---------------------------------------------------------------- (1b) k-mer counter ------
 * Replaces the first two steps of the reference README's pipeline (README.md:37-49), `jellyfish count -m K` and
 * `jellyfish dump -c`: the short reads are counted on GPU `device` and the table is built from the counts there, with no
 * count file in between.  The contract (docs/kmer_counting.md): in every record, every window of K consecutive bytes
 * that are all one of ACGTacgt counts once; any other byte ends the window; windows never span two records.  k-mers are
 * directional and packed as above.  Counts are 32-bit: a count that would pass 2^32 - 1 fails the counter with
 * TALC_ERR_INVALID, it never wraps.  One host thread uses a counter at a time (as a talc_ctx).  There is no host counter:
 * without a GPU talc_counter_create fails with TALC_ERR_DEVICE. */
typedef struct talc_counter talc_counter;   /* replaces `jellyfish count` + `dump -c` (README.md:37-49) */
/* expected_distinct: a hint that sizes the first hash (0: small); the hash grows on the device as needed. */
int talc_counter_create(const talc_params* p, int device, uint64_t expected_distinct, talc_counter** out);
/* bases / offsets[n_reads+1] as for talc_batch_create.  Returns once the caller's buffers can be reused, without waiting
 * for the kernel; the calls are ordered on the counter's stream.  TALC_ERR_NOMEM names the distinct count reached. */
int talc_counter_add(talc_counter* c, const char* bases, const uint64_t* offsets, uint32_t n_reads);
/* {windows counted, distinct k-mers, distinct k-mers with count >= p->min_count} (waits for the queued batches) */
int talc_counter_stats(talc_counter* c, uint64_t stats[3]);
/* the k-mers with count >= min_count, in no particular order; kmers == NULL: only *n_out.  TALC_ERR_CAPACITY (with
 * *n_out set) when capacity < *n_out. */
int talc_counter_fetch(talc_counter* c, uint32_t min_count, uint64_t* kmers, uint32_t* counts,
                       uint64_t capacity, uint64_t* n_out);
/* The k-mers with count >= p->min_count as a staged device table, as talc_table_build_device makes from a dump that
 * lists the same counts (then junction colouring from junction_path if not NULL, and the homopolymer de-colouring);
 * stats (may be NULL) = {distinct k-mers ("lines read"), kept, malformed junction lines}.  The counter is spent
 * afterwards: only talc_counter_destroy may follow. */
int talc_counter_build_table(talc_counter* c, const char* junction_path, talc_table** out, int64_t stats[3]);
void talc_counter_destroy(talc_counter* c);
/* The short-read filter (docs/sr_filter.md): a 3' adapter clip and a quality floor applied to every batch on the device
 * before it is counted.  Per record S of L bytes: a start p is accepted for an adapter A of m letters when, with
 * o = min(m, L - p) and mm = the number of i < o where S[p+i] and A[i] differ after upper-casing (a byte of S outside
 * ACGTacgt always differs), o >= min_overlap and 100 mm <= max_error_pct o.  clip = the smallest accepted p over all
 * adapters, L without one.  Bytes [clip, L) and every byte j < clip with quality q[j] < 33 + min_qual (Phred+33) are
 * counted as 'N'; everything else is counted as talc_counter_add counts it.  No adapters and min_qual 0: the filter is off
 * and talc_counter_add does exactly what it does on a counter whose filter was never set. */
/* before the first add / add_fastq / add_counts: TALC_ERR_STATE afterwards or on a spent counter.
 * adapters: NUL-terminated, comma-separated, NULL or "" for none; at most 4, each 1..64 letters of ACGTacgt.
 * min_qual 0 (off) or 1..93; min_overlap 0 (: 5) .. 64 and not above the shortest adapter; max_error_pct 0..30. */
int talc_counter_set_filter(talc_counter* c, uint32_t min_qual, const char* adapters,
                            uint32_t min_overlap /* 0: 5 */, uint32_t max_error_pct);
/* talc_counter_add with one quality byte per base, same offsets; quals may be NULL (no floor for this batch).
 * talc_counter_add on a filtered counter acts as this call with quals == NULL.  A filtered counter refuses a record of
 * 2^32 bytes or more (TALC_ERR_INVALID).  talc_counter_stats()[0] counts the windows after masking. */
int talc_counter_add_fastq(talc_counter* c, const char* bases, const char* quals,
                           const uint64_t* offsets, uint32_t n_reads);
/* {records filtered, records with clip < L, bytes clipped (sum of L - clip), bytes below the floor among [0, clip)}
 * (waits for the queued batches); all zero while the filter is off */
int talc_counter_filter_stats(talc_counter* c, uint64_t stats[4]);
/* test hook: the filter alone on one batch. masked_out: the batch's bytes after the pass, record by
 * record without separators, n bytes; clip_out[n_reads]. Counts nothing. */
int talc_test_counter_mask(talc_counter* c, const char* bases, const char* quals, const uint64_t* offsets,
                           uint32_t n_reads, char* masked_out, uint32_t* clip_out);

/* ---------------------------------------------------------------- (1c) both strands ------
 * For short reads that are not forward-stranded, and for `jellyfish count -C` counts (docs/both_strands.md).  rc(x) is
 * the reverse complement of a packed k-mer, canon(x) = min(x, rc(x)) as unsigned integers (A<C<G<T, Jellyfish's -C).
 * The folded count C(y) of a canonical k-mer y is the sum of the counts of every observation whose canonical form is y:
 * a window of a read counts once (a palindromic window too), a counted k-mer `x c` adds c to C(canon(x)), lines of the
 * same k-mer ADD UP (the one deliberate difference from the directional route's first-line-wins), a count of 0 adds
 * nothing.  The table stores, for every y with C(y) >= min_count, y and rc(y) with count C(y) (a palindrome once): an
 * ordinary talc_table, as talc_table_from_arrays_device makes from those entries.  The fold runs on the GPU; there is no
 * host fold: without a GPU these calls fail with TALC_ERR_DEVICE, like the counter. */
/* before the first add / add_counts; TALC_ERR_STATE afterwards or on a spent counter.  A both-strands counter keys every
 * window by canon(x): talc_counter_fetch returns canonical k-mers, talc_counter_stats {windows + entries added, distinct
 * canonical k-mers, canonical k-mers with C >= min_count}, talc_counter_build_table stores both strands of the latter
 * (stats = {distinct canonical k-mers, k-mers stored in the table, malformed junction lines}). */
int talc_counter_set_both_strands(talc_counter* c, int on);
/* counted k-mers (host arrays) into the counter: a directional counter adds counts[i] to kmers[i], a both-strands counter to
 * canon(kmers[i]); may be mixed with talc_counter_add; a k-mer wider than 2K bits is TALC_ERR_INVALID.  An entry with
 * count 0 adds nothing and is not among the "entries added" of talc_counter_stats.  Returns when the entries are in. */
int talc_counter_add_counts(talc_counter* c, const uint64_t* kmers, const uint32_t* counts, uint64_t n);
/* talc_table_build_device / talc_table_from_arrays_device on both strands: a both-strands counter fed by
 * talc_counter_add_counts, then its table.  MIN_COUNT applies to the folded sum.  The text dump is parsed on the device
 * when talc_table_build_device would parse it there, else by the host's tokeniser or the .jf reader.  stats (may be
 * NULL) = {lines read, k-mers stored in the table, malformed lines}. */
int talc_table_build_device_both_strands(const char* dump_path, const char* junction_path, const talc_params* p,
                                         int device, talc_table** out, int64_t stats[3]);
int talc_table_from_arrays_device_both_strands(const uint64_t* kmers, const uint32_t* counts, uint64_t n,
                                               const talc_params* p, int device, talc_table** out);

/* ---------------------------------------------------------------- (1d) k-mer spectrum ------
 * Replaces `jellyfish histo`, the command between counting and correcting (docs/kmer_spectrum.md): the number of distinct
 * k-mers per count, from the counter's hash on the device, and the MIN_COUNT that spectrum suggests.
 * hist has high + 2 entries: hist[c], 1 <= c <= high, the k-mers with count c; hist[high + 1] those with a larger count;
 * hist[0] the used slots with count 0 (0 in practice; the bin stays so that index equals count).
 * stats: distinct = the k-mers, unique = those with count 1, total = the sum of all counts, max_count = the largest. */
typedef struct talc_spectrum_stats { uint64_t distinct, unique, total, max_count; } talc_spectrum_stats;

/* hist: high + 2 entries as above (may be NULL), stats may be NULL.  high: 0 means 10000; otherwise 2 .. 16382, else
 * TALC_ERR_INVALID.  Waits for the queued batches.  Does not spend the counter and changes nothing fetch, stats or
 * build_table return; may be called any number of times, between adds too.  TALC_ERR_STATE on a spent counter.
 * A both-strands counter's spectrum is that of the canonical k-mers with their folded counts. */
int talc_counter_histo(talc_counter* c, uint32_t high, uint64_t* hist, talc_spectrum_stats* stats);

/* Measurement: device time (ms) of the last k_count_histo of this counter. */
int talc_counter_get_histo_timing(const talc_counter* c, float* histo_ms);

/* The same spectrum over the k-mers a table stores: every stored k-mer once with its count.  A both-strands table
 * stores both strands, so both are counted.  Needs the table's image on `device` (a device-built table, or after
 * talc_table_upload(t, device)): TALC_ERR_STATE otherwise.  stats->distinct == talc_table_size(t). */
int talc_table_histo(talc_table* t, int device, uint32_t high, uint64_t* hist, talc_spectrum_stats* stats);

/* Host, pure, needs no GPU.  The solidity threshold a spectrum suggests: its first local minimum.
 * limit: 0 means 32.  L = min(limit, high - 1).
 * valley = the smallest c in [1, L] with hist[c + 1] > 0 and hist[c] <= hist[c + 1]; 0 when there is none.
 * A spectrum that only falls, as shallow RNA-seq does, has no valley.
 * *chosen = max(2, valley) when there is a valley, else fallback.
 * TALC_ERR_INVALID: hist or chosen NULL, high < 2, fallback == 0.  valley_out may be NULL. */
int talc_spectrum_threshold(const uint64_t* hist, uint32_t high, uint32_t limit, uint32_t fallback,
                            uint32_t* chosen, uint32_t* valley_out);

/* Replaces p->min_count of the counter (>= 1, else TALC_ERR_INVALID; TALC_ERR_STATE on a spent counter).
 * talc_counter_stats()[2] and talc_counter_build_table use the new value.  The table carries it, so a context on that
 * table must be created with it (the existing rule of talc_ctx_create). */
int talc_counter_set_min_count(talc_counter* c, uint32_t min_count);

/* ---------------------------------------------------------------- (2) per-read surface ---
 * Replaces, for a whole batch, the loop body of main.cpp:247-308:
 *   Read(id, seq); getLength()>K; reCoverage(); defineStructure2(); correct2(); getCorrSeq()
 * (Read.hpp:43-77) including the -rev handling of main.cpp:253,286. */

/* p->k and p->min_count must be the table's: the fast-forward reads "exactly one successor >= MIN_COUNT" as
 * "the other three are absent" (tagNextNodes, Explorer.cpp:1281-1297), which only holds when the table was
 * filtered with the same MIN_COUNT (Jellyfish.cpp:260). */
int talc_ctx_create(talc_table* t, const talc_params* p, int device, talc_ctx** out);
void talc_ctx_destroy(talc_ctx* c);

/* Upload a batch: `bases` are raw characters (any case; anything but ACGT becomes N exactly
 * like SeqAn's Dna5 conversion), concatenated; offsets[n_reads+1].  Caller-owned, not retained. */
int talc_batch_create(talc_ctx* c, const char* bases, const uint64_t* offsets, uint32_t n_reads,
                      talc_batch** out);
void talc_batch_destroy(talc_batch* b);

/* Read::reCoverage (Read.cpp:174-195) for every read of the batch: the k-mer probe kernel.
 * Results stay on the device — as the hits only: a bitmap word per 64 positions plus the {count, colour} pairs of the
 * k-mers that are in the table; talc_batch_fetch_coverage expands them into the reference's dense vector. */
int talc_batch_coverage(talc_ctx* c, talc_batch* b);
/* counts/jcounts: one entry per k-mer, reads concatenated (read r contributes max(0,L_r-K+1)
 * entries); kmer_offsets[n_reads+1] (may be NULL); n_in_kmers[n_reads] = #{count > min_count}
 * (Read.cpp:190, may be NULL). */
int talc_batch_fetch_coverage(talc_ctx* c, talc_batch* b, uint32_t* counts, uint32_t* jcounts,
                              uint64_t* kmer_offsets, int32_t* n_in_kmers);
uint64_t talc_batch_num_kmers(const talc_batch* b);
uint64_t talc_batch_num_bases(const talc_batch* b);
/* Test hook, not part of the reference surface: what the coverage kernel leaves beside the colour of every k-mer it
 * found in the table, in the dense layout of talc_batch_fetch_coverage (one byte per k-mer position): bits 0-2 the
 * k-mer's out-degree towards RIGHT, bits 3-5 towards LEFT (getOutDegree, Jellyfish.cpp:383-393, 0..4 each), bit 6 "the
 * degrees are known"; 0 for a position whose k-mer is not in the table.  The structure kernel and the anchor search read
 * these instead of probing. */
int talc_batch_fetch_coverage_degrees(talc_ctx* c, talc_batch* b, uint8_t* degrees);

/* The whole hot path on the device: coverage -> structure (defineStructure2) -> path search
 * (correct2) -> reassembly.  Synchronous: returns when the corrected records are in HBM. */
int talc_batch_correct(talc_ctx* c, talc_batch* b);
/* Test hooks, not part of the reference surface.  talc_batch_structure runs the hot path up to and including
 * defineStructure2 (encode, coverage, the structure kernel: the very launches talc_batch_correct starts with) and stops:
 * nothing of the path search runs, so the region lists are as the structure kernel left them (the search edits them in
 * place).  talc_batch_fetch_structure then returns, per read: status (TALC_READ_CORRECTED = a structure was defined),
 * n_regions, lambda (m_priorLambda_noise, Read.cpp:268-269, the double as it is), in_span (sum of end - start + 1 over
 * the regions); region_offsets[n_reads + 1] and, for region i of the batch, regions[2 i], regions[2 i + 1] = start and
 * end (k-mer positions) and region_hits[i] = the index of the start's pair among the read's hits (tile base + hits of
 * the tile below it) with bit 31 set when every position of the region is a hit of one coverage tile; head_counts[16 r
 * ..] = the counts of read r's first 16 k-mer positions (0 beyond its last; all 0 for reads that are too short or have
 * no solid k-mer).  Every output may be NULL; region_capacity = room of regions / region_hits in regions
 * (TALC_ERR_CAPACITY when too small: call once with both NULL to learn region_offsets[n_reads]).  Valid until the next
 * talc_batch_correct on the batch. */
int talc_batch_structure(talc_ctx* c, talc_batch* b);
int talc_batch_fetch_structure(talc_ctx* c, talc_batch* b, int32_t* status, uint32_t* n_regions, double* lambda,
                               uint32_t* in_span, uint64_t* region_offsets, uint32_t* regions, uint32_t* region_hits,
                               uint64_t region_capacity, uint32_t* head_counts);
/* Test hook.  On a batch talc_batch_structure has run on: orders the work queue as talc_batch_correct does before its
 * search and returns it — order[n_reads], read numbers, heaviest bucket first — with bucket[r], the bucket of read r as
 * the host computes it from the read's state and the gap scale the device derived for the batch (the same function the
 * kernels use), and that scale itself (in 1/256) in bucket[n_reads]: bucket has room for n_reads + 1 words.
 * bucket[order[i]] never decreases with i; the order inside a bucket is arbitrary. */
int talc_batch_order(talc_ctx* c, talc_batch* b, uint32_t* order, uint32_t* bucket);
/* Total corrected size (bytes) so the caller can allocate; valid after talc_batch_correct. */
uint64_t talc_batch_corrected_bytes(const talc_batch* b);
/* out: corrected (or passed-through) sequences as upper-case ACGTN text, concatenated in input
 * order; out_offsets[n_reads+1]; status[n_reads] (talc_read_status).  Reads that were not
 * corrected are returned exactly as the reference leaves mySeqs[r] (Dna5-converted; still
 * reverse-complemented under -rev, main.cpp:253 vs :286). */
int talc_batch_fetch_corrected(talc_ctx* c, talc_batch* b, char* out, uint64_t out_capacity,
                               uint64_t* out_offsets, int32_t* status);

/* The correction map (docs/correction_map.md): which stretches of every record are solid stretches of the read, which were
 * replaced by a path through the short-read graph, and which are weak stretches that stayed as they came — what LoRDEC
 * reports as lower case.  talc_ctx_set_map(c, 1) makes every later talc_batch_correct of the context keep it (default off;
 * the records, statuses and counters of a correction do not depend on it).
 *
 * A read with status TALC_READ_CORRECTED has exactly 2 R + 1 segments, R its number of IN regions: head, solid 0, between 0,
 * solid 1, ..., solid R-1, tail, segments of length 0 included.  With regS / regE the regions' first and last k-mer
 * positions as correct2 leaves them (accepted anchors move region ends inward):
 *   solid i    raw [regS[i], regE[i] + K), kind SOLID, out_len = raw_len
 *   between i  raw_start = regE[i] + K, raw_len = max(0, regS[i+1] - raw_start); CORRECTED with the bridge's length as
 *              out_len (which may be 0: the K < len < 2K rule of cutAnchors) when a bridge was accepted, else RAW with
 *              out_len = raw_len
 *   head       raw [0, regS[0]);  tail  raw [regE[R-1] + K, L): CORRECTED with the edge's length when the edge search
 *              succeeded, else RAW — a failed search, an absent border, one longer than max_border_length
 * Every other read (too short, no solid k-mer, no structure, TALC_READ_ERROR) has one RAW segment {0, L, 0, L}.
 * out_start runs on without gaps and the out_len of a read add up to its record's length.  Coordinates are those of the
 * read as the caller gave it and of the record as talc_batch_fetch_corrected returns it: under -rev the segments of a
 * corrected read are flipped (order reversed, raw_start = L - raw_start - raw_len, out_start = outLen - out_start - out_len). */
typedef enum talc_segment_kind { TALC_SEG_SOLID = 0, TALC_SEG_CORRECTED = 1, TALC_SEG_RAW = 2 } talc_segment_kind;
typedef struct talc_segment { uint32_t kind, raw_start, raw_len, out_start, out_len; } talc_segment;
int talc_ctx_set_map(talc_ctx* c, int on);
/* segments of the whole batch; 0 unless the batch's last correction ran with the map on */
uint64_t talc_batch_num_segments(const talc_batch* b);
/* segs: the batch's segments, reads in input order; seg_offsets[n_reads + 1] (may be NULL).  segs == NULL fills only the
 * offsets.  TALC_ERR_CAPACITY (the message names the count needed) when capacity is too small, TALC_ERR_STATE when the
 * batch's last correction ran with the map off. */
int talc_batch_fetch_map(talc_ctx* c, talc_batch* b, talc_segment* segs, uint64_t capacity, uint64_t* seg_offsets);
/* talc_batch_fetch_corrected with every base of a RAW segment in lower case: same offsets, same statuses, same bytes but
 * for the case.  Needs the map (TALC_ERR_STATE without).  The masked records are a second device buffer, made on first use. */
int talc_batch_fetch_corrected_masked(talc_ctx* c, talc_batch* b, char* out, uint64_t out_capacity, uint64_t* out_offsets,
                                      int32_t* status);
/* Measurement: device time (ms) of the context's last map kernels — k_pack_map (the last mapped correction) and
 * k_mask_case (the last masked fetch that had to make its buffer).  Either pointer may be NULL. */
int talc_ctx_get_map_timing(const talc_ctx* c, float* pack_map_ms, float* mask_case_ms);

/* The solidity report (docs/solidity.md): how much of every read the short reads support, before and after the correction —
 * what lordec-stat reports, and what the last column of the reference's stats header (nbInKmers2, Read.cpp:392,413) was to hold.
 * For a sequence S of L bases: n = max(0, L - K + 1); c[i] = the table count of S[i, i + K), 0 when the k-mer is absent or
 * holds an N; position i is solid when c[i] >= MIN_COUNT. */
typedef struct talc_solidity {
  uint32_t n_kmers;       /* n */
  uint32_t n_solid;       /* #{i : c[i] >= MIN_COUNT}                      (header: nbSolidKmers) */
  uint32_t n_in;          /* #{i : c[i] >  MIN_COUNT}, Read.cpp:190        (header: nbInKmers / nbInKmers2) */
  uint32_t n_regions;     /* maximal runs of solid positions               (header: nbSolidReg; no n > 1 condition) */
  uint32_t solid_bases;   /* bases of S covered by at least one solid k-mer: | U [i, i+K) | */
  uint32_t longest_weak;  /* longest run of consecutive non-solid positions, 0 when none */
} talc_solidity;
/* One device pass per row, nothing written per position.  Every read gets a raw row — S = the read as the correction sees
 * it: Dna5-converted, reverse-complemented under -rev — and, when the batch has been corrected, a corrected row: S = its
 * record as talc_batch_fetch_corrected returns it, in that same orientation (under -rev the reverse complement of a
 * corrected read's record; a passed-through record already is in it).  A read that was passed through (too short, no solid
 * k-mer, no structure, TALC_READ_ERROR) has a corrected row equal to its raw row; a read with L < K has all zeros.
 * May be called on any batch: before a correction it computes the raw rows only.  It changes nothing a later
 * talc_batch_correct, talc_batch_fetch_map or talc_batch_fetch_corrected reads. */
int talc_batch_solidity(talc_ctx* c, talc_batch* b);
/* raw / corrected: n_reads rows each, either may be NULL.  TALC_ERR_STATE when talc_batch_solidity has not run since the
 * batch's last correction, and when `corrected` is asked for and the batch had not been corrected when it ran. */
int talc_batch_fetch_solidity(talc_ctx* c, talc_batch* b, talc_solidity* raw, talc_solidity* corrected);
/* Measurement: device time (ms) of the two k_solidity launches of the context's last talc_batch_solidity (corrected: 0 when
 * there were no records).  Either pointer may be NULL. */
int talc_ctx_get_solidity_timing(const talc_ctx* c, float* raw_ms, float* corrected_ms);

/* Trimmed and split output (docs/trim_split.md): the records of a corrected batch cut at their uncorrected stretches, on
 * the device, so that only the kept bytes cross to the host — what lordec-trim and lordec-trim-split make of LoRDEC's
 * lower case.  Everything is in record coordinates: the record as talc_batch_fetch_corrected returns it, the segments as
 * talc_batch_fetch_map returns them.  A byte of a record is weak when it lies in a RAW segment, trusted when it lies in a
 * SOLID or CORRECTED one; segments with out_len 0 hold no byte and never start, end or split anything.
 *   TALC_PIECES_SPLIT  the pieces of a read are its maximal runs of trusted bytes, in record order
 *   TALC_PIECES_TRIM   at most one piece per read: from its first trusted byte to its last, inclusive; weak stretches inside
 *                      it stay (with soft_mask in lower case: the bytes talc_batch_fetch_corrected_masked has there)
 * A piece of fewer than min_len bytes is dropped (0 keeps all).  A read without a trusted byte — every read that was passed
 * through — has no piece.  The pieces of a batch are ordered by read (input order), then by out_start.
 *
 * talc_batch_pieces needs a correction that kept the map (TALC_ERR_STATE otherwise); a mode outside the enum is
 * TALC_ERR_INVALID; soft_mask is ignored in split mode (a piece has no weak byte).  A later call on the same batch replaces
 * the earlier result.  It changes nothing that talc_batch_fetch_corrected, talc_batch_fetch_corrected_masked,
 * talc_batch_fetch_map, talc_batch_solidity or a later talc_batch_correct reads. */
typedef enum talc_piece_mode { TALC_PIECES_TRIM = 1, TALC_PIECES_SPLIT = 2 } talc_piece_mode;
typedef struct talc_piece { uint32_t read, out_start, out_len; } talc_piece;   /* read index in the batch; range of its record */
int talc_batch_pieces(talc_ctx* c, talc_batch* b, int mode, uint32_t min_len, int soft_mask);
/* pieces / their bytes of the whole batch; 0 unless talc_batch_pieces ran since the batch's last correction */
uint64_t talc_batch_num_pieces(const talc_batch* b);
uint64_t talc_batch_pieces_bytes(const talc_batch* b);
/* out: the bytes of the pieces, concatenated; piece_offsets[n_pieces + 1] into it; pieces[n_pieces]; read_piece_offsets[n_reads
 * + 1]: the pieces of read r are pieces[read_piece_offsets[r] .. read_piece_offsets[r + 1]).  Every output may be NULL (out ==
 * NULL with pieces == NULL fills only the offsets).  TALC_ERR_CAPACITY (the message names the size needed) when out_capacity
 * (bytes) or piece_capacity (entries) is too small; TALC_ERR_STATE when talc_batch_pieces has not run since the batch's last
 * correction. */
int talc_batch_fetch_pieces(talc_ctx* c, talc_batch* b, char* out, uint64_t out_capacity, uint64_t* piece_offsets,
                            talc_piece* pieces, uint64_t piece_capacity, uint64_t* read_piece_offsets);
/* Measurement: device time (ms) of k_piece_count and k_piece_pack of the context's last talc_batch_pieces.  Either pointer
 * may be NULL. */
int talc_ctx_get_pieces_timing(const talc_ctx* c, float* count_ms, float* pack_ms);

/* The edit scripts of a correction (docs/correction_edits.md): for every read the run-length list of operations that turns
 * `raw` — the read as the caller gave it, Dna5-converted to upper case — into `rec`, its record as talc_batch_fetch_corrected
 * returns it, segment by segment of the map as talc_batch_fetch_map returns it (under -rev: already in the caller's
 * orientation).  An op is one uint32_t, len << 4 | code, with BAM's codes: I 1 (a base of rec that raw has not), D 2 (a base
 * of raw that rec has not), = 7, X 8.  The script of a read is the concatenation, in segment order, of one part per segment:
 *   SOLID or RAW   out_len x '='; nothing is compared (in a corrected read these stretches of raw and rec are equal)
 *   CORRECTED      with a = raw[raw_start, +raw_len), b = rec[out_start, +out_len), n = |a|, m = |b|:
 *                  n == 0: m x I;  m == 0: n x D;  both 0: nothing;
 *                  n m > max_cells: not aligned — n x D, then m x I, and the segment counts as unaligned;
 *                  otherwise the canonical optimal alignment under unit costs, bytes compared as they are (N == N): with
 *                  D[i][j] the edit distance of a[:i] and b[:j], walk back from (n, m); take the diagonal ('=' or X) when
 *                  i, j > 0 and D[i-1][j-1] + (a[i-1] != b[j-1]) == D[i][j]; else D when i > 0 and D[i-1][j] + 1 ==
 *                  D[i][j]; else I; reverse.  The rule is applied in the caller's orientation.
 * Adjacent equal ops are merged over the whole read, across segment boundaries; an empty read has no op.
 * A read that was passed through has one RAW segment and the script L '='.  Under -rev its record is the reverse complement
 * of the input (main.cpp:253), so that script relates the record to the read as the correction sees it, not as the caller
 * gave it.
 * Row: n_ins and n_del include the bases of unaligned segments, n_unaligned counts those segments, n_ops the read's ops;
 * n_match + n_mismatch + n_del is the read's length, n_match + n_mismatch + n_ins its record's.
 *
 * talc_batch_edits needs a correction that kept the map (TALC_ERR_STATE otherwise).  max_cells: 0 is the default, 1 << 26.
 * One deviation from "every pair of at most max_cells cells is aligned": the alignment's device scratch is bounded by 1 GiB
 * whatever the batch, and one pair may take half of it, so a max_cells beyond 1 << 29 acts as 1 << 29 — a pair of more cells
 * than that is not aligned (n x D, m x I, counted in n_unaligned) however large max_cells is.  A later call on the same batch
 * replaces the earlier result.  It changes nothing that talc_batch_fetch_corrected,
 * talc_batch_fetch_corrected_masked, talc_batch_fetch_map, talc_batch_solidity, talc_batch_pieces or a later
 * talc_batch_correct reads. */
typedef struct talc_edit_row { uint32_t n_match, n_mismatch, n_ins, n_del, n_ops, n_unaligned; } talc_edit_row;
int talc_batch_edits(talc_ctx* c, talc_batch* b, uint64_t max_cells);
/* ops of the whole batch; 0 unless talc_batch_edits ran since the batch's last correction */
uint64_t talc_batch_num_edit_ops(const talc_batch* b);
/* ops: the batch's ops, reads in input order; op_offsets[n_reads + 1]: the ops of read r are ops[op_offsets[r] ..
 * op_offsets[r + 1]); rows[n_reads].  Each may be NULL (ops == NULL fills only offsets and rows).  TALC_ERR_CAPACITY (the
 * message names the count needed) when op_capacity is too small; TALC_ERR_STATE when talc_batch_edits has not run since the
 * batch's last correction. */
int talc_batch_fetch_edits(talc_ctx* c, talc_batch* b, uint32_t* ops, uint64_t op_capacity, uint64_t* op_offsets,
                           talc_edit_row* rows);
/* Measurement: device time (ms) of the context's last edit scripts — align_ms both runs of k_edit_align (the first counts a
 * part's runs, the second writes them), pack_ms k_edit_count and k_edit_pack.  Either pointer may be NULL. */
int talc_ctx_get_edits_timing(const talc_ctx* c, float* align_ms, float* pack_ms);
/* Test hook, not part of the reference surface: the device routine on one pair of ASCII sequences, as the one CORRECTED
 * segment of a one-read batch: its merged script (ops may be NULL: only *n_ops; TALC_ERR_CAPACITY when op_capacity is too
 * small) and *distance = the edit distance the alignment found (la + lb when a side is empty, -1 when the pair is over
 * max_cells and was not aligned).  n_ops and distance may be NULL. */
int talc_test_edit_script(talc_ctx* c, const char* a, uint32_t la, const char* b, uint32_t lb, uint64_t max_cells,
                          uint32_t* ops, uint64_t op_capacity, uint64_t* n_ops, int32_t* distance);
/* Test hook: talc_batch_edits with scratch_bytes (128 .. 1 << 30) in place of the 1 GiB budget, so that the alignments of a
 * small batch run in several rounds; TALC_ERR_INVALID when one pair alone does not fit.  Same result as talc_batch_edits. */
int talc_test_batch_edits(talc_ctx* c, talc_batch* b, uint64_t max_cells, uint64_t scratch_bytes);
/* Test hook: the text-dump parser alone, on a file of any size (talc_table_build_device takes the device route only from
 * 8 MiB on, with chunks of 32 MiB and at most 8 reader threads).  where = 1: the file goes to GPU `device` in chunks of
 * chunk_bytes (1 .. 1 << 30) read by at most reader_threads (1 .. 64) threads and is parsed there; line i of the file at
 * index i of kmers_out / counts_out, lines below min_count included; *kept_out = lines with count >= min_count, *flags_out
 * != 0 when some line is not canonical (the arrays then mean nothing).  where = 0: the host parser, unfiltered, no GPU
 * needed (device, chunk_bytes, reader_threads ignored): one entry per line it read whose k-mer is K letters of ACGT;
 * *kept_out = entries with count >= min_count, *flags_out = (lines read that gave no entry) << 32 | lines without two
 * tokens, so that lines read = *n_lines_out + (*flags_out >> 32).  *n_lines_out = entries; kmers_out and counts_out NULL:
 * only the three numbers (each of those pointers may be NULL); TALC_ERR_CAPACITY when capacity (entries) is too small,
 * with the three numbers set. */
int talc_test_parse_text(const char* path, uint32_t k, uint32_t min_count, int where, int device, uint64_t chunk_bytes,
                         int reader_threads, uint64_t* kmers_out, uint32_t* counts_out, uint64_t capacity,
                         uint64_t* n_lines_out, uint64_t* kept_out, uint64_t* flags_out);
/* Test hooks: poisoned allocations and red zones.  No result may depend on what device memory held before, and no kernel
 * may write outside its buffers; sanitizers cannot say so for device code, these hooks can.  talc_test_set_poison sets a
 * process-wide setting for the allocations made from then on, in every thread: byte = -1 switches it off, 0 .. 255 is the
 * poison; guard_bytes (a multiple of 256, at most 1 MiB) is the size of the red zones.  While it is on, every device buffer
 * the library hands out — a fresh one or one from a context's cache — is filled with byte over its whole capacity before
 * it is used, and has guard_bytes of ~byte in front of it and behind it; the search scratch, the edge boxes and a retry
 * stage are poisoned again before every k_search launch.  When a buffer is given back (to the cache, and again to the
 * runtime) both red zones are read back and compared; a mismatch is counted, nothing aborts.  A buffer made under one
 * setting may be given back under another.  Off, the hooks cost one relaxed load per allocation.  What they cannot see: a
 * read past a red zone, and a stray write that lands inside the same buffer (one wave's scratch slot spilling into the
 * next one's).  TALC_ERR_INVALID for a byte or a guard size outside these ranges. */
int talc_test_set_poison(int byte, uint32_t guard_bytes);
/* The setting as it is now: *byte = -1 when off.  Either pointer may be NULL. */
int talc_test_get_poison(int* byte, uint32_t* guard_bytes);
/* out = {buffers checked, violations, bytes asked for of the first offender, its side << 32 | the offset of the first
 * changed byte inside that red zone}; side 0 is the zone in front of the buffer, 1 the one behind it.  Process-wide, since
 * the library was loaded. */
int talc_test_guard_report(uint64_t out[4]);
/* How many requests the contexts' caches have served with a buffer used before, while the setting was on. */
uint64_t talc_test_cache_reuses(void);
/* Proves that the hooks do something; needs the setting on with red zones (TALC_ERR_STATE otherwise) and a GPU.  Makes one
 * buffer of 1000 bytes of its own and one cached buffer of 1000 bytes served from a used buffer of 2000, reads them back,
 * writes one byte just behind the first and one just in front of the second (both land in the red zones, the library's
 * own memory) and gives both back.  out = {fills: bit 0 the first buffer's bytes are the poison, bit 1 its red zones are
 * ~poison, bits 2 and 3 the same for the cached buffer, its slack included: 15 when all is as specified; the violations
 * the two writes caused: 2; where the first buffer's was found, where the second's was: side << 32 | offset}.  Its
 * checks do not enter talc_test_guard_report. */
int talc_test_guard_selftest(uint64_t out[4]);
/* Test hooks: allocations that fail on request (docs/out_of_memory.md).  talc_test_fail_alloc arms a process-wide setting:
 * kinds is a mask, bit 0 the device requests (every buffer the library asks the runtime for; a request a context's cache
 * serves from its pool is none), bit 1 the page-locked host requests; 0 switches the hook off, a value above 3 is
 * TALC_ERR_INVALID (as are skip < 0 and a real other than 0 or 1).  From the arming call on, the requests of the selected
 * kinds are numbered from 0 in the order they are made, and requests skip .. skip + count - 1 fail; count 0 fails nothing
 * and only counts.  real 0: the library answers the request with hipErrorOutOfMemory itself; real 1: it asks the runtime
 * for 2^60 bytes instead and passes on what the runtime answers, so that the runtime's own error state is that of a true
 * failure.  Switching off keeps the report's numbers.  Off, the hook costs one relaxed load per request. */
int talc_test_fail_alloc(uint32_t kinds, int64_t skip, uint32_t count, int real);
/* out = {device requests seen since the arming call, page-locked requests seen, failures injected, the owner of the last
 * injected failure (1 a buffer of its own, 2 a context's cache, 3 a page-locked buffer, 4 a page-locked host block; 0: none),
 * the bytes it asked for, the code the runtime returned for the last real = 1 failure, the device buffers the library holds
 * now (since it was loaded; the arming call does not reset it), the kinds armed}.  Needs no device. */
int talc_test_alloc_report(uint64_t out[8]);
/* Test hook: the retry passes of the context's last correction (talc_batch_correct, talc_correct_batch, or the one-read
 * correction inside talc_batch_trace_read).  Reads whose per-wave scratch overflowed in the first pass are searched again in
 * a stage with capacities x 8, what is still flagged behind it in one with x 64.  out = {reads the x 8 stage searched, reads
 * the x 64 stage searched, reads still flagged behind the last stage that ran (talc_timing.n_failed: they leave as they
 * came, TALC_READ_ERROR), stages that were refused (the scratch or the work list did not fit: the passes end there)}.  A
 * stage that was refused searched 0 reads; a correction without an overflow reports four zeros.  The library switch
 * TALC_TEST_TINY_CAPS = 1, 2, 3 shrinks the capacities of the first pass, of the x 8 stage as well, of
 * every stage, so that reads get to each of these ends.  Needs no device. */
int talc_test_retry_report(const talc_ctx* c, uint32_t out[4]);

/* Auto strand (docs/auto_strand.md): the k-mer table is directional and a long cDNA read arrives in either orientation; -rev
 * (talc_params.reverse) turns the whole file.  With auto strand every read is corrected in the orientation the short reads
 * support, chosen on the device before the read is encoded.  For a read of L raw bytes, S its Dna5 conversion (acgt accepted
 * in lower case, every other byte N): n = max(0, L - K + 1); f[i] = the table count of S[i, i + K), r[i] = the table count of
 * the reverse complement of S[i, i + K); a count is 0 when the k-mer is absent or holds an N; a palindromic k-mer (even K)
 * counts in both.  The multiset {r[i]} is that of the forward counts of revcomp(S): the rc fields are what a -rev context's
 * raw solidity row reports. */
typedef struct talc_strand {
  uint32_t n_kmers;     /* n */
  uint32_t fwd_solid;   /* #{i : f[i] >= MIN_COUNT} */
  uint32_t fwd_in;      /* #{i : f[i] >  MIN_COUNT}  (Read.cpp:190: what reCoverage counts) */
  uint32_t rc_solid;    /* #{i : r[i] >= MIN_COUNT} */
  uint32_t rc_in;       /* #{i : r[i] >  MIN_COUNT} */
  uint32_t reverse;     /* the choice: 1 iff rc_in > fwd_in, or rc_in == fwd_in and rc_solid > fwd_solid; else 0 */
} talc_strand;
/* A read with L < K has an all-zero row; every tie chooses forward; with an empty table every row is zero apart from n_kmers.
 * With auto strand on, every entry point that needs the batch's codes (talc_batch_coverage, _structure, _correct, _solidity,
 * talc_correct_batch) first runs the vote if it has not yet run on that batch, and from then on read r is treated exactly as
 * a -rev context treats it when rows[r].reverse is 1 and exactly as a plain context does when it is 0: everything fetched —
 * record, status, masked record, map segments, both solidity rows, pieces, edit ops and row, read-stats row — is byte for
 * byte what the chosen one of the two fixed contexts returns for that read, the reference's quirk included that a read passed
 * through under -rev comes out reverse-complemented (main.cpp:253).  Toggling the setting between two calls on one batch has
 * the batch encoded again at the next call that needs codes, as if it were new (what it held from earlier calls is gone).
 * Default off: nothing changes.  TALC_ERR_INVALID when the context's params have reverse set. */
int talc_ctx_set_auto_strand(talc_ctx* c, int on);
/* The vote alone, on any batch, auto strand on or off (once per batch: a later call finds the rows there). */
int talc_batch_strand(talc_ctx* c, talc_batch* b);
/* rows: n_reads rows.  TALC_ERR_STATE when no vote has run on b. */
int talc_batch_fetch_strand(talc_ctx* c, talc_batch* b, talc_strand* rows);
/* Measurement: device time (ms) of the context's last k_strand_vote. */
int talc_ctx_get_strand_timing(const talc_ctx* c, float* vote_ms);

/* Per-base support (docs/base_support.md): one byte for every base, how many of the k-mers that hold it the short reads
 * confirm.  S, n, c[i] and solid[i] as for the solidity report above.  For a base j, 0 <= j < L, with lo = max(0, j - K + 1)
 * and hi = min(j, n - 1):
 *   span[j]  = hi - lo + 1, the k-mer positions whose k-mer holds base j (1 .. K); 0 when n = 0;
 *   cover[j] = #{ i in [lo, hi] : solid[i] }; 0 when n = 0.
 * With the solidity row of the same S: the sum of cover[j] over j is K * n_solid, and #{ j : cover[j] > 0 } is solid_bases. */
enum { TALC_SUPPORT_RAW = 0, TALC_SUPPORT_RECORD = 1 };
typedef struct talc_support_params {
  uint32_t source;     /* TALC_SUPPORT_RAW | TALC_SUPPORT_RECORD */
  uint32_t phred;      /* 0: byte = cover[j] (0..K);  1: byte = 33 + qmin + ((qmax - qmin) * cover[j]) / span[j], integer
                          division; 33 + qmin where span[j] == 0 */
  uint32_t qmin, qmax; /* phred only: 0 <= qmin <= qmax <= 93, else TALC_ERR_INVALID */
} talc_support_params;
/* RAW: S is the read as the correction sees it (Dna5-converted; reverse-complemented under -rev or when auto strand flagged
 * it), and the bytes are laid out as the input reads were given, with the batch's input offsets.  RECORD: S is the record
 * talc_batch_fetch_corrected returns in that same orientation (the corrected row of the solidity report: read back to front
 * and complemented when the read is TALC_READ_CORRECTED without overflow and reverse or its auto-strand flag holds; a record
 * that was passed through as it stands), and the bytes are laid out as the records, with the records' offsets.  Either way
 * byte j of read r describes byte j of what the caller holds: where S was obtained by reverse complement it is the value of
 * S's position L - 1 - j.  May be called on any batch (RECORD: TALC_ERR_STATE before talc_batch_correct); runs k_encode on a
 * batch never encoded and, with auto strand on, the vote if it has not run.  It writes only its own buffer — nothing a later
 * talc_batch_correct, _fetch_map, _solidity, _pieces or _edits reads is touched — and a later call replaces the result. */
int talc_batch_support(talc_ctx* c, talc_batch* b, const talc_support_params* p);
/* Bytes of the last talc_batch_support of b (0 when there is none since the last correction). */
uint64_t talc_batch_support_bytes(const talc_batch* b);
/* out: the bytes (may be NULL), out_offsets: n_reads + 1 entries (may be NULL) — the numbers talc_batch_fetch_corrected
 * writes for RECORD, the input offsets for RAW.  TALC_ERR_STATE when talc_batch_support has not run on b since its last
 * correction; TALC_ERR_CAPACITY, naming the bytes needed, when out_capacity is too small. */
int talc_batch_fetch_support(talc_ctx* c, talc_batch* b, uint8_t* out, uint64_t out_capacity, uint64_t* out_offsets);
/* Measurement: device time (ms) of the k_base_support launch of the context's last talc_batch_support. */
int talc_ctx_get_support_timing(const talc_ctx* c, float* support_ms);

/* Long-read end clean-up (docs/read_ends.md): cDNA primers and poly-A/T tails at the two ends of every read, found on the
 * device from the batch's raw bytes — as the caller gave them, before any orientation (-rev, auto strand).  A byte is
 * upper-cased; a byte outside ACGT is its own letter: it matches no adapter letter and is neither A nor T.
 * Head rule H(S) for a read S of L bytes:
 *   adapter  T = S[0, min(L, window)).  For adapter a of m letters, D_a[e], 1 <= e <= |T|, is the smallest unit-cost edit
 *            distance between the adapter and any substring of T that ends at e (Sellers: top row 0, first column i).
 *            k_a = floor(max_error_pct * m / 100); e is accepted when D_a[e] <= k_a; the adapter's match is the accepted e
 *            with the smallest D_a[e], the largest e among ties; the head's adapter is the one whose match has the largest e,
 *            the lowest index among ties.  adapter_len = e, adapter = index + 1, adapter_err = D; all 0 without a match.
 *   poly-T   U = S[adapter_len, min(L, adapter_len + window)); score(j) = sum over i < j of (+1 if U[i] is 'T', else -2);
 *            p = the smallest j that maximises score; poly_len = p when poly_min > 0 and p >= poly_min, else 0.
 * The tail is H(revcomp(S)): an adapter's reverse complement near the end, and a poly-A run.  Each end is evaluated on the
 * whole read; head = head_adapter_len + head_poly_len, tail likewise; kept_start = head,
 * kept_len = L - head - min(tail, L - head).  orient = +1 when only the tail has a poly run, -1 when only the head has. */
typedef struct talc_end_row {
  uint32_t head_adapter_len, head_poly_len, tail_adapter_len, tail_poly_len;
  uint8_t  head_adapter, head_adapter_err, tail_adapter, tail_adapter_err;  /* adapter: 0 none, else 1-based */
  uint32_t kept_start, kept_len;
  int32_t  orient;
} talc_end_row;
/* adapters: NUL-terminated, comma-separated, NULL or "" for none; at most 4, each 12..64 letters of ACGTacgt.
 * max_error_pct 0..30; poly_min 0 (off) or 8..window; window 0 (: 512) or 32..4096.  TALC_ERR_INVALID names the bad value.
 * No adapters and poly_min 0 switches the clean-up off: nothing of it exists then. */
int talc_ctx_set_ends(talc_ctx* c, const char* adapters, uint32_t max_error_pct, uint32_t poly_min,
                      uint32_t window /* 0: 512 */);
/* The scan (k_read_ends) on the batch's raw bytes, with the context's setting.  On a batch made by
 * talc_batch_create_clipped the rows are those of the scan that made it — of the original reads — and nothing is launched.
 * TALC_ERR_STATE when the clean-up is off (and the batch holds no rows of its making). */
int talc_batch_ends(talc_ctx* c, talc_batch* b);
/* rows: n_reads rows.  TALC_ERR_STATE when no scan has run on b. */
int talc_batch_fetch_ends(talc_ctx* c, talc_batch* b, talc_end_row* rows);
/* talc_batch_create of the kept intervals: the raw bytes go to the device once, the scan runs on them, and the kept
 * intervals are gathered on the device into the batch's text (k_gather).  From then on every call on the batch returns,
 * byte for byte, what it returns on talc_batch_create of the reads clipped on the host — under -rev and auto strand too.
 * TALC_ERR_STATE when the clean-up is off. */
int talc_batch_create_clipped(talc_ctx* c, const char* bases, const uint64_t* offsets, uint32_t n_reads,
                              talc_batch** out);
/* Measurement: device time (ms) of the context's last k_read_ends and the k_gather of its last clipped batch.  Either pointer may be NULL. */
int talc_ctx_get_ends_timing(const talc_ctx* c, float* scan_ms, float* gather_ms);

/* Chimeric long reads (docs/chimeras.md): the adapters of the end clean-up searched over the whole of every read, on both
 * strands, and the reads cut where they are found.  Codes as above: bytes are upper-cased, a byte outside ACGT matches nothing.
 * Adapter a of m letters gives two patterns, strand 0 the adapter and strand 1 its reverse complement, both matched against
 * the read S (L bytes) as it lies.  For a pattern, D[e], 1 <= e <= L, is the Sellers distance of the pattern against the
 * substrings of S that end at e (top row 0, first column i); k_a = floor(max_error_pct * m / 100); C[e] = min(D[e], k_a + 1);
 * w = ceil(m / 2).  Column e is a hit end when C[e] <= k_a, C[e] < C[e'] for every e < e' <= min(L, e + w), and
 * C[e] <= C[e'] for every max(1, e - w) <= e' < e.  The hit is [e - j, e), j the smallest j >= 0 for which the global
 * unit-cost edit distance of the pattern and S[e - j, e) is D[e]; err = D[e].  A batch's hits are ordered by
 * (read, end, adapter, strand). */
typedef struct talc_chimera_hit {
  uint32_t read, start, end;
  uint8_t  adapter;  /* 1-based */
  uint8_t  strand;   /* 0 as given, 1 reverse complement */
  uint8_t  err;
  uint8_t  pad;
} talc_chimera_hit;  /* 16 bytes */
/* The pieces of a read with at least one hit are the maximal non-empty intervals of [0, L) that no hit's [start, end)
 * covers, in order; those shorter than min_piece are dropped and the kept ones numbered from 1 (such a read may keep none).
 * A read without a hit is one piece [0, L) with ordinal 0, whatever its length. */
typedef struct talc_split_piece {
  uint32_t read, start, len;
  uint32_t ordinal;  /* 1-based among the read's kept pieces; 0 for an uncut read */
} talc_split_piece;
/* on != 0 switches the scan on with its own bound max_error_pct (0..30) and min_piece; the adapters are those of the
 * context's ends setting at the time of each scan.  TALC_ERR_INVALID names the bad value and changes nothing. */
int talc_ctx_set_chimera(talc_ctx* c, int on, uint32_t max_error_pct, uint32_t min_piece);
/* The scan (k_read_chimera) on the batch's raw bytes; on a plain batch once per setting, on a batch made by
 * talc_batch_create_split never: its hits are those of the source reads.  TALC_ERR_STATE while the setting is off or the
 * ends setting holds no adapter (and the batch holds no hits of its making), and on a batch made by
 * talc_batch_create_clipped: it no longer holds the reads as they came, in which the hits are positions. */
int talc_batch_chimera(talc_ctx* c, talc_batch* b);
uint64_t talc_batch_num_chimera_hits(const talc_batch* b);
/* hits: capacity entries (may be NULL with capacity 0); read_hit_offsets: one per scanned read, plus one (may be NULL).
 * TALC_ERR_CAPACITY names the size needed; TALC_ERR_STATE when no scan has run on b. */
int talc_batch_fetch_chimera(talc_ctx* c, talc_batch* b, talc_chimera_hit* hits, uint64_t capacity, uint64_t* read_hit_offsets);
/* talc_batch_create of the kept pieces: the bytes go to the device once, the scan runs on them, the host computes the
 * pieces from the hits and k_gather fills the batch's text.  The batch has one read per piece.  clip != 0 (needs the
 * end clean-up, else TALC_ERR_STATE): the pieces are gathered into a staging text and the batch is made from it as
 * talc_batch_create_clipped makes one, so the end rule applies to every piece.  From then on every call on the batch
 * returns, byte for byte, what it returns on talc_batch_create of the pieces cut (and clipped) on the host. */
int talc_batch_create_split(talc_ctx* c, const char* bases, const uint64_t* offsets, uint32_t n_reads, int clip,
                            talc_batch** out);
uint64_t talc_batch_num_split_pieces(const talc_batch* b);
/* pieces: talc_batch_num_split_pieces rows; read_piece_offsets: n_reads + 1 of the source reads.  Either may be NULL.
 * TALC_ERR_STATE on a batch that talc_batch_create_split did not make. */
int talc_batch_fetch_split(talc_ctx* c, talc_batch* b, talc_split_piece* pieces, uint64_t* read_piece_offsets);
/* Measurement: device time (ms) of the context's last k_read_chimera and the k_gather of its last split batch's pieces.  Either pointer may be NULL. */
int talc_ctx_get_chimera_timing(const talc_ctx* c, float* scan_ms, float* gather_ms);

/* Barcode demultiplexing (docs/demux.md): the sample barcode of every read, called on the device from the batch's raw bytes.
 * B barcodes of one length m; k = floor(max_error_pct * m / 100).  Codes as above: bytes are upper-cased, a byte outside ACGT
 * matches nothing.  End rule E(S) for a read S of L bytes: T = S[0, min(L, window)); for barcode b, D_b[e], 1 <= e <= |T|,
 * is the Sellers distance of the barcode against the substrings of T that end at e (top row 0, first column i);
 * d_b = min over e of D_b[e] (m when T is empty); c_b = min(d_b, k + 1).  best is the b with the smallest c_b, the lowest
 * index among ties; it is accepted when c_best <= k: err = c_best, end = the largest e with D_best[e] = d_best,
 * margin = (the smallest c_b of the other barcodes, k + 1 when there is none) - err; otherwise best, err, end and margin
 * are 0.  The end calls best when it is accepted and margin >= min_margin.  The head is E(S), the tail E(revcomp(S)); each
 * end is evaluated on the whole read.  With h and t the two calls (0: none): h == t != 0 gives barcode h, status BOTH;
 * only h gives status HEAD_ONLY and only t TAIL_ONLY, with that barcode when both_ends is 0 and barcode 0 when it is 1;
 * h != t, both called, gives barcode 0, status CONFLICT; neither gives 0, NONE. */
enum talc_demux_status { TALC_DEMUX_NONE = 0, TALC_DEMUX_BOTH = 1, TALC_DEMUX_HEAD_ONLY = 2, TALC_DEMUX_TAIL_ONLY = 3, TALC_DEMUX_CONFLICT = 4 };
typedef struct talc_demux_row {
  uint8_t  barcode, status;                  /* barcode: 0 none, else 1-based in the order given */
  uint8_t  head_best, head_err, head_margin; /* filled whenever the end's best is accepted, called or not */
  uint8_t  tail_best, tail_err, tail_margin;
  uint32_t head_end, tail_end;               /* tail_end counts from the read's end */
} talc_demux_row;  /* 16 bytes */
/* barcodes: NUL-terminated, comma-separated; 1..96 of one length 12..64, letters of ACGTacgt; NULL or "" switches the
 * setting off.  max_error_pct 0..30; min_margin 0..k + 1; window 0 (: 256) or 32..4096; both_ends 0 or 1.  TALC_ERR_INVALID
 * names the bad value and changes nothing.  The barcodes' match masks live in a small device buffer of the context, written
 * here and freed with the context.  Never switched on: nothing of it exists. */
int talc_ctx_set_demux(talc_ctx* c, const char* barcodes, uint32_t max_error_pct, uint32_t min_margin,
                       uint32_t window /* 0: 256 */, int both_ends);
/* The scan (k_read_demux) on the batch's raw bytes; on a plain batch once per setting.  talc_batch_create_clipped and
 * talc_batch_create_split run it themselves on the reads as they came when the setting is on, and on such a batch nothing
 * is ever launched: its rows are those.  TALC_ERR_STATE when the setting is off (and the batch holds no rows of its making). */
int talc_batch_demux(talc_ctx* c, talc_batch* b);
/* rows: one per source read — n_reads of a plain or clipped batch, the reads a split batch was made from.
 * TALC_ERR_STATE when no scan has run on b. */
int talc_batch_fetch_demux(talc_ctx* c, talc_batch* b, talc_demux_row* rows);
/* Measurement: device time (ms) of the context's last k_read_demux; 0 after a talc_batch_demux that found the rows made. */
int talc_ctx_get_demux_timing(const talc_ctx* c, float* scan_ms);

/* UMI read-out (docs/umi.md): one degenerate pattern found at either end of every read, aligned on the device, and the
 * read's bases under the pattern's degenerate positions reported.  pattern: m = 12..64 letters of ACGTRYSWKMBDHVN in
 * either case; a letter stands for its IUPAC set of bases; the degenerate positions are those whose set has more than one
 * base, u = 1..32 of them.  k = floor(max_error_pct * m / 100).  Codes as above: a read byte is upper-cased, a byte outside
 * ACGT matches nothing.  End rule U(S) for a read S of L bytes, T = S[0, min(L, window)): D[i][j] is the Sellers matrix of
 * the pattern against T (top row 0, first column i, substitution 0 when T[j-1] is in the set of pattern letter i, else 1,
 * indel 1); d = min over j >= 1 of D[m][j], m for an empty T; the end is accepted when d <= k: err = d, stop = the largest
 * j with D[m][j] = d.  The canonical alignment is the traceback from (m, stop) that at (i, j), i > 0, takes the first that
 * holds of: the diagonal, when j > 0 and D[i-1][j-1] + cost = D[i][j]; up, when D[i-1][j] + 1 = D[i][j] (pattern letter i
 * faces a gap); left (T[j-1] is an inserted base).  It ends at i = 0, and start is the j it ends at.  The UMI is u
 * characters, one per degenerate position in pattern order: the upper-cased text base the diagonal step put under it
 * (mismatches included), N when that byte is not of ACGT, - when the position faces a gap.  The head is U(S), the tail
 * U(revcomp(S)): the UMI of a tail hit is in the pattern's orientation, start and stop count from the read's end.  The
 * read's UMI is that of the accepted end with the smaller err, the head's on equal err. */
typedef struct talc_umi_row {
  uint8_t  end, err, other_err, umi_len;     /* end: 1 head, 2 tail, 0 none; other_err: the other end's err when it is
                                                accepted too, else 255; umi_len: u, 0 without a UMI */
  uint32_t start, stop;                      /* 0 without a UMI */
  uint32_t kept_start, kept_len;             /* always set: cut_head = stop when end = 1, cut_tail = stop when end = 2;
                                                with head and tail what the end clean-up claims (0 on a plain batch and
                                                without it), head' = max(head, cut_head), tail' likewise:
                                                kept_start = head', kept_len = L - head' - min(tail', L - head') */
  char     umi[32];                          /* zero-padded */
  uint32_t pad_;
} talc_umi_row;  /* 56 bytes */
/* pattern: NUL-terminated; NULL or "" switches the setting off.  max_error_pct 0..30; window 0 (: 256) or 32..4096.
 * TALC_ERR_INVALID names the bad value and changes nothing.  Never switched on: nothing of it exists.  With the setting
 * on, talc_batch_create_clipped (allowed then with the end clean-up off too) and the clipping of talc_batch_create_split
 * run the scan on the text the end scan runs on, once per read or piece, and cut at kept_start, kept_len; the end rows
 * stay what the end scan wrote. */
int talc_ctx_set_umi(talc_ctx* c, const char* pattern, uint32_t max_error_pct, uint32_t window /* 0: 256 */);
/* The scan (k_read_umi) on the batch's raw bytes; on a plain batch once per setting.  On a clipped or split batch nothing
 * is ever launched: its rows are those of the scan that made it.  TALC_ERR_STATE when the setting is off and the batch
 * holds no rows. */
int talc_batch_umi(talc_ctx* c, talc_batch* b);
/* rows: one per read of the batch.  TALC_ERR_STATE when no scan has run on b. */
int talc_batch_fetch_umi(talc_ctx* c, talc_batch* b, talc_umi_row* rows);
/* Measurement: device time (ms) of the context's last k_read_umi; 0 after a talc_batch_umi that found the rows made. */
int talc_ctx_get_umi_timing(const talc_ctx* c, float* scan_ms);

/* The rows Read::outputBasicReadStats (Read.cpp:418-433) appends to <o>.stats_basics.txt — the reference has the call
 * commented out (main.cpp:305), so its file only ever holds the header; the numbers exist on the device anyway.
 * stats5[5 r ..] = {row written (length > K, main.cpp:262), raw length, sum over the IN regions of end - start + 1 as
 * they stand after the read's last step (Read.cpp:423), number of IN regions, length of the correction (0 unless the
 * read was corrected)}.  Valid after talc_batch_correct. */
int talc_batch_fetch_read_stats(talc_ctx* c, talc_batch* b, int64_t* stats5);

/* Same records, copied device-to-device into a caller-owned DEVICE buffer (e.g. a tensor that
 * is then gathered over RCCL); out_offsets/status are host arrays and may be NULL. */
int talc_batch_copy_corrected_device(talc_ctx* c, talc_batch* b, void* device_out, uint64_t out_capacity,
                                     uint64_t* out_offsets, int32_t* status);

/* Convenience: create + correct + fetch + destroy. */
int talc_correct_batch(talc_ctx* c, const char* bases, const uint64_t* offsets, uint32_t n_reads,
                       char* out, uint64_t out_capacity, uint64_t* out_offsets, int32_t* status);

/* ---------------------------------------------------------------- measurement -----------
 * HIP-event timings (ms) of the kernels launched by the last talc_batch_coverage /
 * talc_batch_correct call on this context's stream, and work counters. */
typedef struct talc_timing {
  float encode_ms;        /* ASCII -> Dna5 codes (+ reverse complement) */
  float coverage_ms;      /* k-mer probe kernel (a4) */
  float structure_ms;     /* defineStructure2 kernel (a5-a9) */
  float search_ms;        /* path-search kernel (a10-a22) */
  float emit_ms;          /* reassembly / output kernel */
  float retry_ms;         /* second pass for reads whose scratch overflowed */
  uint64_t n_kmers;       /* k-mers probed by the coverage kernel */
  uint64_t n_bases;       /* raw bases in the batch */
  uint64_t n_trail_steps; /* successor probes issued by the search kernel (Trail-steps) */
  uint64_t n_dp_cells;    /* DP cells evaluated by the search kernel */
  uint32_t n_retried;     /* reads that needed the big-scratch retry pass */
  uint32_t n_failed;      /* reads with TALC_READ_ERROR */
} talc_timing;
int talc_ctx_get_timing(const talc_ctx* c, talc_timing* out);

/* Debug hook: textual trace of one read of a batch (regions, anchors, per-gap results) in the
 * same line format as the test oracle's trace; used to localise divergences.  Returns the
 * number of bytes needed (including the NUL). */
int64_t talc_batch_trace_read(talc_ctx* c, talc_batch* b, uint32_t read_index, char* buf, uint64_t cap);

/* Test hook: one wave-cooperative DP primitive on the device (mode 0: alignment score,
 * 1: seed-and-extend, 2: k-mer window search, 3: successor tagging); out: 12 ints; not part of the
 * reference surface.  Mode 3 tags by the count model's formula (p1 == 0: a = 4 counts, 4 colours and the count as nine
 * little-endian 32-bit words, p0 = complex; out = 4 tags and 4 distances), or (p1 != 0) as the search does: through
 * the context's threshold table for counts below 4096, the formula beyond; a = p2 such records (at least one), out =
 * max(12, p2) ints, out[i] = the tags of record i in 4 bits each (tag & 15) | "the table was used" << 16. */
int talc_test_dp(talc_ctx* c, int mode, const char* a, int la, const char* b, int lb, int p0, int p1, int p2, int p3,
                 int32_t* out);

#ifdef __cplusplus
}
#endif
#endif /* TALC_HIP_H */
