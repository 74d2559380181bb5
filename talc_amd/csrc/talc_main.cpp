// talc_main.cpp — the drop-in `talc` command line over libtalc_hip.so.
//
// Keeps the reference's CLI / Settings / output-file surface (main.cpp:83-325, Settings.cpp:74-185, io.cpp:26-111,
// Read.cpp:394-415) and replaces its load-everything / per-read OpenMP loop / write-everything (main.cpp:209-310) by a
// pipeline (class Pipeline below): one reader thread parses batches of --batch-reads reads into a small pool of
// page-locked buffers, two workers per GPU (a talc_ctx each, the k-mer table replicated on every GPU) take the batches as
// they come, correct them and format the records, one writer thread appends the batches' text in input order.
// main() is the list of the reference's phases.  Pure host code (g++): it only talks to the C ABI.
//
// Options = the reference's table (same names, defaults, ranges), plus:
//   --gpus N         number of GPUs to use (default: all visible)
//   --batch-reads N  reads per device batch (default: two or more batches per worker — two workers per GPU —, 20000..200000)
//   --read-stats     append the per-read rows of Read::outputBasicReadStats (Read.cpp:418-433) to <o>.stats_basics.txt
//                    (the reference has that call commented out, main.cpp:305, and only ever writes the header)
//   --corr-map       write <o>.map.tsv, the correction map (docs/correction_map.md): one line per segment of every read,
//                    in input order: read_name kind(S|C|R) raw_start raw_len out_start out_len
//   --soft-mask      the bases of <o>.fa that were not corrected (RAW segments) in lower case, as LoRDEC writes them
//   --solidity       write <o>.solidity.tsv, the solidity report (docs/solidity.md): one line per read, in input order, with
//                    the short-read support of the read and of its record; one summary line on stdout
//   --trim          write <o>.trim.fa: every read cut down to the stretch from its first to its last trusted (solid or
//                    corrected) base, cut on the device (docs/trim_split.md); reads without one are left out
//   --split         write <o>.split.fa: every read split at its uncorrected stretches, pieces named name_1, name_2, ...
//   --min-piece-len N  with --trim / --split: pieces of fewer than N bases are dropped (default 0)
//   --corr-edits    write <o>.edits.tsv, the edit script of every read (docs/correction_edits.md): one line per read, in
//                    input order, with the counts of matches, mismatches, insertions and deletions and a CIGAR string
//   --max-edit-cells N  with --corr-edits: a corrected stretch of more than N cells (raw x corrected length) is not aligned
//   --auto-strand    every read is corrected in the orientation the short reads support, chosen on the device (docs/
//                    auto_strand.md); writes <o>.strand.tsv: one line per read, in input order, with the vote and the choice
//   --fastq         write <o>.fq beside <o>.fa: the same records with a quality for every base, made on the device from the
//                    short reads' support of the k-mers that hold it (docs/base_support.md); with --trim / --split also
//                    <o>.trim.fq / <o>.split.fq
//   --qual-range MIN,MAX  with --fastq: the qualities of a base no solid k-mer holds and of one all of them hold (default 2,40)
//   -k accepts 18..31 (the reference stops at 30, main.cpp:115-116; 31 still fits 62 bits)
//   -SR / -j accept a Jellyfish 2 count file (.jf, `jellyfish count` output) as well as the text dump, in either mode
//   -qm jellyfish2 works (the reference's is dead code): with -jf2 DIR the counts come from `DIR/jellyfish
//                    dump` (the tool the reference would have queried k-mer by k-mer, Jellyfish.cpp:323-379), without it
//                    from the native reader of the .jf; with neither a -jf2 nor a .jf the reference's behaviour is kept
//   --SRReads FILE   (repeatable, instead of -SR) short reads, FASTA or FASTQ: their k-mers are counted on the GPU
//                    (talc_counter_*, docs/kmer_counting.md) in place of `jellyfish count` + `dump -c` (README.md:37-49)
//   --SRCountsOut F  with --SRReads: the kept k-mers as `jellyfish dump -c` text, for a later -SR F
//   --both-strands   the k-mer table holds the short reads' support on either strand (docs/both_strands.md): --SRReads
//                    counts canonical k-mers, -SR folds the counts (a `jellyfish count -C` dump, or a directional one) over
//                    reverse complements on the GPU, and every kept k-mer is stored with its reverse complement
//   --SRMinQual Q    with --SRReads: a base of a FASTQ short read whose Phred+33 quality is below Q (0..93, 0: none) is counted as N
//                    (docs/sr_filter.md; `jellyfish count -Q`)
//   --SRAdapter SEQ  (repeatable, up to 4) with --SRReads: every short read is clipped on the GPU from the first place where
//                    SEQ, or a prefix of it that runs over the read's end, matches
//   --SRAdapterOverlap N  with --SRAdapter: the shortest match that clips (default 5)
//   --SRAdapterErr PCT    with --SRAdapter: mismatches allowed, in percent of the matched length (0..30, default 10)
//   --SRHisto        with --SRReads: write <o>.histo.txt, the count spectrum of the counted k-mers as `jellyfish histo` prints it
//                    (docs/kmer_spectrum.md): one line `count k-mers` per count that occurs, the last line gathers the counts above
//                    --SRHistoHigh; one summary line on stdout
//   --SRHistoHigh N  with --SRHisto / --AutoMinCount: the largest count with a line of its own (2..16382, default 10000)
//   --AutoMinCount   with --SRReads: MIN_COUNT is the first local minimum of that spectrum (at least 2; the given --MIN_COUNT
//                    when the spectrum has none), chosen after counting and used for --SRCountsOut, the table and the correction
//   --LRAdapter SEQ  (repeatable, up to 4) a primer to look for at both ends of every long read (docs/read_ends.md): within
//                    --LRAdapterErr PCT (0..30, default 20) per cent of its length in edits, inside the first --LREndWindow N
//                    (32..4096, default 512) bases, and as its reverse complement inside the last; writes <o>.ends.tsv, one
//                    line per read in input order, and one summary line on stdout
//   --LRPolyA N      a poly-T head / poly-A tail of at least N bases (8..LREndWindow; 0: off), behind the primer if there is one
//   --LRClip         the reads are corrected without the ends found: clipped on the GPU, every output is that of the clipped reads
//   --LRChimeras     with --LRAdapter: the adapters are searched over the whole of every read, on both strands, within
//                    --LRChimeraErr PCT (0..30, default 10) per cent of their length in edits (docs/chimeras.md); writes
//                    <o>.chimera.tsv, one line per hit, and one summary line on stdout
//                    (not with --LRClip alone: the hits are positions in the reads as they came)
//   --LRSplit        ... and the reads are cut there on the GPU: the pieces of at least --LRMinPiece N (default 100) bases are
//                    corrected as reads of their own (name_c1, name_c2, ...), every output is that of the pieces; writes
//                    <o>.chimera_pieces.tsv; with --LRClip every piece is clipped
//   --LRBarcodes FILE  a FASTA of 1..96 sample barcodes of one length (docs/demux.md): every read's barcode is called on the GPU
//                    at its head and, reverse-complemented, at its tail, within --LRBarcodeErr PCT (0..30, default 20) per cent
//                    of the length in edits inside --LRBarcodeWindow N (32..4096, default 256) bases, when the runner-up is at
//                    least --LRBarcodeMargin N (default 2) edits worse; --LRBarcodeBothEnds: only reads whose ends agree get a
//                    barcode; writes <o>.demux.tsv (one line per read as it came), <o>.demux_counts.tsv and one summary line;
//                    --LRDemuxOut: every record of <o>.fa also goes to <o>.<name>.fa or <o>.unclassified.fa (a piece of
//                    --LRSplit where its source read goes)
//   --LRUmi PATTERN  a UMI pattern of 12..64 IUPAC letters with 1..32 degenerate ones (docs/umi.md): found on the GPU at every read's
//                    head and, reverse-complemented, at its tail, within --LRUmiErr PCT (0..30, default 10) per cent of its length
//                    in edits inside --LRUmiWindow N (32..4096, default 256) bases, and aligned: the read's bases under the
//                    degenerate letters are its UMI; writes <o>.umi.tsv (one line per read, per piece under --LRSplit) and one
//                    summary line; with --LRClip the reads are cut behind the pattern too, also without --LRAdapter / --LRPolyA
// -t/--num_threads is accepted and ignored (the parallelism is on the device).
// Differences, all documented in INTEGRATION.md: stdout carries the [TALC] banners but none of
// the reference's always-on debug dumps; log lines are written in input order.
#include <omp.h>

#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include <spawn.h>
#include <sys/stat.h>
#include <sys/wait.h>

#include "talc_chimera_plan.h"   // the piece rule, as the library applies it: what a report without --LRSplit would keep
#include "talc_cli_io.h"
#include "talc_hip.h"
#include "talc_jf.h"
#include "talc_kernels_umi.h"   // iupac_set: the letters of --LRUmi, as the library reads them
#include "talc_pure.h"   // the spectrum's threshold rule: its constants, as the library applies them
#include "talc_switches.h"

namespace {

using talc::HostBuf;
using talc::SeqReader;
using Clock = std::chrono::steady_clock;

double secs(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double>(b - a).count(); }
double since(Clock::time_point a) { return secs(a, Clock::now()); }

// every exit releases what these hold; a batch is destroyed before its context, a context before its table
struct TableDel { void operator()(talc_table* t) const { talc_table_destroy(t); } };
struct CtxDel { void operator()(talc_ctx* c) const { talc_ctx_destroy(c); } };
struct BatchDel { void operator()(talc_batch* b) const { talc_batch_destroy(b); } };
using TablePtr = std::unique_ptr<talc_table, TableDel>;
using CtxPtr = std::unique_ptr<talc_ctx, CtxDel>;
using BatchPtr = std::unique_ptr<talc_batch, BatchDel>;

// a library call has failed on this thread: its message, and the exit code of a device error
int libError() {
  std::cerr << "talc: " << talc_last_error() << "\n";
  return 2;
}
int noGpuError() {
  std::cerr << "talc: no MI355X / HIP device visible; the correction path has no CPU fallback\n";
  return 2;
}

struct Options {
  std::string seqFile, outPrefix = "out", queryMode = "memory", dump, jdump, jf2;
  std::vector<std::string> srReads;   // --SRReads, in order
  std::string srCountsOut;            // --SRCountsOut
  talc_params p;
  bool haveK = false, haveSR = false, useJ = false;
  int gpus = -1;
  int nthreads = 1;
  uint32_t batchReads = 200000;
  bool haveBatchReads = false;
  bool readStats = false;
  bool corrMap = false, softMask = false;   // --corr-map, --soft-mask
  bool solidity = false;                    // --solidity
  bool trim = false, split = false;         // --trim, --split
  uint32_t minPieceLen = 0;                 // --min-piece-len
  bool corrEdits = false;                   // --corr-edits
  uint64_t maxEditCells = 0;                // --max-edit-cells (0: the library's default)
  bool autoStrand = false;                  // --auto-strand
  bool bothStrands = false;                 // --both-strands
  uint32_t srMinQual = 0;                   // --SRMinQual (0: no floor)
  std::vector<std::string> srAdapters;      // --SRAdapter, in order
  uint32_t srAdapterOverlap = 0, srAdapterErr = 10;   // --SRAdapterOverlap (0: the library's default), --SRAdapterErr
  bool haveSrMinQual = false, haveSrAdapterOverlap = false, haveSrAdapterErr = false;
  bool srHisto = false, autoMinCount = false;   // --SRHisto, --AutoMinCount
  uint32_t srHistoHigh = 0;                     // --SRHistoHigh (0: the library's default, 10000)
  bool haveSrHistoHigh = false;
  bool srFilter() const { return srMinQual > 0 || !srAdapters.empty(); }
  bool fastq = false, haveQualRange = false;   // --fastq, --qual-range
  uint32_t qmin = 2, qmax = 40;
  std::vector<std::string> lrAdapters;      // --LRAdapter, in order
  uint32_t lrAdapterErr = 20, lrPolyA = 0, lrEndWindow = 512;   // --LRAdapterErr, --LRPolyA (0: off), --LREndWindow
  bool haveLrAdapterErr = false, haveLrPolyA = false, haveLrEndWindow = false;
  bool lrClip = false;                      // --LRClip
  bool lrChimeras = false, lrSplit = false; // --LRChimeras, --LRSplit (docs/chimeras.md)
  uint32_t lrChimeraErr = 10, lrMinPiece = 100;   // --LRChimeraErr, --LRMinPiece
  bool haveLrChimeraErr = false, haveLrMinPiece = false;
  bool lrChimeraScan() const { return lrChimeras || lrSplit; }   // the chimera scan is on
  bool lrEnds() const { return !lrAdapters.empty() || lrPolyA > 0; }   // the long-read end clean-up is on
  std::string lrBarcodesFile;               // --LRBarcodes (docs/demux.md)
  std::vector<std::string> lrBarcodeNames, lrBarcodeSeqs;   // ... its records, in order
  uint32_t lrBarcodeErr = 20, lrBarcodeMargin = 2, lrBarcodeWindow = 256;   // --LRBarcodeErr, --LRBarcodeMargin, --LRBarcodeWindow
  bool haveLrBarcodeErr = false, haveLrBarcodeMargin = false, haveLrBarcodeWindow = false;
  bool lrBarcodeBothEnds = false, lrDemuxOut = false;   // --LRBarcodeBothEnds, --LRDemuxOut
  bool lrDemux() const { return !lrBarcodesFile.empty(); }   // barcode demultiplexing is on
  std::string lrUmiPattern;                 // --LRUmi (docs/umi.md)
  uint32_t lrUmiErr = 10, lrUmiWindow = 256;   // --LRUmiErr (lib.UMI_DEFAULT_ERR: tools/umi_defaults.py), --LRUmiWindow
  bool haveLrUmi = false, haveLrUmiErr = false, haveLrUmiWindow = false;
  bool lrUmi() const { return haveLrUmi; }   // the UMI read-out is on
};

void usage(FILE* f) {
  fprintf(f,
          "TALC: Transcriptome-Aware Long Read Correction (MI355X hot path)\n"
          "SYNOPSIS  talc [OPTIONS] <long reads .fa/.fq> -k K -SR <jellyfish dump>\n"
          "  -o, --output TEXT           prefix of the output files (default: out)\n"
          "  -k, --kmerSize INT          k-mer length, 18..31 (required)\n"
          "  -qm, --query-mode TEXT      memory | jellyfish2 (default: memory)\n"
          "  -SR, --SRCounts TEXT        short-read k-mer counts: `jellyfish dump -c` text or the .jf itself (this or --SRReads)\n"
          "  --SRReads TEXT              short reads (FASTA or FASTQ; repeat for several files): their k-mers are counted on\n"
          "                              the GPU instead of read from -SR (every window of K ACGT bases of a record, directional)\n"
          "  --SRCountsOut TEXT          with --SRReads: write the kept k-mers as `jellyfish dump -c` text (usable as -SR)\n"
          "  --both-strands              take the k-mers on both strands (unstranded short reads, `jellyfish count -C` counts):\n"
          "                              counts are summed over a k-mer and its reverse complement on the GPU, MIN_COUNT applies\n"
          "                              to the sum and both are stored; --SRCountsOut then writes the canonical k-mers (not with\n"
          "                              --auto-strand; docs/both_strands.md)\n"
          "  --SRMinQual INT             with --SRReads: bases of FASTQ short reads with a Phred+33 quality below this (0..93)\n"
          "                              are counted as N (docs/sr_filter.md)\n"
          "  --SRAdapter TEXT            with --SRReads: adapter to clip from the 3' end of every short read, 1..64 letters of\n"
          "                              ACGT (repeat for up to 4 adapters); partial matches over the read's end clip too\n"
          "  --SRAdapterOverlap INT      with --SRAdapter: shortest match that clips, 1..64 and at most the shortest adapter, default 5\n"
          "  --SRAdapterErr INT          with --SRAdapter: mismatches allowed in percent of the matched length, 0..30, default 10\n"
          "  --SRHisto                   with --SRReads: write <o>.histo.txt, the count spectrum of the short reads' k-mers in the\n"
          "                              format of `jellyfish histo` (docs/kmer_spectrum.md)\n"
          "  --SRHistoHigh INT           with --SRHisto / --AutoMinCount: counts above this share the last line, 2..16382, default 10000\n"
          "  --AutoMinCount              with --SRReads: take MIN_COUNT from the first local minimum of that spectrum (at least 2;\n"
          "                              the given --MIN_COUNT stands when the spectrum only falls)\n"
          "  -j, --junctions TEXT        k-mers flanking junctions and their counts\n"
          "  -jf2, --pathToJF2 TEXT      directory of the jellyfish program: -qm jellyfish2 then reads the .jf through\n"
          "                              `jellyfish dump` (without it: the native .jf reader)\n"
          "  --MIN_INNER_SCORE FLOAT     [0.3,0.9] default 0.7\n"
          "  --MIN_BORDER_SCORE FLOAT    [0.5,0.9] default 0.7\n"
          "  --MIN_COUNT INT             >= 2, default 2\n"
          "  --SR_ERROR_RATE DOUBLE      [0.01,0.1] default 0.025\n"
          "  --WINDOW_SIZE INT           >= 6, default 9\n"
          "  --MAX_NB_BRANCHES INT       >= 5, default 7\n"
          "  --ALPHA_FOR_PRED FLOAT      >= 0.67, default 2.57\n"
          "  -t, --num_threads INT       accepted (host threads are not the parallel resource here)\n"
          "  --DEBUG_MODE TEXT           accepted, unused\n"
          "  -rev, --reverse             reverse-complement the long reads before correction\n"
          "  --gpus INT                  GPUs to use (default: all)\n"
          "  --batch-reads INT           reads per device batch (default: at least two batches per worker, 20000..200000)\n"
          "  --read-stats                append per-read rows to <o>.stats_basics.txt (Read.cpp:418-433)\n"
          "  --corr-map                  write <o>.map.tsv: read_name, kind (S solid, C corrected, R raw), raw_start, raw_len,\n"
          "                              out_start, out_len for every stretch of every read (docs/correction_map.md)\n"
          "  --soft-mask                 write the bases that stayed uncorrected (R stretches) in lower case\n"
          "  --solidity                  write <o>.solidity.tsv: k-mers and bases the short reads support, per read, raw and corrected\n"
          "  --trim                      write <o>.trim.fa: each read from its first to its last solid or corrected base (reads\n"
          "                              without one are left out; with --soft-mask the uncorrected stretches inside in lower case)\n"
          "  --split                     write <o>.split.fa: each read cut at its uncorrected stretches, pieces named name_1, name_2, ...\n"
          "  --min-piece-len INT         with --trim / --split: drop pieces of fewer bases, default 0 (docs/trim_split.md)\n"
          "  --corr-edits                write <o>.edits.tsv: matches, mismatches, insertions, deletions and a CIGAR string per read\n"
          "  --max-edit-cells INT        with --corr-edits: do not align a corrected stretch of more cells (raw x corrected\n"
          "                              length), default 67108864; beyond 536870912 it acts as that (docs/correction_edits.md)\n"
          "  --auto-strand               correct every read in the orientation the short reads support (not with -rev); write\n"
          "                              <o>.strand.tsv: solid and IN k-mers of the read and of its reverse complement, + or -\n"
          "  --fastq                     write <o>.fq beside <o>.fa: every record with one quality per base, from the short reads'\n"
          "                              support of the k-mers that hold the base (docs/base_support.md); with --trim / --split\n"
          "                              also <o>.trim.fq / <o>.split.fq\n"
          "  --qual-range MIN,MAX        with --fastq: the quality of a base no solid k-mer holds and of one all of them hold,\n"
          "                              0 <= MIN <= MAX <= 93, default 2,40\n"
          "  --LRAdapter TEXT            primer / adapter to look for at both ends of every long read, 12..64 letters of ACGT (repeat\n"
          "                              for up to 4): found on the GPU within --LREndWindow bases of the head, and as its reverse\n"
          "                              complement of the tail; writes <o>.ends.tsv (docs/read_ends.md)\n"
          "  --LRAdapterErr INT          with --LRAdapter: edits allowed in percent of the adapter's length, 0..30, default 20\n"
          "  --LRPolyA INT               shortest poly-T head / poly-A tail (behind the adapter, if any) to report, 8..LREndWindow;\n"
          "                              0: off (default)\n"
          "  --LREndWindow INT           with --LRAdapter / --LRPolyA: bases of each end that are searched, 32..4096, default 512\n"
          "  --LRClip                    with --LRAdapter / --LRPolyA: correct the reads without the ends found (clipped on the GPU);\n"
          "                              every output is that of the clipped reads under their names\n"
          "  --LRChimeras                with --LRAdapter: look for the adapters inside the reads too, on both strands; writes\n"
          "                              <o>.chimera.tsv (docs/chimeras.md); with --LRClip only together with --LRSplit\n"
          "  --LRSplit                   with --LRAdapter: ... and cut the reads there on the GPU; the pieces are corrected as reads of\n"
          "                              their own (name_c1, name_c2, ...); writes <o>.chimera_pieces.tsv; combines with --LRClip\n"
          "  --LRChimeraErr INT          with --LRChimeras / --LRSplit: edits allowed in percent of the adapter's length, 0..30, default 10\n"
          "  --LRMinPiece INT            with --LRChimeras / --LRSplit: pieces shorter than this are dropped, default 100\n"
          "  --LRBarcodes FILE           FASTA of 1..96 sample barcodes of one length, 12..64 letters of ACGT: every read's barcode is\n"
          "                              called on the GPU at its head and, reverse-complemented, at its tail; writes <o>.demux.tsv and\n"
          "                              <o>.demux_counts.tsv (docs/demux.md); names: 1..32 of A-Za-z0-9_.-, unique, not 'unclassified'\n"
          "  --LRBarcodeErr INT          with --LRBarcodes: edits allowed in percent of the barcode's length, 0..30, default 20\n"
          "  --LRBarcodeMargin INT       with --LRBarcodes: an end calls its best barcode when the runner-up is at least this many edits\n"
          "                              worse, 0..k + 1, default 2\n"
          "  --LRBarcodeWindow INT       with --LRBarcodes: bases of each end that are searched, 32..4096, default 256\n"
          "  --LRBarcodeBothEnds         with --LRBarcodes: only reads whose two ends call the same barcode get it\n"
          "  --LRDemuxOut                with --LRBarcodes: every record of <o>.fa also goes to <o>.<name>.fa or <o>.unclassified.fa\n"
          "  --LRUmi PATTERN             a UMI pattern of 12..64 letters of ACGTRYSWKMBDHVN, 1..32 of them degenerate: found on the GPU at\n"
          "                              every read's head and, reverse-complemented, at its tail, and aligned; the bases under the\n"
          "                              degenerate letters are the read's UMI; writes <o>.umi.tsv (docs/umi.md); with --LRClip the reads\n"
          "                              are cut behind the pattern too; include fixed primer letters: the bare UMI is found by chance\n"
          "  --LRUmiErr INT              with --LRUmi: edits allowed in percent of the pattern's length, 0..30, default 10\n"
          "  --LRUmiWindow INT           with --LRUmi: bases of each end that are searched, 32..4096, default 256\n"
          "  -h, --help / --version\n");
}

[[noreturn]] void parse_error(const std::string& msg) {
  std::cerr << "talc: " << msg << "\n";
  exit(1);  // main.cpp:199: PARSE_ERROR -> return 1
}

double num(const char* s, const char* name) {
  char* end = nullptr;
  double v = strtod(s, &end);
  if (end == s || *end != 0) parse_error(std::string("the given value '") + s + "' cannot be cast for " + name);
  return v;
}
void range(double v, double lo, double hi, const char* name) {
  if (v < lo || v > hi) parse_error(std::string("value out of range for ") + name);
}

// --LRBarcodes: the FASTA's records into o.lrBarcodeNames / o.lrBarcodeSeqs.  The names become file names; every fault is a
// parse error (exit 1, nothing written).
void loadBarcodes(Options& o) {
  std::ifstream f(o.lrBarcodesFile);
  if (!f) parse_error("LRBarcodes: cannot read " + o.lrBarcodesFile);
  std::string line;
  while (std::getline(f, line)) {
    while (!line.empty() && (line.back() == '\r' || line.back() == ' ' || line.back() == '\t')) line.pop_back();
    if (line.empty()) continue;
    if (line[0] == '>') {
      const std::string name = line.substr(1, line.find_first_of(" \t") == std::string::npos ? std::string::npos : line.find_first_of(" \t") - 1);
      if (name.empty() || name.size() > 32 || name.find_first_not_of("ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789_.-") != std::string::npos)
        parse_error("LRBarcodes: the name '" + name + "' cannot be a barcode's: 1..32 of A-Za-z0-9_.- are expected");
      if (name == "unclassified") parse_error("LRBarcodes: the name 'unclassified' is taken by the reads without a barcode");
      for (const std::string& other : o.lrBarcodeNames)
        if (other == name) parse_error("LRBarcodes: the name '" + name + "' is given twice");
      if (o.lrBarcodeNames.size() == 96) parse_error("LRBarcodes: more than 96 barcodes");
      o.lrBarcodeNames.push_back(name);
      o.lrBarcodeSeqs.emplace_back();
    } else {
      if (o.lrBarcodeSeqs.empty()) parse_error("LRBarcodes: " + o.lrBarcodesFile + " does not start with a '>' line");
      o.lrBarcodeSeqs.back() += line;
    }
  }
  if (o.lrBarcodeSeqs.empty()) parse_error("LRBarcodes: no barcode in " + o.lrBarcodesFile);
  for (size_t b = 0; b < o.lrBarcodeSeqs.size(); ++b) {
    const std::string& v = o.lrBarcodeSeqs[b];
    if (v.size() < 12 || v.size() > 64) parse_error("LRBarcodes: the barcode " + o.lrBarcodeNames[b] + " has " + std::to_string(v.size()) + " letters: 12..64 are expected");
    if (v.find_first_not_of("ACGTacgt") != std::string::npos) parse_error("LRBarcodes: the barcode " + o.lrBarcodeNames[b] + " has a letter that is not one of ACGT");
    if (v.size() != o.lrBarcodeSeqs[0].size())
      parse_error("LRBarcodes: the barcode " + o.lrBarcodeNames[b] + " has " + std::to_string(v.size()) + " letters, " + o.lrBarcodeNames[0] + " has " +
                  std::to_string(o.lrBarcodeSeqs[0].size()) + ": one length for all");
  }
  const uint32_t k = o.lrBarcodeErr * (uint32_t)o.lrBarcodeSeqs[0].size() / 100u;
  if (o.lrBarcodeMargin > k + 1) parse_error("value out of range for LRBarcodeMargin: " + std::to_string(o.lrBarcodeMargin) + " is above k + 1 = " + std::to_string(k + 1));
}

Options parse(int argc, const char** argv) {
  Options o;
  talc_params_default(&o.p);
  auto need = [&](int& i) -> const char* {
    if (i + 1 >= argc) parse_error(std::string("option requires an argument: ") + argv[i]);
    return argv[++i];
  };
  auto is = [](const std::string& a, const char* s, const char* l) { return a == std::string("-") + s || a == std::string("--") + l; };
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (is(a, "o", "output")) o.outPrefix = need(i);
    else if (is(a, "k", "kmerSize")) { double v = num(need(i), "k"); range(v, 18, 31, "k"); o.p.k = (uint32_t)v; o.haveK = true; }
    else if (is(a, "qm", "query-mode")) { o.queryMode = need(i); if (o.queryMode != "memory" && o.queryMode != "jellyfish2") parse_error("the given value '" + o.queryMode + "' is not in the list of allowed values [memory, jellyfish2]"); }
    else if (is(a, "SR", "SRCounts")) { o.dump = need(i); o.haveSR = true; }
    else if (a == "--SRReads") o.srReads.push_back(need(i));
    else if (a == "--SRCountsOut") o.srCountsOut = need(i);
    else if (a == "--SRMinQual") {
      const double v = num(need(i), "SRMinQual");
      if (v != (double)(long long)v || v < 0 || v > 93) parse_error("value out of range for SRMinQual: 0..93");
      o.srMinQual = (uint32_t)v; o.haveSrMinQual = true;
    }
    else if (a == "--SRAdapter") {
      const std::string v = need(i);
      if (v.empty() || v.size() > 64) parse_error("the given value '" + v + "' cannot be an SRAdapter: 1..64 letters are expected");
      if (v.find_first_not_of("ACGTacgt") != std::string::npos) parse_error("the given value '" + v + "' cannot be an SRAdapter: it has a letter that is not one of ACGT");
      if (o.srAdapters.size() == 4) parse_error("too many --SRAdapter: at most 4");
      o.srAdapters.push_back(v);
    }
    else if (a == "--SRAdapterOverlap") {
      const double v = num(need(i), "SRAdapterOverlap");
      if (v != (double)(long long)v || v < 1 || v > 64) parse_error("value out of range for SRAdapterOverlap: 1..64");
      o.srAdapterOverlap = (uint32_t)v; o.haveSrAdapterOverlap = true;
    }
    else if (a == "--SRAdapterErr") {
      const double v = num(need(i), "SRAdapterErr");
      if (v != (double)(long long)v || v < 0 || v > 30) parse_error("value out of range for SRAdapterErr: 0..30");
      o.srAdapterErr = (uint32_t)v; o.haveSrAdapterErr = true;
    }
    else if (a == "--SRHisto") o.srHisto = true;
    else if (a == "--AutoMinCount") o.autoMinCount = true;
    else if (a == "--SRHistoHigh") {
      const double v = num(need(i), "SRHistoHigh");
      if (v != (double)(long long)v || v < 2 || v > 16382) parse_error("value out of range for SRHistoHigh: 2..16382");
      o.srHistoHigh = (uint32_t)v; o.haveSrHistoHigh = true;
    }
    else if (is(a, "j", "junctions")) { o.jdump = need(i); o.useJ = true; }
    else if (is(a, "jf2", "pathToJF2")) o.jf2 = need(i);
    else if (is(a, "MIN_INNER_SCORE", "MIN_INNER_SCORE")) { o.p.min_inner_score = num(need(i), "MIN_INNER_SCORE"); range(o.p.min_inner_score, 0.3, 0.9, "MIN_INNER_SCORE"); }
    else if (is(a, "MIN_BORDER_SCORE", "MIN_BORDER_SCORE")) { o.p.min_border_score = num(need(i), "MIN_BORDER_SCORE"); range(o.p.min_border_score, 0.5, 0.9, "MIN_BORDER_SCORE"); }
    else if (is(a, "MIN_COUNT", "MIN_COUNT")) { double v = num(need(i), "MIN_COUNT"); range(v, 2, 4e9, "MIN_COUNT"); o.p.min_count = (uint32_t)v; }
    else if (is(a, "SR_ERROR_RATE", "SR_ERROR_RATE")) { o.p.sr_error_rate = num(need(i), "SR_ERROR_RATE"); range(o.p.sr_error_rate, 0.01, 0.1, "SR_ERROR_RATE"); }
    else if (is(a, "WINDOW_SIZE", "WINDOW_SIZE")) { double v = num(need(i), "WINDOW_SIZE"); range(v, 6, 4e9, "WINDOW_SIZE"); o.p.window_size = (uint32_t)v; }
    else if (is(a, "MAX_NB_BRANCHES", "MAX_NB_BRANCHES")) { double v = num(need(i), "MAX_NB_BRANCHES"); range(v, 5, 64, "MAX_NB_BRANCHES"); o.p.max_nb_competing_paths = (uint32_t)v; }
    else if (is(a, "ALPHA_FOR_PRED", "ALPHA_FOR_PRED")) { o.p.alpha = num(need(i), "ALPHA_FOR_PRED"); range(o.p.alpha, 0.67, 1e300, "ALPHA_FOR_PRED"); }
    else if (is(a, "t", "num_threads")) { double v = num(need(i), "num_threads"); range(v, 1, 1e9, "num_threads"); o.nthreads = (int)v; }
    else if (is(a, "DEBUG_MODE", "DEBUG_MODE")) need(i);
    else if (is(a, "rev", "reverse")) o.p.reverse = 1;
    else if (a == "--gpus") { o.gpus = (int)num(need(i), "gpus"); range(o.gpus, 1, 64, "gpus"); }
    else if (a == "--batch-reads") { double v = num(need(i), "batch-reads"); range(v, 1, 4e9, "batch-reads"); o.batchReads = (uint32_t)v; o.haveBatchReads = true; }
    else if (a == "--read-stats") o.readStats = true;
    else if (a == "--corr-map") o.corrMap = true;
    else if (a == "--soft-mask") o.softMask = true;
    else if (a == "--solidity") o.solidity = true;
    else if (a == "--trim") o.trim = true;
    else if (a == "--split") o.split = true;
    else if (a == "--corr-edits") o.corrEdits = true;
    else if (a == "--max-edit-cells") { double v = num(need(i), "max-edit-cells"); range(v, 1, 9e18, "max-edit-cells"); o.maxEditCells = (uint64_t)v; }
    else if (a == "--auto-strand") o.autoStrand = true;
    else if (a == "--both-strands") o.bothStrands = true;
    else if (a == "--fastq") o.fastq = true;
    else if (a == "--qual-range") {
      const std::string v = need(i);
      const size_t comma = v.find(',');
      if (comma == std::string::npos) parse_error("the given value '" + v + "' cannot be cast for qual-range: MIN,MAX is expected");
      const double lo = num(v.substr(0, comma).c_str(), "qual-range"), hi = num(v.substr(comma + 1).c_str(), "qual-range");
      if (lo != (double)(long long)lo || hi != (double)(long long)hi || lo < 0 || lo > hi || hi > 93) parse_error("value out of range for qual-range: 0 <= MIN <= MAX <= 93");
      o.qmin = (uint32_t)lo; o.qmax = (uint32_t)hi; o.haveQualRange = true;
    }
    else if (a == "--LRAdapter") {
      const std::string v = need(i);
      if (v.size() < 12 || v.size() > 64) parse_error("the given value '" + v + "' cannot be an LRAdapter: 12..64 letters are expected");
      if (v.find_first_not_of("ACGTacgt") != std::string::npos) parse_error("the given value '" + v + "' cannot be an LRAdapter: it has a letter that is not one of ACGT");
      if (o.lrAdapters.size() == 4) parse_error("too many --LRAdapter: at most 4");
      o.lrAdapters.push_back(v);
    }
    else if (a == "--LRAdapterErr") {
      const double v = num(need(i), "LRAdapterErr");
      if (v != (double)(long long)v || v < 0 || v > 30) parse_error("value out of range for LRAdapterErr: 0..30");
      o.lrAdapterErr = (uint32_t)v; o.haveLrAdapterErr = true;
    }
    else if (a == "--LRPolyA") {
      const double v = num(need(i), "LRPolyA");
      if (v != (double)(long long)v || v < 0 || v > 4096 || (v > 0 && v < 8)) parse_error("value out of range for LRPolyA: 0 (off) or 8..LREndWindow");
      o.lrPolyA = (uint32_t)v; o.haveLrPolyA = true;
    }
    else if (a == "--LREndWindow") {
      const double v = num(need(i), "LREndWindow");
      if (v != (double)(long long)v || v < 32 || v > 4096) parse_error("value out of range for LREndWindow: 32..4096");
      o.lrEndWindow = (uint32_t)v; o.haveLrEndWindow = true;
    }
    else if (a == "--LRClip") o.lrClip = true;
    else if (a == "--LRChimeras") o.lrChimeras = true;
    else if (a == "--LRSplit") o.lrSplit = true;
    else if (a == "--LRChimeraErr") {
      const double v = num(need(i), "LRChimeraErr");
      if (v != (double)(long long)v || v < 0 || v > 30) parse_error("value out of range for LRChimeraErr: 0..30");
      o.lrChimeraErr = (uint32_t)v; o.haveLrChimeraErr = true;
    }
    else if (a == "--LRMinPiece") {
      const double v = num(need(i), "LRMinPiece");
      if (v != (double)(long long)v || v < 0 || v > 2e9) parse_error("value out of range for LRMinPiece: 0..2000000000");
      o.lrMinPiece = (uint32_t)v; o.haveLrMinPiece = true;
    }
    else if (a == "--LRBarcodes") o.lrBarcodesFile = need(i);
    else if (a == "--LRBarcodeErr") {
      const double v = num(need(i), "LRBarcodeErr");
      if (v != (double)(long long)v || v < 0 || v > 30) parse_error("value out of range for LRBarcodeErr: 0..30");
      o.lrBarcodeErr = (uint32_t)v; o.haveLrBarcodeErr = true;
    }
    else if (a == "--LRBarcodeMargin") {
      const double v = num(need(i), "LRBarcodeMargin");
      if (v != (double)(long long)v || v < 0 || v > 20) parse_error("value out of range for LRBarcodeMargin: 0..k + 1");
      o.lrBarcodeMargin = (uint32_t)v; o.haveLrBarcodeMargin = true;
    }
    else if (a == "--LRBarcodeWindow") {
      const double v = num(need(i), "LRBarcodeWindow");
      if (v != (double)(long long)v || v < 32 || v > 4096) parse_error("value out of range for LRBarcodeWindow: 32..4096");
      o.lrBarcodeWindow = (uint32_t)v; o.haveLrBarcodeWindow = true;
    }
    else if (a == "--LRUmi") { o.lrUmiPattern = need(i); o.haveLrUmi = true; }
    else if (a == "--LRUmiErr") {
      const double v = num(need(i), "LRUmiErr");
      if (v != (double)(long long)v || v < 0 || v > 30) parse_error("value out of range for LRUmiErr: 0..30");
      o.lrUmiErr = (uint32_t)v; o.haveLrUmiErr = true;
    }
    else if (a == "--LRUmiWindow") {
      const double v = num(need(i), "LRUmiWindow");
      if (v != (double)(long long)v || v < 32 || v > 4096) parse_error("value out of range for LRUmiWindow: 32..4096");
      o.lrUmiWindow = (uint32_t)v; o.haveLrUmiWindow = true;
    }
    else if (a == "--LRBarcodeBothEnds") o.lrBarcodeBothEnds = true;
    else if (a == "--LRDemuxOut") o.lrDemuxOut = true;
    else if (a == "--min-piece-len") { double v = num(need(i), "min-piece-len"); range(v, 0, 4e9, "min-piece-len"); o.minPieceLen = (uint32_t)v; }
    else if (a == "-h" || a == "--help") { usage(stdout); exit(0); }
    else if (a == "--version") { std::cout << "talc version: 1.01\nLast update: September 2019\n"; exit(0); }
    else if (a.size() > 1 && a[0] == '-') parse_error("unknown option: " + a);
    else {
      if (!o.seqFile.empty()) parse_error("too many arguments");
      o.seqFile = a;
    }
  }
  if (o.seqFile.empty()) parse_error("not enough arguments were provided");
  if (!o.haveK) parse_error("option requires a value: -k, --kmerSize");
  if (o.haveSrMinQual && o.srReads.empty()) parse_error("--SRMinQual needs --SRReads");
  if (!o.srAdapters.empty() && o.srReads.empty()) parse_error("--SRAdapter needs --SRReads");
  if (o.haveSrAdapterOverlap && o.srAdapters.empty()) parse_error("--SRAdapterOverlap needs --SRAdapter");
  if (o.haveSrAdapterErr && o.srAdapters.empty()) parse_error("--SRAdapterErr needs --SRAdapter");
  if (o.srHisto && o.srReads.empty()) parse_error("--SRHisto needs --SRReads");
  if (o.autoMinCount && o.srReads.empty()) parse_error("--AutoMinCount needs --SRReads");
  if (o.haveSrHistoHigh && !o.srHisto && !o.autoMinCount) parse_error("--SRHistoHigh needs --SRHisto or --AutoMinCount");
  for (const std::string& ad : o.srAdapters)
    if (ad.size() < (o.srAdapterOverlap ? o.srAdapterOverlap : 5u))
      parse_error("value out of range for SRAdapterOverlap: " + std::to_string(o.srAdapterOverlap ? o.srAdapterOverlap : 5u) +
                  " is above the length of the adapter " + ad);
  if (!o.haveSR && o.srReads.empty()) parse_error("option requires a value: -SR, --SRCounts");
  if (o.haveSR && !o.srReads.empty()) parse_error("-SR and --SRReads exclude each other: give the counts or the short reads");
  if (!o.srReads.empty() && o.queryMode == "jellyfish2") parse_error("--SRReads counts the k-mers itself: it does not go with -qm jellyfish2");
  if (!o.srCountsOut.empty() && o.srReads.empty()) parse_error("--SRCountsOut needs --SRReads");
  if (o.haveQualRange && !o.fastq) parse_error("--qual-range needs --fastq");
  if (o.autoStrand && o.p.reverse) parse_error("--auto-strand chooses every read's orientation: it does not go with -rev");
  if (o.bothStrands && o.autoStrand)
    parse_error("--both-strands makes the k-mer table symmetric, so every vote of --auto-strand is a tie: they do not go together");
  if (o.haveLrAdapterErr && o.lrAdapters.empty()) parse_error("--LRAdapterErr needs --LRAdapter");
  if (o.haveLrEndWindow && !o.lrEnds()) parse_error("--LREndWindow needs --LRAdapter or --LRPolyA");
  if (o.haveLrUmiErr && !o.lrUmi()) parse_error("--LRUmiErr needs --LRUmi");
  if (o.haveLrUmiWindow && !o.lrUmi()) parse_error("--LRUmiWindow needs --LRUmi");
  if (o.lrUmi()) {
    const std::string& v = o.lrUmiPattern;
    if (v.size() < 12 || v.size() > 64) parse_error("LRUmi: " + std::to_string(v.size()) + " letters: 12..64 are expected");
    uint32_t u = 0;
    for (size_t i = 0; i < v.size(); ++i) {
      const uint32_t set = talc::iupac_set((uint8_t)v[i]);
      if (!set) parse_error("LRUmi: letter " + std::to_string(i + 1) + " is not one of ACGTRYSWKMBDHVN");
      u += (set & (set - 1)) ? 1 : 0;
    }
    if (u < 1 || u > 32) parse_error("LRUmi: " + std::to_string(u) + " degenerate letters: 1..32 are expected");
  }
  if (o.lrClip && !o.lrEnds() && !o.lrUmi()) parse_error("--LRClip needs --LRAdapter or --LRPolyA, or --LRUmi");
  if (o.lrChimeras && o.lrAdapters.empty()) parse_error("--LRChimeras needs --LRAdapter");
  if (o.lrSplit && o.lrAdapters.empty()) parse_error("--LRSplit needs --LRAdapter");
  // (a clipped batch no longer holds the reads as they came, and the hits are positions in those: only the split route scans
  //  before it clips)
  if (o.lrChimeras && o.lrClip && !o.lrSplit) parse_error("--LRChimeras with --LRClip needs --LRSplit: the report is of the reads as they came, which a clipped run no longer holds");
  if (o.haveLrChimeraErr && !(o.lrChimeraScan() && !o.lrAdapters.empty())) parse_error("--LRChimeraErr needs --LRAdapter and --LRChimeras or --LRSplit");
  if (o.haveLrMinPiece && !(o.lrChimeraScan() && !o.lrAdapters.empty())) parse_error("--LRMinPiece needs --LRAdapter and --LRChimeras or --LRSplit");
  if (o.lrPolyA > o.lrEndWindow) parse_error("value out of range for LRPolyA: " + std::to_string(o.lrPolyA) + " is above LREndWindow " + std::to_string(o.lrEndWindow));
  if (o.haveLrBarcodeErr && !o.lrDemux()) parse_error("--LRBarcodeErr needs --LRBarcodes");
  if (o.haveLrBarcodeMargin && !o.lrDemux()) parse_error("--LRBarcodeMargin needs --LRBarcodes");
  if (o.haveLrBarcodeWindow && !o.lrDemux()) parse_error("--LRBarcodeWindow needs --LRBarcodes");
  if (o.lrBarcodeBothEnds && !o.lrDemux()) parse_error("--LRBarcodeBothEnds needs --LRBarcodes");
  if (o.lrDemuxOut && !o.lrDemux()) parse_error("--LRDemuxOut needs --LRBarcodes");
  if (o.lrDemux()) loadBarcodes(o);
  o.p.use_junctions = o.useJ ? 1 : 0;
  return o;
}

// Settings.cpp:160-185
void outputConfig(const Options& o, const std::string& statFile) {
  std::ofstream f(o.outPrefix + ".config.txt", std::ios_base::trunc);
  f << "TALC: Parameters used for sample: " << o.outPrefix << "\n"
    << "****************************" << "\n"
    << "INPUT=" << o.seqFile << "\n"
    << "OUTPUT=" << o.outPrefix << "\n"
    << "STATS=" << statFile << "\n"
    << "****************************" << "\n"
    << "KmerSize=" << o.p.k << "\n"
    << "Junction mode activated? " << (o.useJ ? 1 : 0) << "\n"
    << "queryMode=" << o.queryMode << "\n";
  for (const std::string& ad : o.lrAdapters) f << "LRAdapter=" << ad << "\n";
  if (o.haveLrAdapterErr) f << "LRAdapterErr=" << o.lrAdapterErr << "\n";
  if (o.haveLrPolyA) f << "LRPolyA=" << o.lrPolyA << "\n";
  if (o.haveLrEndWindow) f << "LREndWindow=" << o.lrEndWindow << "\n";
  if (o.lrClip) f << "LRClip=1" << "\n";
  if (o.lrChimeras) f << "LRChimeras=1" << "\n";
  if (o.lrSplit) f << "LRSplit=1" << "\n";
  if (o.haveLrChimeraErr) f << "LRChimeraErr=" << o.lrChimeraErr << "\n";
  if (o.haveLrMinPiece) f << "LRMinPiece=" << o.lrMinPiece << "\n";
  if (o.lrUmi()) f << "LRUmi=" << o.lrUmiPattern << "\n";
  if (o.haveLrUmiErr) f << "LRUmiErr=" << o.lrUmiErr << "\n";
  if (o.haveLrUmiWindow) f << "LRUmiWindow=" << o.lrUmiWindow << "\n";
  if (o.lrDemux()) f << "LRBarcodes=" << o.lrBarcodesFile << "\n";
  if (o.haveLrBarcodeErr) f << "LRBarcodeErr=" << o.lrBarcodeErr << "\n";
  if (o.haveLrBarcodeMargin) f << "LRBarcodeMargin=" << o.lrBarcodeMargin << "\n";
  if (o.haveLrBarcodeWindow) f << "LRBarcodeWindow=" << o.lrBarcodeWindow << "\n";
  if (o.lrBarcodeBothEnds) f << "LRBarcodeBothEnds=1" << "\n";
  if (o.lrDemuxOut) f << "LRDemuxOut=1" << "\n";
  if (o.bothStrands) f << "Both strands? 1" << "\n";
  if (o.haveSrMinQual) f << "SRMinQual=" << o.srMinQual << "\n";
  for (const std::string& ad : o.srAdapters) f << "SRAdapter=" << ad << "\n";
  if (o.haveSrAdapterOverlap) f << "SRAdapterOverlap=" << o.srAdapterOverlap << "\n";
  if (o.haveSrAdapterErr) f << "SRAdapterErr=" << o.srAdapterErr << "\n";
  if (o.srHisto) f << "SRHisto=1" << "\n";
  if (o.haveSrHistoHigh) f << "SRHistoHigh=" << o.srHistoHigh << "\n";
  if (o.autoMinCount) f << "AutoMinCount=1" << "\n";
  f
    << "****************************" << "\n"
    << "MIN_INNER_SCORE=" << o.p.min_inner_score << "\n"
    << "MIN_BORDER_SCORE=" << o.p.min_border_score << "\n"
    << "MAX_NB_BRANCHES=" << o.p.max_nb_competing_paths << "\n"
    << "ALPHA=" << o.p.alpha << "\n"
    << "MIN_SR_COUNT=" << o.p.min_count << "\n"
    << "WINDOW_SIZE=" << o.p.window_size << "\n"
    << "****************************" << std::endl;
}

// Read.cpp:394-415
void setBasicReadStatsHeader(const std::string& statFile) {
  std::ofstream f(statFile, std::ios_base::trunc);
  f << "read_name\traw_length\twhead_length\twtail_length\tnbInKmers\tnbSolidKmers\tnbSolidReg\tnbInWeakReg\tnbInCorrReg\t"
       "CorrHead?\tCorrHeadLen\tCorrTail?\tCorrTailLen\tCorrlength\tnbInKmers2\n";
}

// the three files next to <o>.config.txt
struct Files {
  const std::string fa, stats, log, map, solidity, trim, split, edits, strand, fq, trimFq, splitFq, ends, chimera, chimeraPieces, demux, demuxCounts, umi, prefix;
  explicit Files(const std::string& prefix)
      : fa(prefix + ".fa"), stats(prefix + ".stats_basics.txt"), log(prefix + ".log"), map(prefix + ".map.tsv"), solidity(prefix + ".solidity.tsv"),
        trim(prefix + ".trim.fa"), split(prefix + ".split.fa"), edits(prefix + ".edits.tsv"), strand(prefix + ".strand.tsv"),
        fq(prefix + ".fq"), trimFq(prefix + ".trim.fq"), splitFq(prefix + ".split.fq"), ends(prefix + ".ends.tsv"),
        chimera(prefix + ".chimera.tsv"), chimeraPieces(prefix + ".chimera_pieces.tsv"), demux(prefix + ".demux.tsv"), demuxCounts(prefix + ".demux_counts.tsv"),
        umi(prefix + ".umi.tsv"), prefix(prefix) {}
  // --LRDemuxOut: where the records of barcode b (0-based; the number of barcodes: unclassified) go
  std::string demuxFa(const Options& o, size_t b) const { return prefix + "." + (b < o.lrBarcodeNames.size() ? o.lrBarcodeNames[b] : std::string("unclassified")) + ".fa"; }
};

// the temporary dumps of -qm jellyfish2 -jf2: gone once the table is built, whichever way that ends
struct TmpDumps {
  std::vector<std::string> files;
  ~TmpDumps() { for (const auto& f : files) std::remove(f.c_str()); }
};

// a Jellyfish 2 count file by its first bytes (talc_jf.h)
bool isJfFile(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  char h[16];
  f.read(h, sizeof h);
  return talc::jfLooksLike(h, (size_t)f.gcount());
}

// `DIR/jellyfish dump -c [-L minCount] -o out file.jf` as a child process (no shell): the program the reference's
// jellyfish2 mode names (io_pathToJF + "/" + "jellyfish", Jellyfish.cpp:340), asked once for the whole table instead of
// once per look-up.  Runs before anything touches the GPU.
extern "C" char** environ;
bool jellyfishDump(const std::string& dir, const std::string& jf, uint32_t minCount, const std::string& out, std::string& why) {
  const std::string tool = dir + "/jellyfish", lower = std::to_string(minCount);
  std::vector<const char*> av = {tool.c_str(), "dump", "-c"};
  if (minCount > 1) { av.push_back("-L"); av.push_back(lower.c_str()); }
  av.push_back("-o"); av.push_back(out.c_str());
  av.push_back(jf.c_str());
  av.push_back(nullptr);
  pid_t pid = 0;
  const int rc = posix_spawn(&pid, tool.c_str(), nullptr, nullptr, const_cast<char* const*>(av.data()), environ);
  if (rc != 0) { why = "cannot run " + tool + ": " + strerror(rc); return false; }
  int status = 0;
  while (waitpid(pid, &status, 0) < 0)
    if (errno != EINTR) { why = "waitpid failed for " + tool; return false; }
  if (!WIFEXITED(status) || WEXITSTATUS(status) != 0) {
    why = tool + " dump " + jf + " ended with " + (WIFEXITED(status) ? "exit code " + std::to_string(WEXITSTATUS(status)) : std::string("a signal"));
    return false;
  }
  return true;
}

// --SRHisto / --AutoMinCount (docs/kmer_spectrum.md): the spectrum of the counted k-mers from the device, once.  --SRHisto
// writes it as `jellyfish histo` prints it with its defaults: a line `count k-mers` for every count 1 .. high + 1 that
// occurs, ascending, the last one gathering the counts above high.  --AutoMinCount replaces MIN_COUNT, in the counter and
// in o.p (what --SRCountsOut, the table and every context then use), by the spectrum's first local minimum.
int spectrumOfCounts(Options& o, talc_counter* ctr, float* histoMs) {
  const uint32_t high = o.srHistoHigh ? o.srHistoHigh : talc::kSpectrumDefaultHigh;
  std::vector<uint64_t> hist(high + 2);
  talc_spectrum_stats ss;
  if (talc_counter_histo(ctr, high, hist.data(), &ss) != TALC_OK) return libError();
  if (talc_counter_get_histo_timing(ctr, histoMs) != TALC_OK) return libError();
  if (o.srHisto) {
    const std::string path = o.outPrefix + ".histo.txt";
    FILE* f = fopen(path.c_str(), "w");
    if (!f) { std::cerr << "talc: cannot write " << path << "\n"; return 2; }
    for (uint32_t c = 1; c <= high + 1; ++c)
      if (hist[c]) fprintf(f, "%u %llu\n", c, (unsigned long long)hist[c]);
    if (fclose(f) != 0) { std::cerr << "talc: cannot write " << path << "\n"; return 2; }
    std::cout << "[TALC]: k-mer spectrum: " << ss.distinct << " distinct, " << ss.unique << " unique, " << ss.total << " total, max " << ss.max_count << std::endl;
  }
  if (o.autoMinCount) {
    uint32_t chosen = 0, valley = 0;
    if (talc_spectrum_threshold(hist.data(), high, 0, o.p.min_count, &chosen, &valley) != TALC_OK) return libError();
    if (talc_counter_set_min_count(ctr, chosen) != TALC_OK) return libError();
    o.p.min_count = chosen;
    std::cout << "[TALC]: MIN_COUNT from the k-mer spectrum: " << chosen;
    if (valley) std::cout << " (first minimum at " << valley << ")" << std::endl;
    else std::cout << " (no minimum up to " << talc::spectrum_last_candidate(high, 0) << "; the given value stands)" << std::endl;
  }
  return 0;
}

// --SRReads: every short-read file read once, front to back (a pipe works), in batches of about 64 MB of bases handed to
// the GPU counter, which copies them and returns while its kernel runs, so reading the next batch overlaps counting this
// one.  Then the spectrum (--SRHisto, --AutoMinCount: o.p.min_count becomes the chosen value), --SRCountsOut, then the table
// (junction colouring with -j).  Returns 0, or the exit code after a message.
int countShortReads(Options& o, const talc::Switches& sw, TablePtr& table, int64_t st[3]) {
  if (talc_device_count() <= 0) return noGpuError();
  talc_counter* ctr = nullptr;
  if (talc_counter_create(&o.p, 0, 0, &ctr) != TALC_OK) return libError();
  struct Guard { talc_counter*& c; ~Guard() { talc_counter_destroy(c); } } guard{ctr};
  if (o.bothStrands && talc_counter_set_both_strands(ctr, 1) != TALC_OK) return libError();
  // the short-read filter (docs/sr_filter.md): a filtered run hands every file's batches over on their own, a FASTQ file's
  // with its qualities when there is a floor to apply
  const bool filtered = o.srFilter();
  if (filtered) {
    std::string ads;
    for (const std::string& ad : o.srAdapters) ads += (ads.empty() ? "" : ",") + ad;
    if (talc_counter_set_filter(ctr, o.srMinQual, ads.c_str(), o.srAdapterOverlap, o.srAdapterErr) != TALC_OK) return libError();
  }
  const size_t kBatchBytes = 64u << 20;
  std::string buf, qbuf;
  std::vector<uint64_t> offs{0};
  buf.reserve(kBatchBytes + (1u << 20));
  bool withQuals = false;   // the batch being read carries qualities
  double readS = 0, addS = 0;
  uint64_t nRecords = 0, nBytes = 0, nBatches = 0;
  auto flush = [&]() -> bool {
    if (offs.size() < 2) return true;
    const auto ta = Clock::now();
    const bool ok = (filtered ? talc_counter_add_fastq(ctr, buf.data(), withQuals ? qbuf.data() : nullptr, offs.data(), (uint32_t)(offs.size() - 1))
                              : talc_counter_add(ctr, buf.data(), offs.data(), (uint32_t)(offs.size() - 1))) == TALC_OK;
    const double dt = since(ta);
    addS += dt;
    if (sw.timing == 2) fprintf(stderr, "[talc-count] batch %llu: %zu records, %zu bytes, counter add (pack + queue) %.4f s\n", (unsigned long long)nBatches, offs.size() - 1, buf.size(), dt);
    ++nBatches;
    buf.clear();
    qbuf.clear();
    offs.assign(1, 0);
    return ok;
  };
  const auto t0 = Clock::now();
  for (const std::string& file : o.srReads) {
    SeqReader r(file);
    if (!r.ok()) { std::cerr << "talc: " << file << " is not a FASTA or FASTQ file that can be read\n"; return 2; }
    std::string id;
    uint64_t rec = 0;
    if (filtered) {   // (a batch is one file's: its records have qualities or they have none)
      nBytes += buf.size();
      if (!flush()) return libError();
      withQuals = o.srMinQual > 0 && r.fastq();
      if (o.srMinQual > 0 && !r.fastq())
        std::cerr << "[talc] warning: " << file << " is FASTA: it has no qualities, --SRMinQual does not apply to it\n";
    }
    auto tr = Clock::now();
    auto bases = [&](const char* p, size_t n) { buf.append(p, n); return true; };
    auto quals = [&](const char* p, size_t n) { if (withQuals) qbuf.append(p, n); return true; };
    while (r.next(id, bases, quals)) {
      ++rec;
      if (r.truncated()) { std::cerr << "talc: " << file << ": FASTQ record " << rec << " (" << id << ") is malformed: its qualities are shorter than its sequence\n"; return 2; }
      offs.push_back(buf.size());
      if (buf.size() >= kBatchBytes) {
        readS += since(tr);
        nBytes += buf.size();
        if (!flush()) return libError();
        tr = Clock::now();
      }
    }
    readS += since(tr);
    if (!r.ok()) { std::cerr << "talc: " << file << ": FASTQ record " << rec + 1 << " (after '" << id << "') is malformed: it does not start with '@'\n"; return 2; }
    nRecords += rec;
  }
  nBytes += buf.size();
  if (!flush()) return libError();
  if (filtered) {
    uint64_t fs[4];
    if (talc_counter_filter_stats(ctr, fs) != TALC_OK) return libError();
    std::cout << "[TALC]: short-read filter: " << fs[0] << " records, " << fs[1] << " clipped at an adapter, " << fs[2] << " bases clipped, " << fs[3]
              << " bases below the quality floor" << std::endl;
  }
  float histoMs = 0;
  if (o.srHisto || o.autoMinCount)
    if (const int ec = spectrumOfCounts(o, ctr, &histoMs)) return ec;
  const auto t1 = Clock::now();
  if (!o.srCountsOut.empty()) {   // `jellyfish dump -c` text of the kept k-mers (--both-strands: of the canonical ones, as after count -C)
    uint64_t n = 0;
    if (talc_counter_fetch(ctr, o.p.min_count, nullptr, nullptr, 0, &n) != TALC_OK) return libError();
    std::vector<uint64_t> km(std::max<uint64_t>(n, 1));
    std::vector<uint32_t> ct(std::max<uint64_t>(n, 1));
    if (talc_counter_fetch(ctr, o.p.min_count, km.data(), ct.data(), n, &n) != TALC_OK) return libError();
    FILE* f = fopen(o.srCountsOut.c_str(), "w");
    if (!f) { std::cerr << "talc: cannot write " << o.srCountsOut << "\n"; return 2; }
    const uint32_t K = o.p.k;
    std::vector<char> line(K + 16);
    for (uint64_t i = 0; i < n; ++i) {
      for (uint32_t j = 0; j < K; ++j) line[j] = "ACGT"[(km[i] >> (2 * (K - 1 - j))) & 3];
      const int m = snprintf(line.data() + K, 16, " %u\n", ct[i]);
      fwrite(line.data(), 1, K + (size_t)m, f);
    }
    if (fclose(f) != 0) { std::cerr << "talc: cannot write " << o.srCountsOut << "\n"; return 2; }
  }
  const auto t2 = Clock::now();
  talc_table* built = nullptr;
  if (talc_counter_build_table(ctr, o.useJ ? o.jdump.c_str() : nullptr, &built, st) != TALC_OK) return libError();
  table.reset(built);
  if (sw.timing) {
    char spectrum[64] = "";   // (with --SRHisto / --AutoMinCount only: the line of a run without them is as it was)
    if (o.srHisto || o.autoMinCount) snprintf(spectrum, sizeof spectrum, ", spectrum kernel %.3f ms", histoMs);
    fprintf(stderr, "[talc] short reads: %zu file(s), %llu records, %llu bytes in %llu batches; read %.3f s (%.4f s per batch), counter add (pack + queue) %.3f s "
                    "(%.4f s per batch), counts out %.3f s, last batches + table build %.3f s, counting stage %.3f s%s\n",
            o.srReads.size(), (unsigned long long)nRecords, (unsigned long long)nBytes, (unsigned long long)nBatches, readS,
            nBatches ? readS / (double)nBatches : 0.0, addS, nBatches ? addS / (double)nBatches : 0.0, secs(t1, t2), since(t2), since(t0), spectrum);
  }
  return 0;
}

// One batch of reads on its way through the pipeline: read -> corrected on a device -> written, in input order.
struct Chunk {
  uint64_t index = 0;
  std::vector<std::string> ids;
  std::vector<uint64_t> offsets{0};     // into the chunk's input buffer
  int inBuf = -1;                       // which page-locked input buffer of the pool holds the reads
  std::vector<int32_t> status;
  std::vector<int64_t> stats;           // 5 per read (--read-stats)
  std::string text, logText, statsText; // what the writer appends to <o>.fa / <o>.log / <o>.stats_basics.txt
  std::string mapText;                  // ... and to <o>.map.tsv (--corr-map)
  std::string solText;                  // ... and to <o>.solidity.tsv (--solidity)
  uint64_t solSums[4] = {0, 0, 0, 0};   // of the batch's lines: raw solid_bases, raw_length, corrected solid_bases, corr_length
  std::string trimText, splitText;      // ... and to <o>.trim.fa / <o>.split.fa (--trim, --split)
  uint64_t pieceSums[4] = {0, 0, 0, 0}; // of the batch: trimmed reads, their bases, split pieces, their bases
  std::string editText;                 // ... and to <o>.edits.tsv (--corr-edits)
  uint64_t editSums[6] = {0, 0, 0, 0, 0, 0};   // of the batch's corrected reads: =, X, I, D bases, the reads, segments not aligned
  std::vector<talc_strand> strand;      // --auto-strand: the vote of every read (empty without)
  std::string strandText;               // ... and the lines of <o>.strand.tsv
  uint64_t strandSums[2] = {0, 0};      // reads taken forward, reverse
  std::string fqText, trimFqText, splitFqText;   // ... and to <o>.fq, <o>.trim.fq, <o>.split.fq (--fastq)
  std::string endsText;                 // ... and to <o>.ends.tsv (--LRAdapter, --LRPolyA)
  uint64_t endSums[4] = {0, 0, 0, 0};   // of the batch: reads, those with an adapter at either end, those with a poly run, bases outside the kept intervals
  std::string chimeraText, chimeraPiecesText;   // ... and to <o>.chimera.tsv, <o>.chimera_pieces.tsv (--LRChimeras, --LRSplit)
  uint64_t chimeraSums[6] = {0, 0, 0, 0, 0, 0};   // of the batch: reads, hits, reads with a hit, pieces kept, pieces dropped, their bases
  std::string umiText;                  // ... and to <o>.umi.tsv (--LRUmi)
  uint64_t umiSums[5] = {0, 0, 0, 0, 0};   // of the batch: reads, a UMI at the head only, at the tail only, both ends accepted, none
  std::string demuxText;                // ... and to <o>.demux.tsv (--LRBarcodes)
  uint64_t demuxSums[6] = {0, 0, 0, 0, 0, 0};   // of the batch: reads, classified at both ends, head only, tail only, conflicts, the rest
  std::vector<uint64_t> demuxCounts;    // per barcode, then unclassified: reads, their bases as they came
  std::vector<uint8_t> recBarcode;      // the barcode of every record's source read (0: none)
  std::vector<size_t> textEnd;          // --LRDemuxOut: where every record ends in `text`
  // the read was corrected as under -rev: the whole file's -rev, or the read's own vote
  bool reversed(const talc_params& p, size_t r) const { return p.reverse || (!strand.empty() && strand[r].reverse); }
};

// the lines of <o>.strand.tsv for one batch (k.status, k.strand filled)
const char* const kStrandHeader = "read_name\tstatus\tn_kmers\tfwd_solid\tfwd_in\trc_solid\trc_in\tstrand\n";
void formatStrand(Chunk& k) {
  char num[128];
  for (size_t r = 0; r < k.ids.size(); ++r) {
    const talc_strand& w = k.strand[r];
    const int m = snprintf(num, sizeof num, "\t%d\t%u\t%u\t%u\t%u\t%u\t%c\n", k.status[r], w.n_kmers, w.fwd_solid, w.fwd_in, w.rc_solid, w.rc_in, w.reverse ? '-' : '+');
    k.strandText += k.ids[r];
    k.strandText.append(num, (size_t)m);
    k.strandSums[w.reverse ? 1 : 0] += 1;
  }
}

// the lines of <o>.ends.tsv for one batch, from the scan's rows (k.offsets: the reads as they came)
const char* const kEndsHeader = "read_name\traw_length\thead_adapter\thead_adapter_len\thead_adapter_err\thead_poly\ttail_adapter\ttail_adapter_len\t"
                                "tail_adapter_err\ttail_poly\tkept_start\tkept_len\torient\n";
void formatEnds(Chunk& k, const talc_end_row* rows) {
  char num[192];
  for (size_t r = 0; r < k.ids.size(); ++r) {
    const talc_end_row& w = rows[r];
    const uint64_t L = k.offsets[r + 1] - k.offsets[r];
    const int m = snprintf(num, sizeof num, "\t%llu\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%d\n", (unsigned long long)L, w.head_adapter, w.head_adapter_len,
                           w.head_adapter_err, w.head_poly_len, w.tail_adapter, w.tail_adapter_len, w.tail_adapter_err, w.tail_poly_len, w.kept_start, w.kept_len,
                           w.orient);
    k.endsText += k.ids[r];
    k.endsText.append(num, (size_t)m);
    k.endSums[0] += 1;
    k.endSums[1] += (w.head_adapter || w.tail_adapter) ? 1 : 0;
    k.endSums[2] += (w.head_poly_len || w.tail_poly_len) ? 1 : 0;
    k.endSums[3] += L - w.kept_len;
  }
}

// the lines of <o>.umi.tsv for one batch from the scan's rows (k.ids, k.offsets: the reads, or the pieces, as they came),
// and the sums
const char* const kUmiHeader = "read_name\tlength\tend\terr\tother_err\tstart\tstop\tumi\tkept_start\tkept_len\n";
void formatUmi(Chunk& k, const talc_umi_row* rows) {
  char num[192];
  for (size_t r = 0; r < k.ids.size(); ++r) {
    const talc_umi_row& w = rows[r];
    const uint64_t L = k.offsets[r + 1] - k.offsets[r];
    char umi[33], other[8];
    const size_t u = w.end ? std::min<size_t>(w.umi_len, 32) : 0;
    memcpy(umi, w.umi, u); umi[u] = 0;
    if (!u) { umi[0] = '-'; umi[1] = 0; }
    if (w.other_err == 255) snprintf(other, sizeof other, "-"); else snprintf(other, sizeof other, "%u", w.other_err);
    const int m = snprintf(num, sizeof num, "\t%llu\t%u\t%u\t%s\t%u\t%u\t%s\t%u\t%u\n", (unsigned long long)L, w.end, w.err, other, w.start, w.stop, umi,
                           w.kept_start, w.kept_len);
    k.umiText += k.ids[r];
    k.umiText.append(num, (size_t)m);
    k.umiSums[0] += 1;
    k.umiSums[!w.end ? 4 : w.other_err != 255 ? 3 : w.end] += 1;
  }
}

// the lines of <o>.demux.tsv for one batch from the scan's rows (k.ids, k.offsets: the reads as they came), the sums and the
// counts; k.recBarcode: every read's barcode
const char* const kDemuxHeader = "read_name\traw_length\tbarcode\tstatus\thead_barcode\thead_err\thead_margin\thead_end\ttail_barcode\ttail_err\ttail_margin\ttail_end\n";
void formatDemux(const Options& o, Chunk& k, const talc_demux_row* rows) {
  const size_t B = o.lrBarcodeNames.size();
  auto name = [&](uint32_t b) -> const char* { return b >= 1 && b <= B ? o.lrBarcodeNames[b - 1].c_str() : "-"; };
  k.demuxCounts.assign(2 * (B + 1), 0);
  k.recBarcode.resize(k.ids.size());
  char num[256];
  for (size_t r = 0; r < k.ids.size(); ++r) {
    const talc_demux_row& w = rows[r];
    const uint64_t L = k.offsets[r + 1] - k.offsets[r];
    const int m = snprintf(num, sizeof num, "\t%llu\t%s\t%u\t%s\t%u\t%u\t%u\t%s\t%u\t%u\t%u\n", (unsigned long long)L, name(w.barcode), w.status, name(w.head_best),
                           w.head_err, w.head_margin, w.head_end, name(w.tail_best), w.tail_err, w.tail_margin, w.tail_end);
    k.demuxText += k.ids[r];
    k.demuxText.append(num, (size_t)m);
    const uint32_t b = w.barcode >= 1 && w.barcode <= B ? w.barcode : 0;
    k.recBarcode[r] = (uint8_t)b;
    const size_t slot = b ? b - 1 : B;
    k.demuxCounts[2 * slot] += 1;
    k.demuxCounts[2 * slot + 1] += L;
    k.demuxSums[0] += 1;
    if (b) k.demuxSums[w.status == TALC_DEMUX_BOTH ? 1 : w.status == TALC_DEMUX_HEAD_ONLY ? 2 : 3] += 1;
    else k.demuxSums[w.status == TALC_DEMUX_CONFLICT ? 4 : 5] += 1;
  }
}

// the lines of <o>.chimera.tsv for one batch from the scan's hits (k.ids, k.offsets: the reads as they came), and the sums:
// the pieces come from the same rule the library cuts by (talc_chimera_plan.h), so a report without --LRSplit says what a
// split would keep
const char* const kChimeraHeader = "read_name\traw_length\tadapter\tstrand\tstart\tend\terr\n";
const char* const kChimeraPiecesHeader = "piece_name\tread_name\tstart\tlen\n";
void formatChimera(Chunk& k, const std::vector<talc_chimera_hit>& hits, const std::vector<uint64_t>& hitOff, uint32_t minPiece,
                   std::vector<talc::SplitPiece>& pieces, std::vector<uint64_t>& pieceOff) {
  char num[160];
  const size_t n = k.ids.size();
  for (size_t r = 0; r < n; ++r)
    for (uint64_t h = hitOff[r]; h < hitOff[r + 1]; ++h) {
      const talc_chimera_hit& w = hits[h];
      const int m = snprintf(num, sizeof num, "\t%llu\t%u\t%c\t%u\t%u\t%u\n", (unsigned long long)(k.offsets[r + 1] - k.offsets[r]), w.adapter, w.strand ? '-' : '+',
                             w.start, w.end, w.err);
      k.chimeraText += k.ids[r];
      k.chimeraText.append(num, (size_t)m);
    }
  static_assert(sizeof(talc::ChimeraHit) == sizeof(talc_chimera_hit), "one record");
  uint64_t dropped = 0, droppedBases = 0;
  talc::split_pieces(reinterpret_cast<const talc::ChimeraHit*>(hits.data()), hitOff.data(), k.offsets.data(), (uint32_t)n, minPiece, pieces, pieceOff, &dropped,
                     &droppedBases);
  k.chimeraSums[0] += n;
  k.chimeraSums[1] += hits.size();
  for (size_t r = 0; r < n; ++r) k.chimeraSums[2] += hitOff[r + 1] > hitOff[r] ? 1 : 0;
  k.chimeraSums[3] += pieces.size();
  k.chimeraSums[4] += dropped;
  k.chimeraSums[5] += droppedBases;
}
// --LRSplit: the chunk's reads become the pieces (name_c<ordinal> for a cut read's, the name itself for an uncut read),
// their lines go to <o>.chimera_pieces.tsv
void takePieces(Chunk& k, const talc_split_piece* pieces, size_t np) {
  std::vector<std::string> ids;
  std::vector<uint64_t> offsets{0};
  ids.reserve(np); offsets.reserve(np + 1);
  char num[96];
  for (size_t p = 0; p < np; ++p) {
    const talc_split_piece& w = pieces[p];
    const std::string& name = k.ids[w.read];
    ids.push_back(w.ordinal ? name + "_c" + std::to_string(w.ordinal) : name);
    offsets.push_back(offsets.back() + w.len);
    const int m = snprintf(num, sizeof num, "\t%u\t%u\n", w.start, w.len);
    k.chimeraPiecesText += ids.back();
    k.chimeraPiecesText += '\t';
    k.chimeraPiecesText += name;
    k.chimeraPiecesText.append(num, (size_t)m);
  }
  k.ids.swap(ids);
  k.offsets.swap(offsets);
}

// the lines of <o>.edits.tsv for one batch (k.status filled; oo: the records' offsets; the ops of read r are ops[po[r] ..
// po[r + 1])): read_name status raw_length corr_length, five fields of the row, as_seen — '-' when the record is in the
// orientation the correction worked in rather than the caller's (-rev or a read voted reverse, passed through) —, and the
// ops as text
const char* const kEditsHeader = "read_name\tstatus\traw_length\tcorr_length\tn_match\tn_mismatch\tn_ins\tn_del\tn_unaligned\tas_seen\tcigar\n";
void formatEdits(const Options& o, Chunk& k, const uint32_t* ops, const uint64_t* po, const talc_edit_row* rows, const uint64_t* oo) {
  char num[256];
  for (size_t r = 0; r < k.ids.size(); ++r) {
    const talc_edit_row& w = rows[r];
    const bool corrected = k.status[r] == TALC_READ_CORRECTED;
    const int m = snprintf(num, sizeof num, "\t%d\t%llu\t%llu\t%u\t%u\t%u\t%u\t%u\t%c\t", k.status[r], (unsigned long long)(k.offsets[r + 1] - k.offsets[r]),
                           (unsigned long long)(oo[r + 1] - oo[r]), w.n_match, w.n_mismatch, w.n_ins, w.n_del, w.n_unaligned, (k.reversed(o.p, r) && !corrected) ? '-' : '+');
    k.editText += k.ids[r];
    k.editText.append(num, (size_t)m);
    if (po[r] == po[r + 1]) k.editText += '*';
    for (uint64_t i = po[r]; i < po[r + 1]; ++i) {
      const uint32_t code = ops[i] & 15u;
      k.editText += std::to_string(ops[i] >> 4);
      k.editText += code == 7u ? '=' : code == 8u ? 'X' : code == 1u ? 'I' : 'D';
    }
    k.editText += '\n';
    if (corrected) { k.editSums[0] += w.n_match; k.editSums[1] += w.n_mismatch; k.editSums[2] += w.n_ins; k.editSums[3] += w.n_del; k.editSums[4] += 1; k.editSums[5] += w.n_unaligned; }
  }
}

// the records of <o>.trim.fa or <o>.split.fa for one batch: the pieces of read r are po[rpo[r]] .. po[rpo[r + 1]] of
// `bytes`; a trimmed read keeps its name, split pieces are name_1, name_2, ... counting the kept ones; lines of 70 columns
void formatPieces(const Chunk& k, bool split, const char* bytes, const uint64_t* po, const uint64_t* rpo, std::string& text, uint64_t sums[2]) {
  for (size_t r = 0; r < k.ids.size(); ++r)
    for (uint64_t i = rpo[r]; i < rpo[r + 1]; ++i) {
      text += '>'; text += k.ids[r];
      if (split) { text += '_'; text += std::to_string(i - rpo[r] + 1); }
      text += '\n';
      const size_t L = (size_t)(po[i + 1] - po[i]);
      for (size_t p = 0; p < L; p += 70) { text.append(bytes + po[i] + p, std::min<size_t>(70, L - p)); text += '\n'; }
      sums[0] += 1; sums[1] += L;
    }
}

// one FASTQ record: @name, the sequence on one line, +, the qualities
void appendFastq(std::string& text, const std::string& id, uint64_t piece, const char* seq, const char* qual, size_t L) {
  text += '@'; text += id;
  if (piece) { text += '_'; text += std::to_string(piece); }
  text += '\n';
  text.append(seq, L); text += "\n+\n";
  text.append(qual, L); text += '\n';
}

// the records of <o>.fq for one batch: the records of <o>.fa (recs, oo) with the batch's quality bytes, which lie as the records do
void formatFastq(Chunk& k, const char* recs, const char* qual, const uint64_t* oo) {
  for (size_t r = 0; r < k.ids.size(); ++r) appendFastq(k.fqText, k.ids[r], 0, recs + oo[r], qual + oo[r], (size_t)(oo[r + 1] - oo[r]));
}

// the records of <o>.trim.fq or <o>.split.fq: the pieces as formatPieces names them; a piece's qualities are those of its
// place in the record (pieces[i].out_start of read r's record, which starts at oo[r])
void formatPiecesFastq(const Chunk& k, bool split, const char* bytes, const uint64_t* po, const talc_piece* pieces, const uint64_t* rpo, const char* qual,
                       const uint64_t* oo, std::string& text) {
  for (size_t r = 0; r < k.ids.size(); ++r)
    for (uint64_t i = rpo[r]; i < rpo[r + 1]; ++i)
      appendFastq(text, k.ids[r], split ? i - rpo[r] + 1 : 0, bytes + po[i], qual + oo[r] + pieces[i].out_start, (size_t)(po[i + 1] - po[i]));
}

// the lines of <o>.solidity.tsv for one batch (k.status filled; oo: the records' offsets): read_name status raw_length
// corr_length, the six fields of the raw row, the six of the corrected row; and the batch's share of the summary line
const char* const kSolidityHeader = "read_name\tstatus\traw_length\tcorr_length\traw_n_kmers\traw_n_solid\traw_n_in\traw_n_regions\traw_solid_bases\t"
                                    "raw_longest_weak\tcorr_n_kmers\tcorr_n_solid\tcorr_n_in\tcorr_n_regions\tcorr_solid_bases\tcorr_longest_weak\n";
void formatSolidity(Chunk& k, const talc_solidity* raw, const talc_solidity* cor, const uint64_t* oo) {
  char num[256];
  for (size_t r = 0; r < k.ids.size(); ++r) {
    const uint64_t rawLen = k.offsets[r + 1] - k.offsets[r], corLen = oo[r + 1] - oo[r];
    const talc_solidity &a = raw[r], &b = cor[r];
    const int m = snprintf(num, sizeof num, "\t%d\t%llu\t%llu\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\n", k.status[r], (unsigned long long)rawLen,
                           (unsigned long long)corLen, a.n_kmers, a.n_solid, a.n_in, a.n_regions, a.solid_bases, a.longest_weak, b.n_kmers, b.n_solid,
                           b.n_in, b.n_regions, b.solid_bases, b.longest_weak);
    k.solText += k.ids[r];
    k.solText.append(num, (size_t)m);
    k.solSums[0] += a.solid_bases; k.solSums[1] += rawLen; k.solSums[2] += b.solid_bases; k.solSums[3] += corLen;
  }
}

// the lines of <o>.map.tsv for one batch: the segments of read r are segs[so[r] .. so[r + 1]); those with both lengths 0
// are left out
void formatMap(Chunk& k, const talc_segment* segs, const uint64_t* so) {
  char num[96];
  for (size_t r = 0; r < k.ids.size(); ++r)
    for (uint64_t i = so[r]; i < so[r + 1]; ++i) {
      const talc_segment& g = segs[i];
      if (g.raw_len == 0 && g.out_len == 0) continue;
      const int m = snprintf(num, sizeof num, "\t%c\t%u\t%u\t%u\t%u\n", g.kind == TALC_SEG_SOLID ? 'S' : g.kind == TALC_SEG_CORRECTED ? 'C' : 'R',
                             g.raw_start, g.raw_len, g.out_start, g.out_len);
      k.mapText += k.ids[r];
      k.mapText.append(num, (size_t)m);
    }
}

// the text of one batch: '>' id, the sequence wrapped at 70 columns (io.cpp:50-75); the log and stats lines of its reads
void formatChunk(const Options& o, Chunk& k, const char* recs, const uint64_t* oo) {
  const size_t n = k.ids.size();
  size_t need = 0;
  for (size_t r = 0; r < n; ++r) { const size_t L = (size_t)(oo[r + 1] - oo[r]); need += k.ids[r].size() + 2 + L + (L + 69) / 70; }
  k.text.resize(need);
  char* w = &k.text[0];
  for (size_t r = 0; r < n; ++r) {
    // (a read that exhausted the device scratch is written through unchanged, like any read the reference fails on:
    //  it logs and goes on, main.cpp:298-303)
    const char* msg = k.status[r] == TALC_READ_NO_STRUCTURE ? "Unable to define convenient structure."       // main.cpp:290
                      : k.status[r] == TALC_READ_NO_SOLID_KMER ? "No solid kmer could be found."             // main.cpp:294
                      : k.status[r] == TALC_READ_ERROR ? "Device scratch exhausted; read left uncorrected." : nullptr;
    if (msg) { k.logText += "[Read: "; k.logText += k.ids[r]; k.logText += " ]: "; k.logText += msg; k.logText += '\n'; }
    if (o.readStats && k.stats.size() == 5 * n && k.stats[5 * r]) {   // Read.cpp:425-431
      k.statsText += "\n" + k.ids[r] + "\t" + std::to_string(k.stats[5 * r + 1]) + "\t" + std::to_string(k.stats[5 * r + 2]) + "\t" +
                     std::to_string(k.stats[5 * r + 3]) + "\t" + std::to_string(k.stats[5 * r + 4]);
    }
    *w++ = '>';
    memcpy(w, k.ids[r].data(), k.ids[r].size()); w += k.ids[r].size();
    *w++ = '\n';
    const char* q = recs + oo[r];
    const size_t L = (size_t)(oo[r + 1] - oo[r]);
    for (size_t p = 0; p < L; p += 70) { const size_t m = std::min<size_t>(70, L - p); memcpy(w, q + p, m); w += m; *w++ = '\n'; }
    if (o.lrDemuxOut) k.textEnd.push_back((size_t)(w - k.text.data()));
  }
  k.text.resize((size_t)(w - k.text.data()));
}

// no table at all (main.cpp:240, see prepareCounts): pass-through with the reference's statuses; the Dna5 conversion and
// -rev still apply
void passThrough(const Options& o, Chunk& c, const HostBuf& in) {
  const size_t n = c.ids.size();
  c.status.assign(n, TALC_READ_SKIPPED_SHORT);
  if (o.readStats) c.stats.assign(5 * n, 0);
  std::string all;
  std::vector<uint64_t> oo(n + 1, 0);
  if (o.autoStrand) {   // (no table: every count is 0, every read stays forward)
    c.strand.assign(n, talc_strand{0u, 0u, 0u, 0u, 0u, 0u});
    for (size_t r = 0; r < n; ++r) { const uint64_t L = c.offsets[r + 1] - c.offsets[r]; c.strand[r].n_kmers = L >= o.p.k ? (uint32_t)(L - o.p.k + 1) : 0u; }
  }
  for (size_t r = 0; r < n; ++r) {
    std::string q(in.p + c.offsets[r], c.offsets[r + 1] - c.offsets[r]);
    for (auto& ch : q) { ch = (ch == 'a' || ch == 'A') ? 'A' : (ch == 'c' || ch == 'C') ? 'C' : (ch == 'g' || ch == 'G') ? 'G' : (ch == 't' || ch == 'T') ? 'T' : 'N'; }
    if (o.p.reverse) {
      std::string rcs(q.size(), 'N');
      for (size_t i = 0; i < q.size(); ++i) { char ch = q[q.size() - 1 - i]; rcs[i] = ch == 'A' ? 'T' : ch == 'C' ? 'G' : ch == 'G' ? 'C' : ch == 'T' ? 'A' : 'N'; }
      q = rcs;
    }
    if (q.size() > o.p.k) {
      c.status[r] = TALC_READ_NO_SOLID_KMER;
      if (o.readStats) { c.stats[5 * r] = 1; c.stats[5 * r + 1] = (int64_t)q.size(); }
    }
    if (o.softMask) for (auto& ch : q) ch = (char)(ch | 0x20);   // (nothing was corrected: one RAW segment per read)
    all += q;
    oo[r + 1] = all.size();
  }
  if (o.corrMap) {
    std::vector<talc_segment> segs(n);
    std::vector<uint64_t> so(n + 1);
    for (size_t r = 0; r <= n; ++r) so[r] = r;
    for (size_t r = 0; r < n; ++r) { const uint32_t L = (uint32_t)(oo[r + 1] - oo[r]); segs[r] = talc_segment{TALC_SEG_RAW, 0u, L, 0u, L}; }
    formatMap(c, segs.data(), so.data());
  }
  if (o.solidity) {   // (no table: every count is 0, every position weak; the record is the read)
    std::vector<talc_solidity> rows(n, talc_solidity{0u, 0u, 0u, 0u, 0u, 0u});
    for (size_t r = 0; r < n; ++r) { const uint64_t L = oo[r + 1] - oo[r]; rows[r].n_kmers = rows[r].longest_weak = L >= o.p.k ? (uint32_t)(L - o.p.k + 1) : 0u; }
    formatSolidity(c, rows.data(), rows.data(), oo.data());
  }
  if (o.corrEdits) {   // (nothing was corrected: every read is L '=')
    std::vector<uint32_t> ops;
    std::vector<uint64_t> po(n + 1, 0);
    std::vector<talc_edit_row> rows(n, talc_edit_row{0u, 0u, 0u, 0u, 0u, 0u});
    for (size_t r = 0; r < n; ++r) {
      const uint32_t L = (uint32_t)(oo[r + 1] - oo[r]);
      if (L) { ops.push_back(L << 4 | 7u); rows[r].n_match = L; rows[r].n_ops = 1; }
      po[r + 1] = ops.size();
    }
    formatEdits(o, c, ops.data(), po.data(), rows.data(), oo.data());
  }
  if (o.autoStrand) formatStrand(c);
  if (o.fastq) {   // (no table: no k-mer is solid, every base has the lowest quality)
    const std::string qual(all.size(), (char)(33 + o.qmin));
    formatFastq(c, all.data(), qual.data(), oo.data());
  }
  formatChunk(o, c, all.data(), oo.data());
}

struct Scan {   // what the first pass over the read file found
  uint64_t nReads = 0;
  bool fastq = false;
};

// what one worker's time went into ([talc-timing]: device_busy_s_sum_over_workers and device_parts_s), and the reads it
// had to leave uncorrected; one per worker, added up once the workers have ended
struct WorkerTally {
  double supportMs = 0;   // --fastq: the device time of k_base_support, summed over the worker's batches
  double busy = 0, ctx = 0, create = 0, correct = 0, fetch = 0, text = 0, waitChunk = 0;
  uint64_t readErrors = 0;
};
struct PipelineTotals {
  double readerBusy = 0, writerBusy = 0;   // the three busy times overlap
  uint64_t bases = 0, batches = 0;
  uint64_t strandSums[2] = {0, 0};         // --auto-strand: reads taken forward, reverse
  uint64_t solSums[4] = {0, 0, 0, 0};      // --solidity: the sums of four columns of <o>.solidity.tsv (Chunk::solSums)
  uint64_t pieceSums[4] = {0, 0, 0, 0};    // --trim / --split: trimmed reads, their bases, split pieces, their bases
  uint64_t editSums[6] = {0, 0, 0, 0, 0, 0};   // --corr-edits: Chunk::editSums
  uint64_t endSums[4] = {0, 0, 0, 0};          // --LRAdapter / --LRPolyA: Chunk::endSums
  uint64_t chimeraSums[6] = {0, 0, 0, 0, 0, 0};   // --LRChimeras / --LRSplit: Chunk::chimeraSums
  uint64_t demuxSums[6] = {0, 0, 0, 0, 0, 0};     // --LRBarcodes: Chunk::demuxSums
  uint64_t umiSums[5] = {0, 0, 0, 0, 0};          // --LRUmi: Chunk::umiSums
  WorkerTally workers;
};

// The correction phase (replaces main.cpp:209-310).  The READER parses batches of --batch-reads reads straight into
// page-locked buffers of a pool of workers + 2 (input order = batch index); two WORKERS per logical GPU (own context and
// stream each: one batch's transfers run under the other's kernels) take a batch, correct it and turn the records into
// the text of <o>.fa themselves, so that formatting runs in parallel; the WRITER appends the finished batches' text
// strictly by batch index.  At most workers + 2 finished batches wait for the writer, the one it waits for excepted.
class Pipeline {
 public:
  // ndev logical GPUs on nphys devices (logical GPU d on device d mod nphys); ndev == 0: no table, one pass-through worker
  Pipeline(const Options& o, const talc::Switches& sw, const Files& files, talc_table* table, int ndev, int nphys, const Scan& scan)
      : o_(o), sw_(sw), files_(files), table_(table), ndev_(ndev), nphys_(nphys), nWorkers_(ndev ? 2 * ndev : 1), nInBufs_(nWorkers_ + 2), inBufs_(nInBufs_) {
    // what a batch's reads take, from the file's size and the scan's read count
    struct stat sb;
    if (ndev && scan.nReads > 0 && stat(o.seqFile.c_str(), &sb) == 0)
      batchBytesEstimate_ = (uint64_t)((double)sb.st_size / (double)scan.nReads * (double)std::min<uint64_t>(o.batchReads, scan.nReads) * (scan.fastq ? 0.55 : 1.05)) + (1u << 20);
    for (int i = 0; i < nInBufs_; ++i) q_.freeIn.push_back(i);
    q_.workersLeft = nWorkers_;
  }
  int workers() const { return nWorkers_; }
  // runs the three kinds of threads to the end of the input, `of` being the open <o>.fa; false: failure() says why
  bool run(std::ofstream of, PipelineTotals& tot);
  const std::string& failure() const { return q_.failMsg; }

 private:
  struct ReaderSide {   // the reader thread's own
    SeqReader in;
    double busy = 0;
    uint64_t bases = 0, batches = 0;
    explicit ReaderSide(const std::string& file) : in(file) {}
  };
  struct WriterSide {   // the writer thread's own
    std::ofstream of, lf, sf, mf, yf, tf, pf, ef, wf, qf, tqf, pqf, xf, cf, cpf, df, uf;
    uint64_t umiSums[5] = {0, 0, 0, 0, 0};
    std::vector<std::ofstream> bf;        // --LRDemuxOut: one per barcode, then unclassified
    uint64_t demuxSums[6] = {0, 0, 0, 0, 0, 0};
    std::vector<uint64_t> demuxCounts;    // Chunk::demuxCounts, summed
    double busy = 0;
    uint64_t strandSums[2] = {0, 0}, endSums[4] = {0, 0, 0, 0}, chimeraSums[6] = {0, 0, 0, 0, 0, 0};
    uint64_t solSums[4] = {0, 0, 0, 0}, pieceSums[4] = {0, 0, 0, 0}, editSums[6] = {0, 0, 0, 0, 0, 0};
  };
  bool fail(std::string msg);
  void readerMain(ReaderSide& r);
  void workerMain(int device, WorkerTally& t);
  void correctChunks(int device, WorkerTally& t);
  bool correctOnDevice(talc_ctx* ctx, Chunk& c, HostBuf& outb, WorkerTally& t);
  bool fetchPieces(talc_ctx* ctx, talc_batch* b, Chunk& c, bool split, const char* qual, const uint64_t* oo);
  void writerMain(WriterSide& w);   // io.cpp:50-75 + SeqFileOut FASTA writer, io.cpp:105-111 log lines

  // immutable once constructed
  const Options& o_;
  const talc::Switches& sw_;
  const Files& files_;
  talc_table* const table_;
  const int ndev_, nphys_, nWorkers_, nInBufs_;
  uint64_t batchBytesEstimate_ = 0;
  // input buffer i is used by one thread at a time: the reader once it has taken i off freeIn, then the worker that holds
  // the Chunk naming it, until that worker puts i back
  std::vector<HostBuf> inBufs_;
  struct Shared {
    std::mutex mu;   // guards every other member of this struct (`failed` is written under it and may be read without)
    std::condition_variable cvFree, cvReady, cvDone, cvRoom;
    std::vector<int> freeIn;
    std::deque<std::unique_ptr<Chunk>> ready;
    bool readerDone = false;
    std::map<uint64_t, std::unique_ptr<Chunk>> finished;
    int workersLeft = 0;
    uint64_t nextToWrite = 0;
    std::atomic<bool> failed{false};
    std::string failMsg;
  } q_;
};

// the first message wins; every waiter wakes up and ends.  Always false, for `return fail(...)`.
bool Pipeline::fail(std::string msg) {
  std::lock_guard<std::mutex> g(q_.mu);
  if (!q_.failed) q_.failMsg = std::move(msg);
  q_.failed = true;
  q_.cvFree.notify_all(); q_.cvReady.notify_all(); q_.cvDone.notify_all(); q_.cvRoom.notify_all();
  return false;
}

bool Pipeline::run(std::ofstream of, PipelineTotals& tot) {
  ReaderSide rd(o_.seqFile);
  WriterSide wr;
  wr.of = std::move(of);
  if (o_.corrMap) {
    wr.mf.open(files_.map, std::ios_base::trunc);
    if (!wr.mf) return fail("cannot write " + files_.map);
  }
  if (o_.solidity) {
    wr.yf.open(files_.solidity, std::ios_base::trunc);
    if (!wr.yf) return fail("cannot write " + files_.solidity);
    wr.yf << kSolidityHeader;
  }
  if (o_.trim) {   // (without a table both files exist and stay empty: nothing has a trusted base)
    wr.tf.open(files_.trim, std::ios_base::trunc);
    if (!wr.tf) return fail("cannot write " + files_.trim);
  }
  if (o_.split) {
    wr.pf.open(files_.split, std::ios_base::trunc);
    if (!wr.pf) return fail("cannot write " + files_.split);
  }
  if (o_.fastq) {   // (without a table the piece files exist and stay empty, as <o>.trim.fa and <o>.split.fa do)
    wr.qf.open(files_.fq, std::ios_base::trunc);
    if (!wr.qf) return fail("cannot write " + files_.fq);
    if (o_.trim) { wr.tqf.open(files_.trimFq, std::ios_base::trunc); if (!wr.tqf) return fail("cannot write " + files_.trimFq); }
    if (o_.split) { wr.pqf.open(files_.splitFq, std::ios_base::trunc); if (!wr.pqf) return fail("cannot write " + files_.splitFq); }
  }
  if (o_.corrEdits) {
    wr.ef.open(files_.edits, std::ios_base::trunc);
    if (!wr.ef) return fail("cannot write " + files_.edits);
    wr.ef << kEditsHeader;
  }
  if (o_.autoStrand) {
    wr.wf.open(files_.strand, std::ios_base::trunc);
    if (!wr.wf) return fail("cannot write " + files_.strand);
    wr.wf << kStrandHeader;
  }
  if (o_.lrEnds()) {
    wr.xf.open(files_.ends, std::ios_base::trunc);
    if (!wr.xf) return fail("cannot write " + files_.ends);
    wr.xf << kEndsHeader;
  }
  if (o_.lrChimeraScan()) {
    wr.cf.open(files_.chimera, std::ios_base::trunc);
    if (!wr.cf) return fail("cannot write " + files_.chimera);
    wr.cf << kChimeraHeader;
    if (o_.lrSplit) {
      wr.cpf.open(files_.chimeraPieces, std::ios_base::trunc);
      if (!wr.cpf) return fail("cannot write " + files_.chimeraPieces);
      wr.cpf << kChimeraPiecesHeader;
    }
  }
  if (o_.lrUmi()) {
    wr.uf.open(files_.umi, std::ios_base::trunc);
    if (!wr.uf) return fail("cannot write " + files_.umi);
    wr.uf << kUmiHeader;
  }
  if (o_.lrDemux()) {
    wr.df.open(files_.demux, std::ios_base::trunc);
    if (!wr.df) return fail("cannot write " + files_.demux);
    wr.df << kDemuxHeader;
    wr.demuxCounts.assign(2 * (o_.lrBarcodeNames.size() + 1), 0);
    if (o_.lrDemuxOut) {   // (a barcode without a read keeps an empty file)
      wr.bf.resize(o_.lrBarcodeNames.size() + 1);
      for (size_t b = 0; b < wr.bf.size(); ++b) {
        wr.bf[b].open(files_.demuxFa(o_, b), std::ios_base::trunc);
        if (!wr.bf[b]) return fail("cannot write " + files_.demuxFa(o_, b));
      }
    }
  }
  if (batchBytesEstimate_) {
    // the page-locked buffers are allocated once, at the estimated size, by as many threads as there are buffers (an
    // allocation of a few hundred MB takes tens of milliseconds)
    std::vector<std::thread> th;
    for (HostBuf& b : inBufs_) th.emplace_back(&HostBuf::reserve, &b, (size_t)batchBytesEstimate_);
    for (auto& t : th) t.join();
  }
  std::vector<WorkerTally> tally(nWorkers_);
  {
    std::thread reader(&Pipeline::readerMain, this, std::ref(rd)), writer(&Pipeline::writerMain, this, std::ref(wr));
    std::vector<std::thread> workers;
    for (int i = 0; i < nWorkers_; ++i) workers.emplace_back(&Pipeline::workerMain, this, ndev_ ? (i / 2) % nphys_ : -1, std::ref(tally[i]));
    for (auto& w : workers) w.join();
    reader.join();
    writer.join();
  }
  wr.of.close();
  if (wr.mf.is_open()) wr.mf.close();
  if (wr.yf.is_open()) wr.yf.close();
  if (wr.tf.is_open()) wr.tf.close();
  if (wr.pf.is_open()) wr.pf.close();
  if (wr.ef.is_open()) wr.ef.close();
  if (wr.wf.is_open()) wr.wf.close();
  if (wr.qf.is_open()) wr.qf.close();
  if (wr.tqf.is_open()) wr.tqf.close();
  if (wr.pqf.is_open()) wr.pqf.close();
  if (wr.xf.is_open()) wr.xf.close();
  if (wr.df.is_open()) wr.df.close();
  if (wr.uf.is_open()) wr.uf.close();
  for (int i = 0; i < 5; ++i) tot.umiSums[i] = wr.umiSums[i];
  for (auto& f : wr.bf) f.close();
  if (o_.lrDemux() && !q_.failed) {
    std::ofstream cf(files_.demuxCounts, std::ios_base::trunc);
    if (!cf) return fail("cannot write " + files_.demuxCounts);
    cf << "barcode\treads\tbases\n";
    const size_t B = o_.lrBarcodeNames.size();
    for (size_t b = 0; b <= B; ++b) cf << (b < B ? o_.lrBarcodeNames[b] : std::string("unclassified")) << "\t" << wr.demuxCounts[2 * b] << "\t" << wr.demuxCounts[2 * b + 1] << "\n";
  }
  for (int i = 0; i < 6; ++i) tot.demuxSums[i] = wr.demuxSums[i];
  for (int i = 0; i < 2; ++i) tot.strandSums[i] = wr.strandSums[i];
  for (int i = 0; i < 4; ++i) { tot.solSums[i] = wr.solSums[i]; tot.pieceSums[i] = wr.pieceSums[i]; tot.endSums[i] = wr.endSums[i]; }
  for (int i = 0; i < 6; ++i) tot.chimeraSums[i] = wr.chimeraSums[i];
  for (int i = 0; i < 6; ++i) tot.editSums[i] = wr.editSums[i];
  tot.readerBusy = rd.busy; tot.bases = rd.bases; tot.batches = rd.batches;
  tot.writerBusy = wr.busy;
  for (const WorkerTally& t : tally) {
    WorkerTally& s = tot.workers;
    s.busy += t.busy; s.ctx += t.ctx; s.create += t.create; s.correct += t.correct; s.fetch += t.fetch; s.text += t.text; s.waitChunk += t.waitChunk;
    s.readErrors += t.readErrors; s.supportMs += t.supportMs;
  }
  return !q_.failed;
}

void Pipeline::readerMain(ReaderSide& r) {
  std::string id;
  while (!q_.failed) {
    int bi = -1;
    {
      std::unique_lock<std::mutex> g(q_.mu);
      q_.cvFree.wait(g, [&] { return q_.failed || !q_.freeIn.empty(); });
      if (q_.failed) break;
      bi = q_.freeIn.back(); q_.freeIn.pop_back();
    }
    const auto tr0 = Clock::now();
    std::unique_ptr<Chunk> c(new Chunk());
    HostBuf& in = inBufs_[bi];
    in.len = 0;
    c->inBuf = bi;
    size_t refused = 0;   // the size the buffer could not grow to
    auto sink = [&](const char* q, size_t m) { if (!in.append(q, m)) refused = in.len + m; return refused == 0; };
    while (c->ids.size() < o_.batchReads && r.in.next(id, sink)) {
      c->ids.push_back(id);
      c->offsets.push_back(in.len);
    }
    r.busy += since(tr0);
    if (refused) { fail("no host memory: the input buffer of a batch cannot grow to " + std::to_string(refused) + " bytes"); break; }
    if (c->ids.empty()) { std::lock_guard<std::mutex> g(q_.mu); q_.freeIn.push_back(bi); break; }
    c->index = r.batches++;
    r.bases += in.len;
    std::lock_guard<std::mutex> g(q_.mu);
    q_.ready.push_back(std::move(c));
    q_.cvReady.notify_one();
  }
  std::lock_guard<std::mutex> g(q_.mu);
  q_.readerDone = true;
  q_.cvReady.notify_all();
}

void Pipeline::workerMain(int device, WorkerTally& t) {
  correctChunks(device, t);
  std::lock_guard<std::mutex> g(q_.mu);
  --q_.workersLeft;
  q_.cvDone.notify_all();
}

// device < 0: the pass-through worker
void Pipeline::correctChunks(int device, WorkerTally& t) {
  CtxPtr ctx;
  if (device >= 0) {
    const auto tc0 = Clock::now();
    talc_ctx* made = nullptr;
    if (talc_ctx_create(table_, &o_.p, device, &made) != TALC_OK) { fail(talc_last_error()); return; }
    ctx.reset(made);
    if ((o_.corrMap || o_.softMask || o_.trim || o_.split || o_.corrEdits) && talc_ctx_set_map(made, 1) != TALC_OK) { fail(talc_last_error()); return; }
    if (o_.autoStrand && talc_ctx_set_auto_strand(made, 1) != TALC_OK) { fail(talc_last_error()); return; }
    if (o_.lrEnds()) {
      std::string adapters;
      for (const std::string& ad : o_.lrAdapters) adapters += (adapters.empty() ? "" : ",") + ad;
      if (talc_ctx_set_ends(made, adapters.c_str(), o_.lrAdapterErr, o_.lrPolyA, o_.lrEndWindow) != TALC_OK) { fail(talc_last_error()); return; }
    }
    if (o_.lrChimeraScan() && talc_ctx_set_chimera(made, 1, o_.lrChimeraErr, o_.lrMinPiece) != TALC_OK) { fail(talc_last_error()); return; }
    if (o_.lrUmi() && talc_ctx_set_umi(made, o_.lrUmiPattern.c_str(), o_.lrUmiErr, o_.lrUmiWindow) != TALC_OK) { fail(talc_last_error()); return; }
    if (o_.lrDemux()) {
      std::string barcodes;
      for (const std::string& bc : o_.lrBarcodeSeqs) barcodes += (barcodes.empty() ? "" : ",") + bc;
      if (talc_ctx_set_demux(made, barcodes.c_str(), o_.lrBarcodeErr, o_.lrBarcodeMargin, o_.lrBarcodeWindow, o_.lrBarcodeBothEnds ? 1 : 0) != TALC_OK) { fail(talc_last_error()); return; }
    }
    t.ctx += since(tc0);
  }
  HostBuf outb;   // the corrected records of this worker's batches, kept for the whole run
  if (ctx && batchBytesEstimate_) outb.reserve(batchBytesEstimate_ + batchBytesEstimate_ / 16);   // (one page-locked allocation, not a dozen doublings)
  while (!q_.failed) {
    const auto tw0 = Clock::now();
    std::unique_ptr<Chunk> c;
    {
      std::unique_lock<std::mutex> g(q_.mu);
      q_.cvReady.wait(g, [&] { return q_.failed || !q_.ready.empty() || q_.readerDone; });
      if (q_.failed || q_.ready.empty()) break;
      c = std::move(q_.ready.front()); q_.ready.pop_front();
    }
    t.waitChunk += since(tw0);
    if (!ctx) passThrough(o_, *c, inBufs_[c->inBuf]);
    else if (!correctOnDevice(ctx.get(), *c, outb, t)) return;
    std::unique_lock<std::mutex> g(q_.mu);
    q_.freeIn.push_back(c->inBuf); c->inBuf = -1;
    q_.cvFree.notify_one();
    // (the batch the writer waits for always gets in; the others wait while the writer is more than a few batches behind)
    q_.cvRoom.wait(g, [&] { return q_.failed || c->index == q_.nextToWrite || q_.finished.size() < (size_t)nWorkers_ + 2; });
    q_.finished[c->index] = std::move(c);
    q_.cvDone.notify_one();
  }
}

// --trim / --split: the batch's records cut on the device, only the kept bytes fetched, and turned into the file's text
// (qual: the batch's quality bytes with the records' offsets oo, for the pieces' FASTQ records; null without --fastq)
bool Pipeline::fetchPieces(talc_ctx* ctx, talc_batch* b, Chunk& c, bool split, const char* qual, const uint64_t* oo) {
  if (talc_batch_pieces(ctx, b, split ? TALC_PIECES_SPLIT : TALC_PIECES_TRIM, o_.minPieceLen, o_.softMask ? 1 : 0) != TALC_OK) return fail(talc_last_error());
  const uint64_t np = talc_batch_num_pieces(b), nb = talc_batch_pieces_bytes(b);
  std::vector<char> bytes(std::max<uint64_t>(nb, 1));
  std::vector<uint64_t> po(np + 1), rpo(c.ids.size() + 1);
  std::vector<talc_piece> pieces(qual ? std::max<uint64_t>(np, 1) : 0);
  if (talc_batch_fetch_pieces(ctx, b, bytes.data(), nb, po.data(), qual ? pieces.data() : nullptr, qual ? np : 0, rpo.data()) != TALC_OK) return fail(talc_last_error());
  formatPieces(c, split, bytes.data(), po.data(), rpo.data(), split ? c.splitText : c.trimText, c.pieceSums + (split ? 2 : 0));
  if (qual) formatPiecesFastq(c, split, bytes.data(), po.data(), pieces.data(), rpo.data(), qual, oo, split ? c.splitFqText : c.trimFqText);
  return true;
}

// one batch through the device and into text; false after fail()
bool Pipeline::correctOnDevice(talc_ctx* ctx, Chunk& c, HostBuf& outb, WorkerTally& t) {
  uint32_t n = (uint32_t)c.ids.size();
  const auto td0 = Clock::now();
  struct Busy { double& sum; Clock::time_point t0; ~Busy() { sum += since(t0); } } busy{t.busy, td0};   // batch create .. the batch's release
  talc_batch* made = nullptr;
  const int mrc = o_.lrSplit  ? talc_batch_create_split(ctx, inBufs_[c.inBuf].p, c.offsets.data(), n, o_.lrClip ? 1 : 0, &made)
                  : o_.lrClip ? talc_batch_create_clipped(ctx, inBufs_[c.inBuf].p, c.offsets.data(), n, &made)
                              : talc_batch_create(ctx, inBufs_[c.inBuf].p, c.offsets.data(), n, &made);
  if (mrc != TALC_OK) return fail(talc_last_error());
  BatchPtr b(made);
  if (o_.lrDemux()) {   // the scan sees the reads as they came: a clipped or split batch ran it on them while it was made
    std::vector<talc_demux_row> rows(std::max<uint32_t>(n, 1));
    if (talc_batch_demux(ctx, b.get()) != TALC_OK || talc_batch_fetch_demux(ctx, b.get(), rows.data()) != TALC_OK) return fail(talc_last_error());
    formatDemux(o_, c, rows.data());
  }
  if (o_.lrChimeraScan()) {   // the scan sees the reads as they came (never a clipped batch: parse()); with --LRSplit it has made the batch, whose reads are the kept pieces from here on
    if (talc_batch_chimera(ctx, b.get()) != TALC_OK) return fail(talc_last_error());
    std::vector<talc_chimera_hit> hits(talc_batch_num_chimera_hits(b.get()));
    std::vector<uint64_t> hitOff((size_t)n + 1);
    if (talc_batch_fetch_chimera(ctx, b.get(), hits.data(), hits.size(), hitOff.data()) != TALC_OK) return fail(talc_last_error());
    std::vector<talc::SplitPiece> ruled;
    std::vector<uint64_t> ruledOff;
    formatChimera(c, hits, hitOff, o_.lrMinPiece, ruled, ruledOff);
    if (o_.lrSplit) {
      std::vector<talc_split_piece> pieces(std::max<uint64_t>(talc_batch_num_split_pieces(b.get()), 1));
      const size_t np = (size_t)talc_batch_num_split_pieces(b.get());
      if (talc_batch_fetch_split(ctx, b.get(), pieces.data(), nullptr) != TALC_OK) return fail(talc_last_error());
      static_assert(sizeof(talc::SplitPiece) == sizeof(talc_split_piece), "one record");
      if (np != ruled.size() || (np && memcmp(pieces.data(), ruled.data(), np * sizeof(talc_split_piece)) != 0))   // (the sums above are those of these very rows)
        return fail("the split batch's " + std::to_string(np) + " pieces are not the " + std::to_string(ruled.size()) + " the piece rule gives for its hits");
      if (o_.lrDemux()) {   // a piece goes where its source read goes
        std::vector<uint8_t> of(np);
        for (size_t p = 0; p < np; ++p) of[p] = c.recBarcode[pieces[p].read];
        c.recBarcode.swap(of);
      }
      takePieces(c, pieces.data(), np);
      n = (uint32_t)np;
    }
  }
  c.status.assign(n, TALC_READ_SKIPPED_SHORT);
  if (o_.lrEnds()) {   // the scan sees the reads as they came; with --LRClip it has made the batch, whose reads are the kept intervals from here on
    std::vector<talc_end_row> rows(std::max<uint32_t>(n, 1));
    if (talc_batch_ends(ctx, b.get()) != TALC_OK || talc_batch_fetch_ends(ctx, b.get(), rows.data()) != TALC_OK) return fail(talc_last_error());
    formatEnds(c, rows.data());
    if (o_.lrClip && !o_.lrUmi()) for (uint32_t r = 0; r < n; ++r) c.offsets[r + 1] = c.offsets[r] + rows[r].kept_len;
  }
  if (o_.lrUmi()) {   // a clipped or split batch ran the scan while it was made, on its reads or pieces as they came; with --LRClip the rows hold the combined intervals
    std::vector<talc_umi_row> rows(std::max<uint32_t>(n, 1));
    if (talc_batch_umi(ctx, b.get()) != TALC_OK || talc_batch_fetch_umi(ctx, b.get(), rows.data()) != TALC_OK) return fail(talc_last_error());
    formatUmi(c, rows.data());
    if (o_.lrClip) for (uint32_t r = 0; r < n; ++r) c.offsets[r + 1] = c.offsets[r] + rows[r].kept_len;
  }
  t.create += since(td0);
  const auto tk0 = Clock::now();
  // < 0: a real HIP / argument error stops the run; TALC_WARN_READ_ERRORS (> 0) is a complete batch in which some
  // reads kept their input sequence (status TALC_READ_ERROR -> a .log line), and the run goes on
  const int crc = talc_batch_correct(ctx, b.get());
  if (crc < 0) return fail(talc_last_error());
  t.correct += since(tk0);
  const auto tf0 = Clock::now();
  const uint64_t total = talc_batch_corrected_bytes(b.get());
  std::vector<uint64_t> oo(n + 1);
  if (!outb.reserve(std::max<uint64_t>(total, 1))) return fail("no host memory: " + std::to_string(total) + " bytes for the corrected records of a batch");
  const int frc = o_.softMask ? talc_batch_fetch_corrected_masked(ctx, b.get(), outb.p, total, oo.data(), c.status.data())
                              : talc_batch_fetch_corrected(ctx, b.get(), outb.p, total, oo.data(), c.status.data());
  if (frc != TALC_OK) return fail(talc_last_error());
  if (o_.autoStrand) {   // the vote ran before the batch was encoded: the rows come beside the records
    c.strand.resize(n);
    if (talc_batch_fetch_strand(ctx, b.get(), c.strand.data()) != TALC_OK) return fail(talc_last_error());
    formatStrand(c);
  }
  if (o_.corrMap) {   // fetched here, beside the records; the writer appends the lines in batch order
    std::vector<talc_segment> segs(std::max<uint64_t>(talc_batch_num_segments(b.get()), 1));
    std::vector<uint64_t> so(n + 1);
    if (talc_batch_fetch_map(ctx, b.get(), segs.data(), segs.size(), so.data()) != TALC_OK) return fail(talc_last_error());
    formatMap(c, segs.data(), so.data());
  }
  if (o_.solidity) {   // one more device pass over the reads and over the records, while both are in HBM
    std::vector<talc_solidity> raw(std::max<uint32_t>(n, 1)), cor(std::max<uint32_t>(n, 1));
    if (talc_batch_solidity(ctx, b.get()) != TALC_OK || talc_batch_fetch_solidity(ctx, b.get(), raw.data(), cor.data()) != TALC_OK) return fail(talc_last_error());
    formatSolidity(c, raw.data(), cor.data(), oo.data());
  }
  std::vector<char> qual;
  if (o_.fastq) {   // one more device pass over the records while they are in HBM; one byte per base crosses, beside the records
    const talc_support_params sp = {TALC_SUPPORT_RECORD, 1u, o_.qmin, o_.qmax};
    if (talc_batch_support(ctx, b.get(), &sp) != TALC_OK) return fail(talc_last_error());
    qual.resize(std::max<uint64_t>(talc_batch_support_bytes(b.get()), 1));
    if (talc_batch_fetch_support(ctx, b.get(), (uint8_t*)qual.data(), qual.size(), nullptr) != TALC_OK) return fail(talc_last_error());
    float ms = 0;
    talc_ctx_get_support_timing(ctx, &ms);
    t.supportMs += ms;
    formatFastq(c, outb.p, qual.data(), oo.data());
  }
  const char* q = o_.fastq ? qual.data() : nullptr;
  if (o_.trim && !fetchPieces(ctx, b.get(), c, false, q, oo.data())) return false;
  if (o_.split && !fetchPieces(ctx, b.get(), c, true, q, oo.data())) return false;
  if (o_.corrEdits) {   // aligned on the device while the reads and the records are in HBM; only the ops cross
    if (talc_batch_edits(ctx, b.get(), o_.maxEditCells) != TALC_OK) return fail(talc_last_error());
    const uint64_t nops = talc_batch_num_edit_ops(b.get());
    std::vector<uint32_t> ops(std::max<uint64_t>(nops, 1));
    std::vector<uint64_t> po(n + 1);
    std::vector<talc_edit_row> rows(std::max<uint32_t>(n, 1));
    if (talc_batch_fetch_edits(ctx, b.get(), ops.data(), nops, po.data(), rows.data()) != TALC_OK) return fail(talc_last_error());
    formatEdits(o_, c, ops.data(), po.data(), rows.data(), oo.data());
  }
  if (o_.readStats) {
    c.stats.resize(5ull * n);
    if (talc_batch_fetch_read_stats(ctx, b.get(), c.stats.data()) != TALC_OK) return fail(talc_last_error());
  }
  t.fetch += since(tf0);
  const auto tu0 = Clock::now();
  formatChunk(o_, c, outb.p, oo.data());
  t.text += since(tu0);
  if (sw_.timing == 2) {   // per batch: where this worker's time went
    talc_timing tm; talc_ctx_get_timing(ctx, &tm);
    fprintf(stderr, "[talc-batch] reads %u: create+H2D %.3f s, correct %.3f s (kernels: coverage %.1f structure %.1f search %.1f retry %.1f ms), fetch %.3f s, text %.3f s\n",
            n, secs(td0, tk0), secs(tk0, tf0), tm.coverage_ms, tm.structure_ms, tm.search_ms, tm.retry_ms, secs(tf0, tu0), since(tu0));
  }
  if (crc > 0) for (uint32_t i = 0; i < n; ++i) t.readErrors += c.status[i] == TALC_READ_ERROR ? 1 : 0;
  return true;
}

void Pipeline::writerMain(WriterSide& w) {
  while (true) {
    std::unique_ptr<Chunk> c;
    {
      std::unique_lock<std::mutex> g(q_.mu);
      auto next = [&] { return !q_.finished.empty() && q_.finished.begin()->first == q_.nextToWrite; };
      q_.cvDone.wait(g, [&] { return next() || q_.workersLeft == 0 || q_.failed; });
      if (!next()) break;   // (no worker left, or a failure)
      c = std::move(q_.finished.begin()->second);
      q_.finished.erase(q_.finished.begin());
    }
    const auto tw0 = Clock::now();
    if (!c->logText.empty()) { if (!w.lf.is_open()) w.lf.open(files_.log, std::ios_base::app); w.lf << c->logText; w.lf.flush(); }
    if (!c->statsText.empty()) { if (!w.sf.is_open()) w.sf.open(files_.stats, std::ios_base::app); w.sf << c->statsText; }
    w.of.write(c->text.data(), (std::streamsize)c->text.size());
    if (w.mf.is_open()) w.mf.write(c->mapText.data(), (std::streamsize)c->mapText.size());
    if (w.yf.is_open()) {
      w.yf.write(c->solText.data(), (std::streamsize)c->solText.size());
      for (int i = 0; i < 4; ++i) w.solSums[i] += c->solSums[i];
    }
    if (w.tf.is_open()) w.tf.write(c->trimText.data(), (std::streamsize)c->trimText.size());
    if (w.pf.is_open()) w.pf.write(c->splitText.data(), (std::streamsize)c->splitText.size());
    for (int i = 0; i < 4; ++i) w.pieceSums[i] += c->pieceSums[i];
    if (w.ef.is_open()) w.ef.write(c->editText.data(), (std::streamsize)c->editText.size());
    for (int i = 0; i < 6; ++i) w.editSums[i] += c->editSums[i];
    if (w.wf.is_open()) w.wf.write(c->strandText.data(), (std::streamsize)c->strandText.size());
    if (w.qf.is_open()) w.qf.write(c->fqText.data(), (std::streamsize)c->fqText.size());
    if (w.tqf.is_open()) w.tqf.write(c->trimFqText.data(), (std::streamsize)c->trimFqText.size());
    if (w.pqf.is_open()) w.pqf.write(c->splitFqText.data(), (std::streamsize)c->splitFqText.size());
    for (int i = 0; i < 2; ++i) w.strandSums[i] += c->strandSums[i];
    if (w.xf.is_open()) w.xf.write(c->endsText.data(), (std::streamsize)c->endsText.size());
    for (int i = 0; i < 4; ++i) w.endSums[i] += c->endSums[i];
    if (w.cf.is_open()) w.cf.write(c->chimeraText.data(), (std::streamsize)c->chimeraText.size());
    if (w.cpf.is_open()) w.cpf.write(c->chimeraPiecesText.data(), (std::streamsize)c->chimeraPiecesText.size());
    for (int i = 0; i < 6; ++i) w.chimeraSums[i] += c->chimeraSums[i];
    if (w.uf.is_open()) {
      w.uf.write(c->umiText.data(), (std::streamsize)c->umiText.size());
      for (int i = 0; i < 5; ++i) w.umiSums[i] += c->umiSums[i];
    }
    if (w.df.is_open()) {
      w.df.write(c->demuxText.data(), (std::streamsize)c->demuxText.size());
      for (int i = 0; i < 6; ++i) w.demuxSums[i] += c->demuxSums[i];
      for (size_t i = 0; i < c->demuxCounts.size() && i < w.demuxCounts.size(); ++i) w.demuxCounts[i] += c->demuxCounts[i];
      size_t from = 0;
      for (size_t r = 0; r < c->textEnd.size() && r < c->recBarcode.size() && !w.bf.empty(); ++r) {
        const size_t slot = c->recBarcode[r] ? c->recBarcode[r] - 1u : w.bf.size() - 1;
        if (slot < w.bf.size() && c->textEnd[r] <= c->text.size()) w.bf[slot].write(c->text.data() + from, (std::streamsize)(c->textEnd[r] - from));
        from = c->textEnd[r];
      }
    }
    w.busy += since(tw0);
    std::lock_guard<std::mutex> g(q_.mu);
    ++q_.nextToWrite;
    q_.cvRoom.notify_all();
  }
}

// ---- the phases of main(), in the reference's order.  An int result is 0 to go on, else the exit code after a message.

// first pass over the read file: format check and record count only (the reads themselves stream through in batches later)
bool scanReads(const Options& o, Scan& scan) {
  std::cout << "[TALC]: Attempting to load sequences." << std::endl;
  SeqReader probe(o.seqFile);
  scan.fastq = probe.fastq();
  if (probe.ok() && !probe.fastq()) {   // FASTA: the records are the lines that start with '>'
    const long long n = talc::countFastaRecords(o.seqFile);
    if (n >= 0) scan.nReads = (uint64_t)n;
  } else if (probe.ok()) {
    std::string id, seq;
    while (probe.next(id, seq)) ++scan.nReads;
  }
  if (!probe.ok()) {
    std::cout << "[TALC]: ISSUE WITH INPUT FILES" << std::endl;
    return false;
  }
  std::cout << "[TALC]: Hmm...it seems the sequence file is OK." << std::endl;
  std::cout << "[TALC]: " << scan.nReads << " long read(s) loaded" << std::endl;
  return true;
}

// -qm jellyfish2 (the reference: no table, one `jellyfish query` child per look-up — and never reached):
// the same counts as ONE table, from the tool's dump when -jf2 names it (o.dump / o.jdump then name the temporary dumps),
// else from the .jf itself; memory mode takes a .jf too.  haveTable false: a jellyfish2 run that names neither the
// program nor a .jf keeps the reference's behaviour, main.cpp:240: its loop runs on an EMPTY map (the jellyfish2 code path
// is dead), every read longer than K logs "No solid kmer could be found."
int prepareCounts(Options& o, TmpDumps& tmp, bool& haveTable) {
  haveTable = o.queryMode == "memory";
  if (o.queryMode == "jellyfish2" && !o.jf2.empty()) {
    std::string why;
    const std::string sr = o.outPrefix + ".SRCounts.dump.tmp", jn = o.outPrefix + ".junctions.dump.tmp";
    std::cout << "[TALC]: jellyfish2 mode: " << o.jf2 << "/jellyfish dump of " << o.dump << std::endl;
    tmp.files.push_back(sr);
    // (--both-strands: MIN_COUNT applies to the folded sum, so the tool must not drop a line)
    bool ok = jellyfishDump(o.jf2, o.dump, o.bothStrands ? 1 : o.p.min_count, sr, why);
    if (ok && o.useJ) { tmp.files.push_back(jn); ok = jellyfishDump(o.jf2, o.jdump, 0, jn, why); }
    if (!ok) { std::cerr << "talc: " << why << "\n"; return 2; }
    o.dump = sr;
    if (o.useJ) o.jdump = jn;
    haveTable = true;
  } else if (o.queryMode == "jellyfish2" && isJfFile(o.dump)) {
    std::cout << "[TALC]: jellyfish2 mode: reading " << o.dump << " natively" << std::endl;
    haveTable = true;
  }
  return 0;
}

// main.cpp:224-238; tableSize stays 0 without a table
int buildTable(Options& o, const talc::Switches& sw, TablePtr& table, uint64_t& tableSize) {
  int64_t st[3] = {0, 0, 0};
  int rc = TALC_OK;
  if (!o.srReads.empty()) {   // --SRReads: counted on the GPU, no count file in between
    std::cout << "[TALC]: Building the SR-" << (o.useJ ? "cdBG" : "dBG") << " from the k-mers of " << o.srReads.size() << " short-read file(s)";
    if (o.useJ) std::cout << " and count file: " << o.jdump;
    std::cout << std::endl;
    if (const int ec = countShortReads(o, sw, table, st)) return ec;
  } else {
    if (o.useJ) std::cout << "[TALC]: Building the SR-cdBG from count files: " << o.dump << " and " << o.jdump << std::endl;
    else std::cout << "[TALC]: Building the SR-dBG from count file: " << o.dump << std::endl;
    // the insert loop of buildCDBG runs on the first GPU when there is one (same table, ~10x faster on a 50 M dump)
    talc_table* built = nullptr;
    if (o.bothStrands)   // folded on the GPU; there is no host fold
      rc = talc_table_build_device_both_strands(o.dump.c_str(), o.useJ ? o.jdump.c_str() : nullptr, &o.p, 0, &built, st);
    else
      rc = (talc_device_count() > 0)
               ? talc_table_build_device(o.dump.c_str(), o.useJ ? o.jdump.c_str() : nullptr, &o.p, 0, &built, st)
               : talc_table_build(o.dump.c_str(), o.useJ ? o.jdump.c_str() : nullptr, &o.p, &built, st);
    table.reset(built);
  }
  if (rc != TALC_OK) {
    // an unreadable dump leaves the reference with an empty map (Jellyfish.cpp:249-251); anything else is fatal
    libError();
    if (rc != TALC_ERR_IO) return 2;
  } else {
    tableSize = talc_table_size(table.get());
    std::cout << "There were " << st[0] << " k-mers retrieved from database." << std::endl;
    std::cout << "In the whole, we have kept " << st[1] << "k-mers, whose counts were over the specified threshold." << std::endl;
  }
  std::cout << "[TALC]: SR-dBG contains " << tableSize << " nodes." << std::endl;
  return 0;
}

// the devices of this run, the table on each of them, and the batch size when --batch-reads did not give it
int chooseDevices(Options& o, const talc::Switches& sw, talc_table* table, uint64_t nReads, int& ndev, int& nphys) {
  nphys = talc_device_count();
  if (nphys <= 0) return noGpuError();
  ndev = nphys;
  // TALC_FAKE_GPUS=n (a rehearsal hook for one-GPU boxes): the sharder runs as if n GPUs were present, logical GPU d on
  // physical device d mod the real count — the same worker threads, contexts, dealing and ordered merge
  if (sw.fakeGpus) ndev = (int)sw.fakeGpus;
  if (o.gpus > 0) ndev = std::min(ndev, o.gpus);
  for (int d = 0; d < std::min(ndev, nphys); ++d)
    if (talc_table_upload(table, d) != TALC_OK) { std::cerr << "talc: device error: " << talc_last_error() << "\n"; return 2; }
  std::cout << "[TALC]: correcting on " << ndev << " GPU(s); k-mer table replicated (" << talc_table_device_bytes(table) / 1e9 << " GB each)" << std::endl;
  if (!o.haveBatchReads) {
    // at least two batches per worker (two workers per GPU) so that every worker's transfers find kernels to hide
    // under and the last batches end together; not below 20000 reads (a small batch leaves k_search's 5120 waves a
    // long tail), not above 200000
    const uint64_t per = (nReads + (uint64_t)ndev * 4 - 1) / ((uint64_t)ndev * 4);
    o.batchReads = (uint32_t)std::min<uint64_t>(200000, std::max<uint64_t>(20000, per));
  }
  return 0;
}

// the reference's own split (main.cpp:213-236: loading the reads, building the graph; :311-313: the correction), in
// wall-clock seconds instead of CPU minutes, then the same as JSON.  t: start, scanned, table built, uploaded, done.
void report(const Clock::time_point t[5], const PipelineTotals& p, const Scan& scan, uint32_t batchReads, int ndev, int workers) {
  const double phase = secs(t[3], t[4]);
  const WorkerTally& w = p.workers;
  fprintf(stderr, "[talc] scan=%.3fs table=%.3fs upload=%.3fs read+correct+write=%.3fs (%.3g bases/s, %llu batches of <= %u reads) total=%.3fs\n",
          secs(t[0], t[1]), secs(t[1], t[2]), secs(t[2], t[3]), phase, phase > 0 ? (double)p.bases / phase : 0.0,
          (unsigned long long)p.batches, batchReads, secs(t[0], t[4]));
  fprintf(stderr, "[talc-timing] {\"scan_s\": %.4f, \"table_parse_build_s\": %.4f, \"upload_s\": %.4f, \"correct_phase_s\": %.4f, "
                  "\"reader_busy_s\": %.4f, \"device_busy_s_sum_over_workers\": %.4f, \"writer_busy_s\": %.4f, \"total_s\": %.4f, "
                  "\"device_parts_s\": {\"ctx_create\": %.4f, \"batch_create_h2d\": %.4f, \"correct\": %.4f, \"fetch_d2h\": %.4f, \"records_to_text\": %.4f, \"waiting_for_reader\": %.4f}, "
                  "\"reads\": %llu, \"bases\": %llu, \"batches\": %llu, \"batch_reads\": %u, \"gpus\": %d, \"workers\": %d}\n",
          secs(t[0], t[1]), secs(t[1], t[2]), secs(t[2], t[3]), phase, p.readerBusy, w.busy, p.writerBusy, secs(t[0], t[4]),
          w.ctx, w.create, w.correct, w.fetch, w.text, w.waitChunk,
          (unsigned long long)scan.nReads, (unsigned long long)p.bases, (unsigned long long)p.batches, batchReads, ndev, workers);
}

}  // namespace

static int run(int argc, const char** argv) {
  bool bothStrands = false;   // (the banner comes before the arguments are parsed)
  for (int i = 1; i < argc; ++i) bothStrands |= std::string(argv[i]) == "--both-strands";
  std::cout << "******************************************************\n"
            << "* TALC : Transcriptome-Aware Long Read Correction    *\n"
            << "*----------------------------------------------------*\n"
            << "*                                                    *\n"
            << (bothStrands ? "* Kmers are taken on both strands                    *\n" : "* Kmers are assumed directional                      *\n")
            << "******************************************************" << std::endl;
  std::cout << "[TALC]: Parsing arguments" << std::endl;
  Options o = parse(argc, argv);
  const talc::Switches sw = talc::read_switches();   // (TALC_TIMING, TALC_FAKE_GPUS, TALC_TEST_POISON)
  if (sw.poisonByte >= 0 && talc_test_set_poison(sw.poisonByte, sw.poisonGuard) != TALC_OK) { std::cerr << "talc: " << talc_last_error() << "\n"; return 2; }
  const Files files(o.outPrefix);
  outputConfig(o, files.stats);          // Settings.cpp:122
  setBasicReadStatsHeader(files.stats);  // main.cpp:204

  Clock::time_point t[5];
  t[0] = Clock::now();
  Scan scan;
  if (!scanReads(o, scan)) return 0;   // main.cpp:219,323: prints and falls off main
  t[1] = Clock::now();

  TablePtr table;
  uint64_t tableSize = 0;
  bool haveTable = false;
  {
    TmpDumps tmp;
    if (const int ec = prepareCounts(o, tmp, haveTable)) return ec;
    if (haveTable)
      if (const int ec = buildTable(o, sw, table, tableSize)) return ec;
  }
  t[2] = Clock::now();
  if (!haveTable && o.lrDemux()) {
    std::cerr << "talc: --LRBarcodes looks at the reads on the GPU, beside the k-mer table: this run has no table (-qm jellyfish2 without -jf2 or a .jf)\n";
    return 2;
  }
  if (!haveTable && o.lrUmi()) {
    std::cerr << "talc: --LRUmi looks at the reads on the GPU, beside the k-mer table: this run has no table (-qm jellyfish2 without -jf2 or a .jf)\n";
    return 2;
  }
  if (!haveTable && o.lrEnds()) {
    std::cerr << "talc: --LRAdapter / --LRPolyA look at the reads on the GPU, beside the k-mer table: this run has no table (-qm jellyfish2 without -jf2 or a .jf)\n";
    return 2;
  }
  if (haveTable && tableSize == 0) {
    std::cout << "[TALC]: The de Bruijn Graph is empty...Correction aborted." << std::endl;  // main.cpp:319-320
    return 1;
  }
  std::cout << "[TALC]: Good news, there are nodes in the de Bruijn Graph." << std::endl;
  std::cout << "[TALC]: Maybe we can try and correct some long reads, then?" << std::endl;

  int ndev = 0, nphys = 0;
  if (haveTable)
    if (const int ec = chooseDevices(o, sw, table.get(), scan.nReads, ndev, nphys)) return ec;
  t[3] = Clock::now();

  std::cout << "Specified output file name: " << files.fa << std::endl;
  std::ofstream of(files.fa, std::ios_base::trunc);
  if (!of) { std::cerr << "ERROR: Could not open the file " << files.fa << "\n"; return 2; }
  Pipeline pipeline(o, sw, files, table.get(), ndev, nphys, scan);
  PipelineTotals totals;
  const bool ok = pipeline.run(std::move(of), totals);
  t[4] = Clock::now();
  if (!ok) { std::cerr << "talc: device error: " << pipeline.failure() << "\n"; return 2; }
  if (totals.workers.readErrors)
    std::cerr << "talc: " << totals.workers.readErrors << " read(s) exhausted the device scratch and were written uncorrected (see " << files.log << ")\n";
  if (o.solidity) {
    const uint64_t* y = totals.solSums;
    char line[200];
    snprintf(line, sizeof line, "[TALC]: solid bases: raw %llu of %llu (%.2f %%), corrected %llu of %llu (%.2f %%)", (unsigned long long)y[0], (unsigned long long)y[1],
             y[1] ? 100.0 * (double)y[0] / (double)y[1] : 0.0, (unsigned long long)y[2], (unsigned long long)y[3], y[3] ? 100.0 * (double)y[2] / (double)y[3] : 0.0);
    std::cout << line << std::endl;
  }
  if (o.trim || o.split) {
    const uint64_t* y = totals.pieceSums;
    std::string line = "[TALC]: ";
    if (o.trim) line += "trimmed: " + std::to_string(y[0]) + " reads, " + std::to_string(y[1]) + " bases";
    if (o.trim && o.split) line += "; ";
    if (o.split) line += "split: " + std::to_string(y[2]) + " pieces, " + std::to_string(y[3]) + " bases";
    std::cout << line << std::endl;
  }
  if (o.corrEdits) {
    const uint64_t* y = totals.editSums;
    std::cout << "[TALC]: edits: " << y[0] << " matches, " << y[1] << " mismatches, " << y[2] << " insertions, " << y[3] << " deletions in " << y[4]
              << " corrected reads (" << y[5] << " segments not aligned)" << std::endl;
  }
  if (o.autoStrand)
    std::cout << "[TALC]: strand: " << totals.strandSums[0] << " forward, " << totals.strandSums[1] << " reverse of " << totals.strandSums[0] + totals.strandSums[1]
              << " reads" << std::endl;
  if (o.lrEnds()) {
    const uint64_t* y = totals.endSums;
    std::cout << "[TALC]: read ends: " << y[0] << " reads, " << y[1] << " with an adapter, " << y[2] << " with a poly run, " << y[3] << " bases "
              << (o.lrClip ? "clipped" : "found (not clipped: no --LRClip)") << std::endl;
  }
  if (o.lrChimeraScan()) {
    const uint64_t* y = totals.chimeraSums;
    std::cout << "[TALC]: chimeras: " << y[0] << " reads, " << y[1] << " hits in " << y[2] << " reads, " << y[3] << " pieces kept, " << y[4]
              << " pieces dropped (" << y[5] << " bases)" << std::endl;
  }
  if (o.lrDemux()) {
    const uint64_t* y = totals.demuxSums;
    std::cout << "[TALC]: demux: " << y[0] << " reads, " << y[1] + y[2] + y[3] << " classified (" << y[1] << " both ends, " << y[2] << " head only, " << y[3]
              << " tail only), " << y[4] << " conflicts, " << y[5] << " without a barcode" << std::endl;
  }
  if (o.lrUmi()) {
    const uint64_t* y = totals.umiSums;
    std::cout << "[TALC]: umi: " << y[0] << " reads, " << y[1] << " at the head, " << y[2] << " at the tail, " << y[3] << " at both ends, " << y[4] << " without"
              << std::endl;
  }
  std::cout << "[TALC]: Looks like we are done now." << std::endl;
  if (sw.timing && o.fastq && ndev)
    fprintf(stderr, "[talc-lib] base support: %llu batches, k_base_support %.3f ms\n", (unsigned long long)totals.batches, totals.workers.supportMs);
  report(t, totals, scan, o.batchReads, ndev, pipeline.workers());
  return 0;
}

// (the table and the contexts are gone when run() has returned: their buffers' red zones have been checked)
int main(int argc, const char** argv) {
  const int ec = run(argc, argv);
  int byte = -1;
  uint32_t guard = 0;
  talc_test_get_poison(&byte, &guard);
  if (byte < 0) return ec;
  uint64_t r[4] = {0, 0, 0, 0};
  talc_test_guard_report(r);
  fprintf(stderr, "[talc-poison] byte %d, red zones of %u bytes: %llu buffers checked, %llu violations", byte, guard, (unsigned long long)r[0], (unsigned long long)r[1]);
  if (r[1]) fprintf(stderr, "; the first at a buffer of %llu bytes, %s it, byte %llu of the red zone", (unsigned long long)r[2], (r[3] >> 32) ? "behind" : "in front of", (unsigned long long)(r[3] & 0xFFFFFFFFull));
  fprintf(stderr, "\n");
  return r[1] ? 3 : ec;
}
