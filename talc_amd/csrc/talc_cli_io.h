// talc_cli_io.h — the CLI's sequence input and its growable host buffer (host only; talc_main.cpp).  Used by the
// long-read pipeline and by the --SRReads counting stage alike; page-locked memory comes from the C ABI.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include <fcntl.h>
#include <unistd.h>

#include "talc_hip.h"

namespace talc {

// lines of a file through one large buffer (read(2) in 8 MB pieces, memchr for the line ends): the streaming reader's
// std::getline loop was what bounded the whole correction phase once the GPU side had become quick (1 GB/s of FASTA)
class LineReader {
 public:
  explicit LineReader(const std::string& file) : buf_(8u << 20) { fd_ = open(file.c_str(), O_RDONLY); }
  LineReader(const LineReader&) = delete;
  LineReader& operator=(const LineReader&) = delete;
  ~LineReader() { if (fd_ >= 0) close(fd_); }
  bool ok() const { return fd_ >= 0; }
  // the next line without its "\n" / "\r\n"; the pointer is valid until the next call
  bool getline(const char*& p, size_t& len) {
    while (true) {
      const char* nl = (pos_ < end_) ? (const char*)memchr(buf_.data() + pos_, '\n', end_ - pos_) : nullptr;
      if (nl) {
        p = buf_.data() + pos_;
        len = (size_t)(nl - p);
        pos_ = (size_t)(nl - buf_.data()) + 1;
        while (len && (p[len - 1] == '\r' || p[len - 1] == '\n')) --len;
        return true;
      }
      if (eof_) {
        if (pos_ >= end_) return false;
        p = buf_.data() + pos_; len = end_ - pos_; pos_ = end_;   // a last line without a newline
        while (len && (p[len - 1] == '\r' || p[len - 1] == '\n')) --len;
        return true;
      }
      // no line end in what is left: move the tail to the front (grow the buffer for a line longer than it) and read on
      if (pos_ > 0) { memmove(&buf_[0], buf_.data() + pos_, end_ - pos_); end_ -= pos_; pos_ = 0; }
      if (end_ == buf_.size()) buf_.resize(buf_.size() * 2);
      const ssize_t r = read(fd_, &buf_[end_], buf_.size() - end_);
      if (r <= 0) eof_ = true; else end_ += (size_t)r;
    }
  }

 private:
  int fd_ = -1;
  std::vector<char> buf_;
  size_t pos_ = 0, end_ = 0;
  bool eof_ = false;
};

// Streaming FASTA / FASTQ reader (replaces loadSeqData, io.cpp:26-48, which holds the whole file, main.cpp:209-211):
// the format is decided by the first non-empty line ('>' or '@'); id = the whole header line after the marker;
// multi-line sequences are concatenated (blank lines and CRLF are fine); FASTQ qualities are skipped by length.
// Sequences are kept as raw text: the device applies the Dna5 conversion.
class SeqReader {
 public:
  explicit SeqReader(const std::string& file) : in_(file) {
    if (!in_.ok()) { std::cerr << "ERROR: Could not open file " << file << "\n"; ok_ = false; return; }
    while (in_.getline(lp_, ll_)) {   // first non-empty line decides the format
      if (ll_ == 0) continue;
      fastq_ = lp_[0] == '@';
      if (!fastq_ && lp_[0] != '>') ok_ = false;
      pending_ = true;
      break;
    }
  }
  // false: the file cannot be opened, is neither FASTA nor FASTQ, a FASTQ record did not start with '@', or a sink refused
  bool ok() const { return ok_; }
  bool fastq() const { return fastq_; }
  // a FASTQ record whose qualities ran out before its sequence's length (the long-read path reads on regardless)
  bool truncated() const { return truncated_; }
  // The next record: its id, and sink(p, n) called with every piece of its sequence.  False at the end of the file, and
  // false with ok() false from then on when a FASTQ record does not start with '@' or the sink returned false (no memory).
  template <class Sink>
  bool next(std::string& id, Sink&& sink) {
    return next(id, sink, [](const char*, size_t) { return true; });
  }
  // The same, and qsink(p, n) called with every piece of a FASTQ record's qualities: as many bytes as the sequence has
  // (multi-line qualities are joined by length; what a last line holds beyond it is dropped), fewer when truncated().
  template <class Sink, class QSink>
  bool next(std::string& id, Sink&& sink, QSink&& qsink) {
    if (!ok_) return false;
    if (!pending_) {
      while (true) {
        if (!in_.getline(lp_, ll_)) return false;
        if (fastq_ ? ll_ != 0 : (ll_ != 0 && lp_[0] == '>')) break;
      }
    }
    pending_ = false;
    if (fastq_) {
      if (lp_[0] != '@') { ok_ = false; return false; }
      id.assign(lp_ + 1, ll_ - 1);
      size_t n = 0;
      while (in_.getline(lp_, ll_)) { if (ll_ != 0 && lp_[0] == '+') break; if (ll_ && !sink(lp_, ll_)) { ok_ = false; return false; } n += ll_; }
      size_t got = 0;
      while (got < n && in_.getline(lp_, ll_)) {
        if (ll_ && !qsink(lp_, std::min(ll_, n - got))) { ok_ = false; return false; }
        got += ll_;
      }
      if (got < n) truncated_ = true;
      return true;
    }
    id.assign(lp_ + 1, ll_ - 1);
    while (in_.getline(lp_, ll_)) {
      if (ll_ != 0 && lp_[0] == '>') { pending_ = true; break; }
      if (ll_ && !sink(lp_, ll_)) { ok_ = false; return false; }
    }
    return true;
  }
  bool next(std::string& id, std::string& seq) {
    seq.clear();
    return next(id, [&](const char* p, size_t n) { seq.append(p, n); return true; });
  }

 private:
  LineReader in_;
  const char* lp_ = nullptr;
  size_t ll_ = 0;
  bool ok_ = true, fastq_ = false, pending_ = false, truncated_ = false;
};

// number of records of a FASTA file = lines that start with '>' (what SeqReader::next would return one by one), counted
// over 4 MB blocks without building a string per line; -1: cannot open
inline long long countFastaRecords(const std::string& file) {
  FILE* f = fopen(file.c_str(), "rb");
  if (!f) return -1;
  std::vector<char> buf(4u << 20);
  long long n = 0;
  bool atLineStart = true;
  size_t got;
  while ((got = fread(buf.data(), 1, buf.size(), f)) > 0) {
    const char* p = buf.data();
    const char* end = p + got;
    while (p < end) {
      if (atLineStart) { if (*p == '>') ++n; atLineStart = false; }
      const char* nl = (const char*)memchr(p, '\n', (size_t)(end - p));
      if (!nl) break;
      p = nl + 1;
      atLineStart = true;
    }
  }
  fclose(f);
  return n;
}

// a growable host buffer, page-locked when it can be (talc_pinned_alloc; no GPU / no page-locked memory left: pageable
// works too, only slower): the reads of a batch are parsed straight into one and the corrected records come back into
// another, so both directions are DMA transfers that run beside the kernels of the GPU's other worker
struct HostBuf {
  char* p = nullptr;
  size_t cap = 0, len = 0;
  bool pinned = false;
  HostBuf() = default;
  HostBuf(const HostBuf&) = delete;
  HostBuf& operator=(const HostBuf&) = delete;
  ~HostBuf() { release(); }
  void release() { if (pinned) talc_pinned_free(p); else free(p); p = nullptr; }
  bool reserve(size_t n) {
    if (n <= cap) return true;
    size_t nc = std::max<size_t>(n, std::max<size_t>(cap * 2, 1u << 20));
    bool pin = true;
    char* q = (char*)talc_pinned_alloc(nc);
    if (!q) { q = (char*)malloc(nc); pin = false; }
    if (!q) return false;
    if (len) memcpy(q, p, len);
    release();
    p = q; cap = nc; pinned = pin;
    return true;
  }
  bool append(const char* s, size_t n) {
    if (!reserve(len + n)) return false;
    memcpy(p + len, s, n);
    len += n;
    return true;
  }
};

}  // namespace talc
