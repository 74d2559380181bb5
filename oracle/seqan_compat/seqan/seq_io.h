// seqan_compat/seqan/seq_io.h — CPU ORACLE (TEST INFRASTRUCTURE, NOT PRODUCT CODE).  See basic.h.
//
// SeqFileIn / SeqFileOut as io.cpp and utils.cpp use them.  Every position here is the one
// oracle/talc_oracle.cpp loadSeqData() / outputSeqData() already takes, so that a later
// disagreement with real SeqAn is a finding about both:
//   * the format is taken from the first non-empty line: '>' FASTA, '@' FASTQ; anything else
//     is unrecognised and open() fails (main.cpp:219,323 then print "ISSUE WITH INPUT FILES"
//     and leave with 0); a file that cannot be opened fails the same way; an empty file opens
//     and holds no record;
//   * the id is the whole header line after the marker; CR and LF end a line; blank lines
//     are skipped; a FASTA sequence runs over any number of lines; a FASTQ sequence runs to
//     the '+' line, and as many quality characters as it has bases are then skipped;
//   * a FASTQ record that does not start with '@' throws (io.cpp:42 returns 1);
//   * writeRecords writes FASTA: '>' id, then the sequence wrapped at 70 columns.
#pragma once
#include <fstream>

#include "basic.h"

namespace seqan {

struct SeqFileIn {
  std::ifstream in;
  bool fastq = false;
};

inline void compatChomp(std::string& l) {
  while (!l.empty() && (l.back() == '\r' || l.back() == '\n')) l.pop_back();
}

inline bool open(SeqFileIn& f, const char* name) {
  f.in.open(name);
  if (!f.in) return false;
  std::string line;
  std::streampos at = f.in.tellg();
  while (std::getline(f.in, line)) {
    compatChomp(line);
    if (line.empty()) { at = f.in.tellg(); continue; }
    if (line[0] != '>' && line[0] != '@') return false;
    f.fastq = (line[0] == '@');
    break;
  }
  f.in.clear();
  f.in.seekg(at);
  return true;
}

template <typename TId, typename TSeq>
inline void readRecords(StringSet<TId>& ids, StringSet<TSeq>& seqs, SeqFileIn& f) {
  std::string line, id, raw;
  bool have = false;
  while (std::getline(f.in, line)) {
    compatChomp(line);
    if (f.fastq) {
      if (line.empty()) continue;
      if (line[0] != '@') throw std::runtime_error("FASTQ record does not start with '@'");
      id = line.substr(1);
      raw.clear();
      while (std::getline(f.in, line)) {
        compatChomp(line);
        if (!line.empty() && line[0] == '+') break;
        raw += line;
      }
      size_t got = 0;
      while (got < raw.size() && std::getline(f.in, line)) {
        compatChomp(line);
        got += line.size();
      }
      ids.strings.push_back(TId(id));
      seqs.strings.push_back(TSeq(raw));
    } else {
      if (!line.empty() && line[0] == '>') {
        if (have) { ids.strings.push_back(TId(id)); seqs.strings.push_back(TSeq(raw)); }
        id = line.substr(1);
        raw.clear();
        have = true;
      } else if (have) {
        raw += line;
      }
    }
  }
  if (!f.fastq && have) { ids.strings.push_back(TId(id)); seqs.strings.push_back(TSeq(raw)); }
}

struct SeqFileOut {
  std::ofstream out;
};

inline bool open(SeqFileOut& f, const char* name) {
  f.out.open(name, std::ios_base::trunc);
  return (bool)f.out;
}

template <typename TId, typename TSeq>
inline void writeRecord(SeqFileOut& f, const TId& id, const TSeq& seq) {
  f.out << '>' << id << '\n';
  const std::string s = seq.str();
  for (size_t p = 0; p < s.size(); p += 70) f.out << s.substr(p, 70) << '\n';
}

template <typename TId, typename TSeq>
inline void writeRecords(SeqFileOut& f, const StringSet<TId>& ids, const StringSet<TSeq>& seqs) {
  for (size_t r = 0; r < ids.strings.size(); ++r) writeRecord(f, ids.strings[r], seqs.strings[r]);
}

// stub: only io.cpp outputSequalData, which nothing calls
template <typename TId, typename TSeq, typename TQual>
inline void writeRecords(SeqFileOut&, const StringSet<TId>&, const StringSet<TSeq>&, const StringSet<TQual>&) {
  compatMissing("writeRecords(file, ids, seqs, quals)");
}

}  // namespace seqan
