// seqan_compat/seqan/align.h — CPU ORACLE (TEST INFRASTRUCTURE, NOT PRODUCT CODE).  See basic.h.
//
// Score<int, Simple>, AlignConfig, Align with rows / row / assignSource, the alignment
// graph over a StringSet, and the score that globalAlignment / localAlignment return.
// The scores are shim::globalAlignmentScore / shim::localAlignmentScore
// (oracle/seqan_shim.hpp).  Sequence 0 (row 0, first string of the set) is the horizontal
// one, as in oracle/talc_oracle.cpp (Trail::Overlapscore, computeIDScore).
//
// No traceback is made, so the rows never hold gaps; the gap iterators that only
// utils.cpp InnerEditAlignment / BorderEditAlignment read are stubs that abort (basic.h).
#pragma once
#include "../../seqan_shim.hpp"
#include "basic.h"

namespace seqan {

template <typename TValue, typename TSpec>
struct Score;
template <>
struct Score<int, Simple> {
  int match, mismatch, gap;
  Score(int m, int mm, int g) : match(m), mismatch(mm), gap(g) {}
  talc_oracle::shim::SimpleScore shim() const {
    talc_oracle::shim::SimpleScore s = {match, mismatch, gap};
    return s;
  }
};

template <bool TOP, bool LEFT, bool RIGHT, bool BOTTOM>
struct AlignConfig {};

// ---- Align
template <typename TSource, typename TSpec = ArrayGaps>
struct Gaps {
  std::string source;
};
struct GapsIterator {};  // stub
template <typename TSource, typename TSpec = ArrayGaps>
struct Align {
  std::vector<Gaps<TSource, TSpec> > rowsData;
};
template <typename T> struct Row;
template <typename TSource, typename TSpec>
struct Row<Align<TSource, TSpec> > { typedef Gaps<TSource, TSpec> Type; };
template <typename T> struct Iterator;
template <typename TSource, typename TSpec>
struct Iterator<Gaps<TSource, TSpec> > { typedef GapsIterator Type; };

template <typename TSource, typename TSpec>
inline std::vector<Gaps<TSource, TSpec> >& rows(Align<TSource, TSpec>& a) { return a.rowsData; }
template <typename TSource, typename TSpec>
inline Gaps<TSource, TSpec>& row(Align<TSource, TSpec>& a, size_t i) { return a.rowsData[i]; }
template <typename TSource, typename TSpec, typename TSeq>
inline void assignSource(Gaps<TSource, TSpec>& g, const TSeq& s) { g.source = s.str(); }

template <typename TSource, typename TSpec>
inline GapsIterator begin(Gaps<TSource, TSpec>&) { compatMissing("begin(row)"); }
template <typename TSource, typename TSpec>
inline GapsIterator end(Gaps<TSource, TSpec>&) { compatMissing("end(row)"); }
inline bool isGap(const GapsIterator&) { compatMissing("isGap(iterator)"); }
inline GapsIterator& operator++(GapsIterator&) { compatMissing("++iterator"); }
inline GapsIterator& operator--(GapsIterator&) { compatMissing("--iterator"); }
inline bool operator!=(const GapsIterator&, const GapsIterator&) { compatMissing("iterator != iterator"); }

// ---- alignment graph over two strings
template <typename TStringSet> struct Alignment {};
template <typename TSpec> struct Graph;
template <typename TStringSet>
struct Graph<Alignment<TStringSet> > {
  std::string seq0, seq1;
  template <typename TSet>
  Graph(const TSet& set) : seq0(set.strings[0].str()), seq1(set.strings[1].str()) {}
};

// ---- scores
template <typename TSet, bool T, bool L, bool R, bool B>
inline int globalAlignment(Graph<Alignment<TSet> >& g, const Score<int, Simple>& sc, AlignConfig<T, L, R, B>, LinearGaps) {
  return talc_oracle::shim::globalAlignmentScore(g.seq0, g.seq1, sc.shim(), T, L, R, B);
}
template <typename TSet>
inline int globalAlignment(Graph<Alignment<TSet> >& g, const Score<int, Simple>& sc) {
  return talc_oracle::shim::globalAlignmentScore(g.seq0, g.seq1, sc.shim());
}
template <typename TSource, typename TSpec>
inline int globalAlignment(Align<TSource, TSpec>& a, const Score<int, Simple>& sc) {
  return talc_oracle::shim::globalAlignmentScore(a.rowsData[0].source, a.rowsData[1].source, sc.shim());
}
template <typename TSource, typename TSpec>
inline int globalAlignment(Align<TSource, TSpec>& a, const Score<int, Simple>& sc, LinearGaps) {
  return globalAlignment(a, sc);
}
template <typename TSource, typename TSpec>
inline int localAlignment(Align<TSource, TSpec>& a, const Score<int, Simple>& sc) {
  return talc_oracle::shim::localAlignmentScore(a.rowsData[0].source, a.rowsData[1].source, sc.shim());
}
template <typename TSource, typename TSpec>
inline int localAlignment(Align<TSource, TSpec>& a, const Score<int, Simple>& sc, LinearGaps) {
  return localAlignment(a, sc);
}

}  // namespace seqan
