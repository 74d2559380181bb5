// seqan_compat/seqan/basic.h — CPU ORACLE (TEST INFRASTRUCTURE, NOT PRODUCT CODE)
//
// A small header set of this project's own, reachable as <seqan/...>, that offers exactly
// the part of the SeqAn2 API the TALC 1.01 sources call, so that those sources compile
// unmodified into oracle/_ref/ (oracle/Makefile, target `ref`).  It is not SeqAn and holds
// none of its text.  docs/reference_pin.md says what this pins and what it does not.
//
// This file: alphabets, String, StringSet, the free container functions, segments.
// The other <seqan/*.h> headers of this directory build on it:
//   sequence.h stream.h           nothing of their own (the sources include them by habit)
//   store.h                       brings in align.h (utils.hpp relies on that)
//   seq_io.h                      SeqFileIn / SeqFileOut, readRecords / writeRecord(s)
//   find.h                        Finder / Pattern<..., Horspool> / find / beginPosition
//   align.h                       Score, AlignConfig, Align, Graph<Alignment<>>, global/localAlignment
//   seeds.h                       Seed<Simple>, extendSeed(..., GappedXDrop())
//   arg_parse.h                   ArgumentParser
//
// The four algorithms (global score, local score, gapped x-drop extension, first occurrence)
// are NOT restated here: align.h, seeds.h and find.h call oracle/seqan_shim.hpp, which stays
// the one statement of each (pinned by tests/test_oracle_primitives.py).
//
// STUBS.  Operations that only dead code of the reference needs compile, and when called
// print the name of the missing operation and abort():
//   align.h   begin(row), end(row), isGap(it), ++it, --it, it != it   (gap iterators of a
//             Gaps row: utils.cpp InnerEditAlignment / BorderEditAlignment)
//   seq_io.h  writeRecords(file, ids, seqs, quals)                    (io.cpp outputSequalData)
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <exception>
#include <iostream>
#include <map>
#include <stdexcept>
#include <string>
#include <tuple>
#include <type_traits>
#include <vector>

namespace seqan {

[[noreturn]] inline void compatMissing(const char* what) {
  std::fprintf(stderr, "seqan_compat: operation not provided: %s\n", what);
  std::fflush(stderr);
  std::abort();
}

// ---------------------------------------------------------------- tags
struct Simple {};
struct LinearGaps {};
struct ArrayGaps {};
struct Horspool {};
struct GappedXDrop {};
template <typename T = void> struct Dependent {};
template <typename T = void> struct Owner {};
template <typename T = void> struct Alloc {};

typedef std::exception Exception;  // io.cpp catches `Exception const&` and calls what()

// ---------------------------------------------------------------- Dna5
// Dna5 from char: case folded, every character outside ACGT becomes N — the position
// oracle/talc_oracle.cpp toDna5() takes.  The value kept is the ordinal A=0 C=1 G=2 T=3 N=4,
// so that comparison orders A < C < G < T < N (the alphabet's own order, not ASCII's).
struct Dna5 {
  unsigned char value;
  Dna5() : value(0) {}
  Dna5(char c) : value(fromChar(c)) {}
  static unsigned char fromChar(char c) {
    switch (c) {
      case 'A': case 'a': return 0;
      case 'C': case 'c': return 1;
      case 'G': case 'g': return 2;
      case 'T': case 't': return 3;
      default: return 4;
    }
  }
  operator char() const { return "ACGTN"[value]; }
};
inline bool operator==(Dna5 a, Dna5 b) { return a.value == b.value; }
inline bool operator<(Dna5 a, Dna5 b) { return a.value < b.value; }
inline bool operator==(Dna5 a, char b) { return a == Dna5(b); }
inline std::ostream& operator<<(std::ostream& os, Dna5 b) { return os << (char)b; }

// ---------------------------------------------------------------- String
template <typename TValue, typename TSpec = Alloc<> >
class String {
 public:
  typedef std::vector<TValue> TData;
  TData data;

  String() {}
  String(const char* s) { assignChars(s, s ? std::char_traits<char>::length(s) : 0); }
  String(const std::string& s) { assignChars(s.data(), s.size()); }
  String(TValue v) : data(1, v) {}  // utils.cpp formNextKmer: `TSeq tmp(new_base)`
  template <typename U, typename S2>
  String(const String<U, S2>& o) { assignOther(o); }

  String& operator=(const char* s) { assignChars(s, s ? std::char_traits<char>::length(s) : 0); return *this; }
  String& operator=(const std::string& s) { assignChars(s.data(), s.size()); return *this; }
  template <typename U, typename S2>
  String& operator=(const String<U, S2>& o) { assignOther(o); return *this; }

  TValue& operator[](size_t i) { return data[i]; }
  const TValue& operator[](size_t i) const { return data[i]; }

  std::string str() const {
    std::string s(data.size(), '\0');
    for (size_t i = 0; i < data.size(); ++i) s[i] = (char)data[i];
    return s;
  }

 private:
  void assignChars(const char* s, size_t n) {
    data.resize(n);
    for (size_t i = 0; i < n; ++i) data[i] = TValue(s[i]);
  }
  template <typename U, typename S2>
  void assignOther(const String<U, S2>& o) {
    data.resize(o.data.size());
    for (size_t i = 0; i < o.data.size(); ++i) data[i] = TValue((char)o.data[i]);
  }
};

typedef String<char> CharString;
typedef String<Dna5> Dna5String;

// Ordering of a Dna5String as a std::map key (Jellyfish.hpp colouredDBG): lexicographic by
// the alphabet's ordinal, a proper prefix before the longer string.  The oracle's map is
// keyed by text, so the two iterate differently (T and N swap), but the correction path
// never iterates the map: it only looks keys up (Jellyfish.cpp count()/at()/operator[]).
template <typename T, typename S>
inline bool operator<(const String<T, S>& a, const String<T, S>& b) {
  return std::lexicographical_compare(a.data.begin(), a.data.end(), b.data.begin(), b.data.end());
}
template <typename T, typename S>
inline bool operator==(const String<T, S>& a, const String<T, S>& b) {
  return a.data.size() == b.data.size() && std::equal(a.data.begin(), a.data.end(), b.data.begin());
}
template <typename T, typename S>
inline std::ostream& operator<<(std::ostream& os, const String<T, S>& s) {
  for (size_t i = 0; i < s.data.size(); ++i) os << (char)s.data[i];
  return os;
}

// ---------------------------------------------------------------- StringSet
template <typename TString, typename TSpec = Owner<> >
class StringSet {
 public:
  std::vector<TString> strings;
  TString& operator[](size_t i) { return strings[i]; }
  const TString& operator[](size_t i) const { return strings[i]; }
};

// ---------------------------------------------------------------- free container functions
// length(): the size type is size_t for strings and standard containers alike, so
// arithmetic on it in the sources wraps as it does with SeqAn.
template <typename T, typename S> inline size_t length(const String<T, S>& s) { return s.data.size(); }
template <typename T, typename S> inline size_t length(const StringSet<T, S>& s) { return s.strings.size(); }
inline size_t length(const std::string& s) { return s.size(); }

template <typename T, typename A> inline bool empty(const std::vector<T, A>& v) { return v.empty(); }
template <typename K, typename V, typename C, typename A>
inline bool empty(const std::map<K, V, C, A>& m) { return m.empty(); }

template <typename T, typename S> inline void clear(String<T, S>& s) { s.data.clear(); }
template <typename T, typename A> inline void clear(std::vector<T, A>& v) { v.clear(); }

template <typename T, typename A> inline void resize(std::vector<T, A>& v, size_t n) { v.resize(n); }

template <typename T, typename S, typename U>
inline void appendValue(String<T, S>& s, const U& v) { s.data.push_back(T(v)); }
template <typename T, typename S, typename U>
inline void appendValue(StringSet<T, S>& s, const U& v) { s.strings.push_back(T(v)); }

template <typename T, typename S, typename U, typename S2>
inline void append(String<T, S>& s, const String<U, S2>& o) {
  String<T, S> tmp(o);  // a copy first: appending a string to itself is well defined
  s.data.insert(s.data.end(), tmp.data.begin(), tmp.data.end());
}

// erase(s, pos): removes the one value at pos.
template <typename T, typename S> inline void erase(String<T, S>& s, size_t pos) {
  if (pos < s.data.size()) s.data.erase(s.data.begin() + (std::ptrdiff_t)pos);
}

template <typename T, typename S> inline void reverse(String<T, S>& s) { std::reverse(s.data.begin(), s.data.end()); }
template <typename T, typename A> inline void sort(std::vector<T, A>& v) { std::sort(v.begin(), v.end()); }

// reverseComplement in place: A<->T, C<->G, N stays N — as oracle/talc_oracle.cpp
// reverseComplement() has it.
template <typename S> inline void reverseComplement(String<Dna5, S>& s) {
  std::reverse(s.data.begin(), s.data.end());
  for (size_t i = 0; i < s.data.size(); ++i)
    if (s.data[i].value < 4) s.data[i].value = (unsigned char)(3 - s.data[i].value);
}

// toCString: something that converts to `const char*`, lives to the end of the full
// expression, and can be dereferenced for its first character (Jellyfish.cpp:103).
struct CStringHolder {
  std::string s;
  operator const char*() const { return s.c_str(); }
  char operator*() const { return s.c_str()[0]; }
};
template <typename T, typename S> inline CStringHolder toCString(const String<T, S>& s) {
  CStringHolder h;
  h.s = s.str();
  return h;
}

// ---------------------------------------------------------------- segments
// prefix / suffix / infix give a copy.  A position outside the string is undefined in
// SeqAn; here it is clamped, exactly as oracle/talc_oracle.cpp infixS() clamps it (the
// oracle counts such events in its ub counters, and the tests assert there are none).
template <typename T, typename S>
inline String<T, S> infixClamped(const String<T, S>& s, long b, long e) {
  const long n = (long)s.data.size();
  if (b < 0) b = 0;
  if (e > n) e = n;
  String<T, S> r;
  if (e > b) r.data.assign(s.data.begin() + b, s.data.begin() + e);
  return r;
}
template <typename T, typename S, typename P1, typename P2>
inline String<T, S> infix(const String<T, S>& s, P1 b, P2 e) { return infixClamped(s, (long)b, (long)e); }
template <typename T, typename S, typename P>
inline String<T, S> prefix(const String<T, S>& s, P e) { return infixClamped(s, 0, (long)e); }
template <typename T, typename S, typename P>
inline String<T, S> suffix(const String<T, S>& s, P b) { return infixClamped(s, (long)b, (long)s.data.size()); }

}  // namespace seqan
