// seqan_compat/seqan/find.h — CPU ORACLE (TEST INFRASTRUCTURE, NOT PRODUCT CODE).  See basic.h.
//
// Finder / Pattern<..., Horspool> as Trail.cpp:295-298 uses them: each find() moves to the
// next occurrence of the needle and says whether there was one; beginPosition() is where it
// starts.  The search itself is shim::findFirst (oracle/seqan_shim.hpp), called on what lies
// after the previous hit.
#pragma once
#include "../../seqan_shim.hpp"
#include "basic.h"

namespace seqan {

template <typename THaystack, typename TSpec = void>
struct Finder {
  std::string haystack;
  size_t next = 0;  // where the next search starts
  size_t at = 0;    // start of the current occurrence
  template <typename T>
  Finder(const T& h) : haystack(String<char>(h).str()) {}
};

template <typename TNeedle, typename TSpec>
struct Pattern {
  std::string needle;
  template <typename T>
  Pattern(const T& n) : needle(String<char>(n).str()) {}
};

template <typename TH, typename TS, typename TN, typename TP>
inline bool find(Finder<TH, TS>& f, const Pattern<TN, TP>& p) {
  if (f.next > f.haystack.size()) return false;
  const long r = talc_oracle::shim::findFirst(f.haystack.substr(f.next), p.needle);
  if (r < 0) {
    f.next = f.haystack.size() + 1;
    return false;
  }
  f.at = f.next + (size_t)r;
  f.next = f.at + 1;
  return true;
}

template <typename TH, typename TS>
inline size_t beginPosition(const Finder<TH, TS>& f) { return f.at; }

}  // namespace seqan
