// seqan_compat/seqan/seeds.h — CPU ORACLE (TEST INFRASTRUCTURE, NOT PRODUCT CODE).  See basic.h.
//
// Seed<Simple> and extendSeed(seed, database, query, direction, score, xdrop, GappedXDrop())
// as Trail.cpp:372-373,390-391 use them.  The extension is shim::extendSeed
// (oracle/seqan_shim.hpp); the argument order (begin H, begin V, end H, end V; database is
// the horizontal sequence) is the one oracle/talc_oracle.cpp getSeedAndExtension() uses.
#pragma once
#include "../../seqan_shim.hpp"
#include "align.h"
#include "basic.h"

namespace seqan {

enum ExtensionDirection { EXTEND_LEFT, EXTEND_RIGHT };

template <typename TSpec>
struct Seed {
  talc_oracle::shim::Seed s;
  template <typename A, typename B, typename C, typename D>
  Seed(A beginH, B beginV, C endH, D endV) {
    s.beginH = (long)beginH;
    s.beginV = (long)beginV;
    s.endH = (long)endH;
    s.endV = (long)endV;
  }
};

template <typename T> inline size_t beginPositionH(const Seed<T>& x) { return (size_t)x.s.beginH; }
template <typename T> inline size_t beginPositionV(const Seed<T>& x) { return (size_t)x.s.beginV; }
template <typename T> inline size_t endPositionH(const Seed<T>& x) { return (size_t)x.s.endH; }
template <typename T> inline size_t endPositionV(const Seed<T>& x) { return (size_t)x.s.endV; }

template <typename TSeedSpec, typename TDb, typename TQuery>
inline void extendSeed(Seed<TSeedSpec>& seed, const TDb& database, const TQuery& query, ExtensionDirection direction,
                       const Score<int, Simple>& sc, int scoreDropOff, GappedXDrop) {
  talc_oracle::shim::extendSeed(seed.s, database.str(), query.str(),
                                direction == EXTEND_LEFT ? talc_oracle::shim::EXTEND_LEFT
                                                         : talc_oracle::shim::EXTEND_RIGHT,
                                sc.shim(), scoreDropOff);
}

}  // namespace seqan
