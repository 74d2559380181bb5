// seqan_compat/seqan/store.h — CPU ORACLE (TEST INFRASTRUCTURE, NOT PRODUCT CODE).  See basic.h.
// utils.hpp names seqan::Graph<seqan::Alignment<...> > with only this header to bring it in,
// and Trajectory.cpp uses Align the same way, so this header brings in align.h.
#pragma once
#include "align.h"
#include "basic.h"
