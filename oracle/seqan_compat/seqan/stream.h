// seqan_compat/seqan/stream.h — CPU ORACLE (TEST INFRASTRUCTURE, NOT PRODUCT CODE).  See basic.h.
// The sources include this header by habit; everything they use of it is in basic.h.
#pragma once
#include "basic.h"
