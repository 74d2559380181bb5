// talc_switches.h — the environment switches of the library and of the CLI (host only; INTEGRATION.md "Library switches").
// The one place that reads the environment: a table call reads the switches when it starts, talc_ctx_create keeps the
// copy every batch of that context uses, the CLI reads its own at startup.  Ranges are applied here.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <string>

namespace talc {

struct Switches {
  // table calls
  int timing = 0;               // TALC_TIMING: set = 1 (a table build's wall-time split on stderr), "2..." = 2 (the CLI: also per batch)
  bool hostParse = false;       // TALC_HOST_PARSE: a text dump is parsed on the host
  int walk = -1;                // TALC_WALK: -1 unset (walk tables when the device has the room), 0 never, 1 always
  uint32_t filterBits = 20;     // TALC_FILTER_BITS: presence-filter bits per stored k-mer, 4 .. 64
  uint32_t tableSlotsX10 = 0;   // TALC_TABLE_SLOTS_X10: buckets per stored k-mer x 10, 20 .. 80 (0: HostTable::capacity_for decides)
  // contexts
  uint32_t searchSlots = 0;     // TALC_SEARCH_SLOTS: wave slots of a search launch (0: by the device)
  uint32_t seqArena = 0;        // TALC_SEQ_ARENA (test hook): bytes of a first-pass search's Trail arena (0: make_caps's own)
  uint32_t tinyCaps = 0;        // TALC_TEST_TINY_CAPS: a level.  1: first-pass scratch so small that reads go to the retry pass; 2: the
                                // x 8 stage's as well (flagged reads reach a real x 64 stage); 3: every stage's (reads exhaust all three)
  bool failRetryAlloc = false;  // TALC_TEST_FAIL_RETRY_ALLOC: the retry stage is refused
  int edgeTasks = -1;           // TALC_EDGE_TASKS: -1 (unset) the batch's fork share decides, 0 off, 1 on
  uint32_t edgeTaskMin = 150, edgeTaskHeavy = 200, edgeTaskRounds = 0xFFFF, edgeLingerMod = 16;   // TALC_EDGE_TASK_*, TALC_EDGE_LINGER_MOD
  bool edgeRedo = false;        // TALC_TEST_EDGE_REDO: every anchor another wave has run is redone in order
  bool edgeLane = true;         // TALC_TEST_EDGE_LANE=0: an edge search never enters the fused walk-and-score lane
  bool traceSteps = false;      // TALC_TRACE_STEPS: talc_batch_trace_read records every step
  uint32_t fakeGpus = 0;        // TALC_FAKE_GPUS (the CLI): the sharder runs as on a node with this many GPUs (0: the real count)
  int poisonByte = -1;          // TALC_TEST_POISON=<byte>[,<guard>] (the CLI): talc_test_set_poison at startup, the guard report at exit
  uint32_t poisonGuard = 256;
  std::string profReads;        // TALC_PROF_READS (the profile build): a file of one row per read
  bool profPrint = false, profSlow = false;   // TALC_PROF_PRINT, TALC_PROF_SLOW (the profile build): its reports on stderr
};

inline Switches read_switches() {
  auto given = [](const char* name) { return std::getenv(name) != nullptr; };
  auto num = [](const char* name, long unset) { const char* e = std::getenv(name); return e ? std::atol(e) : unset; };
  auto clamped = [&](const char* name, long unset, long lo, long hi) { return (uint32_t)std::min(std::max(num(name, unset), lo), hi); };
  Switches s;
  if (const char* e = std::getenv("TALC_TIMING")) s.timing = e[0] == '2' ? 2 : 1;
  s.hostParse = given("TALC_HOST_PARSE");
  if (given("TALC_WALK")) s.walk = num("TALC_WALK", 0) != 0 ? 1 : 0;
  if (const char* e = std::getenv("TALC_FILTER_BITS")) s.filterBits = (uint32_t)std::min<uint64_t>(64, std::max<uint64_t>(4, std::strtoull(e, nullptr, 10)));
  if (const char* e = std::getenv("TALC_TABLE_SLOTS_X10")) { const uint64_t v = std::strtoull(e, nullptr, 10); if (v >= 20 && v <= 80) s.tableSlotsX10 = (uint32_t)v; }
  s.searchSlots = clamped("TALC_SEARCH_SLOTS", 0, 0, 1L << 30);
  s.seqArena = clamped("TALC_SEQ_ARENA", 0, 0, 1L << 30);
  s.tinyCaps = clamped("TALC_TEST_TINY_CAPS", 0, 0, 3);
  s.failRetryAlloc = given("TALC_TEST_FAIL_RETRY_ALLOC");
  if (given("TALC_EDGE_TASKS")) { const long v = num("TALC_EDGE_TASKS", 0); s.edgeTasks = v == 0 ? 0 : v > 0 ? 1 : -1; }
  s.edgeTaskMin = clamped("TALC_EDGE_TASK_MIN", 150, 0, 1L << 30);
  s.edgeTaskHeavy = clamped("TALC_EDGE_TASK_HEAVY", 200, 0, 1L << 30);
  s.edgeTaskRounds = clamped("TALC_EDGE_TASK_ROUNDS", 0xFFFF, 0, 0xFFFF);
  s.edgeLingerMod = clamped("TALC_EDGE_LINGER_MOD", 16, 1, 1L << 20);
  s.edgeRedo = given("TALC_TEST_EDGE_REDO");
  s.edgeLane = num("TALC_TEST_EDGE_LANE", 1) != 0;
  s.traceSteps = num("TALC_TRACE_STEPS", 0) != 0;
  s.fakeGpus = clamped("TALC_FAKE_GPUS", 0, 0, 1L << 20);
  if (const char* e = std::getenv("TALC_TEST_POISON")) {
    char* end = nullptr;
    const long b = std::strtol(e, &end, 10);
    if (end != e && b >= 0 && b <= 255) {
      s.poisonByte = (int)b;
      if (*end == ',') { const unsigned long g = std::strtoul(end + 1, nullptr, 10); if (g % 256 == 0 && g <= (1ul << 20)) s.poisonGuard = (uint32_t)g; }
    }
  }
  if (const char* e = std::getenv("TALC_PROF_READS")) s.profReads = e;
  s.profPrint = given("TALC_PROF_PRINT");
  s.profSlow = given("TALC_PROF_SLOW");
  return s;
}

}  // namespace talc
