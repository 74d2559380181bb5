// talc_capi_correct.inc — included by talc_capi.hip inside extern "C": the correction pipeline
// (coverage -> structure -> search -> pack) and the fetch / trace entry points.

// every k_search launch of the process gets a number of its own: the alignment rows a wave keeps in its scratch carry
// it, so that a row left by an earlier launch (or by another wave's slot, when the layout has changed) is never taken
// for one of this launch's (24 bits + a high byte no matrix value can have; it wraps after 16 M launches)
static uint32_t next_launch_stamp() {
  static std::atomic<uint32_t> launches{0};
  return 0x01000000u + (launches.fetch_add(1) & 0xFFFFFFu);
}
// the boxes of the first pass: a candidate of an edge search is at most its Trail (K + 1.2 gap + 2 K bases) followed by the
// rest of its reference (gap + K), gap <= MAX_BORDER_LEN + what the start anchors lie inside their region (a longer one
// sends the edge back to the in-order search)
static void ensure_edge_boxes(talc_ctx* c, Stage& st) {
  const uint64_t gap = (uint64_t)c->p.max_border_length + 256;
  const uint32_t seqCap = (uint32_t)align_up((uint64_t)(2.2 * (double)gap) + 4ull * c->p.k + 64, 16);
  const uint64_t need = (uint64_t)st.n_slots * edge_box_bytes(seqCap) + (uint64_t)st.n_slots * 4;
  if (c->sw.edgeTasks == 0 || c->p.max_start_anchors < 2 || c->p.max_start_anchors > EDGE_BOX_ANCHORS ||
      seqCap > (1u << 16) || need > (1ull << 30)) {   // (a border length in the tens of kilobases: not worth a gigabyte)
    st.boxes.reset(); st.boxes_bytes = 0;
    return;
  }
  if (need > st.boxes_bytes || seqCap != st.box_seq_cap) {
    st.boxes.reset(); st.boxes_bytes = 0;   // (the old boxes go before the larger ones are asked for)
    if (st.boxes.alloc(need) != hipSuccess) return;   // (the search runs without)
    st.boxes_bytes = need; st.box_seq_cap = seqCap;
  }
}

static int ensure_stage(talc_ctx* c, Stage& st, uint32_t maxLen, uint32_t scale, uint32_t n_work) {
  // (test hook TALC_TEST_TINY_CAPS: level 1 shrinks the first pass, 2 the x 8 stage as well, 3 every stage)
  const bool tiny = c->sw.tinyCaps >= (scale == 1 ? 1u : scale <= 8 ? 2u : 3u);
  const SearchCaps caps = make_caps(maxLen, c->p.k, scale, scale == 1 ? c->sw.seqArena : 0, tiny);
  if (!caps_hold_read(caps, maxLen))
    return fail(TALC_ERR_NOMEM, "a read of %u bases is beyond the 32-bit capacities of the search scratch", maxLen);
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, c->device));
  // (a retry stage's slots are 8 / 64 times a first-pass slot: one wave per SIMD at x 8 — 28 GB for 2 kb reads, halved below
  //  until it fits —, one per CU at x 64; a batch of nearly clean reads over a branching graph retries by the thousand)
  uint32_t want = (uint32_t)prop.multiProcessorCount * (scale == 1 ? 4u * TALC_SEARCH_WAVES_PER_SIMD : scale <= 8 ? 4u : 1u);
  if (c->sw.searchSlots) want = c->sw.searchSlots;
  const uint32_t wantSlots = std::max<uint32_t>(1, std::min<uint32_t>(want, n_work));
  if (scale > 1 && c->sw.failRetryAlloc)   // test hook: the retry stage does not fit
    return fail(TALC_ERR_NOMEM, "TALC_TEST_FAIL_RETRY_ALLOC: the retry stage is refused");
  // keep the scratch below ~60 % of what is free; the context's cached batch buffers are given back first when that
  // would cost slots (or the allocation itself fails)
  for (int attempt = 0; attempt < 2; ++attempt) {
    uint32_t slots = wantSlots;
    size_t freeB = 0, totalB = 0;
    HIPCHK(hipMemGetInfo(&freeB, &totalB));
    const uint64_t avail = (uint64_t)(0.6 * (double)freeB) + st.scratch_bytes;   // (the stage's own buffer is reused or replaced)
    while (slots > 1 && (uint64_t)slots * caps.slotBytes > avail) slots /= 2;
    const uint64_t need = (uint64_t)slots * caps.slotBytes;
    const bool cramped = slots < wantSlots || (uint64_t)caps.slotBytes > avail;
    if (cramped && attempt == 0 && c->cache.pool_bytes) { c->cache.trim(0); continue; }
    if ((uint64_t)caps.slotBytes > avail && need > st.scratch_bytes)
      return fail(TALC_ERR_NOMEM, "per-wave scratch of %llu bytes does not fit the device", (unsigned long long)caps.slotBytes);
    if (need > st.scratch_bytes) {
      st.scratch.reset(); st.scratch_bytes = 0;   // (the old scratch goes before the larger one is asked for)
      if (st.scratch.alloc(need) != hipSuccess) {
        if (attempt == 0) { c->cache.trim(0); continue; }
        return fail(TALC_ERR_NOMEM, "cannot allocate %llu bytes of search scratch", (unsigned long long)need);
      }
      st.scratch_bytes = need;
    }
    st.n_slots = slots;
    st.caps = caps;
    return TALC_OK;
  }
  return fail(TALC_ERR_NOMEM, "search scratch does not fit the device");
}

struct TraceHost {
  DevBuf<TraceRec> d_recs; DevBuf<uint32_t> d_nrec; DevBuf<uint8_t> d_pool; DevBuf<uint32_t> d_npool;
  uint32_t cap = 0, poolCap = 0;
};

#ifdef TALC_PROF
// the profile build's report of a corrected batch (TALC_PROF_READS / _PRINT / _SLOW); `counters`: the words of c->d_counters below the wave log
static int prof_report(talc_ctx* c, talc_batch* b, const uint64_t* counters) {
  if (!c->sw.profReads.empty()) {   // one row per read (its last pass): the cost estimate, its inputs, the search's duration
    if (FILE* f = fopen(c->sw.profReads.c_str(), "w")) {
      fprintf(f, "read\tlen\tstatus\tregions\tcost_est\thead\ttail\tgap_sum\tfork\tsolid\tticks_100MHz\tgap_sq\tgap_max\tsq640\tsteps\tedge_ticks\tanchors\tanchor_max\tstart\tbridges\tbridge_max\n");
      for (uint32_t r = 0; r < b->n_reads; ++r) {
        const ReadState& st = b->h_state[r];
        fprintf(f, "%u\t%llu\t%d\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\n", r, (unsigned long long)(b->h_offsets[r + 1] - b->h_offsets[r]), st.status,
                st.nRegions, st.costEst, st.pfHead, st.pfTail, st.pfGapSum, st.pfFork, st.pfSolid, st.pfTicks, st.pfGapSq, st.pfGapMax, st.pfShortReg, st.pfSteps, st.pfEdgeTicks, st.pfAnchors, st.pfAnchorMax, st.pfStart, st.pfBridges, st.pfBridgeMax);
      }
      fclose(f);
    }
  }
  if (!c->sw.profPrint) return TALC_OK;
  static const char* nm[] = TALC_PF_NAMES;   // starred entries are totals that contain other entries
  const uint64_t* const cat = counters + kCntProf0;
  const uint64_t tot = cat[PF_TOTAL], t0 = counters[kCntFirstStart], t1 = counters[kCntLastEnd];
  for (int i = 0; i < PF_N; ++i) fprintf(stderr, "[prof] %-10s %14llu cycles  %5.1f%%\n", nm[i], (unsigned long long)cat[i], tot ? 100.0 * cat[i] / tot : 0.0);
  if (t1 > t0 && c->stage.n_slots)
    fprintf(stderr, "[prof] wave utilisation: %.1f%% of %u waves x %.3f ms (first start to last end, 100 MHz counter)\n",
            100.0 * (double)counters[kCntBusy] / ((double)(t1 - t0) * c->stage.n_slots), c->stage.n_slots, (double)(t1 - t0) / 1e5);
  if (counters[kCntQueueDry] != ~0ull && counters[kCntQueueDry] > t0)
    fprintf(stderr, "[prof] the work queue ran dry %.3f ms after the first wave's start\n", (double)(counters[kCntQueueDry] - t0) / 1e5);
  if (c->sw.profSlow && c->stage.n_slots) {   // the record of every wave's last read: the waves that end last
    const uint32_t nw = std::min<uint32_t>(c->stage.n_slots, kCntMaxWaves);
    std::vector<uint64_t> lg(2 * (size_t)nw);
    HIPCHK(hipMemcpy(lg.data(), c->d_counters.get() + kCntWaveLog, lg.size() * 8, hipMemcpyDeviceToHost));
    std::vector<uint32_t> idx(nw);
    for (uint32_t i = 0; i < nw; ++i) idx[i] = i;
    const uint32_t t0w = (uint32_t)t0;   // (the log keeps the low words)
    auto endOf = [&](uint32_t w) { return (uint32_t)((uint32_t)lg[2 * w + 1] - t0w); };
    std::sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b2) { return endOf(a) > endOf(b2); });
    fprintf(stderr, "[slow] wave end times (ms), deciles from the last:");
    for (int d = 0; d <= 10; ++d) fprintf(stderr, " %.1f", endOf(idx[std::min<uint32_t>(nw - 1, (uint32_t)((uint64_t)d * nw / 10))]) / 1e5);
    fprintf(stderr, "\n");
    for (uint32_t i = 0; i < std::min<uint32_t>(nw, 24); ++i) {
      const uint32_t w = idx[i];
      const uint32_t qi = (uint32_t)(lg[2 * w] >> 32), r = (uint32_t)lg[2 * w], st = (uint32_t)(lg[2 * w + 1] >> 32) - t0w;
      const uint64_t L = (b->h_offsets.empty() || r >= b->n_reads) ? 0 : b->h_offsets[r + 1] - b->h_offsets[r];
      fprintf(stderr, "[slow] wave %5u ends %8.3f ms: last read %7u (queue %7u, len %6llu) started %8.3f ms\n", w, endOf(w) / 1e5, r, qi,
              (unsigned long long)L, st / 1e5);
    }
  }
  return TALC_OK;
}
#endif

static uint32_t* batch_stats(talc_ctx* c) { return c->d_hist.get() + kBatchStatsOff; }

// the reads' states as the device has them now, into b->h_state (waits for the stream)
static int fetch_states(talc_ctx* c, talc_batch* b) {
  if (!b->h_state.resize(b->n_reads)) return fail(TALC_ERR_NOMEM, "cannot allocate the host copy of %u read states", b->n_reads);
  if (b->n_reads) HIPCHK(hipMemcpyAsync(b->h_state.data(), b->d_state.get(), b->n_reads * sizeof(ReadState), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return TALC_OK;
}

static TraceBuf trace_buf(const talc_ctx* c, const TraceHost* th) {
  TraceBuf tb = {};
  if (th) { tb.recs = th->d_recs.get(); tb.nrec = th->d_nrec.get(); tb.cap = th->cap; tb.pool = th->d_pool.get(); tb.npool = th->d_npool.get(); tb.poolCap = th->poolCap; tb.steps = c->sw.traceSteps ? 1 : 0; }
  return tb;
}

// encode -> coverage -> k_structure on the context's stream, events kEvBegin .. kEvStructured around them: what run_pipeline and the test hook
// talc_batch_structure share (the hook stops here, so the region lists are still as k_structure left them)
static int launch_structure(talc_ctx* c, talc_batch* b, const TraceBuf& tb, uint32_t traceRead) {
  hipStream_t s = c->stream;
  int rc;
  memset(&c->timing, 0, sizeof c->timing);
  c->timing.n_kmers = b->n_kmers; c->timing.n_bases = b->n_bases;
  if ((rc = launch_encode_coverage(c, b))) return rc;
  HIPCHK(hipMemsetAsync(batch_stats(c), 0, kBatchStatsWords * sizeof(uint32_t), s));
  if (b->n_reads)
    hipLaunchKernelGGL(k_structure, dim3(b->n_reads), dim3(64), 0, s, c->dp, c->view, b->d_codes.get(), b->d_offsets.get(), b->d_koff.get(),
                       b->d_cov.get(), b->d_covw.get(), b->d_nin.get(), b->d_state.get(), b->d_regions.get(), b->d_regoff.get(), b->d_headcov.get(), b->n_reads, tb, traceRead, batch_stats(c));
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(c->ev[kEvStructured], s));
  return TALC_OK;
}

// the work queue (b->d_order): heaviest reads first, by k_structure's estimate
static int order_queue(talc_ctx* c, talc_batch* b) {
  if (!b->n_reads) return TALC_OK;
  hipStream_t s = c->stream;
  uint32_t* const hist = c->d_hist.get();
  HIPCHK(hipMemsetAsync(hist, 0, kOrderBuckets * sizeof(uint32_t), s));
  const unsigned nb = (b->n_reads + kOrderBlock - 1) / kOrderBlock;
  hipLaunchKernelGGL(k_order_scale, dim3(1), dim3(64), 0, s, batch_stats(c));
  hipLaunchKernelGGL(k_order_hist, dim3(nb), dim3(kOrderBlock), 0, s, b->d_state.get(), b->n_reads, hist, batch_stats(c));
  hipLaunchKernelGGL(k_order_scan, dim3(1), dim3(kOrderBuckets), 0, s, hist);
  hipLaunchKernelGGL(k_order_scatter, dim3(nb), dim3(kOrderBlock), 0, s, b->d_state.get(), b->n_reads, hist, b->d_order.get(), batch_stats(c));
  HIPCHK(hipGetLastError());
  return TALC_OK;
}

// One k_search launch: the waves of `st` take the `n_work` reads that `d_work` lists.  `edgeTasks`: the waves may hand edge
// searches to each other through the stage's boxes, where it has them (the first pass; a retry pass searches every edge
// in its own wave)
static int launch_search(talc_ctx* c, talc_batch* b, const Stage& st, const uint32_t* d_work, uint32_t n_work, const TraceBuf& tb,
                         uint32_t traceRead, bool edgeTasks) {
  hipStream_t s = c->stream;
  HIPCHK(hipMemsetAsync(c->d_queue.get(), 0, kQueueWords * sizeof(uint32_t), s));
  // test hook (talc_test_set_poison): the scratch, the boxes and a retry stage outlive a launch; every launch finds them poisoned
  const memcheck::Setting poison = memcheck::setting();
  if (poison.on && st.scratch_bytes) HIPCHK(hipMemsetAsync(st.scratch.get(), poison.byte, st.scratch_bytes, s));
  EdgeTaskArgs ea = {};
  ea.test = c->sw.edgeLane ? 0u : kTestNoEdgeLane;
  if (edgeTasks && st.boxes) {   // the claim counters sit behind the boxes
    ea.boxes = st.boxes.get();
    ea.avail = (uint32_t*)(st.boxes.get() + (uint64_t)st.n_slots * edge_box_bytes(st.box_seq_cap));
    ea.seqCap = st.box_seq_cap;
    ea.minWeak = c->sw.edgeTaskMin; ea.heavy = c->sw.edgeTaskHeavy; ea.heavyRounds = c->sw.edgeTaskRounds;
    ea.lingerMod = c->sw.edgeLingerMod; ea.test |= c->sw.edgeRedo ? kTestEdgeRedo : 0u;
    ea.autoSwitch = c->sw.edgeTasks > 0 ? nullptr : batch_stats(c) + kStatBranching;   // (switched on: whatever the batch looks like)
    if (poison.on) HIPCHK(hipMemsetAsync(ea.boxes, poison.byte, (uint64_t)st.n_slots * edge_box_bytes(st.box_seq_cap), s));   // (not the claim counters)
    HIPCHK(hipMemsetAsync(ea.avail, 0, (uint64_t)st.n_slots * 4, s));
  }
  hipLaunchKernelGGL(k_search, dim3(st.n_slots), dim3(64), 0, s, c->dp, c->view, st.caps, b->d_codes.get(), b->d_offsets.get(),
                     b->d_koff.get(), b->d_cov.get(), b->d_covw.get(), b->d_state.get(), b->d_regions.get(), b->d_regoff.get(), b->d_headcov.get(),
                     c->map ? b->d_regions.get() : nullptr, c->map ? b->d_mapedge.get() : nullptr, b->d_out.get(), b->d_outoff.get(), d_work,
                     n_work, c->d_queue.get(), st.scratch.get(), c->d_counters.get(), tb, traceRead, next_launch_stamp(), ea);
  HIPCHK(hipGetLastError());
  return TALC_OK;
}

// the first pass: every read, in queue order, through the context's stage (kEvSearched after it); the states stay on the device
static int search_first_pass(talc_ctx* c, talc_batch* b, const TraceBuf& tb, uint32_t traceRead) {
  hipStream_t s = c->stream;
  int rc;
  HIPCHK(hipMemsetAsync(c->d_counters.get(), 0, kCounterWords * sizeof(uint64_t), s));
  HIPCHK(hipMemsetAsync(c->d_counters.get() + kCntFirstStart, 0xFF, sizeof(uint64_t), s));   // (profile build: running minimum)
  HIPCHK(hipMemsetAsync(c->d_counters.get() + kCntQueueDry, 0xFF, sizeof(uint64_t), s));
  if (b->n_reads) {
    if ((rc = ensure_stage(c, c->stage, b->max_len, 1, b->n_reads))) return rc;
    ensure_edge_boxes(c, c->stage);
    if ((rc = launch_search(c, b, c->stage, b->d_order.get(), b->n_reads, tb, traceRead, true))) return rc;
  }
  HIPCHK(hipEventRecord(c->ev[kEvSearched], s));
  return TALC_OK;
}

// The offsets of the dense output from the states as the device has them now: b->d_dense_off[0 .. n] and, with the map on,
// b->d_seg_off[0 .. n] (k_emit_sums, k_emit_offsets), and the totals record, which the host waits for: `totals`
// (kTotWords words: reads with overflow set, record bytes, segments) points into the context's page-locked landing area
static int emit_offsets(talc_ctx* c, talc_batch* b, bool map, const uint64_t** totals) {
  hipStream_t s = c->stream;
  const uint32_t n = b->n_reads, nb = emit_blocks(n);
  HIPCHK(b->d_emit.ensure(c->cache, nb + 1));
  HIPCHK(b->d_dense_off.ensure(c->cache, n + 1));
  if (map) HIPCHK(b->d_seg_off.ensure(c->cache, n + 1));
  EmitSum* const sums = b->d_emit.get();
  hipLaunchKernelGGL(k_emit_sums, dim3(nb), dim3(kEmitThreads), 0, s, b->d_state.get(), n, sums);
  hipLaunchKernelGGL(k_emit_offsets, dim3(nb), dim3(kEmitThreads), 0, s, b->d_state.get(), n, sums, b->d_dense_off.get(),
                     map ? b->d_seg_off.get() : nullptr, (unsigned long long*)(sums + nb));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(c->h_land.data(), sums + nb, kTotWords * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  *totals = c->h_land.data();
  return TALC_OK;
}

// retry passes for the reads whose scratch overflowed (kEvRetry0 and kEvRetry1 around them; b->h_state holds the states of the
// first pass, fetch_states): buffers sized from the batch's longest
// read (a path can no longer outgrow its buffer), counted capacities x 8, then x 64 for whatever is still left
static int search_retry_passes(talc_ctx* c, talc_batch* b, const TraceBuf& tb, uint32_t traceRead) {
  hipStream_t s = c->stream;
  int rc;
  std::vector<uint32_t> retry;
  for (uint32_t r = 0; r < b->n_reads; ++r) if (b->h_state[r].overflow) retry.push_back(r);
  c->timing.n_retried = (uint32_t)retry.size();
  uint32_t* const report = c->retryReport;   // reads sent to x 8, to x 64, still flagged at the end, stages refused
  report[2] = (uint32_t)retry.size();
  HIPCHK(hipEventRecord(c->ev[kEvRetry0], s));
  for (uint32_t scale = 8; scale <= 64 && !retry.empty(); scale *= 8) {
    // The first pass has left a complete, valid batch: a retry stage that does not fit the device is not an error of the
    // batch.  The reads still flagged stay as the first pass left them (passed through, overflow set = TALC_READ_ERROR)
    // and the call returns TALC_WARN_READ_ERRORS; negative codes are kept for real HIP errors.
    Stage big;
    if ((rc = ensure_stage(c, big, b->max_len, scale, (uint32_t)retry.size()))) {
      if (rc == TALC_ERR_NOMEM) { ++report[3]; break; }
      return rc;
    }
    DevBuf<uint32_t> d_retry;
    if (d_retry.alloc(retry.size()) != hipSuccess) { ++report[3]; break; }
    report[scale == 8 ? 0 : 1] = (uint32_t)retry.size();
    HIPCHK(hipMemcpyAsync(d_retry.get(), retry.data(), retry.size() * 4, hipMemcpyHostToDevice, s));
    for (uint32_t r : retry) {
      b->h_state[r].overflow = 0;
      HIPCHK(hipMemcpyAsync(b->d_state.get() + r, &b->h_state[r], sizeof(ReadState), hipMemcpyHostToDevice, s));
    }
    if ((rc = launch_search(c, b, big, d_retry.get(), (uint32_t)retry.size(), tb, traceRead, false))) return rc;
    if ((rc = fetch_states(c, b))) return rc;
    d_retry.reset(); big = Stage();   // (both go before the next, larger stage is sized)
    std::vector<uint32_t> again;
    for (uint32_t r : retry) if (b->h_state[r].overflow) again.push_back(r);
    retry.swap(again);
    report[2] = (uint32_t)retry.size();
  }
  HIPCHK(hipEventRecord(c->ev[kEvRetry1], s));
  return TALC_OK;
}

// dense packing: k_pack into b->d_dense, `total` bytes at the offsets emit_offsets left (kEvEmitted after it)
static int pack_dense(talc_ctx* c, talc_batch* b, uint64_t total) {
  hipStream_t s = c->stream;
  HIPCHK(b->d_dense.ensure(c->cache, total));   // the record buffer of an earlier pass over this batch is kept when it is large enough
  if (b->n_reads)
    hipLaunchKernelGGL(k_pack, dim3(b->n_reads), dim3(256), 0, s, b->d_out.get(), b->d_outoff.get(), b->d_state.get(), b->d_dense_off.get(), b->d_dense.get(),
                       b->n_reads, c->p.reverse ? 1 : 0, b->rev_flags());
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(c->ev[kEvEmitted], s));
  return TALC_OK;
}

// the correction map (talc_ctx_set_map): k_pack_map into b->d_segs, `total` segments (2 R + 1 for a read k_search
// reassembled, 1 for every other) at the offsets emit_offsets left (kEvPackMap after it)
static int pack_map(talc_ctx* c, talc_batch* b, uint64_t total) {
  hipStream_t s = c->stream;
  HIPCHK(b->d_segs.ensure(c->cache, total));
  if (b->n_reads)
    hipLaunchKernelGGL(k_pack_map, dim3(b->n_reads), dim3(64), 0, s, b->d_state.get(), b->d_regions.get(), b->d_regoff.get(), b->d_mapedge.get(),
                       b->d_offsets.get(), b->d_seg_off.get(), b->d_segs.get(), b->n_reads, c->p.k, c->p.reverse ? 1 : 0,
                       b->rev_flags());
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(c->ev[kEvPackMap], s));
  return TALC_OK;
}

// The one copy back and the one wait at the end: the states, the offsets and the device counters below the wave log into
// page-locked host memory; then the stage times and the batch's counts into c->timing (`counters`: into the landing area)
static int read_timing(talc_ctx* c, talc_batch* b, bool map, uint32_t n_failed, const uint64_t** counters) {
  hipStream_t s = c->stream;
  const uint32_t n = b->n_reads;
  int rc;
  if (!b->h_state.resize(n) || !b->h_dense_off.resize(n + 1) || (map && !b->h_seg_off.resize(n + 1)))
    return fail(TALC_ERR_NOMEM, "cannot allocate the host copies of %u reads' states and offsets", n);
  uint64_t* const land = c->h_land.data() + kTotWords;
  if (n) HIPCHK(hipMemcpyAsync(b->h_state.data(), b->d_state.get(), (size_t)n * sizeof(ReadState), hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(b->h_dense_off.data(), b->d_dense_off.get(), ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, s));
  if (map) HIPCHK(hipMemcpyAsync(b->h_seg_off.data(), b->d_seg_off.get(), ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(land, c->d_counters.get(), kCntWaveLog * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if ((rc = read_stage_times(c, kEvEmitted))) return rc;
  c->timing.n_trail_steps = land[kCntSteps];
  c->timing.n_dp_cells = land[kCntCells];
  c->timing.n_failed = n_failed;
  if (c->sw.timing)   // (TALC_TIMING: whether this batch's copies were DMA transfers, or page-locking failed and they were staged)
    fprintf(stderr, "[talc-lib] correction: host arrays page-locked: states %d, offsets %d, landing area %d\n", b->h_state.pinned() ? 1 : 0,
            b->h_dense_off.pinned() ? 1 : 0, c->h_land.pinned() ? 1 : 0);
  *counters = land;
  return TALC_OK;
}

static int run_pipeline(talc_ctx* c, talc_batch* b, TraceHost* th, uint32_t traceRead) {
  HIPCHK(hipSetDevice(c->device));
  int rc;
  b->holds.drop_results();
  memset(c->retryReport, 0, sizeof c->retryReport);
  const bool map = c->map;
  if (map) HIPCHK(b->d_mapedge.ensure(c->cache, 2ull * std::max<uint32_t>(b->n_reads, 1)));
  const TraceBuf tb = trace_buf(c, th);
  const uint64_t* counters = nullptr;
  const uint64_t* tot = nullptr;
  if ((rc = launch_structure(c, b, tb, traceRead))) return rc;
  if ((rc = order_queue(c, b))) return rc;
  if ((rc = search_first_pass(c, b, tb, traceRead))) return rc;
  HIPCHK(hipEventRecord(c->ev[kEvRetry0], c->stream));   // (no read overflowed: there is no retry pass between these two)
  HIPCHK(hipEventRecord(c->ev[kEvRetry1], c->stream));
  if ((rc = emit_offsets(c, b, map, &tot))) return rc;
  if (tot[kTotOverflow]) {   // some read's scratch ran out: the states to the host, the retry passes, the offsets again
    if ((rc = fetch_states(c, b))) return rc;
    if ((rc = search_retry_passes(c, b, tb, traceRead))) return rc;
    if ((rc = emit_offsets(c, b, map, &tot))) return rc;
  }
  const uint32_t n_failed = (uint32_t)tot[kTotOverflow];
  if ((rc = pack_dense(c, b, tot[kTotBytes]))) return rc;
  if (map && (rc = pack_map(c, b, tot[kTotSegs]))) return rc;
  if ((rc = read_timing(c, b, map, n_failed, &counters)) || (rc = read_spans(c))) return rc;
#ifdef TALC_PROF
  if ((rc = prof_report(c, b, counters))) return rc;
#endif
  b->holds.corrected = true; b->holds.mapped = map;
  if (c->timing.n_failed) {   // the batch is valid: those reads are passed through unchanged with status TALC_READ_ERROR
    fail(TALC_WARN_READ_ERRORS, "%u read(s) exhausted the device scratch even in the retry pass (status TALC_READ_ERROR)", c->timing.n_failed);
    return TALC_WARN_READ_ERRORS;
  }
  return TALC_OK;
}

int talc_batch_correct(talc_ctx* c, talc_batch* b) {
  if (int rc = belong(c, b, "bad context/batch")) return rc;
  return run_pipeline(c, b, nullptr, 0xFFFFFFFFu);
}

// Test hook (not part of the reference surface): the pipeline up to and including k_structure, nothing of the search.
int talc_batch_structure(talc_ctx* c, talc_batch* b) {
  int rc;
  if ((rc = enter(c, b, "bad context/batch"))) return rc;
  b->holds.drop_results();
  if ((rc = launch_structure(c, b, TraceBuf{}, 0xFFFFFFFFu))) return rc;
  if ((rc = fetch_states(c, b))) return rc;
  if ((rc = read_stage_times(c, kEvStructured)) || (rc = read_spans(c))) return rc;
  b->holds.structured = true;
  return TALC_OK;
}

// Test hook: the work queue of a batch talc_batch_structure has run on (see include/talc_hip.h)
int talc_batch_order(talc_ctx* c, talc_batch* b, uint32_t* order, uint32_t* bucket) {
  if (int rc = belong(c, b, "bad context/batch/buffer", order && bucket)) return rc;
  if (!b->holds.structured) return fail(TALC_ERR_STATE, "talc_batch_structure has not run on this batch (or a correction has run since)");
  HIPCHK(hipSetDevice(c->device));
  int rc;
  if ((rc = order_queue(c, b))) return rc;
  uint32_t scale = 256u;
  if (b->n_reads) {   // (an empty batch has no queue, and nothing has set the scale)
    HIPCHK(hipMemcpyAsync(order, b->d_order.get(), (size_t)b->n_reads * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&scale, batch_stats(c) + kStatGapScale, 4, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  for (uint32_t r = 0; r < b->n_reads; ++r) bucket[r] = order_bucket(b->h_state[r], scale);
  bucket[b->n_reads] = scale;
  return TALC_OK;
}

// Test hook: what k_structure left for every read of the batch (see include/talc_hip.h)
int talc_batch_fetch_structure(talc_ctx* c, talc_batch* b, int32_t* status, uint32_t* n_regions, double* lambda, uint32_t* in_span,
                               uint64_t* region_offsets, uint32_t* regions, uint32_t* region_hits, uint64_t region_capacity,
                               uint32_t* head_counts) {
  if (int rc = belong(c, b, "bad context/batch")) return rc;
  if (!b->holds.structured) return fail(TALC_ERR_STATE, "talc_batch_structure has not run on this batch (or a correction has run since)");
  HIPCHK(hipSetDevice(c->device));
  uint64_t total = 0;
  for (uint32_t r = 0; r < b->n_reads; ++r) {
    const ReadState& st = b->h_state[r];
    if (status) status[r] = read_status(st);
    if (n_regions) n_regions[r] = st.nRegions;
    if (lambda) lambda[r] = st.lambda;
    if (in_span) in_span[r] = st.inSpan;
    if (region_offsets) region_offsets[r] = total;
    total += st.nRegions;
  }
  if (region_offsets) region_offsets[b->n_reads] = total;
  if ((regions || region_hits) && total) {
    if (region_capacity < total) return fail(TALC_ERR_CAPACITY, "region buffers too small: need %llu regions", (unsigned long long)total);
    // a read's slot: regCap starts, regCap ends, regCap hit words (k_structure)
    std::vector<uint32_t> h(3 * (size_t)b->h_regoff[b->n_reads]);
    HIPCHK(hipMemcpy(h.data(), b->d_regions.get(), h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    uint64_t at = 0;
    for (uint32_t r = 0; r < b->n_reads; ++r) {
      const uint64_t cap = b->h_regoff[r + 1] - b->h_regoff[r];
      const uint32_t* rs = h.data() + 3 * b->h_regoff[r];
      for (uint32_t i = 0; i < b->h_state[r].nRegions && i < cap; ++i, ++at) {
        if (regions) { regions[2 * at] = rs[i]; regions[2 * at + 1] = rs[cap + i]; }
        if (region_hits) region_hits[at] = rs[2 * cap + i];
      }
    }
  }
  if (head_counts && b->n_reads) {   // (k_structure leaves the reads it does not analyse without head counts: 0 here)
    HIPCHK(hipMemcpy(head_counts, b->d_headcov.get(), (size_t)b->n_reads * kHeadCov * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (uint32_t r = 0; r < b->n_reads; ++r)
      if (b->h_state[r].status == TALC_READ_SKIPPED_SHORT || b->h_state[r].status == TALC_READ_NO_SOLID_KMER)
        memset(head_counts + (size_t)r * kHeadCov, 0, kHeadCov * sizeof(uint32_t));
  }
  return TALC_OK;
}

uint64_t talc_batch_corrected_bytes(const talc_batch* b) { return (b && b->holds.has_records()) ? b->h_dense_off[b->n_reads] : 0; }

// the records of a corrected batch into `out` (a host or a device buffer: `kind`; null: offsets and statuses only)
static int corrected_out(talc_ctx* c, talc_batch* b, void* out, uint64_t out_capacity, uint64_t* out_offsets, int32_t* status,
                         hipMemcpyKind kind, const char* what, bool masked = false) {
  if (!b->holds.has_records()) return fail(TALC_ERR_STATE, "talc_batch_correct has not run on this batch");
  HIPCHK(hipSetDevice(c->device));
  const uint64_t total = b->h_dense_off[b->n_reads];
  if (out_offsets) memcpy(out_offsets, b->h_dense_off.data(), (b->n_reads + 1) * 8);
  if (status)
    for (uint32_t r = 0; r < b->n_reads; ++r) status[r] = read_status(b->h_state[r]);
  return copy_out(c, out, out_capacity, masked ? b->d_masked.get() : b->d_dense.get(), total, 1, kind, what, "bytes");
}

int talc_batch_fetch_corrected(talc_ctx* c, talc_batch* b, char* out, uint64_t out_capacity, uint64_t* out_offsets,
                               int32_t* status) {
  if (int rc = belong(c, b, "bad context/batch")) return rc;
  return corrected_out(c, b, out, out_capacity, out_offsets, status, hipMemcpyDeviceToHost, "output buffer");
}

uint64_t talc_batch_num_segments(const talc_batch* b) { return (b && b->holds.has_map()) ? b->h_seg_off[b->n_reads] : 0; }

// what every call that reads the map does after its arguments: the batch has one; then the context's device is made current
static int enter_map(talc_ctx* c, const talc_batch* b) {
  if (!b->holds.has_records()) return fail(TALC_ERR_STATE, "talc_batch_correct has not run on this batch");
  if (!b->holds.has_map()) return fail(TALC_ERR_STATE, "the batch's last correction kept no correction map (talc_ctx_set_map)");
  HIPCHK(hipSetDevice(c->device));
  return TALC_OK;
}

int talc_batch_fetch_map(talc_ctx* c, talc_batch* b, talc_segment* segs, uint64_t capacity, uint64_t* seg_offsets) {
  int rc;
  if ((rc = belong(c, b, "bad context/batch"))) return rc;
  if ((rc = enter_map(c, b))) return rc;
  const uint64_t total = b->h_seg_off[b->n_reads];
  if (seg_offsets) memcpy(seg_offsets, b->h_seg_off.data(), (b->n_reads + 1) * 8);
  return copy_out(c, segs, capacity, b->d_segs.get(), total, sizeof(talc_segment), hipMemcpyDeviceToHost, "segment buffer", "segments");
}

// the second record buffer, on first use: a copy of the dense records, then k_mask_case over the RAW segments (kSpanMaskCase)
static int mask_dense(talc_ctx* c, talc_batch* b) {
  if (b->holds.has_mask()) return TALC_OK;
  hipStream_t s = c->stream;
  const uint64_t total = b->h_dense_off[b->n_reads];
  HIPCHK(b->d_masked.ensure(c->cache, total));
  if (total) HIPCHK(hipMemcpyAsync(b->d_masked.get(), b->d_dense.get(), total, hipMemcpyDeviceToDevice, s));
  int rc = c->span[kSpanMaskCase].around(s, [&] {
    if (b->n_reads)
      hipLaunchKernelGGL(k_mask_case, dim3(b->n_reads), dim3(256), 0, s, b->d_segs.get(), b->d_seg_off.get(), b->d_dense_off.get(), b->d_masked.get(), b->n_reads);
  });
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(s));
  if ((rc = read_spans(c))) return rc;
  b->holds.masked = true;
  return TALC_OK;
}

int talc_batch_fetch_corrected_masked(talc_ctx* c, talc_batch* b, char* out, uint64_t out_capacity, uint64_t* out_offsets,
                                      int32_t* status) {
  int rc;
  if ((rc = belong(c, b, "bad context/batch"))) return rc;
  if ((rc = enter_map(c, b))) return rc;
  if (out && (rc = mask_dense(c, b))) return rc;
  return corrected_out(c, b, out, out_capacity, out_offsets, status, hipMemcpyDeviceToHost, "output buffer", true);
}

// ---- trimmed and split output (docs/trim_split.md): k_piece_count over the map, the reads' offsets on the host (as
// pack_dense and pack_map make theirs), k_piece_pack into buffers sized exactly (kSpanPieceCount, kSpanPiecePack)
int talc_batch_pieces(talc_ctx* c, talc_batch* b, int mode, uint32_t min_len, int soft_mask) {
  if (int rc = belong(c, b, "bad context/batch")) return rc;
  if (mode != TALC_PIECES_TRIM && mode != TALC_PIECES_SPLIT) return fail(TALC_ERR_INVALID, "piece mode %d is neither TALC_PIECES_TRIM nor TALC_PIECES_SPLIT", mode);
  int rc;
  if ((rc = enter_map(c, b))) return rc;
  hipStream_t s = c->stream;
  const uint32_t n = b->n_reads;
  b->holds.pieced = false;
  const bool masked = mode == TALC_PIECES_TRIM && soft_mask;   // (a split piece has no weak byte)
  if (masked && (rc = mask_dense(c, b))) return rc;
  HIPCHK(b->d_piece_count.ensure(c->cache, n));
  rc = c->span[kSpanPieceCount].around(s, [&] {
    if (n) hipLaunchKernelGGL(k_piece_count, dim3(n), dim3(64), 0, s, b->d_segs.get(), b->d_seg_off.get(), n, mode, min_len, b->d_piece_count.get());
  });
  if (rc) return rc;
  std::vector<PieceCount> counts(n);
  if (n) HIPCHK(hipMemcpyAsync(counts.data(), b->d_piece_count.get(), (size_t)n * sizeof(PieceCount), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  b->h_read_piece_off.resize(n + 1); b->h_read_byte_off.resize(n + 1);
  uint64_t np = 0, nb = 0;
  for (uint32_t r = 0; r < n; ++r) {
    b->h_read_piece_off[r] = np; b->h_read_byte_off[r] = nb;
    np += counts[r].n; nb += counts[r].bytes;
  }
  b->h_read_piece_off[n] = np; b->h_read_byte_off[n] = nb;
  // exactly what the pieces take; the buffers of an earlier call are kept when they are large enough
  HIPCHK(b->d_pieces.ensure(c->cache, np)); HIPCHK(b->d_piece_off.ensure(c->cache, np));
  HIPCHK(b->d_piece_bytes.ensure(c->cache, nb));
  HIPCHK(b->d_read_piece_off.ensure(c->cache, n + 1)); HIPCHK(b->d_read_byte_off.ensure(c->cache, n + 1));
  HIPCHK(hipMemcpyAsync(b->d_read_piece_off.get(), b->h_read_piece_off.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(b->d_read_byte_off.get(), b->h_read_byte_off.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
  rc = c->span[kSpanPiecePack].around(s, [&] {
    if (n && np)
      hipLaunchKernelGGL(k_piece_pack, dim3(n), dim3(256), 0, s, b->d_segs.get(), b->d_seg_off.get(), masked ? b->d_masked.get() : b->d_dense.get(),
                         b->d_dense_off.get(), n, mode, min_len, b->d_read_piece_off.get(), b->d_read_byte_off.get(), b->d_pieces.get(),
                         b->d_piece_off.get(), b->d_piece_bytes.get());
  });
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(s));
  if ((rc = read_spans(c))) return rc;
  b->holds.pieced = true;
  return TALC_OK;
}

uint64_t talc_batch_num_pieces(const talc_batch* b) { return (b && b->holds.has_pieces()) ? b->h_read_piece_off[b->n_reads] : 0; }
uint64_t talc_batch_pieces_bytes(const talc_batch* b) { return (b && b->holds.has_pieces()) ? b->h_read_byte_off[b->n_reads] : 0; }

int talc_batch_fetch_pieces(talc_ctx* c, talc_batch* b, char* out, uint64_t out_capacity, uint64_t* piece_offsets, talc_piece* pieces,
                            uint64_t piece_capacity, uint64_t* read_piece_offsets) {
  if (int rc = belong(c, b, "bad context/batch")) return rc;
  if (!b->holds.has_pieces()) return fail(TALC_ERR_STATE, "talc_batch_pieces has not run on this batch since its last correction");
  HIPCHK(hipSetDevice(c->device));
  const uint64_t np = b->h_read_piece_off[b->n_reads], nb = b->h_read_byte_off[b->n_reads];
  if (read_piece_offsets) memcpy(read_piece_offsets, b->h_read_piece_off.data(), (b->n_reads + 1) * 8);
  if (out && out_capacity < nb) return fail(TALC_ERR_CAPACITY, "piece byte buffer too small: need %llu bytes", (unsigned long long)nb);
  if (pieces && piece_capacity < np) return fail(TALC_ERR_CAPACITY, "piece buffer too small: need %llu pieces", (unsigned long long)np);
  hipStream_t s = c->stream;
  if (piece_offsets) {
    if (np) HIPCHK(hipMemcpyAsync(piece_offsets, b->d_piece_off.get(), np * 8, hipMemcpyDeviceToHost, s));
    piece_offsets[np] = nb;
  }
  if (pieces && np) HIPCHK(hipMemcpyAsync(pieces, b->d_pieces.get(), np * sizeof(talc_piece), hipMemcpyDeviceToHost, s));
  if (out && nb) HIPCHK(hipMemcpyAsync(out, b->d_piece_bytes.get(), nb, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return TALC_OK;
}

// ---- the solidity report (docs/solidity.md): k_solidity over the batch's codes (the raw rows) and, once the batch is
// corrected, over the dense records as talc_batch_fetch_corrected returns them (the corrected rows).  One launch: the rows of
// `src` into `rows`, timed by `span`
static int launch_solidity(talc_ctx* c, talc_batch* b, const BatchSource& src, CachedBuf<SolidityRow>& rows, Span& span) {
  HIPCHK(rows.ensure(c->cache, b->n_reads));
  return span.around(c->stream, [&] {
    if (b->n_reads)
      hipLaunchKernelGGL(k_solidity, dim3(b->n_reads), dim3(64), 0, c->stream, c->view, src.bytes, src.d_off, src.states, src.records,
                         c->p.reverse ? 1 : 0, b->rev_flags(), c->p.min_count, b->n_reads, rows.get());
  });
}

int talc_batch_solidity(talc_ctx* c, talc_batch* b) {
  int rc;
  if ((rc = enter(c, b, "bad context/batch"))) return rc;
  if ((rc = prepare_strand(c, b))) return rc;   // (a batch encoded under the other setting is no longer corrected either)
  const bool records = b->holds.has_records();
  b->holds.solidity = b->holds.solidityCorrected = false;
  if (!b->holds.encoded && (rc = launch_encode(c, b))) return rc;
  if ((rc = launch_solidity(c, b, batch_source(b, false), b->d_sol_raw, c->span[kSpanSolidityRaw]))) return rc;
  c->span[kSpanSolidityRecords].skip();   // (a batch without records: the time of their rows is 0, not an earlier batch's)
  if (records && (rc = launch_solidity(c, b, batch_source(b, true), b->d_sol_corr, c->span[kSpanSolidityRecords]))) return rc;
  HIPCHK(hipStreamSynchronize(c->stream));
  if ((rc = read_spans(c))) return rc;
  b->holds.solidity = true; b->holds.solidityCorrected = records;
  return TALC_OK;
}

int talc_batch_fetch_solidity(talc_ctx* c, talc_batch* b, talc_solidity* raw, talc_solidity* corrected) {
  if (int rc = belong(c, b, "bad context/batch")) return rc;
  if (!b->holds.has_solidity(false)) return fail(TALC_ERR_STATE, "talc_batch_solidity has not run on this batch since its last correction");
  if (corrected && !b->holds.has_solidity(true)) return fail(TALC_ERR_STATE, "the batch had not been corrected when talc_batch_solidity ran: it has no corrected rows");
  HIPCHK(hipSetDevice(c->device));
  const size_t bytes = (size_t)b->n_reads * sizeof(talc_solidity);
  if (raw && bytes) HIPCHK(hipMemcpyAsync(raw, b->d_sol_raw.get(), bytes, hipMemcpyDeviceToHost, c->stream));
  if (corrected && bytes) HIPCHK(hipMemcpyAsync(corrected, b->d_sol_corr.get(), bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return TALC_OK;
}

// Read::outputBasicReadStats (Read.cpp:418-433) for every read of a corrected batch
int talc_batch_fetch_read_stats(talc_ctx* c, talc_batch* b, int64_t* stats5) {
  if (int rc = belong(c, b, "bad context/batch/buffer", stats5)) return rc;
  if (!b->holds.has_records()) return fail(TALC_ERR_STATE, "talc_batch_correct has not run on this batch");
  const uint32_t K = c->p.k;
  for (uint32_t r = 0; r < b->n_reads; ++r) {
    const ReadState& st = b->h_state[r];
    const uint64_t L = b->h_offsets[r + 1] - b->h_offsets[r];
    int64_t* o = stats5 + 5ull * r;
    const bool row = L > K;                                  // main.cpp:262: the call sits inside this test
    const bool corrected = st.status == TALC_READ_CORRECTED && !st.overflow;
    o[0] = row ? 1 : 0;
    o[1] = row ? (int64_t)L : 0;
    o[2] = (row && st.status != TALC_READ_NO_SOLID_KMER && st.status != TALC_READ_SKIPPED_SHORT) ? (int64_t)st.inSpan : 0;
    o[3] = (row && st.status != TALC_READ_NO_SOLID_KMER && st.status != TALC_READ_SKIPPED_SHORT) ? (int64_t)st.nRegions : 0;
    o[4] = (row && corrected) ? (int64_t)st.outLen : 0;      // m_correction stays empty unless correct2 ran
  }
  return TALC_OK;
}

int talc_batch_copy_corrected_device(talc_ctx* c, talc_batch* b, void* device_out, uint64_t out_capacity,
                                     uint64_t* out_offsets, int32_t* status) {
  if (int rc = belong(c, b, "bad context/batch/buffer", device_out)) return rc;
  return corrected_out(c, b, device_out, out_capacity, out_offsets, status, hipMemcpyDeviceToDevice, "device buffer");
}

int talc_correct_batch(talc_ctx* c, const char* bases, const uint64_t* offsets, uint32_t n_reads, char* out,
                       uint64_t out_capacity, uint64_t* out_offsets, int32_t* status) {
  talc_batch* b = nullptr;
  int rc = talc_batch_create(c, bases, offsets, n_reads, &b);
  if (rc) return rc;
  rc = talc_batch_correct(c, b);
  int rc2 = (rc >= 0) ? talc_batch_fetch_corrected(c, b, out, out_capacity, out_offsets, status) : rc;
  talc_batch_destroy(b);
  return rc2 ? rc2 : rc;
}

int64_t talc_batch_trace_read(talc_ctx* c, talc_batch* b, uint32_t read_index, char* buf, uint64_t cap) {
  if (int rc = enter(c, b, "bad context/batch/read index", b && read_index < b->n_reads)) return rc;
  // a one-read batch from the resident raw bases
  const uint64_t off = b->h_offsets[read_index], len = b->h_offsets[read_index + 1] - off;
  std::vector<char> raw(std::max<uint64_t>(len, 1));
  if (len) HIPCHK(hipMemcpy(raw.data(), b->d_raw.get() + off, len, hipMemcpyDeviceToHost));
  uint64_t offs[2] = {0, len};
  talc_batch* one = nullptr;
  int rc = talc_batch_create(c, raw.data(), offs, 1, &one);
  if (rc) return rc;
  const std::unique_ptr<talc_batch> tbch(one);
  TraceHost th;
  th.cap = 1u << 18; th.poolCap = 1u << 24;
  HIPCHK(th.d_recs.alloc(th.cap));
  HIPCHK(th.d_nrec.alloc(1)); HIPCHK(th.d_npool.alloc(1));
  HIPCHK(th.d_pool.alloc(th.poolCap));
  HIPCHK(hipMemsetAsync(th.d_nrec.get(), 0, 4, c->stream)); HIPCHK(hipMemsetAsync(th.d_npool.get(), 0, 4, c->stream));   // (the null stream is not ordered with c->stream)
  rc = run_pipeline(c, tbch.get(), &th, 0);
  std::ostringstream os;
  uint32_t nrec = 0, npool = 0;
  HIPCHK(hipMemcpy(&nrec, th.d_nrec.get(), 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(&npool, th.d_npool.get(), 4, hipMemcpyDeviceToHost));
  nrec = std::min(nrec, th.cap); npool = std::min(npool, th.poolCap);
  std::vector<TraceRec> recs(nrec);
  std::vector<uint8_t> pool(std::max<uint32_t>(npool, 1));
  if (nrec) HIPCHK(hipMemcpy(recs.data(), th.d_recs.get(), (size_t)nrec * sizeof(TraceRec), hipMemcpyDeviceToHost));
  if (npool) HIPCHK(hipMemcpy(pool.data(), th.d_pool.get(), npool, hipMemcpyDeviceToHost));
  const int stv = tbch->h_state.empty() ? -1 : read_status(tbch->h_state[0]);
  os << "STATUS " << stv << "\n";
  for (auto& e : recs) {
    char x[64];
    snprintf(x, sizeof x, "%a", e.x);
    os << e.kind << " " << e.a << " " << e.b << " " << e.c << " " << e.d << " " << x << " ";
    for (uint32_t i = 0; i < e.slen && e.soff + i < npool; ++i) os << code_to_ascii(pool[e.soff + i]);
    os << "\n";
  }
  if (tbch->holds.has_records()) {
    const uint64_t total = tbch->h_dense_off[1];
    std::vector<char> o(std::max<uint64_t>(total, 1));
    if (total) HIPCHK(hipMemcpy(o.data(), tbch->d_dense.get(), total, hipMemcpyDeviceToHost));
    os << "OUT " << std::string(o.data(), total) << "\n";
  }
  const std::string str = os.str();
  if (buf && str.size() + 1 <= cap) memcpy(buf, str.c_str(), str.size() + 1);
  return (int64_t)str.size() + 1;
}

// Test hook (not part of the reference surface): run one wave-cooperative DP primitive on the
// device.  a, b: Dna5 codes given as ASCII; see k_test_dp for the modes.  out: 12 ints (mode 3 with p1 set: max(12, p2)).
int talc_test_dp(talc_ctx* c, int mode, const char* a, int la, const char* b, int lb, int p0, int p1, int p2, int p3,
                 int32_t* out) {
  if (!c || !out) return fail(TALC_ERR_INVALID, "null argument");
  const bool tagTable = mode == 3 && p1 != 0;   // one word per record, p2 records
  if (tagTable && (p2 < 0 || (long long)la < 36ll * std::max(p2, 1))) return fail(TALC_ERR_INVALID, "mode 3: %d records need %lld bytes", p2, 36ll * std::max(p2, 1));
  const size_t nout = tagTable ? (size_t)std::max(p2, 12) : 12;
  HIPCHK(hipSetDevice(c->device));
  std::vector<uint8_t> ha(std::max(la, 1)), hb(std::max(lb, 1));
  for (int i = 0; i < la; ++i) ha[i] = (mode == 3) ? (uint8_t)a[i] : ascii_to_code((uint8_t)a[i]);
  for (int i = 0; i < lb; ++i) hb[i] = ascii_to_code((uint8_t)b[i]);
  DevBuf<uint8_t> da, db; DevBuf<int> ddp, dout;
  const uint32_t dpCap = (uint32_t)std::max(std::max(la, lb), 2048) + 16;   // (>= 2048: the phased x-drop keeps its hand-over state there)
  HIPCHK(da.alloc(ha.size())); HIPCHK(db.alloc(hb.size()));
  HIPCHK(ddp.alloc(3ull * dpCap + ROW_MAX_REF + 16)); HIPCHK(dout.alloc(nout + 4));   // (+ mode 7's kept row)
  HIPCHK(hipMemcpy(da.get(), ha.data(), ha.size(), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(db.get(), hb.data(), hb.size(), hipMemcpyHostToDevice));
  HIPCHK(hipMemsetAsync(dout.get(), 0, (nout + 4) * 4, c->stream));   // same stream as the kernel: the null stream is not ordered with it
  hipLaunchKernelGGL(k_test_dp, dim3(1), dim3(64), 0, c->stream, mode, da.get(), la, db.get(), lb, p0, p1, p2, p3, (int)c->p.k, ddp.get(), dpCap, dout.get(),
                     c->p.alpha, c->p.sr_error_rate, (int)c->p.min_count, c->dp.thr, c->dp.thrN);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(out, dout.get(), nout * 4, hipMemcpyDeviceToHost));
  return TALC_OK;
}
