// talc_capi_counter.inc — the k-mer counter (talc_kernels_count.h), the k-mer spectrum and the both-strands table builders
// that are made of a counter.  Included by talc_capi.hip at file scope: types and static helpers first, the entry points in
// the one extern "C" block at the end.
//
// The counter replaces `jellyfish count -m K` + `jellyfish dump -c` (README.md:37-49).  One stream; talc_counter_add copies the
// caller's records into one of two page-locked staging slots (one separator byte after each record), queues the copy to
// the device and the count kernel, and returns.  Growth: counter_make_room.  A both-strands counter (docs/both_strands.md)
// keys everything by the canonical k-mer and expands the kept ones to both strands when the table is built.

// One slot of the double buffer: what a batch stages on the host (the filter's qualities and offsets travel with the text)
// and the event behind the last copy that reads it
struct CounterStage {
  PinnedBuf text, quals, offsets;
  hipEvent_t done = nullptr;
  bool busy = false;   // `done` has been recorded and not yet waited for
};

// TALC_TIMING: the event pairs around every launch of one kind of kernel
struct LaunchTimer {
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pairs;
  ~LaunchTimer() { for (auto& p : pairs) { hipEventDestroy(p.first); hipEventDestroy(p.second); } }
  // launch() on `stream`, between the events of a new pair when `timing` (a complete pair is kept at once; half a pair never)
  template <class Launch>
  int around(bool timing, hipStream_t stream, Launch launch) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (timing && hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess) pairs.push_back({e0, e1});
    else { if (e0) hipEventDestroy(e0); e0 = e1 = nullptr; }
    if (e1) HIPCHK(hipEventRecord(e0, stream));
    launch();
    HIPCHK(hipGetLastError());
    if (e1) HIPCHK(hipEventRecord(e1, stream));
    return TALC_OK;
  }
  double ms() const {
    double sum = 0;
    for (auto& p : pairs) { float ms = 0; if (hipEventElapsedTime(&ms, p.first, p.second) == hipSuccess) sum += ms; }
    return sum;
  }
};

struct talc_counter {
  talc_params p;
  int device = 0;
  Switches sw;
  hipStream_t stream = nullptr;
  DevBuf<CountSlot> tab;
  uint64_t cap() const { return tab.size(); }   // slots, a power of two
  DevBuf<unsigned long long> dStats;   // [0] windows counted, [1] distinct, [2] compaction output counter
  DevBuf<uint32_t> dOverflow;
  CounterStage stage[2];
  int next = 0;
  DevBuf<uint8_t> dText;
  uint64_t distinctKnown = 0;   // exact distinct k-mers at the last synchronisation
  uint64_t winsSince = 0;       // windows (upper bound) queued since then
  uint64_t winsTotal = 0;       // windows (upper bound) over every batch: counts cannot pass it
  bool spent = false;
  bool bothStrands = false;     // keys are canon(x); the table gets y and rc(y) (talc_counter_set_both_strands)
  bool started = false;         // something has been added: the mode is fixed
  bool countsAdded = false;     // talc_counter_add_counts was used: a count no longer stays below the windows counted
  // the short-read filter (talc_counter_set_filter, docs/sr_filter.md): nothing of it exists while it is off
  bool filterOn = false;
  SrFilter filt{0, 0, 0};
  DevBuf<SrAdapters> dAdapters;            // empty: no adapters
  DevBuf<unsigned long long> dFiltStats;   // {records, records clipped, bytes clipped, bytes below the floor}
  DevBuf<uint8_t> dQual;
  DevBuf<uint64_t> dOffs;
  // TALC_TIMING
  LaunchTimer countTimer, maskTimer;   // around every k_count_batch, every k_sr_mask
  uint64_t nBatches = 0, nBytes = 0, nGrows = 0;
  double packS = 0, growS = 0;
  Span histo;   // the last k_count_histo
  ~talc_counter() {
    (void)hipSetDevice(device);
    for (auto& s : stage) if (s.done) hipEventDestroy(s.done);
    if (stream) hipStreamDestroy(stream);
  }
};

// What an entry point that takes a counter checks: the counter and the `rest` of its arguments are there, and the table has
// not been built from it
static int counter_usable(const talc_counter* c, bool rest = true) {
  if (!c || !rest) return fail(TALC_ERR_INVALID, "null argument");
  if (c->spent) return fail(TALC_ERR_STATE, "the counter's table has been built");
  return TALC_OK;
}

// the exact counters from the device (synchronises the stream); fails when a count has passed 2^32 - 1
static int counter_sync(talc_counter* c, unsigned long long st[2]) {
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  uint32_t ovf = 0;
  HIPCHK(hipMemcpy(st, c->dStats.get(), 2 * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(&ovf, c->dOverflow.get(), 4, hipMemcpyDeviceToHost));
  if (ovf) return fail(TALC_ERR_INVALID, "a k-mer count passed 2^32 - 1 (counts are 32-bit); the counter is unusable");
  c->distinctKnown = st[1];
  c->winsSince = 0;
  return TALC_OK;
}

// slots with count >= thr: how many (outK == nullptr) or the arrays themselves (device pointers of outCap entries);
// expand: both strands of every kept (canonical) k-mer, *n = 2 * kept - palindromes
static int counter_compact(talc_counter* c, uint32_t thr, uint64_t* outK, uint32_t* outC, uint64_t outCap, uint64_t* n, bool expand = false) {
  HIPCHK(hipMemsetAsync(c->dStats.get() + 2, 0, 8, c->stream));
  const dim3 grid((unsigned)((c->cap() + 4 * 64 * kCompactRows - 1) / (4 * 64 * kCompactRows)));
  auto* const kernel = expand ? k_count_compact<true> : k_count_compact<false>;
  if (c->cap()) hipLaunchKernelGGL(kernel, grid, dim3(256), 0, c->stream, c->tab.get(), c->cap(), thr, c->p.k, outK, outC, outCap, c->dStats.get() + 2);
  HIPCHK(hipGetLastError());
  unsigned long long v = 0;
  HIPCHK(hipMemcpyAsync(&v, c->dStats.get() + 2, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  *n = v;
  return TALC_OK;
}

// the n entries that a counting counter_compact(c, thr, ..., expand) has just found, as device arrays of exactly that size
// (`nomem`: the caller's wording, n its one argument)
static int counter_kept_arrays(talc_counter* c, uint32_t thr, bool expand, uint64_t n, const char* nomem, DevBuf<uint64_t>& dK, DevBuf<uint32_t>& dC) {
  if (dK.alloc(std::max<uint64_t>(n, 1)) != hipSuccess || dC.alloc(std::max<uint64_t>(n, 1)) != hipSuccess) { return fail(TALC_ERR_NOMEM, nomem, (unsigned long long)n); }
  uint64_t got = 0;
  if (int rc = counter_compact(c, thr, dK.get(), dC.get(), n, &got, expand)) return rc;
  if (got != n) return fail(TALC_ERR_STATE, "the counter changed between two compactions (%llu, %llu)", (unsigned long long)n, (unsigned long long)got);
  return TALC_OK;
}

// The growth rule, stated here only: `from` slots doubled until `need` keys fill no more than this share of them
// (tools/spectrum_bench.py replays it)
static uint64_t counter_capacity_for(uint64_t need, uint64_t from) {
  while ((double)need > 0.7 * (double)from) from *= 2;
  return from;
}

// a larger hash that holds `need` distinct k-mers; the old slots are rehashed on the device
static int counter_grow(talc_counter* c, uint64_t need) {
  Stopwatch watch;
  const uint64_t nc = counter_capacity_for(need, c->cap());
  DevBuf<CountSlot> nt;
  if (nt.alloc(nc) != hipSuccess) {
    return fail(TALC_ERR_NOMEM, "the k-mer counter cannot grow to %llu slots (%llu bytes) after %llu distinct k-mers",
                (unsigned long long)nc, (unsigned long long)(nc * sizeof(CountSlot)), (unsigned long long)c->distinctKnown);
  }
  hipLaunchKernelGGL(k_count_init, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, c->stream, nt.get(), nc);
  hipLaunchKernelGGL(k_count_rehash, dim3((unsigned)((c->cap() + 255) / 256)), dim3(256), 0, c->stream, c->tab.get(), c->cap(), nt.get(), nc - 1);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  c->tab = std::move(nt);   // (frees the old slots)
  ++c->nGrows;
  c->growS += watch.seconds();
  return TALC_OK;
}

// Room for up to `bound` new keys before they are queued: the host's bound first, the exact number (a synchronisation) only
// when the bound says they might not fit, and a larger hash only when the exact number says so too
static int counter_make_room(talc_counter* c, uint64_t bound) {
  auto fits = [c](uint64_t keys) { return counter_capacity_for(keys, c->cap()) == c->cap(); };
  if (fits(c->distinctKnown + c->winsSince + bound)) return TALC_OK;
  unsigned long long st[2];
  if (int rc = counter_sync(c, st)) return rc;
  return fits(c->distinctKnown + bound) ? TALC_OK : counter_grow(c, c->distinctKnown + bound);
}

// a step of talc_counter_create: what does not fit is TALC_ERR_NOMEM, every other failure a device error
static int counter_rc(hipError_t e, const char* what) {
  if (e == hipSuccess) return TALC_OK;
  return fail(e == hipErrorOutOfMemory ? TALC_ERR_NOMEM : TALC_ERR_DEVICE, "k-mer counter: %s: %s", what, hipGetErrorString(e));
}

// a batch's records: the offsets must not decrease; *wins = the windows of K bytes the raw lengths hold (an upper bound of
// what is counted).  The filter keeps a record's length in 32 bits.
static int counter_check_batch(const talc_counter* c, const uint64_t* offsets, uint32_t n_reads, bool filtered, uint64_t* wins) {
  const uint32_t K = c->p.k;
  uint64_t w = 0;
  for (uint32_t r = 0; r < n_reads; ++r) {
    if (offsets[r + 1] < offsets[r]) return fail(TALC_ERR_INVALID, "offsets must not decrease (read %u)", r);
    const uint64_t L = offsets[r + 1] - offsets[r];
    if (filtered && L >= (1ull << 32)) return fail(TALC_ERR_INVALID, "read %u has %llu bytes: the short-read filter takes records below 2^32 bytes", r, (unsigned long long)L);
    w += L >= K ? L - K + 1 : 0;
  }
  *wins = w;
  return TALC_OK;
}

// A page-locked staging buffer / a device buffer of the counter's batches as it is when it holds `need` units, else the old
// one goes and max(need, floor) are asked for
static int counter_pinned(PinnedBuf& buf, uint64_t need, uint64_t floor) {
  if (buf.size() >= need) return TALC_OK;
  const uint64_t want = std::max<uint64_t>(need, floor);
  if (buf.alloc(want) != hipSuccess) { return fail(TALC_ERR_NOMEM, "cannot allocate %llu bytes of pinned staging memory", (unsigned long long)want); }
  return TALC_OK;
}
template <class T>
static int counter_devbuf(talc_counter* c, DevBuf<T>& buf, uint64_t need, uint64_t floor) {
  if (buf.size() >= need) return TALC_OK;
  HIPCHK(hipStreamSynchronize(c->stream));   // (the previous kernel may still read the old buffer)
  const uint64_t want = std::max<uint64_t>(need, floor);
  if (buf.alloc(want) != hipSuccess) {
    return fail(TALC_ERR_NOMEM, "cannot allocate %llu bytes for a batch of the k-mer counter (%llu distinct k-mers so far)",
                (unsigned long long)(want * sizeof(T)), (unsigned long long)c->distinctKnown);
  }
  return TALC_OK;
}

// a batch's records (of `src`: bases or qualities) into a staging buffer of nbytes, one separator after each
static int counter_pack(PinnedBuf& into, const char* src, const uint64_t* offsets, uint32_t n_reads, uint64_t nbytes) {
  if (int rc = counter_pinned(into, nbytes, 1u << 20)) return rc;
  char* dst = into.get();
  const uint64_t o0 = offsets[0];
#pragma omp parallel for schedule(static) if (n_reads > 100000)
  for (long r = 0; r < (long)n_reads; ++r) {
    const uint64_t at = offsets[r] - o0 + (uint64_t)r;
    memcpy(dst + at, src + offsets[r], offsets[r + 1] - offsets[r]);
    dst[at + offsets[r + 1] - offsets[r]] = '\n';
  }
  return TALC_OK;
}

// The filter's part of a batch whose text sits in slot s: the qualities (the text's layout; nullptr: none) and the
// offsets staged beside it, their copies and k_sr_mask queued behind the text's copy.  Every byte the kernel reads of the
// quality and offset buffers is written here, for this batch.  dClip: the test hook's clip positions (device), which leaves
// the filter's counters alone; else nullptr.
static int counter_queue_mask(talc_counter* c, CounterStage& s, const char* quals, const uint64_t* offsets, uint32_t n_reads, uint64_t nbytes, uint32_t* dClip) {
  Stopwatch packing;
  const uint64_t noffs = (uint64_t)n_reads + 1;
  if (int rc = counter_pinned(s.offsets, noffs * 8, 1u << 16)) return rc;
  memcpy(s.offsets.get(), offsets, noffs * 8);
  if (quals)
    if (int rc = counter_pack(s.quals, quals, offsets, n_reads, nbytes)) return rc;
  c->packS += packing.seconds();
  if (int rc = counter_devbuf(c, c->dOffs, noffs, 1u << 13)) return rc;
  HIPCHK(hipMemcpyAsync(c->dOffs.get(), s.offsets.get(), noffs * 8, hipMemcpyHostToDevice, c->stream));
  if (quals) {
    if (int rc = counter_devbuf(c, c->dQual, nbytes, 1u << 20)) return rc;
    HIPCHK(hipMemcpyAsync(c->dQual.get(), s.quals.get(), nbytes, hipMemcpyHostToDevice, c->stream));
  }
  const uint32_t nblk = std::min<uint32_t>((n_reads + kSrWaves - 1) / kSrWaves, kSrMaxBlocks);
  return c->maskTimer.around(c->sw.timing, c->stream, [&] {
    hipLaunchKernelGGL(k_sr_mask, dim3(nblk), dim3(kSrThreads), 0, c->stream, c->dText.get(), quals ? c->dQual.get() : (const uint8_t*)nullptr,
                       c->dOffs.get(), n_reads, c->dAdapters.get(), c->filt, dClip ? (unsigned long long*)nullptr : c->dFiltStats.get(), dClip);
  });
}

// A batch staged: its bytes into the next staging slot, once the copies that last read the slot are done, their copy to the
// device text queued, and the filter's part when `mask`.  The tail: the slot's event behind every copy that reads its
// buffers, the slot busy, and only then the mask step's status (a slot whose mask step failed is busy all the same).
static int counter_stage_batch(talc_counter* c, const char* bases, const char* quals, const uint64_t* offsets, uint32_t n_reads, uint64_t nbytes,
                               bool mask, uint32_t* dClip) {
  Stopwatch packing;
  CounterStage& s = c->stage[c->next];
  c->next ^= 1;
  if (s.busy) { HIPCHK(hipEventSynchronize(s.done)); s.busy = false; }
  if (int rc = counter_pack(s.text, bases, offsets, n_reads, nbytes)) return rc;
  c->packS += packing.seconds();
  if (int rc = counter_devbuf(c, c->dText, nbytes, 1u << 20)) return rc;
  HIPCHK(hipMemcpyAsync(c->dText.get(), s.text.get(), nbytes, hipMemcpyHostToDevice, c->stream));
  const int rcMask = mask ? counter_queue_mask(c, s, quals, offsets, n_reads, nbytes, dClip) : TALC_OK;
  HIPCHK(hipEventRecord(s.done, c->stream));
  s.busy = true;
  return rcMask;
}

static int counter_add_records(talc_counter* c, const char* bases, const char* quals, const uint64_t* offsets, uint32_t n_reads) {
  if (int rc = counter_usable(c, !n_reads || (bases && offsets))) return rc;
  if (!n_reads) return TALC_OK;
  c->started = true;
  const uint32_t K = c->p.k;
  uint64_t wins = 0;   // (of the raw lengths: masking only removes windows, so the growth bound below stays one)
  if (int rc = counter_check_batch(c, offsets, n_reads, c->filterOn, &wins)) return rc;
  const uint64_t nbytes = offsets[n_reads] - offsets[0] + n_reads;   // one separator after each record
  HIPCHK(hipSetDevice(c->device));
  if (int rc = counter_make_room(c, wins)) return rc;
  if (int rc = counter_stage_batch(c, bases, quals, offsets, n_reads, nbytes, c->filterOn, nullptr)) return rc;
  c->winsTotal += wins;
  const bool checked = c->countsAdded || c->winsTotal >= 0xFFFFFFFFull;   // below that no count can reach 2^32
  const uint64_t nblk = (nbytes + kCountTile - 1) / kCountTile;
  if (nblk >= (1ull << 31)) return fail(TALC_ERR_INVALID, "batch of %llu bytes is too large", (unsigned long long)nbytes);
  auto* const kernel = c->bothStrands ? (checked ? k_count_batch<true, true> : k_count_batch<false, true>)
                                      : (checked ? k_count_batch<true, false> : k_count_batch<false, false>);
  const int rc = c->countTimer.around(c->sw.timing, c->stream, [&] {
    hipLaunchKernelGGL(kernel, dim3((unsigned)nblk), dim3(kCountThreads), 0, c->stream, c->dText.get(), nbytes, K, c->tab.get(), c->cap() - 1,
                       c->dStats.get(), c->dOverflow.get());
  });
  if (rc) return rc;
  c->winsSince += wins;
  ++c->nBatches;
  c->nBytes += nbytes;
  return TALC_OK;
}

// "ACGT,acgt" -> base codes; false with *why set for what talc_counter_set_filter refuses
static bool parse_adapters(const char* text, SrAdapters& out, const char** why) {
  memset(&out, 0, sizeof out);
  if (!text || !*text) return true;
  const char* p = text;
  while (true) {
    const char* e = strchr(p, ',');
    const size_t m = e ? (size_t)(e - p) : strlen(p);
    if (out.n == (uint32_t)kSrMaxAdapters) { *why = "more than 4 adapters"; return false; }
    if (m == 0) { *why = "an empty adapter"; return false; }
    if (m > (size_t)kSrMaxAdapterLen) { *why = "an adapter of more than 64 letters"; return false; }
    for (size_t i = 0; i < m; ++i) {
      const uint8_t code = ascii_to_code((uint8_t)p[i]);
      if (code >= 4) { *why = "an adapter with a letter that is not one of ACGTacgt"; return false; }
      out.code[out.n][i] = code;
    }
    out.len[out.n++] = (uint32_t)m;
    if (!e) return true;
    p = e + 1;
  }
}

// n counted k-mers as device arrays into the hash (k_count_add_counts); the arrays may be freed on return.  Growth as for
// a batch of n windows: every entry may be a new key.
static int counter_add_counts_device(talc_counter* c, const uint64_t* dK, const uint32_t* dC, uint64_t n) {
  if (!n) return TALC_OK;
  c->started = c->countsAdded = true;
  HIPCHK(hipSetDevice(c->device));
  if (int rc = counter_make_room(c, n)) return rc;
  const uint64_t nblk = (n + kCountThreads - 1) / kCountThreads;
  if (nblk >= (1ull << 31)) return fail(TALC_ERR_INVALID, "%llu counted k-mers are too many for one call", (unsigned long long)n);
  auto* const kernel = c->bothStrands ? k_count_add_counts<true> : k_count_add_counts<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)nblk), dim3(kCountThreads), 0, c->stream, dK, dC, n, c->p.k, c->tab.get(), c->cap() - 1, c->dStats.get(),
                     c->dOverflow.get());
  HIPCHK(hipGetLastError());
  c->winsSince += n;
  HIPCHK(hipStreamSynchronize(c->stream));   // (the caller's arrays are read until here)
  return TALC_OK;
}

// The counter's table.  lines: the build-from-a-file callers' {lines read, -, malformed lines} (nullptr: the distinct
// k-mers are the "lines read"); finish false: no colouring, no de-colouring (the from_arrays builders).
static int counter_build_table(talc_counter* c, const char* junction_path, talc_table** out, int64_t stats[3], const DumpStats* lines, bool finish) {
  Stopwatch watch;
  unsigned long long st[2];
  int rc = counter_sync(c, st);
  if (rc) return rc;
  const double tWait = watch.lap();
  uint64_t kept = 0;   // entries for the builder: both strands of every kept k-mer of a both-strands counter
  const bool expand = c->bothStrands;
  if ((rc = counter_compact(c, c->p.min_count, nullptr, nullptr, 0, &kept, expand))) return rc;
  if (kept >= 0xFFFFFFFEull)
    return fail(TALC_ERR_INVALID, expand ? "%llu k-mers (both strands of those that reach MIN_COUNT) are too many: the device builder takes fewer than 2^32-2"
                                         : "%llu k-mers reach MIN_COUNT: the device builder takes fewer than 2^32-2", (unsigned long long)kept);
  DumpStats ds;
  ds.nread = lines ? lines->nread : (int64_t)st[1];
  ds.nkept = (int64_t)kept;
  ds.nbad = lines ? lines->nbad : 0;
  double tCompact = watch.lap();
  // The kept k-mers as arrays, the builder over them, the colouring: everything that allocates.  spendFirst: the hash and
  // the batches' buffers go once the kept k-mers are copied out, before the builder allocates its buckets, and the
  // counter is spent from there on; else they go when the table is there.  On failure nothing is left of the build.
  auto build = [&](bool spendFirst, talc_table** made) -> int {
    auto spend = [&] {
      c->tab.reset();
      c->dText.reset(); c->dQual.reset(); c->dOffs.reset();
      c->spent = true;
    };
    watch.lap();
    DevBuf<uint64_t> dK; DevBuf<uint32_t> dC;
    if (int brc = counter_kept_arrays(c, c->p.min_count, expand, kept, "cannot allocate the %llu kept k-mers", dK, dC)) return brc;
    if (spendFirst) spend();
    tCompact += watch.lap();
    TablePtr t;
    if (int brc = build_table_from_device_arrays(std::move(dK), std::move(dC), kept, kept, &c->p, c->device, t, 0.0, 0.0, c->sw)) return brc;
    if (finish) {
      if (int brc = table_finish(std::move(t), junction_path, &c->p, ds, made, stats)) return brc;
    } else {
      if (stats) { stats[0] = ds.nread; stats[1] = ds.nkept; stats[2] = ds.nbad; }
      *made = t.release();
    }
    if (!spendFirst) spend();
    return TALC_OK;
  };
  // Beside the hash where the device has the room for it (docs/out_of_memory.md): a -3 there leaves the counter as it
  // was, at the price of the work done so far, and the build is made once more the frugal way.  Where the free memory
  // does not hold the kept arrays, the buckets and the builder's bids beside the hash, the frugal way is taken at once,
  // as it always was; a -3 from there on leaves the counter spent.
  size_t freeB = 0, totalB = 0;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemGetInfo(&freeB, &totalB));
  const uint64_t besideBytes = kept * (8 + 4 + 2 * 4) + 2 * HostTable::capacity_for(kept, (uint64_t)totalB, c->sw.tableSlotsX10) * sizeof(Bucket);
  talc_table* made = nullptr;
  rc = (uint64_t)freeB >= besideBytes ? build(false, &made) : TALC_ERR_NOMEM;
  if (rc == TALC_ERR_NOMEM) rc = build(true, &made);
  if (rc) return rc;
  if (c->sw.timing) {
    const double kms = c->countTimer.ms();
    char mask[96] = "";   // (a filtered counter only: the line of an unfiltered one is as it was)
    if (c->filterOn) {
      const double mms = c->maskTimer.ms();
      snprintf(mask, sizeof mask, ", mask kernels %.3f ms (%.3f ms per batch)", mms, c->nBatches ? mms / (double)c->nBatches : 0.0);
    }
    fprintf(stderr, "[talc-lib] k-mer counter: %llu batches, %.0f MB, %llu windows, %llu distinct, %llu kept; pack %.3f s, count kernels %.3f ms "
                    "(%.3f ms per batch), %llu grows %.3f s, last batch wait %.3f s, compaction %.3f s%s\n",
            (unsigned long long)c->nBatches, (double)c->nBytes / 1e6, st[0], st[1], (unsigned long long)kept, c->packS, kms,
            c->nBatches ? kms / (double)c->nBatches : 0.0, (unsigned long long)c->nGrows, c->growS,
            tWait, tCompact, mask);
  }
  *out = made;
  return TALC_OK;
}

// ---- the k-mer spectrum (talc_kernels_spectrum.h, docs/kmer_spectrum.md).  Replaces `jellyfish histo`.  One pass of
// k_count_histo over the counter's hash, or of k_table_histo over a table's RIGHT buckets; the threshold rule itself is
// talc_pure.h's.
static int spectrum_high(uint32_t* high) {
  if (*high == 0) *high = kSpectrumDefaultHigh;
  if (*high < 2 || *high > kSpectrumMaxHigh)
    return fail(TALC_ERR_INVALID, "high=%u: the spectrum takes 2 .. %u (0: %u)", *high, kSpectrumMaxHigh, kSpectrumDefaultHigh);
  return TALC_OK;
}

// the CU count of a device, asked once per device and process (the properties query is slow beside a pass over a small hash)
static int spectrum_cu_count(int device, int* cus) {
  static std::mutex lock;
  static std::map<int, int> known;
  std::lock_guard<std::mutex> g(lock);
  auto it = known.find(device);
  if (it == known.end()) {
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    it = known.emplace(device, std::max(prop.multiProcessorCount, 1)).first;
  }
  *cus = it->second;
  return TALC_OK;
}

// One spectrum pass on `stream` of the current device over n slots, of which a workgroup takes groupSlots per trip: the
// output words zeroed, the kernel launched by launch(grid, lds bytes, out) inside `span` (when given, and read), the bins
// and totals copied to hist / stats (either may be NULL).  The grid: a workgroup per trip, at most the fixed number per CU.
template <class Launch>
static int run_spectrum(int device, hipStream_t stream, uint64_t n, uint64_t groupSlots, uint32_t high, uint64_t* hist, talc_spectrum_stats* stats,
                        Span* span, Launch launch) {
  const uint32_t bins = high + 2;
  DevBuf<unsigned long long> dOut;
  HIPCHK(dOut.alloc(bins + SPECTRUM_TOTALS));
  HIPCHK(hipMemsetAsync(dOut.get(), 0, (uint64_t)(bins + SPECTRUM_TOTALS) * 8, stream));
  int cus = 1;
  if (int rc = spectrum_cu_count(device, &cus)) return rc;
  const uint64_t grid = std::min<uint64_t>((n + groupSlots - 1) / groupSlots, (uint64_t)cus * kSpectrumGridPerCu);
  // (no slots, a table of capacity 0: nothing is launched, the zeroed words are the answer and the span times nothing)
  auto pass = [&] { if (grid) launch(dim3((unsigned)grid), (size_t)spectrum_lds_words(bins) * 4, dOut.get()); };
  if (span) { if (int rc = span->around(stream, pass)) return rc; }
  else { pass(); HIPCHK(hipGetLastError()); }
  std::vector<unsigned long long> h(bins + SPECTRUM_TOTALS);
  HIPCHK(hipMemcpyAsync(h.data(), dOut.get(), h.size() * 8, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  if (span) if (int rc = span->read()) return rc;
  if (hist) for (uint32_t b = 0; b < bins; ++b) hist[b] = h[b];
  if (stats) {
    stats->distinct = h[bins + SPECTRUM_DISTINCT]; stats->unique = h[bins + SPECTRUM_UNIQUE];
    stats->total = h[bins + SPECTRUM_TOTAL]; stats->max_count = h[bins + SPECTRUM_MAX];
  }
  return TALC_OK;
}

// the counter of the both-strands table builders below, for as long as one of them runs
struct CounterOwner { talc_counter* c = nullptr; ~CounterOwner() { talc_counter_destroy(c); } };

extern "C" {

int talc_counter_create(const talc_params* p, int device, uint64_t expected_distinct, talc_counter** out) {
  int rc = check_params(p);
  if (rc) return rc;
  if (!out) return fail(TALC_ERR_INVALID, "null argument");
  const int ndev = talc_device_count();
  if (device < 0 || device >= ndev)
    return fail(TALC_ERR_DEVICE, "no GPU %d for the k-mer counter (%d visible); there is no host counter", device, ndev);
  auto c = std::make_unique<talc_counter>();
  c->p = *p; c->device = device; c->sw = read_switches();
  const uint64_t cap = counter_capacity_for(expected_distinct, 1u << 16);   // 1 MiB without a hint
  if ((rc = counter_rc(hipSetDevice(device), "hipSetDevice"))) return rc;
  if ((rc = counter_rc(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking), "hipStreamCreate"))) return rc;
  for (auto& s : c->stage)
    if ((rc = counter_rc(hipEventCreateWithFlags(&s.done, hipEventDisableTiming), "hipEventCreate"))) return rc;
  if ((rc = counter_rc(c->tab.alloc(cap), "hash allocation"))) return rc;
  if ((rc = counter_rc(c->dStats.alloc(4), "counter allocation"))) return rc;
  if ((rc = counter_rc(c->dOverflow.alloc(1), "counter allocation"))) return rc;
  if ((rc = counter_rc(hipMemsetAsync(c->dStats.get(), 0, 4 * 8, c->stream), "hipMemset"))) return rc;
  if ((rc = counter_rc(hipMemsetAsync(c->dOverflow.get(), 0, 4, c->stream), "hipMemset"))) return rc;
  hipLaunchKernelGGL(k_count_init, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, c->stream, c->tab.get(), cap);
  if ((rc = counter_rc(hipGetLastError(), "k_count_init"))) return rc;
  *out = c.release();
  return TALC_OK;
}

int talc_counter_add(talc_counter* c, const char* bases, const uint64_t* offsets, uint32_t n_reads) {
  return counter_add_records(c, bases, nullptr, offsets, n_reads);
}

int talc_counter_add_fastq(talc_counter* c, const char* bases, const char* quals, const uint64_t* offsets, uint32_t n_reads) {
  return counter_add_records(c, bases, quals, offsets, n_reads);
}

int talc_counter_set_filter(talc_counter* c, uint32_t min_qual, const char* adapters, uint32_t min_overlap, uint32_t max_error_pct) {
  if (!c) return fail(TALC_ERR_INVALID, "null argument");
  if (min_qual > 93) return fail(TALC_ERR_INVALID, "min_qual=%u: the quality floor is 0 (off) or 1..93 (Phred+33)", min_qual);
  if (max_error_pct > 30) return fail(TALC_ERR_INVALID, "max_error_pct=%u: at most 30", max_error_pct);
  if (min_overlap > (uint32_t)kSrMaxAdapterLen) return fail(TALC_ERR_INVALID, "min_overlap=%u: at most 64", min_overlap);
  SrAdapters packed;
  const char* why = nullptr;
  if (!parse_adapters(adapters, packed, &why)) return fail(TALC_ERR_INVALID, "short-read filter: %s", why);
  if (!min_overlap) min_overlap = 5;
  for (uint32_t a = 0; a < packed.n; ++a)
    if (min_overlap > packed.len[a])
      return fail(TALC_ERR_INVALID, "min_overlap=%u is above the shortest adapter's length %u", min_overlap, packed.len[a]);
  if (int rc = counter_usable(c)) return rc;
  if (c->started) return fail(TALC_ERR_STATE, "the counter already holds k-mers: the filter is chosen before the first add");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));   // (a test-hook pass of an earlier setting may still run)
  c->filterOn = false;
  c->dAdapters.reset();
  c->dFiltStats.reset();
  c->filt = SrFilter{min_qual, min_overlap, max_error_pct};
  if (!packed.n && !min_qual) return TALC_OK;   // off: talc_counter_add does what it does without a filter
  if (c->dFiltStats.alloc(4) != hipSuccess) { return fail(TALC_ERR_NOMEM, "cannot allocate the filter's counters"); }
  HIPCHK(hipMemsetAsync(c->dFiltStats.get(), 0, 4 * 8, c->stream));
  if (packed.n) {
    if (c->dAdapters.alloc(1) != hipSuccess) { return fail(TALC_ERR_NOMEM, "cannot allocate the filter's adapters"); }
    HIPCHK(hipMemcpy(c->dAdapters.get(), &packed, sizeof packed, hipMemcpyHostToDevice));
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  c->filterOn = true;
  return TALC_OK;
}

int talc_counter_filter_stats(talc_counter* c, uint64_t stats[4]) {
  if (int rc = counter_usable(c, stats)) return rc;
  stats[0] = stats[1] = stats[2] = stats[3] = 0;
  if (!c->filterOn) return TALC_OK;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(stats, c->dFiltStats.get(), 4 * 8, hipMemcpyDeviceToHost));
  return TALC_OK;
}

// Test hook: the filter alone on one batch, through the counter's own staging and device buffers.  Counts nothing and
// leaves the filter's counters alone.
int talc_test_counter_mask(talc_counter* c, const char* bases, const char* quals, const uint64_t* offsets, uint32_t n_reads, char* masked_out,
                           uint32_t* clip_out) {
  if (int rc = counter_usable(c, !n_reads || (bases && offsets && clip_out))) return rc;
  if (!n_reads) return TALC_OK;
  uint64_t wins = 0;
  if (int rc = counter_check_batch(c, offsets, n_reads, true, &wins)) return rc;
  const uint64_t nbytes = offsets[n_reads] - offsets[0] + n_reads;
  if (nbytes > n_reads && !masked_out) return fail(TALC_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(c->device));
  DevBuf<uint32_t> dClip;
  if (dClip.alloc(n_reads) != hipSuccess) { return fail(TALC_ERR_NOMEM, "cannot allocate %u clip positions", n_reads); }
  if (int rc = counter_stage_batch(c, bases, quals, offsets, n_reads, nbytes, true, dClip.get())) return rc;
  std::vector<char> text(nbytes);
  HIPCHK(hipMemcpyAsync(text.data(), c->dText.get(), nbytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(clip_out, dClip.get(), (uint64_t)n_reads * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (uint32_t r = 0; r < n_reads; ++r)
    memcpy(masked_out + (offsets[r] - offsets[0]), text.data() + (offsets[r] - offsets[0] + r), offsets[r + 1] - offsets[r]);
  return TALC_OK;
}

int talc_counter_set_both_strands(talc_counter* c, int on) {
  if (int rc = counter_usable(c)) return rc;
  if (c->started) return fail(TALC_ERR_STATE, "the counter already holds k-mers: the strand mode is chosen before the first add");
  c->bothStrands = on != 0;
  return TALC_OK;
}

int talc_counter_add_counts(talc_counter* c, const uint64_t* kmers, const uint32_t* counts, uint64_t n) {
  if (int rc = counter_usable(c, !n || (kmers && counts))) return rc;
  if (!n) return TALC_OK;
  const uint64_t wide = ~((1ULL << (2 * c->p.k)) - 1);
  uint64_t nWide = 0;
#pragma omp parallel for reduction(+ : nWide) if (n > 1000000)
  for (long i = 0; i < (long)n; ++i) nWide += (kmers[i] & wide) ? 1 : 0;
  if (nWide) return fail(TALC_ERR_INVALID, "%llu of the counted k-mers are wider than 2 K = %u bits", (unsigned long long)nWide, 2 * c->p.k);
  HIPCHK(hipSetDevice(c->device));
  DevBuf<uint64_t> dK; DevBuf<uint32_t> dC;
  if (dK.alloc(n) != hipSuccess || dC.alloc(n) != hipSuccess) { return fail(TALC_ERR_NOMEM, "cannot allocate %llu counted k-mers on the device", (unsigned long long)n); }
  HIPCHK(hipMemcpy(dK.get(), kmers, n * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dC.get(), counts, n * 4, hipMemcpyHostToDevice));
  return counter_add_counts_device(c, dK.get(), dC.get(), n);
}

int talc_counter_stats(talc_counter* c, uint64_t stats[3]) {
  int rc = counter_usable(c, stats);
  if (rc) return rc;
  unsigned long long st[2];
  if ((rc = counter_sync(c, st))) return rc;
  uint64_t kept = 0;
  if ((rc = counter_compact(c, c->p.min_count, nullptr, nullptr, 0, &kept))) return rc;
  stats[0] = st[0]; stats[1] = st[1]; stats[2] = kept;
  return TALC_OK;
}

int talc_counter_fetch(talc_counter* c, uint32_t min_count, uint64_t* kmers, uint32_t* counts, uint64_t capacity, uint64_t* n_out) {
  int rc = counter_usable(c, !kmers || counts);
  if (rc) return rc;
  unsigned long long st[2];
  if ((rc = counter_sync(c, st))) return rc;
  uint64_t n = 0;
  if ((rc = counter_compact(c, min_count, nullptr, nullptr, 0, &n))) return rc;
  if (n_out) *n_out = n;
  if (!kmers) return TALC_OK;
  if (capacity < n) return fail(TALC_ERR_CAPACITY, "%llu k-mers need the output arrays' room, %llu given", (unsigned long long)n,
                                (unsigned long long)capacity);
  DevBuf<uint64_t> dK; DevBuf<uint32_t> dC;
  if ((rc = counter_kept_arrays(c, min_count, false, n, "cannot allocate %llu k-mers for the fetch", dK, dC))) return rc;
  HIPCHK(hipMemcpy(kmers, dK.get(), n * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(counts, dC.get(), n * 4, hipMemcpyDeviceToHost));
  return TALC_OK;
}

int talc_counter_build_table(talc_counter* c, const char* junction_path, talc_table** out, int64_t stats[3]) {
  if (int rc = counter_usable(c, out)) return rc;
  return counter_build_table(c, junction_path, out, stats, nullptr, true);
}

int talc_counter_histo(talc_counter* c, uint32_t high, uint64_t* hist, talc_spectrum_stats* stats) {
  int rc = spectrum_high(&high);
  if (rc) return rc;
  if ((rc = counter_usable(c))) return rc;
  unsigned long long st[2];
  if ((rc = counter_sync(c, st))) return rc;
  const CountSlot* tab = c->tab.get();
  const uint64_t cap = c->cap();
  hipStream_t stream = c->stream;
  return run_spectrum(c->device, stream, cap, spectrum_group_slots<CounterSlots>(), high, hist, stats, &c->histo, [=](dim3 grid, size_t lds, unsigned long long* out) {
    hipLaunchKernelGGL(k_count_histo, grid, dim3(kSpectrumThreads), lds, stream, tab, cap, high, out);
  });
}

int talc_counter_get_histo_timing(const talc_counter* c, float* histo_ms) {
  if (!c || !histo_ms) return fail(TALC_ERR_INVALID, "null argument");
  *histo_ms = c->histo.ms;
  return TALC_OK;
}

int talc_table_histo(talc_table* t, int device, uint32_t high, uint64_t* hist, talc_spectrum_stats* stats) {
  int rc = spectrum_high(&high);
  if (rc) return rc;
  if (!t) return fail(TALC_ERR_INVALID, "null argument");
  auto* at = t->image(device);
  if (!at) return fail(TALC_ERR_STATE, "the table has no image on device %d: build it there or upload it", device);
  HIPCHK(hipSetDevice(device));
  const Bucket* right = at->second.right.get();
  const uint64_t cap = t->h.capacity;
  return run_spectrum(device, nullptr, cap, spectrum_group_slots<TableSlots>(), high, hist, stats, nullptr, [=](dim3 grid, size_t lds, unsigned long long* out) {
    hipLaunchKernelGGL(k_table_histo, grid, dim3(kSpectrumThreads), lds, nullptr, right, cap, high, out);
  });
}

int talc_spectrum_threshold(const uint64_t* hist, uint32_t high, uint32_t limit, uint32_t fallback, uint32_t* chosen, uint32_t* valley_out) {
  if (!hist || !chosen) return fail(TALC_ERR_INVALID, "null argument");
  if (high < 2) return fail(TALC_ERR_INVALID, "high=%u: a spectrum has at least the counts 1 and 2", high);
  if (fallback == 0) return fail(TALC_ERR_INVALID, "fallback=0: MIN_COUNT is at least 1");
  const uint32_t valley = spectrum_valley(hist, high, limit);
  *chosen = spectrum_min_count(valley, fallback);
  if (valley_out) *valley_out = valley;
  return TALC_OK;
}

int talc_counter_set_min_count(talc_counter* c, uint32_t min_count) {
  if (!c) return fail(TALC_ERR_INVALID, "null argument");
  if (min_count < 1) return fail(TALC_ERR_INVALID, "min_count=0: MIN_COUNT is at least 1");
  if (int rc = counter_usable(c)) return rc;
  c->p.min_count = min_count;
  return TALC_OK;
}

// ---- both strands from counted k-mers (docs/both_strands.md).  A both-strands counter fed by add_counts, then its table:
// the fold is a sum per canonical k-mer on the device, MIN_COUNT applies to the sum.  There is no host fold.
int talc_table_from_arrays_device_both_strands(const uint64_t* kmers, const uint32_t* counts, uint64_t n, const talc_params* p, int device,
                                               talc_table** out) {
  if (!out || (n && (!kmers || !counts))) return fail(TALC_ERR_INVALID, "null argument");
  CounterOwner own;
  int rc;
  if ((rc = talc_counter_create(p, device, 0, &own.c))) return rc;
  own.c->bothStrands = true;
  if ((rc = talc_counter_add_counts(own.c, kmers, counts, n))) return rc;
  return counter_build_table(own.c, nullptr, out, nullptr, nullptr, false);
}

int talc_table_build_device_both_strands(const char* dump_path, const char* junction_path, const talc_params* p, int device, talc_table** out,
                                         int64_t stats[3]) {
  if (!dump_path || !out) return fail(TALC_ERR_INVALID, "null argument");
  CounterOwner own;
  int rc;
  if ((rc = talc_counter_create(p, device, 0, &own.c))) return rc;
  own.c->bothStrands = true;
  const Switches sw = own.c->sw;
  Stopwatch watch;
  DumpStats ds;
  struct stat sb;
  if (stat(dump_path, &sb) != 0) return fail(TALC_ERR_IO, "cannot open %s", dump_path);
  const uint64_t size = (uint64_t)sb.st_size;
  bool onDevice = false;
  if (size >= (8u << 20) && !sw.hostParse) {   // the text parsed on the device, as table_from_text_on_device takes it
    char head[64] = {0};
    FILE* f = fopen(dump_path, "rb");
    if (!f) return fail(TALC_ERR_IO, "cannot open %s", dump_path);
    const size_t got = fread(head, 1, sizeof head, f);
    fclose(f);
    DevBuf<uint8_t> dText;
    ParsedText parsed;
    int T = 0;
    if (!jfLooksLike(head, got) && text_to_device(dump_path, size, kDumpChunkBytes, kDumpReaders, device, dText, &T) == 0 &&
        parse_device_text(dText.get(), size, p->k, p->min_count, parsed) == 0 && parsed.stats.flags == 0) {
      dText.reset();
      if ((rc = counter_add_counts_device(own.c, parsed.kmers.get(), parsed.counts.get(), parsed.nlines))) return rc;
      ds.nread = (int64_t)parsed.nlines;
      onDevice = true;
    }
  }
  if (!onDevice) {   // the host's tokeniser or the .jf reader, every line whatever its count
    std::vector<uint64_t> kmers;
    std::vector<uint32_t> counts;
    std::string why;
    if (!parseDumpFile(dump_path, p->k, p->min_count, false, kmers, &counts, nullptr, ds, &why))
      return why.empty() ? fail(TALC_ERR_IO, "cannot open %s", dump_path) : fail(TALC_ERR_INVALID, "%s", why.c_str());
    if ((rc = talc_counter_add_counts(own.c, kmers.data(), counts.data(), kmers.size()))) return rc;
  }
  if (sw.timing)
    fprintf(stderr, "[talc-lib] both strands: %llu lines of %s folded on the device in %.3f s (text parsed on the %s)\n", (unsigned long long)ds.nread,
            dump_path, watch.seconds(), onDevice ? "device" : "host");
  return counter_build_table(own.c, junction_path, out, stats, &ds, true);
}

void talc_counter_destroy(talc_counter* c) {
  if (!c) return;
  if (hipSetDevice(c->device) == hipSuccess && c->stream) hipStreamSynchronize(c->stream);   // (its kernels may still run)
  delete c;
  (void)hipGetLastError();
}

}  // extern "C"
