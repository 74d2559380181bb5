// talc_capi_chimera.inc — host side of the chimera split (docs/chimeras.md, talc_kernels_chimera.h, talc_chimera_plan.h);
// included by talc_capi.hip inside its extern "C" block, after talc_capi_ends.inc.

int talc_ctx_set_chimera(talc_ctx* c, int on, uint32_t max_error_pct, uint32_t min_piece) {
  if (!c) return fail(TALC_ERR_INVALID, "null context");
  if (max_error_pct > 30) return fail(TALC_ERR_INVALID, "max_error_pct=%u: at most 30", max_error_pct);
  if (min_piece > 0x7fffff00u) return fail(TALC_ERR_INVALID, "min_piece=%u: at most %u", min_piece, 0x7fffff00u);
  c->chimeraOn = on != 0;
  c->chimeraPct = max_error_pct;
  c->chimeraMinPiece = min_piece;
  ++c->chimeraGen;
  return TALC_OK;
}

// the scan's setting from the adapters of the ends setting
static ChimeraParams chimera_params_of(const talc_ctx* c) {
  ChimeraParams P;
  memset(&P, 0, sizeof P);
  for (uint32_t a = 0; a < c->ends.nAdapters && a < ENDS_MAX_ADAPTERS; ++a)
    chimera_params_add(P, c->endsCodes[a], c->ends.m[a], code_set, c->chimeraPct);
  return P;
}

static bool chimera_ready(const talc_ctx* c) { return c->chimeraOn && c->ends.nAdapters > 0; }

// k_read_chimera over n_reads reads of `raw` at `off` (device; `offsets` the same on the host), under the context's
// setting: the hits in the contract's order into `hits`, each read's first into `readHitOff`.  The hit buffer starts at
// 1024 + 2 n_reads; the kernel counts every hit, and when they did not fit the buffer grows to the count and the scan runs
// once more.  Returns with the stream idle.  kSpanChimeraScan is the last launch.
static int run_chimera_scan(talc_ctx* c, const uint8_t* raw, const uint64_t* off, const uint64_t* offsets, uint32_t n_reads, std::vector<ChimeraHit>& hits,
                            std::vector<uint64_t>& readHitOff) {
  const ChimeraParams P = chimera_params_of(c);
  CachedBuf<ChimeraHit> d_hits;
  CachedBuf<uint32_t> d_count;
  HIPCHK(d_count.alloc(c->cache, 1));
  uint64_t capacity = 1024ull + 2ull * n_reads;
  uint32_t count = 0;
  for (int pass = 0; pass < 2; ++pass) {
    HIPCHK(d_hits.alloc(c->cache, capacity));
    HIPCHK(hipMemsetAsync(d_count.get(), 0, sizeof(uint32_t), c->stream));
    const int rc = c->span[kSpanChimeraScan].around(c->stream, [&] {
      if (n_reads)
        hipLaunchKernelGGL(k_read_chimera, dim3(n_reads), dim3(64), 0, c->stream, raw, off, n_reads, P, d_hits.get(), (uint32_t)capacity, d_count.get());
    });
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(&count, d_count.get(), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (count <= capacity) break;
    if (pass == 1) return fail(TALC_ERR_DEVICE, "the chimera scan counted %u hits after %llu", count, (unsigned long long)capacity);
    capacity = count;
  }
  hits.resize(count);
  if (count) HIPCHK(hipMemcpy(hits.data(), d_hits.get(), (size_t)count * sizeof(ChimeraHit), hipMemcpyDeviceToHost));
  for (const ChimeraHit& h : hits) {
    const uint64_t L = h.read < n_reads ? offsets[h.read + 1] - offsets[h.read] : 0;
    if (h.read >= n_reads || h.start >= h.end || h.end > L)
      return fail(TALC_ERR_DEVICE, "the chimera scan left a hit [%u, %u) of read %u beyond its %llu bytes", h.start, h.end, h.read, (unsigned long long)L);
  }
  chimera_sort(hits);
  chimera_read_offsets(hits, n_reads, readHitOff);
  return read_spans(c);
}

int talc_batch_chimera(talc_ctx* c, talc_batch* b) {
  int rc;
  if ((rc = belong(c, b, "bad context/batch"))) return rc;
  const bool made = b->holds.chimera && (b->holds.split || (chimera_ready(c) && b->chimeraGen == c->chimeraGen && b->chimeraEndsGen == c->endsGen));
  if (made) return TALC_OK;
  if (b->holds.clipped) return fail(TALC_ERR_STATE, "a clipped batch no longer holds the reads as they came: scan a plain batch, or make a split one (talc_batch_create_split)");
  if (!c->chimeraOn) return fail(TALC_ERR_STATE, "the chimera scan is off (talc_ctx_set_chimera)");
  if (!c->ends.nAdapters) return fail(TALC_ERR_STATE, "the chimera scan has no adapter to look for (talc_ctx_set_ends)");
  HIPCHK(hipSetDevice(c->device));
  b->holds.chimera = false;
  if ((rc = run_chimera_scan(c, b->d_raw.get(), b->d_offsets.get(), b->h_offsets.data(), b->n_reads, b->h_hits, b->h_read_hit_off))) return rc;
  b->chimeraGen = c->chimeraGen;
  b->chimeraEndsGen = c->endsGen;
  b->holds.chimera = true;
  return TALC_OK;
}

uint64_t talc_batch_num_chimera_hits(const talc_batch* b) { return b && b->holds.chimera ? b->h_hits.size() : 0; }

int talc_batch_fetch_chimera(talc_ctx* c, talc_batch* b, talc_chimera_hit* hits, uint64_t capacity, uint64_t* read_hit_offsets) {
  if (int rc = belong(c, b, "bad context/batch")) return rc;
  if (!b->holds.chimera) return fail(TALC_ERR_STATE, "no chimera scan has run on this batch (talc_batch_chimera, talc_batch_create_split)");
  if (b->h_hits.size() > capacity || (!hits && !b->h_hits.empty()))
    return fail(TALC_ERR_CAPACITY, "hits: room for %llu, %llu needed", (unsigned long long)(hits ? capacity : 0), (unsigned long long)b->h_hits.size());
  if (!b->h_hits.empty()) memcpy(hits, b->h_hits.data(), b->h_hits.size() * sizeof(ChimeraHit));
  if (read_hit_offsets) memcpy(read_hit_offsets, b->h_read_hit_off.data(), b->h_read_hit_off.size() * sizeof(uint64_t));
  return TALC_OK;
}

static const char* split_refusal(const talc_ctx* c) {   // (clip needs the end clean-up on; a setting with an adapter is on)
  if (!c->chimeraOn) return "the chimera scan is off (talc_ctx_set_chimera)";
  return c->ends.nAdapters ? nullptr : "the chimera scan has no adapter to look for (talc_ctx_set_ends)";
}
// The bytes go up once into a staging buffer (stage_reads); the scan runs on them; the host computes the pieces
// (split_pieces); k_gather copies every piece to its place: into the new batch's text (batch_build), or, with clip, into a
// second staging text from which the batch is made as a clipped one (clipped_from_staged).
int talc_batch_create_split(talc_ctx* c, const char* bases, const uint64_t* offsets, uint32_t n_reads, int clip, talc_batch** out) {
  if (!out) return fail(TALC_ERR_INVALID, "null argument");
  StagedReads st;
  int rc;
  if ((rc = stage_reads(c, bases, offsets, n_reads, split_refusal, st))) return rc;
  talc_batch* const bp = st.b.get();
  if ((rc = run_chimera_scan(c, st.text.get(), st.off.get(), offsets, n_reads, bp->h_hits, bp->h_read_hit_off))) return rc;
  split_pieces(bp->h_hits.data(), bp->h_read_hit_off.data(), offsets, n_reads, c->chimeraMinPiece, bp->h_split, bp->h_read_split_off, nullptr, nullptr);
  if (bp->h_split.size() > 0xffffff00ull) return fail(TALC_ERR_INVALID, "%llu pieces: more than a batch holds", (unsigned long long)bp->h_split.size());
  const uint32_t n_pieces = (uint32_t)bp->h_split.size();
  std::vector<uint64_t> pieceOff((size_t)n_pieces + 1, 0);
  for (uint32_t p = 0; p < n_pieces; ++p) pieceOff[p + 1] = pieceOff[p] + bp->h_split[p].len;
  CachedBuf<SplitPiece> d_split;
  if ((rc = up(c, d_split, bp->h_split, c->stream))) return rc;
  auto gather = [&](hipStream_t s, uint8_t* dst, const uint64_t* dstOff) {
    return c->span[kSpanChimeraGather].around(s, [&] {
      if (n_pieces)
        hipLaunchKernelGGL(k_gather<SplitPiece>, dim3(n_pieces), dim3(256), 0, s, st.text.get(), st.off.get(), n_reads, d_split.get(), n_pieces, dst, dstOff);
    });
  };
  if (!clip) {
    if ((rc = batch_build(c, bp, pieceOff.data(), n_pieces, [&](hipStream_t s) { return gather(s, bp->d_raw.get(), bp->d_offsets.get()); }))) return rc;
    if (c->umiOn) {   // (docs/umi.md: a row per piece, nothing cut)
      if ((rc = umi_scan(c, bp, bp->d_raw.get(), bp->d_offsets.get(), n_pieces, nullptr))) return rc;
      HIPCHK(hipStreamSynchronize(c->stream));
    }
  } else {
    CachedBuf<uint8_t> dense;
    CachedBuf<uint64_t> denseOff;
    HIPCHK(dense.alloc(c->cache, std::max<uint64_t>(pieceOff[n_pieces], 1)));
    if ((rc = up(c, denseOff, pieceOff, c->stream))) return rc;
    if ((rc = gather(c->stream, dense.get(), denseOff.get()))) return rc;
    if ((rc = clipped_from_staged(c, bp, dense, denseOff, pieceOff.data(), n_pieces))) return rc;
  }
  if ((rc = read_spans(c))) return rc;
  bp->chimeraGen = c->chimeraGen;
  bp->chimeraEndsGen = c->endsGen;
  bp->holds.chimera = bp->holds.split = true;
  *out = st.b.release();
  return TALC_OK;
}

uint64_t talc_batch_num_split_pieces(const talc_batch* b) { return b && b->holds.split ? b->h_split.size() : 0; }

int talc_batch_fetch_split(talc_ctx* c, talc_batch* b, talc_split_piece* pieces, uint64_t* read_piece_offsets) {
  if (int rc = belong(c, b, "bad context/batch")) return rc;
  if (!b->holds.split) return fail(TALC_ERR_STATE, "this batch was not made from pieces (talc_batch_create_split)");
  if (pieces && !b->h_split.empty()) memcpy(pieces, b->h_split.data(), b->h_split.size() * sizeof(SplitPiece));
  if (read_piece_offsets) memcpy(read_piece_offsets, b->h_read_split_off.data(), b->h_read_split_off.size() * sizeof(uint64_t));
  return TALC_OK;
}

int talc_ctx_get_chimera_timing(const talc_ctx* c, float* scan_ms, float* gather_ms) {
  if (!c) return fail(TALC_ERR_INVALID, "null context");
  if (scan_ms) *scan_ms = c->span[kSpanChimeraScan].ms;
  if (gather_ms) *gather_ms = c->span[kSpanChimeraGather].ms;
  return TALC_OK;
}
