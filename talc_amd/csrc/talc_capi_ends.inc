// talc_capi_ends.inc — host side of the long-read end clean-up (docs/read_ends.md, talc_kernels_ends.h); included by
// talc_capi.hip inside its extern "C" block, after talc_capi_support.inc.

int talc_ctx_set_ends(talc_ctx* c, const char* adapters, uint32_t max_error_pct, uint32_t poly_min, uint32_t window) {
  if (!c) return fail(TALC_ERR_INVALID, "null context");
  if (max_error_pct > 30) return fail(TALC_ERR_INVALID, "max_error_pct=%u: at most 30", max_error_pct);
  if (!window) window = 512;
  if (window < 32 || window > ENDS_MAX_WINDOW) return fail(TALC_ERR_INVALID, "window=%u: 32 .. %u (0: 512)", window, (uint32_t)ENDS_MAX_WINDOW);
  if (poly_min && (poly_min < 8 || poly_min > window)) return fail(TALC_ERR_INVALID, "poly_min=%u: 0 (off) or 8 .. window (%u)", poly_min, window);
  EndsParams P;
  uint8_t codes[ENDS_MAX_ADAPTERS][64];
  memset(&P, 0, sizeof P);
  memset(codes, 0, sizeof codes);
  P.polyMin = poly_min; P.window = window;
  for (PatternList it(adapters); it.next(acgt_set);) {
    if (P.nAdapters == ENDS_MAX_ADAPTERS) return fail(TALC_ERR_INVALID, "adapters: more than %u", (uint32_t)ENDS_MAX_ADAPTERS);
    if (it.fault == PATTERN_LENGTH) return fail(TALC_ERR_INVALID, "adapters: adapter %u has %llu letters: 12 .. 64", P.nAdapters + 1, (unsigned long long)it.m);
    if (it.fault) return fail(TALC_ERR_INVALID, "adapters: adapter %u has a letter that is not one of ACGTacgt", P.nAdapters + 1);
    pattern_masks(it.p, it.m, acgt_set, false, false, P.peq[P.nAdapters]);
    for (size_t i = 0; i < it.m; ++i) codes[P.nAdapters][i] = ascii_to_code((uint8_t)it.p[i]);   // (the chimera scan's patterns are made from them)
    P.m[P.nAdapters] = (uint32_t)it.m;
    P.k[P.nAdapters] = (uint32_t)(max_error_pct * it.m / 100);
    ++P.nAdapters;
  }
  c->ends = P;
  memcpy(c->endsCodes, codes, sizeof codes);
  c->endsOn = P.nAdapters || poly_min;
  ++c->endsGen;
  return TALC_OK;
}

// k_read_ends over n_reads reads of `raw` at `off` (device), under the context's setting, into `rows`: kSpanEndsScan
static int launch_ends(talc_ctx* c, const uint8_t* raw, const uint64_t* off, uint32_t n_reads, EndRow* rows) {
  return c->span[kSpanEndsScan].around(c->stream, [&] {
    if (n_reads) hipLaunchKernelGGL(k_read_ends, dim3(n_reads), dim3(64), 0, c->stream, raw, off, n_reads, c->ends, rows);
  });
}

int talc_batch_ends(talc_ctx* c, talc_batch* b) {
  int rc;
  if ((rc = belong(c, b, "bad context/batch"))) return rc;
  const bool made = b->holds.ended && (b->holds.clipped || (c->endsOn && b->endsGen == c->endsGen));
  if (!made && !c->endsOn) return fail(TALC_ERR_STATE, "the end clean-up is off (talc_ctx_set_ends)");
  if (!made && b->holds.clipped)   // (docs/umi.md: clipped by the UMI alone; its bytes are no longer the reads as they came)
    return fail(TALC_ERR_STATE, "a clipped batch holds the end rows of the scan that made it, and the end clean-up was off then");
  HIPCHK(hipSetDevice(c->device));
  if (!made) {
    b->holds.ended = false;
    HIPCHK(b->d_ends.ensure(c->cache, b->n_reads));
    if ((rc = launch_ends(c, b->d_raw.get(), b->d_offsets.get(), b->n_reads, b->d_ends.get()))) return rc;
    b->endsGen = c->endsGen;
    b->holds.ended = true;
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  return read_spans(c);
}

int talc_batch_fetch_ends(talc_ctx* c, talc_batch* b, talc_end_row* rows) {
  if (int rc = belong(c, b, "bad context/batch")) return rc;
  if (!b->holds.ended) return fail(TALC_ERR_STATE, "no end scan has run on this batch (talc_batch_ends, talc_batch_create_clipped)");
  HIPCHK(hipSetDevice(c->device));
  if (rows && b->n_reads) HIPCHK(hipMemcpyAsync(rows, b->d_ends.get(), (size_t)b->n_reads * sizeof(talc_end_row), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return read_spans(c);
}

// What talc_batch_create_clipped and talc_batch_create_split open with: the argument checks (`refusal`: why the context's
// setting cannot make such a batch, or null), an empty batch, the raw bytes and the offsets up once into staging buffers of
// the context's cache (they go back to it when the batch stands), and the barcode scan on them when it is on
// (docs/demux.md: the batch will not hold the reads as they came, its rows are those of the source reads).
struct StagedReads {
  std::unique_ptr<talc_batch> b;
  CachedBuf<uint8_t> text;
  CachedBuf<uint64_t> off;
};
static int stage_reads(talc_ctx* c, const char* bases, const uint64_t* offsets, uint32_t n_reads, const char* (*refusal)(const talc_ctx*), StagedReads& st) {
  if (!c || !offsets || (!bases && n_reads && offsets[n_reads] > 0)) return fail(TALC_ERR_INVALID, "null argument");
  if (const char* const why = refusal(c)) return fail(TALC_ERR_STATE, "%s", why);
  if (offsets[0] != 0) return fail(TALC_ERR_INVALID, "offsets[0] must be 0");
  for (uint32_t r = 0; r < n_reads; ++r) {
    if (offsets[r + 1] < offsets[r]) return fail(TALC_ERR_INVALID, "offsets must be non-decreasing");
    if (offsets[r + 1] - offsets[r] > 0x7fffff00ull) return fail(TALC_ERR_INVALID, "read %u too long", r);
  }
  HIPCHK(hipSetDevice(c->device));
  const uint64_t nb = offsets[n_reads];
  st.b = std::make_unique<talc_batch>();
  st.b->ctx = c;
  HIPCHK(st.text.alloc(c->cache, std::max<uint64_t>(nb, 1)));
  HIPCHK(st.off.alloc(c->cache, (uint64_t)n_reads + 1));
  if (nb) HIPCHK(hipMemcpyAsync(st.text.get(), bases, nb, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(st.off.get(), offsets, ((size_t)n_reads + 1) * 8, hipMemcpyHostToDevice, c->stream));
  return c->demuxOn ? demux_scan(c, st.b.get(), st.text.get(), st.off.get(), n_reads) : TALC_OK;
}

// The rows `d_rows` of the `scan` scan over the staged reads come to the host, which lays the batch out from their kept
// lengths (batch_build, as talc_batch_create); k_gather then fills the batch's text from the staging buffer, device to device.
extern "C++" template <class Row>   // (this file is included inside extern "C")
static int clipped_build(talc_ctx* c, talc_batch* bp, const CachedBuf<uint8_t>& stage, const CachedBuf<uint64_t>& stageOff, const uint64_t* offsets,
                         uint32_t n_reads, const Row* d_rows, const char* scan) {
  std::vector<Row> rows(n_reads);
  if (n_reads) HIPCHK(hipMemcpyAsync(rows.data(), d_rows, (size_t)n_reads * sizeof(Row), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  std::vector<uint64_t> kept((size_t)n_reads + 1, 0);
  for (uint32_t r = 0; r < n_reads; ++r) {
    const uint64_t L = offsets[r + 1] - offsets[r];
    const GatherInterval iv = gather_interval(rows[r], r);
    if ((uint64_t)iv.start + iv.len > L)
      return fail(TALC_ERR_DEVICE, "the %s scan left read %u an interval beyond its %llu bytes", scan, r, (unsigned long long)L);
    kept[r + 1] = kept[r] + iv.len;
  }
  return batch_build(c, bp, kept.data(), n_reads, [&](hipStream_t s) {
    return c->span[kSpanEndsGather].around(s, [&] {
      if (n_reads)
        hipLaunchKernelGGL(k_gather<Row>, dim3(n_reads), dim3(256), 0, s, stage.get(), stageOff.get(), n_reads, d_rows, n_reads, bp->d_raw.get(),
                           bp->d_offsets.get());
    });
  });
}

// The clipped batch `bp` from n_reads reads that stand on the device already (`stage` at `stageOff`, ordered on the
// context's stream; `offsets` are the same offsets on the host): the scans, then clipped_build.  What
// talc_batch_create_clipped does behind its upload, and talc_batch_create_split behind its gather.
// Without the UMI read-out the rows are k_read_ends'.  With it (docs/umi.md) k_read_ends runs when the end clean-up is on,
// and its rows stay what it wrote; k_read_umi runs on the same text, and its rows hold the combined intervals.
static int clipped_from_staged(talc_ctx* c, talc_batch* bp, const CachedBuf<uint8_t>& stage, const CachedBuf<uint64_t>& stageOff, const uint64_t* offsets,
                               uint32_t n_reads) {
  const bool umi = c->umiOn, ends = c->endsOn || !umi;
  int rc;
  if (ends) {
    HIPCHK(bp->d_ends.alloc(c->cache, std::max<uint32_t>(n_reads, 1)));
    if ((rc = launch_ends(c, stage.get(), stageOff.get(), n_reads, bp->d_ends.get()))) return rc;
  }
  if (umi && (rc = umi_scan(c, bp, stage.get(), stageOff.get(), n_reads, ends ? bp->d_ends.get() : nullptr))) return rc;
  rc = umi ? clipped_build(c, bp, stage, stageOff, offsets, n_reads, bp->d_umi.get(), "UMI")
           : clipped_build(c, bp, stage, stageOff, offsets, n_reads, bp->d_ends.get(), "end");
  if (rc) return rc;
  if ((rc = read_spans(c))) return rc;
  bp->endsGen = c->endsGen;
  bp->holds.ended = ends;
  bp->holds.clipped = true;
  return TALC_OK;
}

static const char* clipped_refusal(const talc_ctx* c) {   // (docs/umi.md: the UMI alone clips too)
  return c->endsOn || c->umiOn ? nullptr : "the end clean-up is off (talc_ctx_set_ends)";
}
int talc_batch_create_clipped(talc_ctx* c, const char* bases, const uint64_t* offsets, uint32_t n_reads, talc_batch** out) {
  if (!out) return fail(TALC_ERR_INVALID, "null argument");
  StagedReads st;
  if (int rc = stage_reads(c, bases, offsets, n_reads, clipped_refusal, st)) return rc;
  if (int rc = clipped_from_staged(c, st.b.get(), st.text, st.off, offsets, n_reads)) return rc;
  *out = st.b.release();
  return TALC_OK;
}

int talc_ctx_get_ends_timing(const talc_ctx* c, float* scan_ms, float* gather_ms) {
  if (!c) return fail(TALC_ERR_INVALID, "null context");
  if (scan_ms) *scan_ms = c->span[kSpanEndsScan].ms;
  if (gather_ms) *gather_ms = c->span[kSpanEndsGather].ms;
  return TALC_OK;
}
