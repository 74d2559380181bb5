// talc_capi_demux.inc — host side of the barcode demultiplexing (docs/demux.md, talc_kernels_demux.h); included by
// talc_capi.hip inside its extern "C" block, ahead of talc_capi_ends.inc: the clipped and the split batch run the scan.

int talc_ctx_set_demux(talc_ctx* c, const char* barcodes, uint32_t max_error_pct, uint32_t min_margin, uint32_t window, int both_ends) {
  if (!c) return fail(TALC_ERR_INVALID, "null context");
  DemuxParams P;
  std::vector<uint64_t> peq((size_t)kDemuxMaxBarcodes * 4, 0);
  char why[256];
  if (!demux_make_setting(barcodes, max_error_pct, min_margin, window, both_ends, P, peq.data(), why, sizeof why)) return fail(TALC_ERR_INVALID, "%s", why);
  if (P.nBarcodes) {   // the masks go to the context's table: every call that scans has waited for the stream, none reads it now
    HIPCHK(hipSetDevice(c->device));
    DevBuf<uint64_t> fresh;
    if (!c->d_demux_peq) HIPCHK(fresh.alloc(peq.size()));
    uint64_t* const dst = c->d_demux_peq ? c->d_demux_peq.get() : fresh.get();
    HIPCHK(hipMemcpyAsync(dst, peq.data(), peq.size() * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (fresh) c->d_demux_peq = std::move(fresh);
  }
  c->demux = P;
  c->demuxOn = P.nBarcodes != 0;
  ++c->demuxGen;
  return TALC_OK;
}

// k_read_demux over n_reads reads of `raw` at `off` (device), under the context's setting, into b->d_demux: kSpanDemuxScan.
// The rows are those of the batch from here on.
static int demux_scan(talc_ctx* c, talc_batch* b, const uint8_t* raw, const uint64_t* off, uint32_t n_reads) {
  b->holds.demuxed = false;
  HIPCHK(b->d_demux.ensure(c->cache, n_reads));
  const int rc = c->span[kSpanDemuxScan].around(c->stream, [&] {
    if (n_reads)
      hipLaunchKernelGGL(k_read_demux, dim3(n_reads), dim3(64), demux_lds_bytes(c->demux), c->stream, raw, off, n_reads, c->d_demux_peq.get(), c->demux, b->d_demux.get());
  });
  if (rc) return rc;
  b->n_demux = n_reads;
  b->demuxGen = c->demuxGen;
  b->holds.demuxed = true;
  return TALC_OK;
}

int talc_batch_demux(talc_ctx* c, talc_batch* b) {
  int rc;
  if ((rc = belong(c, b, "bad context/batch"))) return rc;
  const bool remade = b->holds.clipped || b->holds.split;   // such a batch no longer holds the reads as they came
  const bool made = b->holds.demuxed && (remade || (c->demuxOn && b->demuxGen == c->demuxGen));
  if (!made && !c->demuxOn) return fail(TALC_ERR_STATE, "the barcode scan is off (talc_ctx_set_demux)");
  if (!made && remade)
    return fail(TALC_ERR_STATE, "a clipped or split batch no longer holds the reads as they came, and the barcode scan was off when it was made");
  HIPCHK(hipSetDevice(c->device));
  if (made) c->span[kSpanDemuxScan].skip();
  else if ((rc = demux_scan(c, b, b->d_raw.get(), b->d_offsets.get(), b->n_reads))) return rc;
  HIPCHK(hipStreamSynchronize(c->stream));
  return read_spans(c);
}

int talc_batch_fetch_demux(talc_ctx* c, talc_batch* b, talc_demux_row* rows) {
  if (int rc = belong(c, b, "bad context/batch")) return rc;
  if (!b->holds.demuxed) return fail(TALC_ERR_STATE, "no barcode scan has run on this batch (talc_batch_demux, talc_batch_create_clipped, talc_batch_create_split)");
  HIPCHK(hipSetDevice(c->device));
  if (rows && b->n_demux) HIPCHK(hipMemcpyAsync(rows, b->d_demux.get(), (size_t)b->n_demux * sizeof(talc_demux_row), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return read_spans(c);
}

int talc_ctx_get_demux_timing(const talc_ctx* c, float* scan_ms) {
  if (!c) return fail(TALC_ERR_INVALID, "null context");
  if (scan_ms) *scan_ms = c->span[kSpanDemuxScan].ms;
  return TALC_OK;
}
