// talc_capi_umi.inc — host side of the UMI read-out (docs/umi.md, talc_kernels_umi.h); included by talc_capi.hip inside its
// extern "C" block, ahead of talc_capi_ends.inc: the clipped and the split batch run the scan.

int talc_ctx_set_umi(talc_ctx* c, const char* pattern, uint32_t max_error_pct, uint32_t window) {
  if (!c) return fail(TALC_ERR_INVALID, "null context");
  UmiParams P;
  char why[256];
  if (!umi_make_setting(pattern, max_error_pct, window, P, why, sizeof why)) return fail(TALC_ERR_INVALID, "%s", why);
  c->umi = P;
  c->umiOn = P.m != 0;
  ++c->umiGen;
  return TALC_OK;
}

// k_read_umi over n_reads reads of `raw` at `off` (device), under the context's setting, into b->d_umi: kSpanUmiScan.
// ends: the rows of k_read_ends over the same reads, or null.  The rows are those of the batch from here on.
static int umi_scan(talc_ctx* c, talc_batch* b, const uint8_t* raw, const uint64_t* off, uint32_t n_reads, const EndRow* ends) {
  b->holds.umi = false;
  HIPCHK(b->d_umi.ensure(c->cache, std::max<uint32_t>(n_reads, 1)));
  const int rc = c->span[kSpanUmiScan].around(c->stream, [&] {
    if (n_reads) hipLaunchKernelGGL(k_read_umi, dim3(n_reads), dim3(64), umi_lds_bytes(c->umi), c->stream, raw, off, n_reads, c->umi, ends, b->d_umi.get());
  });
  if (rc) return rc;
  b->umiGen = c->umiGen;
  b->holds.umi = true;
  return TALC_OK;
}

int talc_batch_umi(talc_ctx* c, talc_batch* b) {
  int rc;
  if ((rc = belong(c, b, "bad context/batch"))) return rc;
  const bool remade = b->holds.clipped || b->holds.split;   // such a batch keeps the rows of the scan that made it
  const bool made = b->holds.umi && (remade || (c->umiOn && b->umiGen == c->umiGen));
  if (!made && !c->umiOn) return fail(TALC_ERR_STATE, "the UMI read-out is off (talc_ctx_set_umi)");
  if (!made && remade) return fail(TALC_ERR_STATE, "a clipped or split batch holds the UMI rows of the scan that made it, and the UMI read-out was off then");
  HIPCHK(hipSetDevice(c->device));
  if (made) c->span[kSpanUmiScan].skip();
  else if ((rc = umi_scan(c, b, b->d_raw.get(), b->d_offsets.get(), b->n_reads, nullptr))) return rc;
  HIPCHK(hipStreamSynchronize(c->stream));
  return read_spans(c);
}

int talc_batch_fetch_umi(talc_ctx* c, talc_batch* b, talc_umi_row* rows) {
  if (int rc = belong(c, b, "bad context/batch")) return rc;
  if (!b->holds.umi) return fail(TALC_ERR_STATE, "no UMI scan has run on this batch (talc_batch_umi, talc_batch_create_clipped, talc_batch_create_split)");
  HIPCHK(hipSetDevice(c->device));
  if (rows && b->n_reads) HIPCHK(hipMemcpyAsync(rows, b->d_umi.get(), (size_t)b->n_reads * sizeof(talc_umi_row), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return read_spans(c);
}

int talc_ctx_get_umi_timing(const talc_ctx* c, float* scan_ms) {
  if (!c) return fail(TALC_ERR_INVALID, "null context");
  if (scan_ms) *scan_ms = c->span[kSpanUmiScan].ms;
  return TALC_OK;
}
