// talc_capi_support.inc — host side of the per-base support (docs/base_support.md, talc_kernels_support.h); included by
// talc_capi.hip inside its extern "C" block, after talc_capi_edits.inc.

// k_base_support over the batch's codes (RAW) or its dense records (RECORD), timed by kSpanSupport.  The byte buffer is
// the batch's, sized exactly; the buffer of an earlier call is kept when it is large enough.
int talc_batch_support(talc_ctx* c, talc_batch* b, const talc_support_params* p) {
  if (int rc = belong(c, b, "bad context/batch/params", p)) return rc;
  if (p->source != TALC_SUPPORT_RAW && p->source != TALC_SUPPORT_RECORD)
    return fail(TALC_ERR_INVALID, "support source %u is neither TALC_SUPPORT_RAW nor TALC_SUPPORT_RECORD", p->source);
  if (p->phred > 1) return fail(TALC_ERR_INVALID, "phred must be 0 or 1, not %u", p->phred);
  if (p->phred && (p->qmin > p->qmax || p->qmax > 93))
    return fail(TALC_ERR_INVALID, "quality range %u .. %u: 0 <= qmin <= qmax <= 93 is required", p->qmin, p->qmax);
  HIPCHK(hipSetDevice(c->device));
  int rc;
  if ((rc = prepare_strand(c, b))) return rc;   // (a batch encoded under the other setting is no longer corrected either)
  const bool records = p->source == TALC_SUPPORT_RECORD;
  if (records && !b->holds.has_records()) return fail(TALC_ERR_STATE, "talc_batch_correct has not run on this batch: it has no records");
  b->holds.supported = false;
  if (!b->holds.encoded && (rc = launch_encode(c, b))) return rc;
  const BatchSource src = batch_source(b, records);
  HIPCHK(b->d_support.ensure(c->cache, src.h_off[b->n_reads]));
  // (the buffer is an allocation of its own, 256-byte aligned: k_base_support takes a byte's alignment from its offset)
  rc = c->span[kSpanSupport].around(c->stream, [&] {
    if (b->n_reads)
      hipLaunchKernelGGL(k_base_support, dim3(b->n_reads), dim3(64), 0, c->stream, c->view, src.bytes, src.d_off, src.states, src.records,
                         c->p.reverse ? 1 : 0, b->rev_flags(), c->p.min_count, b->n_reads, p->phred ? 1 : 0, p->phred ? p->qmin : 0u,
                         p->phred ? p->qmax - p->qmin : 0u, b->d_support.get());
  });
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(c->stream));
  if ((rc = read_spans(c))) return rc;
  b->holds.supported = true; b->holds.supportRecords = records;
  return TALC_OK;
}

// the offsets of the bytes: the records' for RECORD, the input reads' for RAW
static const uint64_t* support_offsets(const talc_batch* b) { return batch_source(b, b->holds.supportRecords).h_off; }

uint64_t talc_batch_support_bytes(const talc_batch* b) { return (b && b->holds.has_support()) ? support_offsets(b)[b->n_reads] : 0; }

int talc_batch_fetch_support(talc_ctx* c, talc_batch* b, uint8_t* out, uint64_t out_capacity, uint64_t* out_offsets) {
  if (int rc = belong(c, b, "bad context/batch")) return rc;
  if (!b->holds.has_support()) return fail(TALC_ERR_STATE, "talc_batch_support has not run on this batch since its last correction");
  HIPCHK(hipSetDevice(c->device));
  const uint64_t* const off = support_offsets(b);
  const uint64_t total = off[b->n_reads];
  if (out_offsets) memcpy(out_offsets, off, ((size_t)b->n_reads + 1) * 8);
  return copy_out(c, out, out_capacity, b->d_support.get(), total, 1, hipMemcpyDeviceToHost, "support buffer", "bytes");
}

int talc_ctx_get_support_timing(const talc_ctx* c, float* support_ms) {
  if (!c) return fail(TALC_ERR_INVALID, "null context");
  if (support_ms) *support_ms = c->span[kSpanSupport].ms;
  return TALC_OK;
}
