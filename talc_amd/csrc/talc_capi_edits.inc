// talc_capi_edits.inc — host side of the edit scripts (docs/correction_edits.md, talc_kernels_edits.h); included by
// talc_capi.hip inside its extern "C" block, after talc_capi_correct.inc.

// The delta words of the DPs that run side by side never take more than this, whatever the batch: the segments that need
// global words are taken in rounds, each sized by the real dimensions of its pairs.
static constexpr uint64_t kEditScratchBytes = 1ull << 30;
static constexpr uint64_t kEditDefaultCells = 1ull << 26;
// one pair's words must fit a round: at most cells + min(n, m) / 4 + 136 bytes (talc_edit_plan.h), so half the budget in cells.
// A larger max_cells acts as this: a pair of more cells is not aligned whatever the caller allows.
static constexpr uint64_t kEditMaxCells = kEditScratchBytes / 2;

// what an edit run reads — a map, the reads and their records, on the device — ...
struct EditIn {
  const MapSeg* d_segs; const uint64_t* d_seg_off; const uint64_t* h_seg_off;
  const uint8_t* d_raw; const uint64_t* d_raw_off; const uint8_t* d_dense; const uint64_t* d_dense_off;
  uint32_t n_reads;
};
// ... and what it leaves: an EditOut (talc_capi.hip)

// Spans kSpanEditAlignA .. kSpanEditPack: the first k_edit_align rounds, k_edit_count, the second rounds, k_edit_pack.
// scratch_bytes: the budget of the rounds (kEditScratchBytes; the test hook passes a small one to make several rounds).
// first_distance (may be null): the distance the DP of the first task found, -1 when there was no task.
static int run_edits(talc_ctx* c, const EditIn& in, uint64_t max_cells, uint64_t scratch_bytes, EditOut& out, int32_t* first_distance) {
  hipStream_t s = c->stream;
  const uint32_t n = in.n_reads;
  const uint64_t nseg = in.h_seg_off[n];
  if (nseg >> 32) return fail(TALC_ERR_INVALID, "%llu segments in one batch: the edit scripts index them with 32 bits", (unsigned long long)nseg);
  std::vector<MapSeg> hs(nseg);
  if (nseg) HIPCHK(hipMemcpyAsync(hs.data(), in.d_segs, nseg * sizeof(MapSeg), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  // the DPs, in segment order, cut into rounds whose global words fit the budget
  EditPlan plan(scratch_bytes / 8);
  for (uint32_t r = 0; r < n; ++r)
    for (uint64_t j = in.h_seg_off[r]; j < in.h_seg_off[r + 1]; ++j) {
      const MapSeg& g = hs[j];
      if (g.kind != SEG_CORRECTED || edit_part_kind(g.rawLen, g.outLen, max_cells) != EDIT_PART_DP) continue;
      if (!plan.add((uint32_t)j, r, g.rawLen, g.outLen))
        return fail(TALC_ERR_INVALID, "a %u x %u pair needs %llu bytes of alignment scratch, more than the budget", g.rawLen, g.outLen, (unsigned long long)(8 * edit_scratch_words(g.rawLen, g.outLen)));
    }
  plan.finish();
  const std::vector<EditTask>& tasks = plan.tasks;
  const std::vector<size_t>& roundEnd = plan.roundEnd;
  const uint64_t most = plan.mostWords;
  // per segment, per task, per read; the scratch of the largest round
  CachedBuf<EditPart> d_parts; CachedBuf<EditTask> d_tasks; CachedBuf<uint64_t> d_scratch, d_op_off; CachedBuf<EditRow> d_rows;
  HIPCHK(d_parts.alloc(c->cache, std::max<uint64_t>(nseg, 1)));
  HIPCHK(d_scratch.alloc(c->cache, std::max<uint64_t>(most, 1)));
  HIPCHK(d_rows.alloc(c->cache, std::max<uint32_t>(n, 1)));
  HIPCHK(d_op_off.alloc(c->cache, (uint64_t)n + 1));
  int rc;
  if ((rc = up(c, d_tasks, tasks, s))) return rc;
  auto align = [&](int write) {
    size_t t0 = 0;
    for (const size_t t1 : roundEnd) {   // (rounds run one after the other on the stream: they share the scratch)
      if (t1 > t0)
        hipLaunchKernelGGL(k_edit_align, dim3((unsigned)(t1 - t0)), dim3(64), 0, s, d_tasks.get() + t0, (uint32_t)(t1 - t0), in.d_segs, in.d_raw, in.d_raw_off,
                           in.d_dense, in.d_dense_off, d_scratch.get(), d_parts.get(), write, d_op_off.get(), out.d_ops.get());
      if (hipPeekAtLastError() != hipSuccess) return;   // (no round after one that failed; the span reports it)
      t0 = t1;
    }
  };
  Span* const span = c->span;
  if ((rc = span[kSpanEditAlignA].around(s, [&] { align(0); }))) return rc;
  rc = span[kSpanEditCount].around(s, [&] {
    if (n) hipLaunchKernelGGL(k_edit_count, dim3(n), dim3(64), 0, s, in.d_segs, in.d_seg_off, d_parts.get(), n, max_cells, d_rows.get());
  });
  if (rc) return rc;
  out.h_rows.assign(n, EditRow{0u, 0u, 0u, 0u, 0u, 0u});
  if (n) HIPCHK(hipMemcpyAsync(out.h_rows.data(), d_rows.get(), (size_t)n * sizeof(EditRow), hipMemcpyDeviceToHost, s));
  if (first_distance) {
    *first_distance = -1;
    if (!tasks.empty()) HIPCHK(hipMemcpyAsync(first_distance, &d_parts.get()[tasks[0].seg].distance, 4, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  out.h_op_off.resize((size_t)n + 1);
  uint64_t nops = 0;
  for (uint32_t r = 0; r < n; ++r) { out.h_op_off[r] = nops; nops += out.h_rows[r].nOps; }
  out.h_op_off[n] = nops;
  // exactly what the ops take; the buffer of an earlier call is kept when it is large enough
  HIPCHK(out.d_ops.ensure(c->cache, nops));
  HIPCHK(hipMemsetAsync(out.d_ops.get(), 0, std::max<uint64_t>(nops, 1) * sizeof(uint32_t), s));   // the runs are added
  HIPCHK(hipMemcpyAsync(d_op_off.get(), out.h_op_off.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, s));
  if ((rc = span[kSpanEditAlignB].around(s, [&] { align(1); }))) return rc;
  rc = span[kSpanEditPack].around(s, [&] {
    if (n) hipLaunchKernelGGL(k_edit_pack, dim3(n), dim3(64), 0, s, in.d_segs, in.d_seg_off, d_parts.get(), n, max_cells, d_op_off.get(), out.d_ops.get());
  });
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(s));
  return read_spans(c);
}

// 0 is the default; beyond what the scratch budget lets one pair take, the cap is that
static uint64_t effective_max_cells(uint64_t max_cells) { return max_cells == 0 ? kEditDefaultCells : std::min(max_cells, kEditMaxCells); }

static int batch_edits(talc_ctx* c, talc_batch* b, uint64_t max_cells, uint64_t scratch_bytes) {
  int rc;
  if ((rc = belong(c, b, "bad context/batch"))) return rc;
  if ((rc = enter_map(c, b))) return rc;
  b->holds.edited = false;
  const EditIn in = {b->d_segs.get(), b->d_seg_off.get(), b->h_seg_off.data(), b->d_raw.get(), b->d_offsets.get(), b->d_dense.get(), b->d_dense_off.get(), b->n_reads};
  if ((rc = run_edits(c, in, effective_max_cells(max_cells), scratch_bytes, b->edits, nullptr))) return rc;
  b->holds.edited = true;
  return TALC_OK;
}

int talc_batch_edits(talc_ctx* c, talc_batch* b, uint64_t max_cells) { return batch_edits(c, b, max_cells, kEditScratchBytes); }
// Test hook: the same with another scratch budget, so that a small batch takes several rounds
int talc_test_batch_edits(talc_ctx* c, talc_batch* b, uint64_t max_cells, uint64_t scratch_bytes) {
  if (scratch_bytes < 128 || scratch_bytes > kEditScratchBytes) return fail(TALC_ERR_INVALID, "scratch_bytes must be in 128 .. %llu", (unsigned long long)kEditScratchBytes);
  return batch_edits(c, b, max_cells, scratch_bytes);
}

uint64_t talc_batch_num_edit_ops(const talc_batch* b) { return (b && b->holds.has_edits()) ? b->edits.h_op_off[b->n_reads] : 0; }

int talc_batch_fetch_edits(talc_ctx* c, talc_batch* b, uint32_t* ops, uint64_t op_capacity, uint64_t* op_offsets, talc_edit_row* rows) {
  if (int rc = belong(c, b, "bad context/batch")) return rc;
  if (!b->holds.has_edits()) return fail(TALC_ERR_STATE, "talc_batch_edits has not run on this batch since its last correction");
  HIPCHK(hipSetDevice(c->device));
  const uint64_t nops = b->edits.h_op_off[b->n_reads];
  if (op_offsets) memcpy(op_offsets, b->edits.h_op_off.data(), ((size_t)b->n_reads + 1) * 8);
  if (rows && b->n_reads) memcpy(rows, b->edits.h_rows.data(), (size_t)b->n_reads * sizeof(talc_edit_row));
  return copy_out(c, ops, op_capacity, b->edits.d_ops.get(), nops, sizeof(uint32_t), hipMemcpyDeviceToHost, "op buffer", "ops");
}

int talc_ctx_get_edits_timing(const talc_ctx* c, float* align_ms, float* pack_ms) {
  if (!c) return fail(TALC_ERR_INVALID, "null context");
  if (align_ms) *align_ms = c->span[kSpanEditAlignA].ms + c->span[kSpanEditAlignB].ms;
  if (pack_ms) *pack_ms = c->span[kSpanEditCount].ms + c->span[kSpanEditPack].ms;
  return TALC_OK;
}

// Test hook: one read whose map is a single CORRECTED segment {0, la, 0, lb}, a its bases and b its record, through the
// kernels a batch goes through.
int talc_test_edit_script(talc_ctx* c, const char* a, uint32_t la, const char* b, uint32_t lb, uint64_t max_cells, uint32_t* ops,
                          uint64_t op_capacity, uint64_t* n_ops, int32_t* distance) {
  if (!c || (la && !a) || (lb && !b)) return fail(TALC_ERR_INVALID, "null argument");
  int rc;
  max_cells = effective_max_cells(max_cells);
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const MapSeg seg = {SEG_CORRECTED, 0u, la, 0u, lb};
  const uint64_t off[6] = {0, 1, 0, la, 0, lb};   // seg_off, raw_off, dense_off
  CachedBuf<MapSeg> d_seg; CachedBuf<uint64_t> d_off; CachedBuf<uint8_t> d_a, d_b;
  HIPCHK(d_seg.alloc(c->cache, 1)); HIPCHK(d_off.alloc(c->cache, 6));
  HIPCHK(d_a.alloc(c->cache, std::max<uint32_t>(la, 1))); HIPCHK(d_b.alloc(c->cache, std::max<uint32_t>(lb, 1)));
  HIPCHK(hipMemcpyAsync(d_seg.get(), &seg, sizeof seg, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(d_off.get(), off, sizeof off, hipMemcpyHostToDevice, s));
  if (la) HIPCHK(hipMemcpyAsync(d_a.get(), a, la, hipMemcpyHostToDevice, s));
  if (lb) HIPCHK(hipMemcpyAsync(d_b.get(), b, lb, hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));   // (the sources are this frame's and the caller's)
  const EditIn in = {d_seg.get(), d_off.get(), off, d_a.get(), d_off.get() + 2, d_b.get(), d_off.get() + 4, 1u};
  EditOut out;
  int32_t dist = -1;
  if ((rc = run_edits(c, in, max_cells, kEditScratchBytes, out, &dist))) return rc;
  const uint64_t nops = out.h_op_off[1];
  if (n_ops) *n_ops = nops;
  // without a DP: an empty side costs the other's length; a pair that was not aligned has no distance
  if (distance) *distance = (la == 0 || lb == 0) ? (int32_t)(la + lb) : dist;
  if (ops) {
    if (op_capacity < nops) return fail(TALC_ERR_CAPACITY, "op buffer too small: need %llu ops", (unsigned long long)nops);
    if (nops) HIPCHK(hipMemcpy(ops, out.d_ops.get(), nops * sizeof(uint32_t), hipMemcpyDeviceToHost));
  }
  return TALC_OK;
}
