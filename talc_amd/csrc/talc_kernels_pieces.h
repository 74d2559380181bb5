// talc_kernels_pieces.h — trimmed and split output (docs/trim_split.md): the records of a corrected batch cut at their
// uncorrected stretches, on the device, from the correction map (k_pack_map's talc_segment array).  A byte of a record is
// weak when it lies in a RAW segment and trusted otherwise; segments with out_len 0 hold no byte and are looked through.
//   split: the pieces of a read are its maximal runs of trusted bytes;
//   trim:  at most one piece, from the read's first trusted byte to its last (weak stretches inside it stay);
//   a piece of fewer than min_len bytes is dropped.
// k_piece_count leaves {kept pieces, their bytes} per read; the host turns those into offsets; k_piece_pack walks the
// segments again, writes the talc_piece entries and copies the bytes into one dense buffer.
#pragma once
#include "talc_kernels_search.h"   // MapSeg, SEG_RAW

namespace talc {

enum : int { PIECES_TRIM = 1, PIECES_SPLIT = 2 };
struct PieceCount { uint32_t n, bytes; };             // per read: kept pieces, their bytes
struct OutPiece { uint32_t read, outStart, outLen; };    // talc_piece

// One wave walks the segments of one read in order, 64 per pass, and calls emit(keep, rank, byteOff, start, len) once per
// pass on all lanes: a lane with `keep` holds a kept piece that ends in its segment — the rank-th kept piece of the read,
// byteOff kept bytes of the read before it, bytes [start, start + len) of the record.  Returns the read's totals.
//
// Split.  Two ballots per pass: the segments that hold a byte, and of those the trusted ones.  A lane finds its nearest
// non-empty neighbour on either side in those two words (clz / ctz of the word masked to the lanes below / above): a
// piece starts in a trusted segment whose nearest non-empty predecessor is weak or absent, and ends in one whose nearest
// non-empty successor is weak.  Weak and empty segments count 0 in an inclusive wave scan of out_len, so the plain scan
// is already the segmented one: a piece that ends in lane e and started in lane s is incl[e] - excl[s] bytes, s the
// highest start at or below e.  What crosses a pass: whether the last non-empty segment so far was trusted (a piece is
// open; "none seen yet" reads as weak, which starts a piece just the same), and the open piece's start and length so
// far.  An open piece whose next byte, in a later pass, is weak is reported by that weak segment's lane (no start at or
// below it: its length is the carried one); one that is still open after the last pass ends there and lane 0 emits it.
// min_len is applied where a piece ends; rank and byteOff are a popcount and a second scan over the kept ends.
//
// Trim.  The first trusted byte is the out_start of the first trusted non-empty segment, the last the end of the last
// one (out_start runs on without gaps): the lowest and the highest bit of the trusted word, kept across the passes in
// the same two carries, and emitted after the last pass like a split piece that is still open.
template <typename Emit>
TALC_D PieceCount walk_pieces(const MapSeg* __restrict__ segs, uint32_t nseg, int mode, uint32_t min_len, uint32_t lane, Emit emit) {
  const uint64_t below = (1ull << lane) - 1, above = lane == 63u ? 0ull : ~((2ull << lane) - 1);
  PieceCount tot = {0u, 0u};
  bool open = false;                       // split: a piece is open / trim: a trusted byte has been seen
  uint32_t openStart = 0, openLen = 0;     // split: the open piece so far / trim: first trusted byte, end of the last
  for (uint32_t base = 0; base < nseg; base += 64) {
    const uint32_t j = base + lane;
    MapSeg s = {SEG_RAW, 0u, 0u, 0u, 0u};
    if (j < nseg) s = segs[j];
    const uint64_t ne = __ballot(s.outLen > 0u);
    const uint64_t tr = __ballot(s.outLen > 0u && s.kind != SEG_RAW);
    if (mode == PIECES_TRIM) {
      if (tr) {                            // (wave-uniform)
        const uint32_t first = (uint32_t)__shfl((int)s.outStart, __builtin_ctzll(tr), 64);
        const uint32_t end = (uint32_t)__shfl((int)(s.outStart + s.outLen), 63 - __builtin_clzll(tr), 64);
        if (!open) openStart = first;
        openLen = end - openStart;
        open = true;
      }
      continue;
    }
    const bool mine = (tr >> lane) & 1ull;
    const uint32_t v = mine ? s.outLen : 0u;
    uint32_t incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)incl, off, 64); if (lane >= (uint32_t)off) incl += t; }
    const uint32_t passBytes = (uint32_t)__shfl((int)incl, 63, 64);
    const uint64_t lower = ne & below, upper = ne & above;
    const bool prevTrusted = lower ? ((tr >> (63 - __builtin_clzll(lower))) & 1ull) != 0 : open;
    const bool nextWeak = upper != 0 && ((tr >> __builtin_ctzll(upper)) & 1ull) == 0;
    const uint64_t starts = __ballot(mine && !prevTrusted);
    const uint64_t mystarts = starts & (below | (1ull << lane));
    const uint32_t sl = mystarts ? 63u - (uint32_t)__builtin_clzll(mystarts) : 0u;
    const uint32_t exclS = (uint32_t)__shfl((int)(incl - v), (int)sl, 64), startS = (uint32_t)__shfl((int)s.outStart, (int)sl, 64);
    const uint32_t len = mystarts ? incl - exclS : openLen + incl;
    const uint32_t start = mystarts ? startS : openStart;
    const bool closes = open && lower == 0 && ((ne >> lane) & 1ull) != 0 && !mine;   // the pass's first byte is weak: the open piece ends
    const bool keep = (closes || (mine && nextWeak)) && len >= min_len;
    const uint64_t kept = __ballot(keep);
    const uint32_t klen = keep ? len : 0u;
    uint32_t kincl = klen;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)kincl, off, 64); if (lane >= (uint32_t)off) kincl += t; }
    emit(keep, tot.n + (uint32_t)__popcll(kept & below), tot.bytes + kincl - klen, start, len);
    tot.n += (uint32_t)__popcll(kept);
    tot.bytes += (uint32_t)__shfl((int)kincl, 63, 64);
    if (ne) {                              // (wave-uniform) the carries: what the pass's last non-empty segment leaves open
      open = ((tr >> (63 - __builtin_clzll(ne))) & 1ull) != 0;
      if (open && starts) {                // the open piece started in this pass: at the highest start
        const int hs = 63 - __builtin_clzll(starts);
        openStart = (uint32_t)__shfl((int)s.outStart, hs, 64);
        openLen = passBytes - (uint32_t)__shfl((int)(incl - v), hs, 64);
      } else if (open) {
        openLen += passBytes;
      } else {
        openLen = 0;
      }
    }
  }
  // what is still open after the last pass ends there (trim: the one piece)
  const bool keepLast = open && openLen >= min_len;
  emit(lane == 0u && keepLast, tot.n, tot.bytes, openStart, openLen);
  if (keepLast) { tot.n += 1u; tot.bytes += openLen; }
  return tot;
}

// one wave per read: {kept pieces, their bytes}
__global__ void __launch_bounds__(64)
k_piece_count(const MapSeg* __restrict__ segs, const uint64_t* __restrict__ segOff, uint32_t n_reads, int mode, uint32_t min_len,
              PieceCount* __restrict__ counts) {
  const uint32_t r = blockIdx.x;
  if (r >= n_reads) return;
  const uint32_t lane = threadIdx.x;
  const PieceCount c = walk_pieces(segs + segOff[r], (uint32_t)(segOff[r + 1] - segOff[r]), mode, min_len, lane,
                                   [](bool, uint32_t, uint32_t, uint32_t, uint32_t) {});
  if (lane == 0) counts[r] = c;
}

// n bytes from src to dst by the whole block.  dst is written in aligned 4-byte words, each put together from the two
// aligned words of src that hold its bytes; the bytes before dst's first aligned word and the last few go one by one.
// No word is read that does not lie inside [src rounded down to 4, src + n).
TALC_D void block_copy_bytes(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint32_t n) {
  const uint32_t t = threadIdx.x, T = blockDim.x;
  const uint32_t head = min(n, (uint32_t)((4u - ((uintptr_t)dst & 3u)) & 3u));
  const uint32_t sh = (uint32_t)(((uintptr_t)src + head) & 3u);          // of every word's source
  const uint32_t room = n - head, last = sh ? 8u - sh : 4u;              // a word at offset 4 w reads source bytes up to 4 w + last
  const uint32_t nw = room >= last ? (room - last) / 4u + 1u : 0u;
  const uint32_t* const sw = (const uint32_t*)(src + head - sh);
  uint32_t* const dw = (uint32_t*)(dst + head);
  for (uint32_t w = t; w < nw; w += T) {
    const uint32_t lo = sw[w], hi = sh ? sw[w + 1] : 0u;
    dw[w] = (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * sh));
  }
  const uint32_t done = head + 4u * nw;
  for (uint32_t i = t; i < head + (n - done); i += T) { const uint32_t at = i < head ? i : done + (i - head); dst[at] = src[at]; }
}

// one block per read: its first wave walks the segments as k_piece_count did and writes the read's talc_piece entries
// and their byte offsets; then the whole block copies the bytes of every kept piece from the record (`records`: the
// dense records, or the masked ones) to the dense piece buffer.  A piece is never read beyond its record.
__global__ void __launch_bounds__(256)
k_piece_pack(const MapSeg* __restrict__ segs, const uint64_t* __restrict__ segOff, const uint8_t* __restrict__ records,
             const uint64_t* __restrict__ dense_off, uint32_t n_reads, int mode, uint32_t min_len,
             const uint64_t* __restrict__ readPieceOff, const uint64_t* __restrict__ readByteOff, OutPiece* pieces,
             uint64_t* pieceOff, uint8_t* __restrict__ out) {
  const uint32_t r = blockIdx.x;
  if (r >= n_reads) return;
  const uint64_t p0 = readPieceOff[r], b0 = readByteOff[r];
  const uint32_t np = (uint32_t)(readPieceOff[r + 1] - p0);
  if (np == 0) return;                     // (block-uniform)
  if (threadIdx.x < 64) {
    const PieceCount c = walk_pieces(segs + segOff[r], (uint32_t)(segOff[r + 1] - segOff[r]), mode, min_len, threadIdx.x,
                                     [&](bool keep, uint32_t rank, uint32_t byteOff, uint32_t start, uint32_t len) {
                                       if (keep && rank < np) { pieces[p0 + rank] = OutPiece{r, start, len}; pieceOff[p0 + rank] = b0 + byteOff; }
                                     });
    (void)c;
  }
  __syncthreads();                         // (the entries are read back below by the whole block)
  const uint8_t* const rec = records + dense_off[r];
  const uint32_t recLen = (uint32_t)(dense_off[r + 1] - dense_off[r]);
  const uint64_t bEnd = readByteOff[r + 1];
  for (uint32_t i = 0; i < np; ++i) {
    const OutPiece p = pieces[p0 + i];
    const uint64_t at = pieceOff[p0 + i];
    const uint32_t fits = at < bEnd ? (uint32_t)min((uint64_t)p.outLen, bEnd - at) : 0u;             // of the piece buffer
    const uint32_t n = p.outStart < recLen ? min(fits, recLen - p.outStart) : 0u;                     // of the record
    block_copy_bytes(out + at, rec + p.outStart, n);
  }
}

}  // namespace talc
