// talc_kernels_ends.h — long-read end clean-up (docs/read_ends.md): cDNA primers and poly-A/T tails found on the raw bytes
// of a batch, before anything is encoded or oriented.  For a read S of L bytes the head rule H(S) is
//   adapter: T = S[0, min(L, window)); D_a[e] = the smallest unit-cost edit distance between adapter a (m letters) and a
//            substring of T that ends at e (Sellers); accepted when D_a[e] <= k_a = floor(max_error_pct m / 100); the
//            adapter's match is the accepted e with the smallest D, the largest e among ties; the head's adapter is the one
//            whose match ends last, the lowest index among ties;
//   poly-T:  U = S[adapter_len, min(L, adapter_len + window)); score(j) = sum over i < j of (U[i] == 'T' ? +1 : -2); p = the
//            smallest j that maximises score; poly_len = p when poly_min > 0 and p >= poly_min, else 0;
// and the tail rule is H(revcomp(S)): the codes are read back to front and complemented, the reverse complement is never
// written anywhere.  A byte outside ACGTacgt is its own letter: it matches no adapter letter and is neither A nor T.
// k_read_ends leaves one 32-byte talc_end_row per read; k_gather copies the kept intervals into a dense text.
#pragma once
#include "talc_kernels_pieces.h"   // block_copy_bytes
#include "talc_sellers.h"
#include "talc_wave.h"

namespace talc {

enum : uint32_t { ENDS_MAX_ADAPTERS = 4, ENDS_MAX_WINDOW = 4096 };

struct EndRow {   // talc_end_row
  uint32_t headAdapterLen, headPolyLen, tailAdapterLen, tailPolyLen;
  uint8_t headAdapter, headAdapterErr, tailAdapter, tailAdapterErr;
  uint32_t keptStart, keptLen;
  int32_t orient;
};

// The setting as the kernel takes it, by value: everything in it is wave-uniform.  peq[a][c]: bit i set when letter i of
// adapter a has code c (Myers' match masks; a text code of 4 matches nothing and has no mask).
struct EndsParams {
  uint64_t peq[ENDS_MAX_ADAPTERS][4];
  uint32_t m[ENDS_MAX_ADAPTERS], k[ENDS_MAX_ADAPTERS];
  uint32_t nAdapters, polyMin, window, pad_;
};

// One adapter over the staged text s[0, n), dealt over the wave's 64 lanes (sellers_lane, talc_sellers.h): the accepted end
// with the smallest D, the largest among ties, as D << 32 | (0xFFFFFFFF - e); all ones without one.
TALC_D uint64_t adapter_key(const uint8_t* s, uint32_t n, const uint64_t (&peq)[4], uint32_t m, uint32_t k, uint32_t lane) {
  uint32_t c0, c1;
  sellers_chunk(n, 64u, lane, &c0, &c1);
  return wave_min_u64(sellers_lane(s, peq, m, k, c0, c1, ~0ull));
}

// The poly run over the staged text s[0, n): the smallest j that maximises score(j), 0 <= j <= n.  Every lane sums its chunk
// and keeps the chunk's best prefix; an exclusive wave scan of the sums places the chunks, a wave maximum of
// (score, -j) picks the run's end.  score(0) = 0 wins every tie, so only a positive maximum moves the end.
TALC_D uint32_t poly_run(const uint8_t* s, uint32_t n, uint32_t lane) {
  uint32_t c0, c1;
  sellers_chunk(n, 64u, lane, &c0, &c1);
  int32_t sum = 0, bestV = INT32_MIN / 2;
  uint32_t bestJ = 0;
  for (uint32_t j = c0; j < c1; ++j) {
    sum += s[j] == 3u ? 1 : -2;
    if (sum > bestV) { bestV = sum; bestJ = j + 1u; }
  }
  int32_t incl = sum;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) { const int32_t t = __shfl_up(incl, off, 64); if (lane >= (uint32_t)off) incl += t; }
  // (|score| <= 2 * ENDS_MAX_WINDOW: the bias keeps the key's upper half non-negative; an empty chunk has the lowest key)
  const uint64_t key = wave_max_u64(c0 < c1 ? (uint64_t)(uint32_t)(incl - sum + bestV + (1 << 20)) << 32 | (0xFFFFFFFFu - bestJ) : 0ull);
  return (key >> 32) > (1u << 20) ? 0xFFFFFFFFu - (uint32_t)key : 0u;
}

// one wave per read: both ends, then the kept interval and the orientation; lane 0 writes the row
__global__ void __launch_bounds__(64)
k_read_ends(const uint8_t* __restrict__ raw, const uint64_t* __restrict__ offsets, uint32_t n_reads, EndsParams P, EndRow* __restrict__ rows) {
  __shared__ uint8_t s_code[ENDS_MAX_WINDOW];
  const uint32_t r = blockIdx.x;
  if (r >= n_reads) return;
  const uint32_t lane = threadIdx.x;
  const uint64_t rb = offsets[r];
  const uint32_t L = (uint32_t)(offsets[r + 1] - rb);
  const uint8_t* const rd = raw + rb;
  const uint32_t window = min(P.window, (uint32_t)ENDS_MAX_WINDOW);
  uint32_t adLen[2] = {0u, 0u}, adIdx[2] = {0u, 0u}, adErr[2] = {0u, 0u}, poly[2] = {0u, 0u};
#pragma unroll
  for (int end = 0; end < 2; ++end) {
    const bool tail = end == 1;
    if (P.nAdapters) {                                 // (wave-uniform)
      const uint32_t n = min(L, window);
      stage_end(s_code, rd, L, 0u, n, tail, lane, 64u);
      __syncthreads();
      for (uint32_t a = 0; a < P.nAdapters; ++a) {
        const uint64_t best = adapter_key(s_code, n, P.peq[a], P.m[a], P.k[a], lane);
        const uint32_t e = 0xFFFFFFFFu - (uint32_t)best;
        if (best != ~0ull && e > adLen[end]) { adLen[end] = e; adIdx[end] = a + 1u; adErr[end] = (uint32_t)(best >> 32); }
      }
      __syncthreads();                                 // (the poly window is staged into the same bytes)
    }
    if (P.polyMin) {
      const uint32_t from = adLen[end];                // <= L
      const uint32_t n = min(L - from, window);
      stage_end(s_code, rd, L, from, n, tail, lane, 64u);
      __syncthreads();
      const uint32_t p = poly_run(s_code, n, lane);
      poly[end] = p >= P.polyMin ? p : 0u;
      __syncthreads();
    }
  }
  if (lane == 0) {
    const uint32_t head = adLen[0] + poly[0], tl = adLen[1] + poly[1];   // each <= L
    EndRow row;
    row.headAdapterLen = adLen[0]; row.headPolyLen = poly[0]; row.tailAdapterLen = adLen[1]; row.tailPolyLen = poly[1];
    row.headAdapter = (uint8_t)adIdx[0]; row.headAdapterErr = (uint8_t)adErr[0];
    row.tailAdapter = (uint8_t)adIdx[1]; row.tailAdapterErr = (uint8_t)adErr[1];
    row.keptStart = head;
    row.keptLen = L - head - min(tl, L - head);
    row.orient = (poly[1] && !poly[0]) ? 1 : (poly[0] && !poly[1]) ? -1 : 0;
    rows[r] = row;
  }
}

// the kept interval of read i (GatherInterval, talc_sellers.h)
TALC_HD GatherInterval gather_interval(const EndRow& row, uint32_t i) { return GatherInterval{i, row.keptStart, row.keptLen}; }

// one block per record: its interval to the record's place in the dense text `dst`; never beyond the read, never beyond the
// place, and an interval of a read that `src` does not hold is skipped.  The rows are read as they lie on the device: nothing
// is built or uploaded for the gather.
// (block_copy_bytes: aligned words of dst, each from the two aligned words of src that hold its bytes; the leading and
// trailing bytes one by one; no word of src is read that does not hold a byte of the interval)
template <class Row>
__global__ void __launch_bounds__(256)
k_gather(const uint8_t* __restrict__ src, const uint64_t* __restrict__ srcOff, uint32_t n_src_reads, const Row* __restrict__ rows, uint32_t n,
         uint8_t* __restrict__ dst, const uint64_t* __restrict__ dstOff) {
  const uint32_t i = blockIdx.x;
  if (i >= n) return;
  const GatherInterval iv = gather_interval(rows[i], i);
  if (iv.read >= n_src_reads) return;
  const uint32_t L = (uint32_t)(srcOff[iv.read + 1] - srcOff[iv.read]);
  const uint32_t room = (uint32_t)(dstOff[i + 1] - dstOff[i]);
  const uint32_t start = min(iv.start, L);
  const uint32_t len = min(min(iv.len, L - start), room);
  block_copy_bytes(dst + dstOff[i], src + srcOff[iv.read] + start, len);
}

}  // namespace talc
