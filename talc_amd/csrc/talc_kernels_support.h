// talc_kernels_support.h — per-base short-read support (docs/base_support.md): one byte for every base of a sequence.
// For a sequence S of L bases, n = max(0, L - K + 1), solid[i] as in talc_kernels_solidity.h, and a base j:
//   span[j]  = the number of k-mer positions whose k-mer holds base j: [max(0, j - K + 1), min(j, n - 1)], 0 when n = 0;
//   cover[j] = how many of those are solid.
// The byte is cover[j], or 33 + qmin + (qmax - qmin) * cover[j] / span[j] (integer division; 33 + qmin where span is 0).
// k_solidity forms the solid bit of every position and reduces them away; k_base_support keeps them.
#pragma once
#include "talc_kernels_solidity.h"

namespace talc {

// the solid words a pass's bases are counted from: the last word of the pass before, the pass's SOL_UNROLL words, a zero word
#define SUP_WORDS (SOL_UNROLL + 2)
// q / d for d in 1 .. 31 and q <= 93 * 31 is (q * ceil(2^20 / d)) >> 20: the error of the reciprocal times q stays below 2^20
// and the product below 2^32.  Entry 0 is 0, so a base no k-mer holds gets the lowest quality by the same expression.
#define SUP_RCP_SHIFT 20

// One wave per sequence, walked in order, SOL_TILE positions per pass: the sequence view, the window and the probe round
// are talc_kmer_window.h's, the pass and its unroll k_solidity's.  This kernel's own, after the ballots:
//   * the wave-uniform solid words go to LDS (SUP_WORDS of them); cover[j] is the popcount of the K bits that end at
//     position j, a field that lies in two adjacent words: a lane reads those two once for its four bases (K + 3 <= 34 bits);
//   * the output is tiled by absolute address: a lane owns one aligned dword of the output buffer, computes its four bytes
//     and writes them with one dword store.  The passes' boundaries in the sequence are moved back by up to 3 bases so that
//     they fall on dword boundaries of the output (the bases left over are emitted by the next pass, which has the word
//     before), so only the first and the last dword of a read can be partial; their bytes are written one by one;
//   * where S is the reverse complement of what the caller holds (oflip), base j's byte goes to L - 1 - j: a lane's four
//     bases are the same four consecutive positions, packed in the opposite order.
// ascii / state / reverse / rev_flags as k_solidity takes them: RECORD = the dense records with the reads' states, RAW = the
// batch's codes (already in the orientation the correction sees) with state == nullptr.
__global__ void __launch_bounds__(64)
k_base_support(TableView T, const uint8_t* __restrict__ seqs, const uint64_t* __restrict__ offsets, const ReadState* __restrict__ state,
               int ascii, int reverse, const uint8_t* __restrict__ rev_flags, uint32_t min_count, uint32_t n_reads,
               int phred, uint32_t qmin, uint32_t qrange, uint8_t* __restrict__ out) {
  __shared__ uint64_t s_pack[KWIN_PACK_WORDS];
  __shared__ uint64_t s_nmask[KWIN_N_WORDS];
  __shared__ uint64_t s_sol[SUP_WORDS];             // bit (q % 64) of word q / 64: position p0 - 64 + q is solid
  __shared__ uint32_t s_rcp[32];                    // ceil(2^SUP_RCP_SHIFT / d)
  const KmerWindow win = {s_pack, s_nmask};
  const uint32_t r = blockIdx.x;
  if (r >= n_reads) return;
  const uint32_t lane = threadIdx.x;
  const uint32_t K = T.k;
  const uint64_t rb = offsets[r];
  const uint32_t L = (uint32_t)(offsets[r + 1] - rb);
  const uint32_t n = L >= K ? L - K + 1 : 0;
  const bool turned = reverse || (rev_flags && rev_flags[r]);
  // a record k_pack reverse complemented is read back to front (k_solidity); the codes are in S's orientation already
  const bool flip = state != nullptr && turned && state[r].status == TALC_READ_CORRECTED && state[r].overflow == 0;
  const bool oflip = state != nullptr ? flip : turned;   // S runs against the bytes the caller holds
  const SeqView seq = {(const uint8_t TALC_AS1*)(seqs + rb), L, ascii != 0, flip};
  const uint32_t kshift = 64 - 2 * K;
  const uint64_t nkmask = (1ULL << K) - 1;          // K <= 31
  const uint64_t cap = T.capacity;
  const uint32_t rb32 = (uint32_t)rb;               // (its low bits: the alignment of the read's first byte)
  const uint32_t base = phred ? 33u + qmin : 0u;

  if (lane < 32) s_rcp[lane] = lane ? ((1u << SUP_RCP_SHIFT) + lane - 1) / lane : 0u;
  __syncthreads();

  uint64_t prevWord = 0;   // the solid bits of the 64 positions before the pass
  uint32_t E0 = 0;         // bases [0, E0) have been written
  uint32_t p0 = 0;
  do {                     // (a sequence without a k-mer takes one pass without positions: every byte is the lowest)
    const uint32_t cnt = min((uint32_t)SOL_TILE, n - p0);
    uint64_t sol[SOL_UNROLL];
#pragma unroll
    for (int u = 0; u < SOL_UNROLL; ++u) sol[u] = 0;
    if (cnt) {             // (wave-uniform)
      win.stage(seq, p0, cnt + K - 1, lane);
      __syncthreads();
      uint64_t kmer[SOL_UNROLL];
      bool ask[SOL_UNROLL];
#pragma unroll
      for (int u = 0; u < SOL_UNROLL; ++u) {
        const uint32_t q = (uint32_t)u * 64u + lane;
        ask[u] = q < cnt && (win.nbits(q) & nkmask) == 0;             // no N among bases [q, q + K)
        kmer[u] = win.window(q) >> kshift;
      }
      // (the words of groups without a position stay 0)
      probe_round<SOL_UNROLL>(T.right, cap, kmer, ask, cnt, [&](int u, uint32_t c) { sol[u] = __ballot(c >= min_count); });
    }
    if (lane == 0) {
      s_sol[0] = prevWord;
#pragma unroll
      for (int u = 0; u < SOL_UNROLL; ++u) s_sol[1 + u] = sol[u];
      s_sol[SUP_WORDS - 1] = 0;
    }
    prevWord = sol[SOL_UNROLL - 1];
    __syncthreads();                                // (and every lane is done with the window: the next pass stages into it)

    // the bases this pass writes: [E0, E1).  Every k-mer that holds a base below F = p0 + cnt has its bit; the last pass
    // goes on to L (the positions beyond n are zero bits), another one stops at the last dword boundary of the output
    const uint32_t F = p0 + cnt;
    const bool last = F >= n;
    const uint32_t E1 = last ? L : (oflip ? F - ((0u - (rb32 + L - F)) & 3u) : F - ((rb32 + F) & 3u));
    const int32_t a0 = (int32_t)(oflip ? L - E1 : E0), a1 = (int32_t)(oflip ? L - E0 : E1);   // the bytes, from the read's first
    const uint64_t dEnd = (rb + (uint64_t)a1 + 3) >> 2;
    for (uint64_t d = ((rb + (uint64_t)a0) >> 2) + lane; d < dEnd; d += 64) {
      const int32_t o = (int32_t)(int64_t)(4 * d - rb);                  // the dword's first byte: -3 .. L - 1
      const int32_t smin = oflip ? (int32_t)L - 4 - o : o;               // the lowest of its four positions of S
      const uint32_t lo = (uint32_t)(smin - (int32_t)p0 + 64 - (int32_t)K + 1);   // first bit of the lowest field: 28 .. 319
      const uint32_t w = lo >> 6, sh = lo & 63;
      const uint64_t x0 = s_sol[w], x1 = s_sol[w + 1];
      const uint64_t x = (sh == 0) ? x0 : ((x0 >> sh) | (x1 << (64 - sh)));
      uint32_t packed = 0;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int32_t s = smin + m;
        const uint32_t cover = (uint32_t)__popcll((x >> m) & nkmask);
        // (a position outside the sequence has span 0, and a byte that is not written)
        const int32_t span = max(0, min(s, (int32_t)n - 1) - max(0, s - (int32_t)K + 1) + 1);
        const uint32_t byte = phred ? base + ((qrange * cover * s_rcp[span]) >> SUP_RCP_SHIFT) : cover;
        packed |= byte << (8 * (oflip ? 3 - m : m));
      }
      uint8_t* dst = out + 4 * d;
      if (o >= a0 && o + 4 <= a1) {
        *reinterpret_cast<uint32_t*>(dst) = packed;
      } else {                                      // the read's first or last dword: it shares it with its neighbours
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (o + i >= a0 && o + i < a1) dst[i] = (uint8_t)(packed >> (8 * i));
      }
    }
    E0 = E1;
    p0 += SOL_TILE;
  } while (p0 < n);
}

}  // namespace talc
