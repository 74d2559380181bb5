// talc_kernels_strand.h — auto strand (docs/auto_strand.md): which orientation of a read the short reads support.
// The table is directional; a long cDNA read arrives in either orientation.  For a read of L raw bytes, S its Dna5
// conversion (what k_encode applies), n = max(0, L - K + 1), f[i] = the table count of S[i, i + K) and r[i] = the count of
// the reverse complement of S[i, i + K) (0 when the k-mer is absent or holds an N), k_strand_vote leaves six integers
// per read (talc_strand, include/talc_hip.h) and one flag byte, and nothing per position.  It runs on the raw bytes,
// before k_encode: the flag decides how k_encode, k_pack, k_pack_map and k_solidity treat the read.
#pragma once
#include "talc_kernels_build.h"      // dev_revcomp
#include "talc_kmer_window.h"

namespace talc {

struct StrandRow { uint32_t nKmers, fwdSolid, fwdIn, rcSolid, rcIn, reverse; };

// The shape of k_solidity: one wave per read, VOTE_TILE positions per pass, the pass's window staged straight from the raw
// bytes and the round of count lookups as talc_kmer_window.h has them; a k-mer is one funnel shift away, its reverse
// complement comes from it (dev_revcomp), never from a second window.  This kernel's own, per pass:
//   * the hash of every M-mer of the window and of that M-mer's reverse complement go to LDS: the presence filter's block
//     is chosen by a k-mer's minimizer (talc_common.h), and the M-mers of the reverse complement of a k-mer are the reverse
//     complements of the k-mer's own, at the same window positions;
//   * every lane takes VOTE_UNROLL positions 64 apart; the filter words of both orientations of all of them are asked for
//     before the first is looked at.  The filter has no false negatives: what it refuses has count 0, exactly;
//   * the survivors (about 7 % of the forward k-mers of a raw read, next to none in the orientation the short reads do
//     not have) are probed on a masked branch-free path, one orientation at a time and only when some lane has a
//     survivor in it (probe_round);
//   * __ballot turns each group of 64 positions into four words — solid and IN, forward and reverse complement —, the
//     counts are their populations: wave-uniform integer work.
#define VOTE_UNROLL 4
#define VOTE_TILE (64 * VOTE_UNROLL)
static_assert(VOTE_TILE == KWIN_TILE, "a pass is one window");
#define VOTE_MH (VOTE_TILE + 64)   /* M-mer positions of a window: VOTE_TILE + K - M <= VOTE_TILE + 19 */

__global__ void __launch_bounds__(64)
k_strand_vote(TableView T, const uint8_t* __restrict__ raw, const uint64_t* __restrict__ offsets, uint32_t min_count, uint32_t n_reads,
              StrandRow* __restrict__ rows, uint8_t* __restrict__ flags) {
  __shared__ uint64_t s_pack[KWIN_PACK_WORDS];
  __shared__ uint64_t s_nmask[KWIN_N_WORDS];
  __shared__ uint32_t s_mhF[VOTE_MH], s_mhR[VOTE_MH];   // hash of the M-mer that starts at a window position, and of its reverse complement
  static_assert(VOTE_MH + 32 <= 32 * (KWIN_PACK_WORDS - 1), "window() reads the word of an M-mer's first base and the one after it");
  const KmerWindow win = {s_pack, s_nmask};
  const uint32_t r = blockIdx.x;
  if (r >= n_reads) return;
  const uint32_t lane = threadIdx.x;
  const uint32_t K = T.k;
  const uint64_t rb = offsets[r];
  const uint32_t L = (uint32_t)(offsets[r + 1] - rb);
  const uint32_t n = L >= K ? L - K + 1 : 0;
  const SeqView seq = {(const uint8_t TALC_AS1*)(raw + rb), L, true, false};   // raw bytes, as they lie
  const uint32_t kshift = 64 - 2 * K;
  const uint64_t nkmask = (1ULL << K) - 1;          // K <= 31
  const uint64_t cap = T.capacity;                  // >= 64: HostTable::capacity_for never gives less
  const uint32_t M = filter_mmer_len(K);
  const uint32_t nwin = K - M + 1;                  // M-mers per k-mer
  const uint64_t nBlocks = T.filterWords >> 3;
  const uint64_t TALC_AS1* filter = (const uint64_t TALC_AS1*)T.filter;

  StrandRow row = {n, 0u, 0u, 0u, 0u, 0u};
  for (uint32_t p0 = 0; p0 < n; p0 += VOTE_TILE) {
    const uint32_t cnt = min((uint32_t)VOTE_TILE, n - p0);
    const uint32_t wlen = cnt + K - 1;              // p0 + wlen <= L
    win.stage(seq, p0, wlen, lane);
    __syncthreads();
    if (filter) {   // (an M-mer that holds an N belongs only to k-mers that are not asked for: its hash is never looked at)
      for (uint32_t q = lane; q < cnt + nwin - 1; q += 64) {
        const uint64_t mm = win.window(q) >> (64 - 2 * M);
        s_mhF[q] = mmer_hash((uint32_t)mm);
        s_mhR[q] = mmer_hash((uint32_t)dev_revcomp(mm, M));
      }
      __syncthreads();
    }
    // both k-mers of all of the lane's positions, their filter words asked for together
    uint64_t kmF[VOTE_UNROLL], kmR[VOTE_UNROLL];
    uint64_t fwF[VOTE_UNROLL], fwR[VOTE_UNROLL], fmF[VOTE_UNROLL], fmR[VOTE_UNROLL];
    bool ask[VOTE_UNROLL];
#pragma unroll
    for (int u = 0; u < VOTE_UNROLL; ++u) {
      const uint32_t q = (uint32_t)u * 64u + lane;
      ask[u] = q < cnt && (win.nbits(q) & nkmask) == 0;                  // no N among bases [q, q + K)
      kmF[u] = win.window(q) >> kshift;
      kmR[u] = dev_revcomp(kmF[u], K);
      fwF[u] = fwR[u] = ~0ULL; fmF[u] = fmR[u] = 1ULL;               // (no filter: every k-mer asked for is probed)
      if (filter && ask[u]) {
        uint32_t mhF = s_mhF[q], mhR = s_mhR[q];
        for (uint32_t i = 1; i < nwin; ++i) { mhF = min(mhF, s_mhF[q + i]); mhR = min(mhR, s_mhR[q + i]); }
        const FilterHash hF = filter_hash(kmF[u]), hR = filter_hash(kmR[u]);
        fmF[u] = filter_mask(hF); fmR[u] = filter_mask(hR);
        fwF[u] = filter[filter_block_of_min(mhF, nBlocks) * 8 + (hF.y >> 29)];
        fwR[u] = filter[filter_block_of_min(mhR, nBlocks) * 8 + (hR.y >> 29)];
      }
    }
    bool goF[VOTE_UNROLL], goR[VOTE_UNROLL];
    bool someF = false, someR = false;
#pragma unroll
    for (int u = 0; u < VOTE_UNROLL; ++u) {
      goF[u] = ask[u] && (fwF[u] & fmF[u]) == fmF[u];
      goR[u] = ask[u] && (fwR[u] & fmR[u]) == fmR[u];
      someF |= goF[u]; someR |= goR[u];
    }
    // one orientation at a time, the counts end as ballot words
#pragma unroll
    for (int o = 0; o < 2; ++o) {
      if (__ballot(o ? someR : someF) == 0ull) continue;              // (wave-uniform: nothing of this pass survived)
      uint32_t solid = 0, in = 0;
      probe_round<VOTE_UNROLL>(T.right, cap, o ? kmR : kmF, o ? goR : goF, cnt, [&](int, uint32_t c) {
        solid += (uint32_t)__popcll(__ballot(c >= min_count));
        in += (uint32_t)__popcll(__ballot(c > min_count));
      });
      if (o) { row.rcSolid += solid; row.rcIn += in; }
      else { row.fwdSolid += solid; row.fwdIn += in; }
    }
    __syncthreads();                                // (the next pass stages into the same words)
  }
  // the choice: the orientation with more IN k-mers (what reCoverage counts, Read.cpp:190), then with more solid ones;
  // a tie stays forward
  row.reverse = (row.rcIn > row.fwdIn || (row.rcIn == row.fwdIn && row.rcSolid > row.fwdSolid)) ? 1u : 0u;
  if (lane == 0) { rows[r] = row; flags[r] = (uint8_t)row.reverse; }
}

}  // namespace talc
