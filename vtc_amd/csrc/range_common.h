// range_common.h -- what the two count passes of the range search share (range.hip: the fp64 scan; range_many.hip: the MFMA pass over a
// half gallery): the shape limits, the workspace's head that vtc_l2_range_fill reads, and the prefix launch that follows either pass.
#pragma once
#include "search_walk.h"

#include <algorithm>

namespace {
using namespace vtcsweep;

constexpr int RANGE_MAX_Q = 64, RANGE_MAX_D = 2048;
constexpr int RANGE_MAX_BLOCKS = 1024;        // workgroups of a count pass, at most: the count slots per query in the workspace
constexpr int CHUNK_WORDS = 16;               // hit words of a fill wave's unit (512 rows): one chunk base each

// One workgroup per query.  lims[q + 1]: the hits of the queries 0 .. q, from the workgroups' counts.  chunk_base[q][c]: the hits of query
// q in the words before chunk c, a thread a chunk and an exclusive scan over the workgroup, 256 chunks a round.
__global__ __launch_bounds__(256) void range_prefix_kernel(const unsigned *__restrict__ words, const int *__restrict__ cnt, int nblocks, int nwords,
                                                           int nchunks, long long *__restrict__ lims, int *__restrict__ chunk_base) {
  __shared__ long long s_total[4];
  __shared__ int s_wave[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = blockIdx.x;
  long long acc = 0;
  for (long long i = tid; i < (long long)(q + 1) * nblocks; i += 256) acc += cnt[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane == 0) s_total[wave] = acc;
  __syncthreads();
  if (tid == 0) {
    lims[q + 1] = s_total[0] + s_total[1] + s_total[2] + s_total[3];
    if (q == 0) lims[0] = 0;
  }
  const unsigned *wq = words + (size_t)q * nwords;
  int running = 0;
  for (int c0 = 0; c0 < nchunks; c0 += 256) {
    const int c = c0 + tid;
    int n = 0;
    if (c < nchunks) {
#pragma unroll
      for (int k = 0; k < CHUNK_WORDS; ++k) {
        const long long wi = (long long)c * CHUNK_WORDS + k;
        if (wi < nwords) n += __popc(wq[wi]);
      }
    }
    int x = n;                                             // inclusive scan of the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(x, o, 64);
      if (lane >= o) x += y;
    }
    __syncthreads();                                       // the last round's s_wave has been read
    if (lane == 63) s_wave[wave] = x;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      if (v < wave) before += s_wave[v];
      total += s_wave[v];
    }
    if (c < nchunks) chunk_base[(size_t)q * nchunks + c] = running + before + x - n;
    running += total;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
inline bool range_args_ok(int ng, int nq, int d) { return ng >= 1 && nq >= 1 && nq <= RANGE_MAX_Q && d >= 64 && d <= RANGE_MAX_D && d % 64 == 0; }
inline int range_words(int ng) { return (int)(((long long)ng + 31) / 32); }
inline int range_chunks(int ng) { return cdiv(range_words(ng), CHUNK_WORDS); }
// count slots per query the workspace has room for: no pass has more workgroups than groups of four words
inline int range_max_blocks(int ng) { return std::min(RANGE_MAX_BLOCKS, cdiv(range_words(ng), 4)); }
struct RangeWs {
  unsigned *words;          // [nq][ceil(ng / 32)]: FIRST, the documented region of the header
  int *cnt;                 // [nq][workgroups of the count pass]
  int *chunk_base;          // [nq][ceil(words / 16)]
  size_t total;
};
inline RangeWs range_ws(void *ws, int ng, int nq) {
  Bump b(ws);
  RangeWs s;
  s.words = (unsigned *)b.take((size_t)nq * range_words(ng) * sizeof(unsigned));
  s.cnt = (int *)b.take((size_t)nq * range_max_blocks(ng) * sizeof(int));
  s.chunk_base = (int *)b.take((size_t)nq * range_chunks(ng) * sizeof(int));
  s.total = b.off;
  return s;
}
}  // namespace
