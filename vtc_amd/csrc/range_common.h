// range_common.h -- what the two count passes of the range search share (range.hip: the fp64 scan; range_many.hip: the MFMA pass over a
// half gallery): the shape limits, the workspace's head that vtc_l2_range_fill reads, and the prefix launch that follows either pass.
// And what range.hip shares with range_q8.hip: the scan's count and fill kernels and their two calls, templates over the gallery's
// element type (range.hip's head tells what they do); a file holds the instantiations its entries ask for.
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

// Row j is a hit of query q0 + u iff it is live, D is finite and D <= radius2 in fp64.  A query with a NaN / inf, or a slot past the
// last query, takes radius -1: no distance is <= it.  A NaN or negative radius2 needs no case of its own -- no D >= 0 compares <= it.
template <int NQ, int NR, bool MASKED, typename G>
__global__ __launch_bounds__(256) void range_count_kernel(const G *__restrict__ gallery, const float *__restrict__ queries,
                                                          const unsigned *__restrict__ live, const double *__restrict__ radius2, int ng, int nq,
                                                          int d, int nwords, unsigned *__restrict__ words, int *__restrict__ cnt,
                                                          int *__restrict__ nonfinite) {
  static_assert(32 % NR == 0, "a step's rows lie in one word");
  extern __shared__ float4 smem4[];
  __shared__ int wave_cnt[4][NQ];
  const float *qt = reinterpret_cast<const float *>(smem4);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q0 = blockIdx.y * NQ;
  const unsigned dead = load_query_tile<NQ>(queries, q0, nq, d, smem4, nonfinite);      // the scan's tile: a dead query is a row of zeros
  double r2[NQ];
#pragma unroll
  for (int u = 0; u < NQ; ++u) r2[u] = (dead >> u) & 1 ? -1.0 : radius2[q0 + u];

  // ---- the pass: a word a unit.  `avail`: the rows of word w that are live and inside the gallery (wave-uniform, a scalar register).
  int count[NQ];
#pragma unroll
  for (int u = 0; u < NQ; ++u) count[u] = 0;
  bool gallery_bad = false;
  const long long GW = (long long)gridDim.x * 4;
  long long w = (long long)blockIdx.x * 4 + wave;
  unsigned next_word = 0xffffffffu;
  if constexpr (MASKED) {
    if (w < nwords) next_word = live[w];                   // every lane the one address, an ordinary load: requested a unit ahead
  }
  for (; w < nwords; w += GW) {
    const long long left = (long long)ng - w * 32;         // w < nwords: left >= 1
    const unsigned inside = left >= 32 ? 0xffffffffu : (1u << left) - 1;
    const unsigned avail = (unsigned)uniform_of((int)(next_word & inside));
    if constexpr (MASKED) {
      if (w + GW < nwords) next_word = live[w + GW];
    }
    unsigned hit[NQ];
#pragma unroll
    for (int u = 0; u < NQ; ++u) hit[u] = 0;
    for (int s = 0; s < 32 / NR; ++s) {
      const unsigned bits = (avail >> (s * NR)) & ((1u << NR) - 1);
      if (!bits) continue;                                 // nothing live in this step (or past the gallery): no gallery load
      const int j0 = (int)(w * 32) + s * NR;
      int jj[NR];
#pragma unroll
      for (int r = 0; r < NR; ++r) jj[r] = j0 + (NR == 1 || ((bits >> r) & 1) ? r : __ffs((int)bits) - 1);      // a dead slot: a live row of the step
      double dist[NQ * NR];
      wave_dist64_queries<NQ, NR>(qt, gallery, jj, d, lane, dist);
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        if ((bits >> r) & 1) {
          const unsigned bit = 1u << (s * NR + r);
#pragma unroll
          for (int u = 0; u < NQ; ++u) {
            const double cv = dist[u * NR + r];
            if (!(cv < INFINITY)) gallery_bad = true;
            else if (cv <= r2[u]) hit[u] |= bit;
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < NQ; ++u) {
      if (lane == 0 && q0 + u < nq) words[(size_t)(q0 + u) * nwords + w] = hit[u];
      count[u] += __popc(hit[u]);
    }
  }
  if (nonfinite && gallery_bad && lane == 0) atomicOr(nonfinite, 1);

  // ---- the workgroup's count of a query: its own slot, a plain store
  if (lane == 0) {
#pragma unroll
    for (int u = 0; u < NQ; ++u) wave_cnt[wave][u] = count[u];
  }
  __syncthreads();
  if (tid < NQ && q0 + tid < nq)
    cnt[(size_t)(q0 + tid) * gridDim.x + blockIdx.x] = wave_cnt[0][tid] + wave_cnt[1][tid] + wave_cnt[2][tid] + wave_cnt[3][tid];
}

// A wave per (query, chunk of 16 hit words).  The hits in ascending row order, four a step through wave_dist64_queries<1, 4> -- a pair's
// sum does not depend on how many pairs a call forms, so these are the bits the count pass compared.  An absent slot of a step repeats
// the step's first row and is dropped.  Whatever the workspace holds, a row is below n_gallery and a store inside [0, capacity).
template <typename G>
__global__ __launch_bounds__(256) void range_fill_kernel(const G *__restrict__ gallery, const float *__restrict__ queries,
                                                         const unsigned *__restrict__ words, const int *__restrict__ chunk_base,
                                                         const long long *__restrict__ lims, int ng, int d, int nwords, int nchunks,
                                                         long long capacity, long long id_base, long long *__restrict__ ids,
                                                         float *__restrict__ dists, double *__restrict__ dists64) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = blockIdx.y;
  const long long c = (long long)blockIdx.x * 4 + wave;    // wave-uniform
  if (c >= nchunks) return;
  const long long wi = c * CHUNK_WORDS + lane;
  unsigned word = 0;
  if (lane < CHUNK_WORDS && wi < nwords) {
    word = words[(size_t)q * nwords + wi];
    const long long left = (long long)ng - wi * 32;
    if (left < 32) word &= (1u << left) - 1;
  }
  if (!__ballot(word != 0)) return;                        // no hit in these 512 rows: nothing of the gallery is read
  long long p = lims[q] + chunk_base[(size_t)q * nchunks + c];
  const float *qrow = queries + (size_t)q * d;
  for (int l = 0; l < CHUNK_WORDS; ++l) {
    unsigned bits = (unsigned)uniform_of((int)__shfl(word, l, 64));
    const int row0 = (int)((c * CHUNK_WORDS + l) * 32);    // used only where bits != 0: a row of the gallery, below 2^31
    while (bits) {
      if (p >= capacity) return;                           // the result is truncated here: positions only grow
      int jj[4], nv = 0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (bits) {
          jj[r] = row0 + __ffs((int)bits) - 1;
          bits &= bits - 1;
          ++nv;
        } else {
          jj[r] = jj[0];
        }
      }
      double dist[4];
      wave_dist64_queries<1, 4>(qrow, gallery, jj, d, lane, dist);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long long o = p + r;
        if (lane == r && r < nv && o >= 0 && o < capacity) {
          ids[o] = id_base + jj[r];
          if (dists) dists[o] = (float)dist[r];
          if (dists64) dists64[o] = dist[r];
        }
      }
      p += nv;
    }
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
// The count pass's grid is persistent, sized as the scan's: as many workgroups as are resident at once (at most four per CU), never more
// than the workspace has count slots for.  Returns the grid's x.
template <int NQ, int NR, bool MASKED, typename G>
int launch_count(const G *gallery, const float *queries, const unsigned *live, const double *radius2, int ng, int nq, int d, const RangeWs &s,
                 int tiles, int *nonfinite, hipStream_t stream) {
  static ResidentTable resident;                           // of this instantiation
  static_assert(RANGE_MAX_D / 64 == 32, "ResidentTable's columns");
  const size_t lds = (size_t)NQ * d * sizeof(float);
  const int per_cu = resident_per_cu(resident, d, [&] { return max_resident(range_count_kernel<NQ, NR, MASKED, G>, lds, 1); });
  const int blocks = std::max(1, std::min(range_max_blocks(ng), std::min(per_cu, 4) * vtcgemm::num_cus()));
  hipLaunchKernelGGL((range_count_kernel<NQ, NR, MASKED, G>), dim3(blocks, tiles), dim3(256), lds, stream, gallery, queries, live, radius2, ng, nq, d,
                     range_words(ng), s.words, s.cnt, nonfinite);
  return blocks;
}
// the instantiation of the call: the scan's tile shapes (search_walk.h, tile_plan), MASKED by `live`
template <typename G>
int launch_count_of(const G *gallery, const float *queries, const unsigned *live, const double *radius2, int ng, int nq, int d, const RangeWs &s,
                    int *nonfinite, hipStream_t stream) {
  const TilePlan p = tile_plan(nq);
  return with_tile(p, [&](auto tq, auto tr) {
    constexpr int NQ = decltype(tq)::value, NR = decltype(tr)::value;
    return live ? launch_count<NQ, NR, true>(gallery, queries, live, radius2, ng, nq, d, s, p.tiles, nonfinite, stream)
                : launch_count<NQ, NR, false>(gallery, queries, nullptr, radius2, ng, nq, d, s, p.tiles, nonfinite, stream);
  });
}

// vtc_l2_range_count and vtc_l2_range_fill over a gallery of G: the entries (range.hip, range_q8.hip) only choose G.
template <typename G>
int range_count(const void *gallery, const float *queries, const uint32_t *live, const double *radius2, int ng, int nq, int d, int64_t *lims,
                int *nonfinite, void *ws, size_t ws_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  VTC_CHECK(gallery && queries && radius2 && lims, "l2_range_count: null argument");
  VTC_CHECK(ng >= 1, "l2_range_count: n_gallery=%d must be at least 1", ng);
  VTC_CHECK(nq >= 1 && nq <= RANGE_MAX_Q, "l2_range_count: n_queries=%d must be in [1, %d]", nq, RANGE_MAX_Q);
  VTC_CHECK(d >= 64 && d <= RANGE_MAX_D && d % 64 == 0, "l2_range_count: d=%d must be a multiple of 64 in [64, %d]", d, RANGE_MAX_D);
  const RangeWs s = range_ws(ws, ng, nq);
  VTC_CHECK(ws && ws_bytes >= s.total, "l2_range_count: workspace too small (%zu < %zu)", ws_bytes, s.total);
  const int blocks = launch_count_of((const G *)gallery, queries, live, radius2, ng, nq, d, s, nonfinite, stream);
  VTC_LAUNCH_CHECK2("l2_range_count", "count");
  hipLaunchKernelGGL(range_prefix_kernel, dim3(nq), dim3(256), 0, stream, s.words, s.cnt, blocks, range_words(ng), range_chunks(ng),
                     (long long *)lims, s.chunk_base);
  VTC_LAUNCH_CHECK2("l2_range_count", "prefix");
  return 0;
}
template <typename G>
int range_fill(const void *gallery, const float *queries, int ng, int nq, int d, const int64_t *lims, int64_t capacity, int64_t id_base, int64_t *ids,
               float *dists, double *dists64, void *ws, size_t ws_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  VTC_CHECK(gallery && queries && lims && (ids || capacity == 0), "l2_range_fill: null argument");
  VTC_CHECK(ng >= 1, "l2_range_fill: n_gallery=%d must be at least 1", ng);
  VTC_CHECK(nq >= 1 && nq <= RANGE_MAX_Q, "l2_range_fill: n_queries=%d must be in [1, %d]", nq, RANGE_MAX_Q);
  VTC_CHECK(d >= 64 && d <= RANGE_MAX_D && d % 64 == 0, "l2_range_fill: d=%d must be a multiple of 64 in [64, %d]", d, RANGE_MAX_D);
  VTC_CHECK(capacity >= 0, "l2_range_fill: capacity=%lld must be non-negative", (long long)capacity);
  VTC_CHECK(id_base >= 0 && id_base <= INT64_MAX - ng, "l2_range_fill: id_base=%lld must be non-negative (and id_base + n_gallery an int64)",
            (long long)id_base);
  const RangeWs s = range_ws(ws, ng, nq);
  VTC_CHECK(ws && ws_bytes >= s.total, "l2_range_fill: workspace too small (%zu < %zu)", ws_bytes, s.total);
  if (capacity == 0) return 0;                             // nothing to write
  const int nwords = range_words(ng), nchunks = range_chunks(ng);
  hipLaunchKernelGGL(range_fill_kernel<G>, dim3(cdiv(nchunks, 4), nq), dim3(256), 0, stream, (const G *)gallery, queries, s.words, s.chunk_base,
                     (const long long *)lims, ng, d, nwords, nchunks, (long long)capacity, (long long)id_base, (long long *)ids, dists, dists64);
  VTC_LAUNCH_CHECK("l2_range_fill");
  return 0;
}
}  // namespace
