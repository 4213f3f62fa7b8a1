// range_many.hip -- vtc_l2_range_count_many_half: the count pass of the range search for MANY queries (up to 64 a call) over a gallery
// stored as IEEE binary16.  The result is vtc_l2_range_count(gallery, /*half*/ 1, ...)'s, bit for bit -- lims, the hit words at the head of
// the workspace, the bits ORed into nonfinite (include/vtc_hip.h) -- and vtc_l2_range_fill follows it on the same workspace unchanged; only
// the way there differs.  range.hip's scan forms every (query, row) distance in fp64, a gallery pass per started tile of 8 queries.  Here
// the gallery is streamed ONCE through the matrix cores for the APPROXIMATE distance A of search_many.hip, whose bound holds per pair,
//     |A - D| <= eps = many_eps(many_kappa(d), |q|^2, |g|^2)        (derived in many_common.h; A finite, the query not QF_FALLBACK)
// so a pair is decided on the spot: a hit when A + eps <= r, a miss when A - eps > r, and only a pair inside the BAND is decided by its fp64
// distance D -- formed by the function the scan and the fill use, from the bits they read.  A range search keeps no candidate list and needs
// no certificate over unseen rows.  Three launches, whatever the data:
//
//   many_prep_kernel        (many_common.h, search_many.hip's) a wave per query: |q|^2, the scale, the fp16 (hi, lo) B fragments, the dead
//                           and below-range flags, bit 2 of nonfinite; zeroes the counter of the pairs decided in fp64.
//   range_many_pass_kernel  a workgroup is one wave per 16 queries.  The unit of the walk (many_walk, many_common.h, with an item's
//                           fragments, its multiply step and A) is ONE hit word: 32 rows, two MFMA tiles of 16; every wave walks the
//                           workgroup's words, owning the words of its own 16 queries -- one writer a word, a plain store, zero words
//                           included (the workspace is not cleared; a word the walk skips is written where it is skipped), so the
//                           result does not depend on the grid.  Popcounts go into the scan's count slots, one per (query, workgroup).
//   range_prefix_kernel     (range_common.h, range.hip's) lims and the chunk bases, from the words and the counts.
//
// Not here: a grouped (distinct-video) range, more than 64 queries a call, an MFMA pass over fp32 rows (their rows are no MFMA operand).
#include "many_common.h"
#include "range_common.h"

namespace {
using namespace vtcsweep;

struct RangeManyWs {
  RangeWs head;             // range_ws's regions at range_ws's offsets: what vtc_l2_range_fill reads
  ManyPrologue pro;         // what many_prep_kernel writes
  unsigned long long *exact_pairs;      // the documented counter: the pairs of the call decided by their fp64 distance
  size_t total;
};
RangeManyWs range_many_ws(void *ws, int ng, int nq, int d) {
  RangeManyWs s;
  s.head = range_ws(ws, ng, nq);
  Bump b(ws);
  b.off = s.head.total;
  s.pro = many_prologue_ws(b, nq, d);
  s.exact_pairs = (unsigned long long *)b.take(sizeof(unsigned long long));
  s.total = b.off;
  return s;
}

// Row j is a hit of query q iff it is live, D is finite and D <= radius2[q] in fp64 (range.hip).  A dead query -- one with a NaN / inf, a
// slot past the last -- takes radius -1 and offers no pair.  The radius comparisons are made in fp64, so a NaN radius makes every pair a
// band pair, which the exact compare then rejects as the scan does.
template <bool MASKED, int NKS>
__global__ __launch_bounds__(256) void range_many_pass_kernel(const _Float16 *__restrict__ gallery, const float *__restrict__ queries,
                                                              const unsigned *__restrict__ live, const double *__restrict__ radius2,
                                                              const uint4 *__restrict__ qimg, const float *__restrict__ qn_all,
                                                              const float *__restrict__ inv_s_all, const int *__restrict__ qflag, int ng, int nq,
                                                              int d, int nwords, float kappa, unsigned *__restrict__ words, int *__restrict__ cnt,
                                                              unsigned long long *__restrict__ exact_pairs, int *__restrict__ nonfinite) {
  extern __shared__ uint4 smem_range_many[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;        // wave: the group of 16 queries
  const int u = lane & 15, kq = lane >> 4;
  const int nchunks = d / (32 * NKS);                      // an item is NKS MFMA steps of a tile
  const ManyImage<NKS> image(smem_range_many, qimg, d, wave, lane);

  const int q = wave * 16 + u;                             // the lane's query: column u of the MFMA's result
  const float qn = qn_all[q], m2inv_s = -2.f * inv_s_all[q];
  const int flag = qflag[q];
  const bool qdead = (flag & QF_DEAD) != 0, qexact = (flag & QF_FALLBACK) != 0;      // dead covers q >= nq
  const double r2 = qdead ? -1.0 : radius2[q];
  int count = 0;                                           // hits of the lane's query in this workgroup's words
  unsigned hw = 0;                                         // the word being built, of the lane's query (every kq lane the same)
  long long n_exact = 0;                                   // band pairs of the wave: uniform
  bool gallery_bad = false;

  auto put_word = [&](long long w, unsigned v) {          // w < nwords; the one writer of the word
    if (kq == 0 && q < nq) words[(size_t)q * nwords + w] = v;
  };

  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  float nrm = 0.f;
  // tile h (0, 1) of word w, chunk `chunk`; avail: the word's live rows inside the gallery, those of the tile != 0
  auto compute = [&](long long w, int h, unsigned avail, int chunk, const f16x8 (&ga)[NKS]) {
    many_multiply<NKS>(ga, image.item(chunk, lane), acc, nrm);
    if (chunk != nchunks - 1) return;
    // ---- the tile's epilogue: acc[i] = query u x row 4 kq + i of the tile
    const unsigned bits = (avail >> (16 * h)) & 0xffffu;
    nrm = many_row_norm(nrm);                              // every lane: |g|^2 of row u
    if (((bits >> u) & 1) && !(fabsf(nrm) < INFINITY)) gallery_bad = true;      // a live row with a NaN / inf: never a hit, bit 1
    const int row0 = (int)(w * 32) + 16 * h;
    unsigned mine = 0;                                     // bit i: row 4 kq + i of the tile is a hit of query u
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = 4 * kq + i;
      const float gn = __shfl(nrm, r, 64);
      const float A = many_dist(acc[i], qn, gn, m2inv_s);
      const bool pair = ((bits >> r) & 1) && fabsf(gn) < INFINITY && !qdead;
      const double eps = many_eps(kappa, qn, gn);
      const bool bounded = fabsf(A) < INFINITY && !qexact;
      const bool sure_hit = bounded && (double)A + eps <= r2, sure_miss = bounded && (double)A - eps > r2;
      if (pair && sure_hit) mine |= 1u << i;
      unsigned long long m = __ballot(pair && !sure_hit && !sure_miss);
      n_exact += __popcll(m);
      while (m) {                                          // the band: one pair at a time by the whole wave, the scan's bits
        const int from = __ffsll((long long)m) - 1;
        m &= m - 1;
        const int jj[1] = {row0 + 4 * (from >> 4) + i};
        double dist[1];
        wave_dist64_queries<1, 1>(queries + (size_t)(wave * 16 + (from & 15)) * d, gallery, jj, d, lane, dist);
        if (lane == from && dist[0] < INFINITY && dist[0] <= r2) mine |= 1u << i;
      }
    }
    unsigned t16 = mine << (4 * kq);                       // the four bits of the kq lanes -> the tile's 16
    t16 |= __shfl_xor(t16, 16, 64);
    t16 |= __shfl_xor(t16, 32, 64);
    hw |= t16 << (16 * h);
    if (h == 1 || (avail >> 16) == 0) {                    // the word's last live tile
      put_word(w, hw);
      count += __popc(hw);
      hw = 0;
    }
    acc = (f32x4){0.f, 0.f, 0.f, 0.f};
    nrm = 0.f;
  };

  // the unit is a hit word (nwords of them: ceil(ng / 32)); a word with no live row is written as 0 where the walk skips it
  many_walk<MASKED, NKS, 2>(gallery, live, ng, d, u, kq, compute, [&](long long w) { put_word(w, 0); });

  if (kq == 0 && q < nq) cnt[(size_t)q * gridDim.x + blockIdx.x] = count;      // the workgroup's slot of the query: a plain store
  if (wave == 0 && nonfinite && __ballot(gallery_bad) && lane == 0) atomicOr(nonfinite, 1);
  if (lane == 0 && n_exact) atomicAdd(exact_pairs, (unsigned long long)n_exact);
}
}  // namespace

extern "C" size_t vtc_l2_range_many_workspace_bytes(int n_gallery, int n_queries, int d) {
  if (!range_args_ok(n_gallery, n_queries, d)) return 0;
  return range_many_ws(nullptr, n_gallery, n_queries, d).total;
}

extern "C" int vtc_l2_range_count_many_half(const uint16_t *gallery, const float *queries, const uint32_t *live, const double *radius2, int ng,
                                            int nq, int d, int64_t *lims, int *nonfinite, void *ws, size_t ws_bytes, void *stream_) {
  const char *name = "l2_range_count_many_half";
  hipStream_t stream = (hipStream_t)stream_;
  VTC_CHECK(gallery && queries && radius2 && lims, "%s: null argument", name);
  VTC_CHECK(ng >= 1, "%s: n_gallery=%d must be at least 1", name, ng);
  VTC_CHECK(nq >= 1 && nq <= RANGE_MAX_Q, "%s: n_queries=%d must be in [1, %d] (more queries: slice them)", name, nq, RANGE_MAX_Q);
  VTC_CHECK(d >= 64 && d <= RANGE_MAX_D && d % 64 == 0, "%s: d=%d must be a multiple of 64 in [64, %d]", name, d, RANGE_MAX_D);
  const RangeManyWs s = range_many_ws(ws, ng, nq, d);
  VTC_CHECK(ws && ws_bytes >= s.total, "%s: workspace too small (%zu < %zu)", name, ws_bytes, s.total);

  const _Float16 *g = reinterpret_cast<const _Float16 *>(gallery);
  const int qg = many_qgroups(nq), nwords = range_words(ng);
  const int blocks = std::max(1, std::min(range_max_blocks(ng), many_per_cu(nq) * vtcgemm::num_cus()));      // at most the count slots
  auto pass = [&](auto masked, auto steps) -> int {
    constexpr bool MASKED = decltype(masked)::value;
    constexpr int NKS = decltype(steps)::value;
    static PerDeviceOnce attr;
    if (ensure_dynamic_lds(attr, reinterpret_cast<const void *>(&range_many_pass_kernel<MASKED, NKS>), 4 * MANY_IMG_MAX_BYTES, name)) return 1;
    hipLaunchKernelGGL((range_many_pass_kernel<MASKED, NKS>), dim3(blocks), dim3(64 * qg), many_img_lds_bytes(nq, d), stream, g, queries, live,
                       radius2, s.pro.qimg, s.pro.qn, s.pro.inv_s, s.pro.qflag, ng, nq, d, nwords, many_kappa(d), s.head.words, s.head.cnt,
                       s.exact_pairs, nonfinite);
    return 0;
  };

  many_launch_prep(queries, nq, d, s.pro, (int *)s.exact_pairs, 2, nonfinite, stream);
  VTC_LAUNCH_CHECK2(name, "prep");
  if (many_with_pass(live != nullptr, d, pass)) return 1;
  VTC_LAUNCH_CHECK2(name, "pass");
  hipLaunchKernelGGL(range_prefix_kernel, dim3(nq), dim3(256), 0, stream, s.head.words, s.head.cnt, blocks, nwords, range_chunks(ng),
                     (long long *)lims, s.head.chunk_base);
  VTC_LAUNCH_CHECK2(name, "prefix");
  return 0;
}
