// search_many.hip -- vtc_l2_search_many_half: the top-`depth` of MANY queries (up to 64 a pass) over a gallery stored as IEEE binary16.
// The result is vtc_l2_search_half's without groups, bit for bit (include/vtc_hip.h); only the way there differs.  The scan of search.hip
// forms every (query, row) distance in fp64, which at 64 queries is all it does: 8 gallery passes of fp64 arithmetic.  A half row already
// IS an fp16 MFMA operand, so here the gallery is streamed ONCE through the matrix cores for an APPROXIMATE distance A, a few more
// candidates than were asked for are kept, and the exact finish the sweeps use too (exact_list.h: the fp64 re-rank of the candidates, the
// brute-force scan behind an uncertified list) makes the answer exact again.  Four launches, whatever the data:
//
//   many_prep_kernel      a wave per query: |q|^2, the power-of-two scale s, the fp16 (hi, lo) split of s q laid out as the MFMA's B
//                         fragments, the dead / fallback flags of the query; zeroes the call's fallback counter.  (many_common.h)
//   many_pass_kernel      the candidate pass.  A workgroup is one wave per 16 queries; every wave walks the workgroup's tiles of 16 gallery
//                         rows (round-robin over the grid), loads a row tile straight from global memory into A fragments -- a lane's 16
//                         bytes are 8 consecutive halves of one row, no LDS, no conversion -- one item ahead of the one it multiplies,
//                         and keeps its queries' B fragments in the LDS (up to 512 columns: 32 KB a wave; a longer row reloads its
//                         part of them per item).  |g|^2 comes from the loaded fragments (v_dot2_f32_f16).  Per query the wave keeps
//                         the C = cdepth smallest (A, row) in a sorted list in the LDS, an entry per lane, and writes it to the
//                         workspace.  The waves of a workgroup read the same rows (the second to fourth from the caches): a list
//                         per (workgroup, query) is what bounds the number of insertions, the pass's other cost.
//   many_finish_kernel    a workgroup per query merges the workgroups' lists to the C best candidates and A_out, the value no row
//                         outside the list lies below; wave 0 forms the fp64 distances D of the candidates and their order by (D, row)
//                         (rerank64: the bits the scan forms), writes the first `depth`, and CERTIFIES the list:
//                             the list is every live finite row (A_out = +inf),  or  A_out - eps > D_depth   (strictly),
//                         since |A - D| <= eps puts every row outside the list strictly behind the depth-th found, exact ties included.
//                         A query that is not certified is appended to the flagged list.
//   many_fallback_kernel  the flagged queries only (normally none): a workgroup per query scans the live rows in fp64 (fallback_scan, with
//                         the scan's list insertion), and overwrites the query's row of the result.
//
// THE BOUND |A - D| <= eps is derived in many_common.h, with everything else this pass shares with range_many.hip's: the prologue, an item's
// fragments and its multiply step, A itself, the walk over the gallery and the host's choice of the instantiation.  What is here is what
// only the search has: the candidate lists, the finish and its certificate, the fallback.
#include "exact_list.h"
#include "many_common.h"
#include "search_scan.h"

namespace {
using namespace vtcsweep;

constexpr int MANY_MAX_DEPTH = 32;     // at least 21 spare ranks in a lane-per-entry list
constexpr int MANY_MAX_BLOCKS = 1024;  // workgroups of the pass at most (four one-wave workgroups a CU): lists per query in the workspace
// workgroups of the pass the workspace has lists for
inline int many_max_blocks(int ng, int nq) {
  return (int)std::min<long long>(MANY_MAX_BLOCKS / 4 * many_per_cu(nq), ((long long)ng + 15) / 16);
}

struct ManyWs {
  double *dists64;      // [nq][depth]: the documented head
  int *flags;           // flags[0]: the queries the fallback finished (the documented counter); flags[1 ..]: which
  ManyPrologue pro;     // what many_prep_kernel writes
  float *gmax;          // [blocks]
  int *over;            // [blocks][64]
  float *list_a;        // [nq][cdepth][blocks]
  int *list_i;
  size_t total;
};
ManyWs many_ws(void *ws, int ng, int nq, int d, int depth) {
  Bump b(ws);
  ManyWs s;
  const size_t blocks = many_max_blocks(ng, nq), entries = (size_t)nq * exact_cdepth(depth, ng);
  s.dists64 = (double *)b.take((size_t)nq * depth * sizeof(double));
  s.flags = (int *)b.take((1 + MANY_MAX_Q) * sizeof(int));
  s.pro = many_prologue_ws(b, nq, d);
  s.gmax = (float *)b.take(blocks * sizeof(float));
  s.over = (int *)b.take(blocks * MANY_MAX_Q * sizeof(int));
  s.list_a = (float *)b.take(entries * blocks * sizeof(float));
  s.list_i = (int *)b.take(entries * blocks * sizeof(int));
  s.total = b.off;
  return s;
}

// The sorted candidate list of one query: entry e on lane e, ascending A, kept in the LDS ([list][lane], a float and an int: 512 bytes a
// list, 8 KB a wave) so that the list a candidate belongs to is an ADDRESS -- sixteen lists in registers are sixteen copies of the
// insertion behind a branch tree, and took 1.8 times as long per added query (profiles/search_many.md).  Rows arrive in ascending
// order, so a strict compare keeps the lower row of a tie.  tau is the C-th entry (+inf until C rows have come): no row outside the
// list lies below it.
constexpr int MANY_LIST_BYTES = 16 * 64 * (int)(sizeof(float) + sizeof(int));      // of a wave
// lane l's value on lane l + 1: the DPP wave shift, a move instead of __shfl_up's trip through the LDS crossbar (lane 0 keeps its own)
__device__ __forceinline__ int wave_shr1(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xf, 0xf, false); }
// offers the wave-uniform candidate (cv, ci) to the list (la, li) = this lane's entry of it; returns the list's tau afterwards
__device__ __forceinline__ float many_offer(float *la, int *li, float cv, int ci, int lane, int cdepth) {
  float a = *la;
  int i = *li;
  const float cur = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, a), cdepth - 1));
  if (!(cv < cur)) return cur;                             // an earlier row of this step may have lowered tau
  const int pos = __popcll(__ballot(a <= cv));
  const float ua = __builtin_bit_cast(float, wave_shr1(__builtin_bit_cast(int, a)));
  const int ui = wave_shr1(i);
  if (lane > pos) { a = ua; i = ui; }
  if (lane == pos) { a = cv; i = ci; }
  *la = a;
  *li = i;
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, a), cdepth - 1));
}

template <bool MASKED, int NKS>
__global__ __launch_bounds__(256) void many_pass_kernel(const _Float16 *__restrict__ gallery, const unsigned *__restrict__ live,
                                                        const uint4 *__restrict__ qimg, const float *__restrict__ qn_all,
                                                        const float *__restrict__ inv_s_all, const int *__restrict__ qflag, int ng, int nq, int d,
                                                        int cdepth, float *__restrict__ list_a, int *__restrict__ list_i,
                                                        float *__restrict__ gmax_out, int *__restrict__ over_out, int *__restrict__ nonfinite) {
  extern __shared__ uint4 smem_many[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;        // wave: the group of 16 queries
  const int u = lane & 15, kq = lane >> 4;
  const int nchunks = d / (32 * NKS);                      // an item is NKS MFMA steps of a tile
  const ManyImage<NKS> image(smem_many, qimg, d, wave, lane);
  float *la = reinterpret_cast<float *>(smem_many + (size_t)(blockDim.x >> 6) * many_img_vecs(d, NKS)) + wave * (16 * 64 * 2) + lane;
  int *li = reinterpret_cast<int *>(la + 16 * 64);       // the waves' lists follow the images; la[64 v] / li[64 v]: this lane's entry of list v

  const int q = wave * 16 + u;                             // the lane's query: column u of the MFMA's result
  const float qn = qn_all[q], m2inv_s = -2.f * inv_s_all[q];
  const bool qdead = (qflag[q] & QF_DEAD) != 0;
#pragma unroll
  for (int v = 0; v < 16; ++v) la[64 * v] = INFINITY, li[64 * v] = EMPTY_ROW;
  float tau = INFINITY;                                    // of the lane's query
  bool over = false, gallery_bad = false;
  float gmax = 0.f;

  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  float nrm = 0.f;
  // chunk `chunk` of tile t (the walk's unit: its one tile); bits: the tile's live rows inside the gallery
  auto compute = [&](long long t, int, unsigned bits, int chunk, const f16x8 (&ga)[NKS]) {
    many_multiply<NKS>(ga, image.item(chunk, lane), acc, nrm);
    if (chunk != nchunks - 1) return;
    // ---- the tile's epilogue: acc[i] = query u x row 4 kq + i of the tile
    nrm = many_row_norm(nrm);                              // every lane: |g|^2 of row u
    const bool row_live = (bits >> u) & 1, row_fin = fabsf(nrm) < INFINITY;
    if (row_live && !row_fin) gallery_bad = true;
    if (row_live && row_fin) gmax = fmaxf(gmax, nrm);
    const int row0 = (int)(t * 16);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = 4 * kq + i;
      const float gn = __shfl(nrm, r, 64);
      const float A = many_dist(acc[i], qn, gn, m2inv_s);
      const bool cand = ((bits >> r) & 1) && fabsf(gn) < INFINITY && !qdead;
      const bool fin = fabsf(A) < INFINITY;
      if (cand && !fin) over = true;                       // D is finite, A is not: the query goes to the fallback
      unsigned long long m = __ballot(cand && fin && A < tau);
      while (m) {
        const int from = __ffsll((long long)m) - 1;
        m &= m - 1;
        const float cv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, A), from));
        const int ci = row0 + 4 * (from >> 4) + i, v = from & 15;
        const float t = many_offer(la + 64 * v, li + 64 * v, cv, ci, lane, cdepth);      // v is wave-uniform
        if (u == v) tau = t;
      }
    }
    acc = (f32x4){0.f, 0.f, 0.f, 0.f};
    nrm = 0.f;
  };

  many_walk<MASKED, NKS, 1>(gallery, live, ng, d, u, kq, compute, [](long long) {});      // a dead tile leaves nothing behind

  if (wave == 0) {
    const float g = wave_max(gmax);
    if (lane == 0) gmax_out[blockIdx.x] = g;
    if (nonfinite && __ballot(gallery_bad) && lane == 0) atomicOr(nonfinite, 1);
  }
  const unsigned long long ov = __ballot(over);
  if (kq == 0 && q < nq) over_out[(size_t)blockIdx.x * MANY_MAX_Q + q] = ((ov >> u) & 0x0001000100010001ull) != 0;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int qq = wave * 16 + v;
    if (qq < nq && lane < cdepth) {
      const size_t o = ((size_t)qq * cdepth + lane) * gridDim.x + blockIdx.x;
      list_a[o] = la[64 * v];
      list_i[o] = li[64 * v];
    }
  }
}

// the lists the pass wrote, [query][entry][workgroup], as merge_lists reads them
struct ManyLists {
  const float *a;
  const int *i;
  int nlists, cdepth, q;
  template <bool GROUPED>
  __device__ __forceinline__ void get(int l, int e, double &cv, long long &ci, int &cg) const {
    const size_t o = ((size_t)q * cdepth + e) * nlists + l;
    cv = a[o];
    ci = i[o];
  }
};

__global__ __launch_bounds__(256) void many_finish_kernel(const _Float16 *__restrict__ gallery, const float *__restrict__ queries, ManyLists src,
                                                          const float *__restrict__ qn, const int *__restrict__ qflag,
                                                          const float *__restrict__ gmax_parts, const int *__restrict__ over_parts, int ng, int d,
                                                          int depth, float kappa, int64_t id_base, int64_t *__restrict__ ids,
                                                          float *__restrict__ dists, double *__restrict__ dists64, int *__restrict__ flags) {
  __shared__ double sd[4][64];
  __shared__ long long si[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = blockIdx.x, cdepth = src.cdepth, nlists = src.nlists;
  src.q = q;
  const int flag = qflag[q];
  SortedList<long long, EMPTY_ID, false> wl;
  wl.init();
  if (!(flag & QF_DEAD)) merge_lists(wl, src, nlists, wave * 64, 256, cdepth, lane);
  sd[wave][lane] = wl.bd;
  si[wave][lane] = wl.bi;
  __syncthreads();
  if (wave != 0) return;
  merge_lists(wl, LdsLists<long long>{&sd[1][0], &si[1][0], nullptr}, 3, 0, 64, cdepth, lane);
  // the C best candidates by (A, row), lane e the e-th; nothing outside the list lies below a_out
  const double a_out = __shfl(wl.bd, cdepth - 1, 64);
  float gmax = 0.f;
  bool over = false;
  for (int l = lane; l < nlists; l += 64) {
    gmax = fmaxf(gmax, gmax_parts[l]);
    over = over || over_parts[(size_t)l * MANY_MAX_Q + q] != 0;
  }
  gmax = wave_max(gmax);
  over = __ballot(over) != 0;
  const int my = lane < cdepth && wl.bi != EMPTY_ID ? (int)wl.bi : -1;
  const int n_cand = __popcll(__ballot(my >= 0));          // the candidates are the first n_cand lanes
  double md;
  const int rank = rerank64(queries + (size_t)q * d, gallery, my, n_cand, d, lane, md);
  if (my >= 0 && rank < depth) {
    const size_t o = (size_t)q * depth + rank;
    ids[o] = id_base + my;
    if (dists) dists[o] = (float)md;
    dists64[o] = md;
  }
  if (lane >= n_cand && lane < depth) {                    // fewer candidates than depth: the tail (a dead query: the whole row)
    const size_t o = (size_t)q * depth + lane;
    ids[o] = -1;
    if (dists) dists[o] = INFINITY;
    dists64[o] = INFINITY;
  }
  if (flag & QF_DEAD) return;
  const unsigned long long last = __ballot(my >= 0 && rank == depth - 1);
  const double d_depth = last ? __shfl(md, __ffsll((long long)last) - 1, 64) : (double)INFINITY;
  const double eps = many_eps(kappa, qn[q], gmax);
  const bool whole = !(a_out < INFINITY) || n_cand >= ng;  // fewer than C candidates exist, or every row is one: nothing is outside
  const bool sure = !over && !(flag & QF_FALLBACK) && (whole || a_out - eps > d_depth);
  if (!sure && lane == 0) flags[1 + atomicAdd(flags, 1)] = q;
}

// The flagged queries: the brute-force scan over the LIVE rows of the half gallery, a row with a non-finite distance rejected (fallback_scan,
// exact_list.h) -- sixteen waves a query.
__global__ __launch_bounds__(1024) void many_fallback_kernel(const _Float16 *__restrict__ gallery, const float *__restrict__ queries,
                                                             const unsigned *__restrict__ live, int ng, int d, int depth, int64_t id_base,
                                                             const int *__restrict__ flags, int64_t *__restrict__ ids, float *__restrict__ dists,
                                                             double *__restrict__ dists64) {
  __shared__ double sd[16][64];
  __shared__ long long si[16][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n_flagged = flags[0];
  for (int f = blockIdx.x; f < n_flagged; f += gridDim.x) {        // uniform for the workgroup; normally zero trips
    const int q = flags[1 + f];
    const auto m = fallback_scan<true, 16>(queries + (size_t)q * d, gallery, live, ng, d, depth, &sd[0][0], &si[0][0]);
    if (wave == 0) write_result_row(m, q, depth, lane, id_base, ids, dists, dists64);
    __syncthreads();                                       // sd / si are reused by the next flagged query
  }
}

static_assert(MANY_MAX_Q == SEARCH_MAX_Q, "search_args_ok bounds the queries of a call");
bool many_args_ok(int ng, int nq, int d, int depth) { return search_args_ok(ng, nq, d, depth) && depth <= MANY_MAX_DEPTH; }
}  // namespace

extern "C" size_t vtc_l2_search_many_workspace_bytes(int n_gallery, int n_queries, int d, int depth) {
  if (!many_args_ok(n_gallery, n_queries, d, depth)) return 0;
  return many_ws(nullptr, n_gallery, n_queries, d, depth).total;
}

extern "C" int vtc_l2_search_many_half(const uint16_t *gallery, const float *queries, const uint32_t *live, int ng, int nq, int d, int depth,
                                       int64_t id_base, int64_t *ids, float *dists, int *nonfinite, void *ws, size_t ws_bytes, void *stream_) {
  const char *name = "l2_search_many_half";
  hipStream_t stream = (hipStream_t)stream_;
  VTC_CHECK(gallery && queries && ids, "%s: null argument", name);
  if (check_shape(name, ng, nq, MANY_MAX_Q, " (more queries: slice them)", nullptr, &depth, d, id_base)) return 1;
  VTC_CHECK(depth <= MANY_MAX_DEPTH, "%s: depth=%d must be at most %d (deeper: vtc_l2_search_half)", name, depth, MANY_MAX_DEPTH);
  const size_t need = many_ws(nullptr, ng, nq, d, depth).total;
  VTC_CHECK(ws && ws_bytes >= need, "%s: workspace too small (%zu < %zu)", name, ws_bytes, need);

  const ManyWs s = many_ws(ws, ng, nq, d, depth);
  const _Float16 *g = reinterpret_cast<const _Float16 *>(gallery);
  const int qg = many_qgroups(nq), cdepth = exact_cdepth(depth, ng);
  const int blocks = std::min(many_max_blocks(ng, nq), many_per_cu(nq) * vtcgemm::num_cus());
  const size_t lds = many_img_lds_bytes(nq, d) + (size_t)qg * MANY_LIST_BYTES;      // at most all 160 KiB of a CU
  auto pass = [&](auto masked, auto steps) -> int {
    constexpr bool MASKED = decltype(masked)::value;
    constexpr int NKS = decltype(steps)::value;
    static PerDeviceOnce attr;
    if (ensure_dynamic_lds(attr, reinterpret_cast<const void *>(&many_pass_kernel<MASKED, NKS>), 4 * (MANY_IMG_MAX_BYTES + MANY_LIST_BYTES), name)) return 1;
    hipLaunchKernelGGL((many_pass_kernel<MASKED, NKS>), dim3(blocks), dim3(64 * qg), lds, stream, g, live, s.pro.qimg, s.pro.qn, s.pro.inv_s,
                       s.pro.qflag, ng, nq, d, cdepth, s.list_a, s.list_i, s.gmax, s.over, nonfinite);
    return 0;
  };

  many_launch_prep(queries, nq, d, s.pro, s.flags, 1, nonfinite, stream);
  VTC_LAUNCH_CHECK2(name, "prep");
  if (many_with_pass(live != nullptr, d, pass)) return 1;
  VTC_LAUNCH_CHECK2(name, "pass");
  hipLaunchKernelGGL(many_finish_kernel, dim3(nq), dim3(256), 0, stream, g, queries, ManyLists{s.list_a, s.list_i, blocks, cdepth, 0}, s.pro.qn,
                     s.pro.qflag, s.gmax, s.over, ng, d, depth, many_kappa(d), id_base, ids, dists, s.dists64, s.flags);
  VTC_LAUNCH_CHECK2(name, "finish");
  hipLaunchKernelGGL(many_fallback_kernel, dim3(nq), dim3(1024), 0, stream, g, queries, live, ng, d, depth, id_base, s.flags, ids, dists, s.dists64);
  VTC_LAUNCH_CHECK2(name, "fallback");
  return 0;
}
