// search_scan.h -- the scan, the merge, the mark pass, the pair distances and the host driver of the query-time search, shared by the
// files that instantiate them: search.hip (a tile is NQ queries, a list each), search_sets.hip (SET: a tile is NQ members of ONE set
// query, one list), and search_q8.hip / search_sets_q8.hip (the same two tables over q8 rows).  What the
// kernels do and why the merges are exact is told at the head of search.hip.  One scan kernel, one launch site (launch_scan), one
// driver (run_search); the kernels keep internal linkage, so each file holds only the instantiations its entries launch --
// tests/test_build_search_no_spills.py pins search.hip's by name and number, and the SET ones live in search_sets.hip.
#pragma once
#include "exact_list.h"

#include <algorithm>
#include <type_traits>

namespace {
using namespace vtcsweep;

constexpr int SEARCH_MAX_Q = 64, SEARCH_MAX_DEPTH = 64, SEARCH_MAX_D = 2048, SEARCH_MAX_PARTS = 64;
constexpr int SEARCH_MAX_BLOCKS = 1024;       // workgroups of a scan (4 per CU on a 256-CU part): the number of lists per query in the workspace

// The places lists are read from, besides the LDS (LdsLists, exact_list.h).  Each carries the entries' groups (g), which only get<true> reads.
// the lists the scan's workgroups wrote: [query][entry][list], so that the 64 lanes of a merge step read neighbours
struct ScanLists {
  static constexpr bool groups_out = true;                // a grouped merge of these writes out_groups
  const double *d;
  const int *i, *g;
  int nlists, depth, q;
  template <bool GROUPED>
  __device__ __forceinline__ void get(int l, int e, double &cv, long long &ci, int &cg) const {
    const size_t o = ((size_t)q * depth + e) * nlists + l;
    cv = d[o];
    ci = i[o];
    if constexpr (GROUPED) cg = g[o];
  }
};
// The lists of an UNGROUPED set scan with several tiles a set, read as grouped lists in which every row is a group of its own: the
// same row can sit in the lists of different tiles at different distances (a tile knows only its own members' minimum), and the grouped
// insertion keeps the nearer entry of a group -- here of a row -- whichever comes first.  A row is below 2^31: the int is the row.
struct ScanRowLists : ScanLists {
  static constexpr bool groups_out = false;               // the merge writes no out_groups
  template <bool GROUPED>
  __device__ __forceinline__ void get(int l, int e, double &cv, long long &ci, int &cg) const {
    ScanLists::get<false>(l, e, cv, ci, cg);
    cg = (int)ci;
  }
};
// the caller's partial lists [part][query][depth]; an entry with a negative id is empty
struct PartLists {
  static constexpr bool groups_out = true;
  const double *d;
  const int64_t *i;
  const int32_t *g;
  int nq, depth, q;
  template <bool GROUPED>
  __device__ __forceinline__ void get(int l, int e, double &cv, long long &ci, int &cg) const {
    const size_t o = ((size_t)l * nq + q) * depth + e;
    ci = i[o];
    cv = ci < 0 ? INFINITY : d[o];
    if constexpr (GROUPED) cg = g[o];
  }
};
// LDS of the scan: the query tile, then (re-used) the waves' lists of the tile's queries -- SET: of the tile's one set -- 16 bytes an entry
constexpr size_t scan_lds_bytes(int nq_tile, int d, bool set = false) {
  const size_t tile = (size_t)nq_tile * d * sizeof(float), lists = (size_t)(set ? 1 : nq_tile) * 4 * 64 * (sizeof(double) + sizeof(long long));
  return tile > lists ? tile : lists;
}

// What a scan and the mark pass are given, as the host carries it to the one launch site of each.  The kernels take the members as
// parameters of their own (scan_kernel all of them, in this order): a struct member cannot be __restrict__, and without it the compiler schedules the distance
// loop into up to 26 more vector registers (profiles/search_refactor.md).  A field is looked at only by the modes named beside it.
struct ScanArgs {
  const void *gallery;            // [ng][d] of the kernel's G
  const float *queries;           // [nq][d]
  const unsigned *live;           // MASKED: the row mask's words
  const int *groups;              // GROUPED: a group id per row
  const double *after_d;          // AFTER: the cursors' fp64 distances and GLOBAL row ids, and the window's first id (nullable with EXCL:
  const int64_t *after_i;         //   no cursor)
  int64_t id_base;
  const int64_t *exclude;         // EXCL: a GLOBAL row id (ungrouped) or a group (grouped) per query; nullable in the page scan
  const unsigned *ban;            // the page scan: [nq][ceil(n_grp / 32)] bits of banned groups
  int n_grp;                      // the page scan and the mark pass: the groups are in [0, n_grp)
  int ng, nq, d, depth;
  double *part_d;                 // [nq][depth][gridDim.x]: the workgroups' lists
  int *part_i, *part_g;           //   part_g: GROUPED
  int *nonfinite;                 // nullable: bit 1 = the gallery holds a NaN / inf, bit 2 = the queries do
  int set_size = 0;               // SET: the members of every set, nq = sets x set_size (0: the queries are queries)
};

// GROUPED: the row's group is needed only once some query's `beats` is true.  It is loaded EAGERLY all the same, every lane reading the
// one address groups[row] with an ordinary load issued BEFORE the step's gallery loads, and moved to a scalar register only inside the
// insertion.  Loads return in order, so when the row's distances are there -- which every step waits for anyway -- the group has
// arrived: the rejecting path never waits on it, and the insertion never pays a memory round trip of its own, which a lazy load would
// cost exactly while a wave fills its lists and every row is inserted.  The price is NR load instructions and NR registers a step.
//
// EXCL: ungrouped the LOCAL row ex[u] (exclude[q] - id_base inside the window, else -1, which no row is), grouped the group ex[u] as an
// int64 (a value outside int32 is no group: every int32, -1 included, is a legal one).
//
// The page scan drops a row whose group is outside [0, n_grp), which has no bit.  Its cursor compare stays although a complete ban
// implies it: it is scalar and saves the load of the ban word.
//
// SET: the tile's NQ queries are members of ONE set query (set_size members a set, nq = sets x set_size; blockIdx.y runs over (set, tile
// of the set)) and the tile keeps ONE list, NL = 1.  A row's candidate is the fmin of its distances to the tile's members that are not
// dead -- a slot past the set's last member is dead (load_query_tile) -- on values wave_dist64_queries has formed anyway, every lane the
// same bits; it meets `beats` once, and the insertion path is the one above.  exclude[] has one key per SET.  A set scan has no cursor: the
// ungrouped excluding one is the AFTER + EXCL instantiation whose cursor is never loaded nor asked.  The workgroup writes one list per
// tile, list (tile, blockIdx.x) of its set.  The flag rides on the kernel's first parameter, SetOf<G> for G: an eighth template
// parameter would rename every existing instantiation, and a shared body inlined into two kernels compiled the existing scans to other
// code (a longer prologue, two more scalar registers).  The non-SET instantiations are the kernels they were.
template <typename T>
struct SetOf {};                                           // scan_kernel<SetOf<G>, ...>: the SET scan over a gallery of G
template <typename T>
struct ScanElem {
  using type = T;
  static constexpr bool set = false;
};
template <typename T>
struct ScanElem<SetOf<T>> {
  using type = T;
  static constexpr bool set = true;
};
template <typename GT, int NQ, int NR, bool MASKED, bool GROUPED, bool AFTER, bool EXCL>
__global__ __launch_bounds__(256) void scan_kernel(const typename ScanElem<GT>::type *__restrict__ gallery, const float *__restrict__ queries,
                                                   const unsigned *__restrict__ live, const int *__restrict__ groups,
                                                   const double *__restrict__ after_d, const int64_t *__restrict__ after_i, int64_t id_base,
                                                   const int64_t *__restrict__ exclude, const unsigned *__restrict__ ban, int n_grp, int ng, int nq,
                                                   int d, int depth, double *__restrict__ part_d, int *__restrict__ part_i,
                                                   int *__restrict__ part_g, int *__restrict__ nonfinite, int set_size) {
  using G = typename ScanElem<GT>::type;
  constexpr bool SET = ScanElem<GT>::set;
  static_assert(!(AFTER && GROUPED) || EXCL, "the grouped scan with a cursor is the page scan: it carries the (nullable) excluded group");
  static_assert(!EXCL || AFTER || GROUPED, "the excluding scans: the cursor scan, the grouped scan, or both (the page scan)");
  constexpr bool PAGE = GROUPED && AFTER;
  static_assert(!SET || (!PAGE && AFTER == (EXCL && !GROUPED)), "the set scans: plain, grouped, and either with an excluded key");
  constexpr bool CURSOR = AFTER && !SET;
  constexpr int NL = SET ? 1 : NQ;                         // lists of the tile
  extern __shared__ float4 smem4[];
  const float *qt = reinterpret_cast<const float *>(smem4);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  [[maybe_unused]] const int set_tiles = SET ? (set_size + NQ - 1) / NQ : 1, set = SET ? blockIdx.y / set_tiles : 0;
  [[maybe_unused]] const int set_tile = SET ? blockIdx.y - set * set_tiles : 0;
  const int q0 = SET ? set * set_size + set_tile * NQ : blockIdx.y * NQ;
  if constexpr (SET) nq = (set + 1) * set_size;            // the tile's members end with their set
  const unsigned dead = load_query_tile<NQ>(queries, q0, nq, d, smem4, nonfinite);      // bit u: query q0 + u takes no candidates

  SortedList<int, EMPTY_ROW, GROUPED> wl[NL];
#pragma unroll
  for (int u = 0; u < NL; ++u) wl[u].init();
  bool gallery_bad = false;
  [[maybe_unused]] double cd[NQ];                          // the cursors of the tile's queries (AFTER)
  [[maybe_unused]] int cr[NQ];
  if constexpr (CURSOR) load_cursors<NQ, EXCL>(after_d, after_i, id_base, ng, q0, nq, cd, cr);
  [[maybe_unused]] std::conditional_t<GROUPED, long long, int> ex[NL];      // the excluded group / local row of the tile's queries (EXCL)
  if constexpr (EXCL) {
#pragma unroll
    for (int u = 0; u < NL; ++u) {
      long long e;
      if constexpr (SET) e = uniform_of((long long)exclude[set]);
      else if constexpr (PAGE) e = exclude ? uniform_of((long long)exclude[min(q0 + u, nq - 1)]) : INT64_MIN;      // null: no group
      else e = uniform_of((long long)exclude[min(q0 + u, nq - 1)]);
      if constexpr (GROUPED) ex[u] = e;
      else ex[u] = e >= id_base && e - id_base < ng ? (int)(e - id_base) : -1;      // jj[r] is a row of the window: never -1
    }
  }
  [[maybe_unused]] const size_t ban_words = ((size_t)(unsigned)n_grp + 31) >> 5;      // words of a query's row of `ban` (PAGE)
  const long long n_steps = ((long long)ng + NR - 1) / NR, GW = (long long)gridDim.x * 4;
  long long s = (long long)blockIdx.x * 4 + wave;
  unsigned next_word = 0;
  if constexpr (MASKED) {
    if (s < n_steps) next_word = live_word<NR>(live, s);
  }
  for (; s < n_steps; s += GW) {
    unsigned bits = 0;
    if constexpr (MASKED) {
      bits = live_bits<NR>(ng, s, next_word);
      if (s + GW < n_steps) next_word = live_word<NR>(live, s + GW);
      if (!bits) continue;                                 // nothing live in this step: no gallery load
    }
    int jj[NR];
    step_rows<NR, MASKED>(s, bits, ng, jj);
    [[maybe_unused]] int gv[NR];                           // the rows' groups, as loaded (see above): jj[r] is a row of the gallery
    if constexpr (GROUPED) {
#pragma unroll
      for (int r = 0; r < NR; ++r) gv[r] = groups[jj[r]];
    }
    double dist[NQ * NR];
    wave_dist64_queries<NQ, NR>(qt, gallery, jj, d, lane, dist);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      if (row_taken<NR, MASKED>(s, bits, r, ng)) {
#pragma unroll
        for (int u = 0; u < NL; ++u) {
          double cv = dist[u * NR + r];
          const bool bad = !(cv < INFINITY);               // SET: of member 0 -- with finite query terms (load_query_tile) every member's
          if constexpr (SET) {                             // distance is finite iff the gallery row is.  The set's candidate: +inf with
            if (dead & 1) cv = INFINITY;                   // no member alive, which beats nothing
#pragma unroll
            for (int v = 1; v < NQ; ++v) {
              if (!((dead >> v) & 1)) cv = fmin(cv, dist[v * NR + r]);
            }
          }
          if (bad) gallery_bad = true;
          else if ((SET || !((dead >> u) & 1)) && wl[u].beats(cv, jj[r])) {
            if constexpr (CURSOR) {
              if (!(cv > cd[u] || (cv == cd[u] && jj[r] > cr[u]))) continue;      // at or before the cursor (or a NaN cursor)
            }
            int cg = 0;
            if constexpr (GROUPED) cg = uniform_of(gv[r]);
            if constexpr (EXCL && GROUPED) {
              if ((long long)cg == ex[u]) continue;        // a row of the query's excluded group
            } else if constexpr (EXCL) {
              if (jj[r] == ex[u]) continue;                // the query's excluded row
            }
            if constexpr (PAGE) {                          // a group outside [0, n_grp) has no bit, a banned one a row at or before the cursor
              if ((unsigned)cg >= (unsigned)n_grp) continue;
              const unsigned bw = ban[(size_t)(q0 + u) * ban_words + ((unsigned)cg >> 5)];      // q0 + u < nq: the query is not dead
              if ((uniform_of((int)bw) >> (cg & 31)) & 1) continue;
            }
            wl[u].insert(cv, jj[r], cg, lane, depth);
          }
        }
      }
    }
  }
  if (nonfinite && gallery_bad && lane == 0) atomicOr(nonfinite, 1);

  // ---- the workgroup's four lists of a query -> one: wave w merges the queries w, w + 4, ...  An LDS entry is 16 bytes either way:
  // ungrouped a 64-bit index, what merge_lists reads; grouped the row as an int plus its group, so the LDS of a workgroup -- with it the
  // resident workgroups per CU -- is the ungrouped scan's.
  __syncthreads();                                         // every wave is done with the query tile
  using LdsIndex = std::conditional_t<GROUPED, int, long long>;
  double *sd = reinterpret_cast<double *>(smem4);          // [NL][4][64]
  LdsIndex *si = reinterpret_cast<LdsIndex *>(sd + NL * 4 * 64);
  [[maybe_unused]] int *sg = reinterpret_cast<int *>(si) + NL * 4 * 64;      // GROUPED: after the int rows
#pragma unroll
  for (int u = 0; u < NL; ++u) {
    const int o = (u * 4 + wave) * 64 + lane;
    sd[o] = wl[u].bd;
    if constexpr (GROUPED) {
      si[o] = wl[u].bi;
      sg[o] = wl[u].bg;
    } else {
      si[o] = wl[u].bi == EMPTY_ROW ? EMPTY_ID : (long long)wl[u].bi;
    }
  }
  __syncthreads();
  const int nlists = gridDim.x * set_tiles, list = set_tile * gridDim.x + blockIdx.x, out0 = SET ? set : q0;
  for (int u = wave; u < NL; u += 4) {
    if (q0 + u >= nq) break;
    SortedList<long long, EMPTY_ID, GROUPED> m;
    m.init();
    merge_lists(m, LdsLists<LdsIndex>{sd + u * 4 * 64, si + u * 4 * 64, GROUPED ? sg + u * 4 * 64 : nullptr}, 4, 0, 64, depth, lane);
    if (lane < depth) {
      const size_t o = ((size_t)(out0 + u) * depth + lane) * nlists + list;
      part_d[o] = m.bd;
      part_i[o] = m.bi == EMPTY_ID ? EMPTY_ROW : (int)m.bi;
      if constexpr (GROUPED) part_g[o] = m.bg;
    }
  }
}

// One workgroup per query: the first `depth` of the union of the lists by (distance, index); GROUPED, of the distinct groups, a group's
// stale, worse entries from other lists being absorbed by the insertion (out_groups is not looked at otherwise).
template <typename Src, bool GROUPED>
__global__ __launch_bounds__(256) void merge_kernel(Src src, int nlists, int depth, int64_t id_base, int64_t *__restrict__ ids,
                                                    int32_t *__restrict__ out_groups, float *__restrict__ dists, double *__restrict__ dists64) {
  __shared__ double sd[4][64];
  __shared__ long long si[4][64];
  __shared__ int sg[4][64];                               // GROUPED
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = blockIdx.x;
  src.q = q;
  SortedList<long long, EMPTY_ID, GROUPED> wl;
  wl.init();
  merge_lists(wl, src, nlists, wave * 64, 256, depth, lane);
  sd[wave][lane] = wl.bd;
  si[wave][lane] = wl.bi;
  if constexpr (GROUPED) sg[wave][lane] = wl.bg;
  __syncthreads();
  if (wave != 0) return;
  merge_lists(wl, LdsLists<long long>{&sd[1][0], &si[1][0], GROUPED ? &sg[1][0] : nullptr}, 3, 0, 64, depth, lane);
  if (lane < depth) {                                      // write_result_row's block, with the group in its place
    const size_t o = (size_t)q * depth + lane;
    const bool empty = wl.bi == EMPTY_ID;
    ids[o] = empty ? -1 : id_base + wl.bi;
    if constexpr (GROUPED && Src::groups_out) out_groups[o] = empty ? -1 : wl.bg;
    if (dists) dists[o] = empty ? INFINITY : (float)wl.bd;
    if (dists64) dists64[o] = empty ? (double)INFINITY : wl.bd;
  }
}

// The mark pass (vtc_l2_group_mark_before): the scan's walk with the distances of wave_dist64_queries, so the bits the page scan
// compares, and no lists.  A live row with a finite distance that lies AT OR BEFORE query u's cursor, the exact negation of the scan's
// test, sets bit groups[row] of ban[q0 + u]: an atomicOr from one lane.  A NaN cursor therefore marks every such row (and admits
// nothing in the scan), -inf none.  A group outside [0, n_grp) marks nothing: it is checked before the address is formed.  The pass
// only ORs.
template <typename G, int NQ, int NR, bool MASKED>
__global__ __launch_bounds__(256) void mark_kernel(const G *__restrict__ gallery, const float *__restrict__ queries, const unsigned *__restrict__ live,
                                                   const int *__restrict__ groups, const double *__restrict__ after_d,
                                                   const int64_t *__restrict__ after_i, int64_t id_base, int n_grp, int ng, int nq, int d,
                                                   unsigned *__restrict__ ban) {
  extern __shared__ float4 smem4[];
  const float *qt = reinterpret_cast<const float *>(smem4);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q0 = blockIdx.y * NQ;
  const unsigned dead = load_query_tile<NQ>(queries, q0, nq, d, smem4, nullptr);      // bit u: query q0 + u marks nothing
  double cd[NQ];
  int cr[NQ];
  load_cursors<NQ, false>(after_d, after_i, id_base, ng, q0, nq, cd, cr);
  const size_t ban_words = ((size_t)(unsigned)n_grp + 31) >> 5;
  const long long n_steps = ((long long)ng + NR - 1) / NR, GW = (long long)gridDim.x * 4;
  long long s = (long long)blockIdx.x * 4 + wave;
  unsigned next_word = 0;
  if constexpr (MASKED) {
    if (s < n_steps) next_word = live_word<NR>(live, s);
  }
  for (; s < n_steps; s += GW) {
    unsigned bits = 0;
    if constexpr (MASKED) {
      bits = live_bits<NR>(ng, s, next_word);
      if (s + GW < n_steps) next_word = live_word<NR>(live, s + GW);
      if (!bits) continue;                                 // nothing live in this step: no gallery load
    }
    int jj[NR];
    step_rows<NR, MASKED>(s, bits, ng, jj);
    int gv[NR];                                            // loaded before the step's gallery rows, as the scan's
#pragma unroll
    for (int r = 0; r < NR; ++r) gv[r] = groups[jj[r]];
    double dist[NQ * NR];
    wave_dist64_queries<NQ, NR>(qt, gallery, jj, d, lane, dist);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      if (row_taken<NR, MASKED>(s, bits, r, ng)) {
#pragma unroll
        for (int u = 0; u < NQ; ++u) {
          const double cv = dist[u * NR + r];
          if (!(cv < INFINITY) || ((dead >> u) & 1)) continue;
          if (cv > cd[u] || (cv == cd[u] && jj[r] > cr[u])) continue;      // after the cursor: the page scan's business
          const int cg = uniform_of(gv[r]);
          if ((unsigned)cg >= (unsigned)n_grp) continue;                  // no bit: checked before the address is formed
          if (lane == 0) atomicOr(ban + (size_t)(q0 + u) * ban_words + ((unsigned)cg >> 5), 1u << (cg & 31));      // q0 + u < nq: not dead
        }
      }
    }
  }
}

// out[q] = D(queries[q], gallery[rows[q] - id_base]), the fp64 distance with the bits the scans form (the same wave_dist64_core), one
// wave per query; +inf for a row id outside [id_base, id_base + ng) -- -1 included -- whose memory is not touched.  The row is read
// WHETHER OR NOT IT IS LIVE: there is no mask here, a removed row keeps its memory (VideoIndex), and a cursor may stand on one.  The
// query is read as it is: one with a NaN / inf gives a non-finite out[q], which as a cursor admits nothing.
template <typename G>
__global__ __launch_bounds__(256) void pair_dists64_kernel(const G *__restrict__ gallery, const float *__restrict__ queries,
                                                           const int64_t *__restrict__ rows, int ng, int nq, int d, int64_t id_base,
                                                           double *__restrict__ out) {
  const int lane = threadIdx.x & 63, q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= nq) return;                                     // wave-uniform
  const long long row = uniform_of((long long)rows[q]);
  double v = INFINITY;
  if (row >= id_base && row - id_base < ng) {
    const int jj[1] = {(int)(row - id_base)};
    double dist[1];
    wave_dist64_queries<1, 1>(queries + (size_t)q * d, gallery, jj, d, lane, dist);
    v = dist[0];
  }
  if (lane == 0) out[q] = v;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
bool search_args_ok(int ng, int nq, int d, int depth) {
  return ng >= 1 && nq >= 1 && nq <= SEARCH_MAX_Q && depth >= 1 && depth <= SEARCH_MAX_DEPTH && depth <= ng && d >= 64 && d <= SEARCH_MAX_D &&
         d % 64 == 0;
}
// lists per query the workspace has room for: no scan has more workgroups than groups of four rows
int search_max_lists(int ng) { return (int)std::min<long long>(SEARCH_MAX_BLOCKS, ((long long)ng + 3) / 4); }
struct SearchWs {
  double *dists64, *part_d;
  int *part_i, *part_g;     // part_g: the grouped search's third part array, after the two every search has
  size_t total;
};
// nq: the result lists of the call, its queries or its sets; tiles: the tiles of a set, each with lists of its own (1: the queries are queries)
SearchWs search_ws(void *ws, int ng, int nq, int depth, bool grouped, int tiles = 1) {
  Bump b(ws);
  SearchWs s;
  const size_t entries = (size_t)nq * depth, lists = (size_t)tiles * search_max_lists(ng);
  s.dists64 = (double *)b.take(entries * sizeof(double));            // FIRST: the documented region of the header
  s.part_d = (double *)b.take(entries * lists * sizeof(double));
  s.part_i = (int *)b.take(entries * lists * sizeof(int));
  s.part_g = grouped ? (int *)b.take(entries * lists * sizeof(int)) : nullptr;
  s.total = b.off;
  return s;
}

// The scan's grid is persistent: as many workgroups as are resident at once (what the registers and the LDS of this tile shape allow, at
// most four per CU), never more than the workspace has lists for or the gallery has groups of four row steps.  Returns the grid's x.
// Every mode runs the grid of the plain scan (unmasked, ungrouped, no cursor) of its element type and tile, never more than is resident
// of its own instantiation, so all of them leave the same number of lists.  The masked 8 x 1 tile takes fewer registers than the plain
// one and would fit a fourth workgroup per CU; every wave fills lists of its own before it starts rejecting rows, and with all rows live
// at 10^5 rows the fourth workgroup put the masked scan 4.5 - 5.8 % behind the unmasked one instead of 3.4 - 3.6 %.  It was 2.5 % faster
// at 10^6 rows and 4 - 12 % on partly live masks there: the trade is written down in profiles/search_masked.md.
// SET: the same rule among the set scans, whose plain one is the baseline; `tiles` is then sets x tiles of a set.
template <typename G, int NQ, int NR, bool MASKED, bool GROUPED, bool AFTER, bool EXCL, bool SET>
int launch_scan(const ScanArgs &a, int tiles, hipStream_t stream) {
  static ResidentTable resident;                          // of this instantiation
  static_assert(SEARCH_MAX_D / 64 == 32, "ResidentTable's columns");
  const size_t lds = scan_lds_bytes(NQ, a.d, SET);
  using GT = std::conditional_t<SET, SetOf<G>, G>;
  const int per_cu = resident_per_cu(resident, a.d, [&] {
    int n = max_resident(scan_kernel<GT, NQ, NR, false, false, false, false>, lds, 1);
    if constexpr (MASKED || GROUPED || AFTER || EXCL) n = std::min(n, max_resident(scan_kernel<GT, NQ, NR, MASKED, GROUPED, AFTER, EXCL>, lds, n));
    return n;
  });
  const long long n_steps = ((long long)a.ng + NR - 1) / NR;
  const int blocks = (int)std::min<long long>(std::min(search_max_lists(a.ng), std::min(per_cu, 4) * vtcgemm::num_cus()), (n_steps + 3) / 4);
  hipLaunchKernelGGL((scan_kernel<GT, NQ, NR, MASKED, GROUPED, AFTER, EXCL>), dim3(blocks, tiles), dim3(256), lds, stream,
                     static_cast<const G *>(a.gallery), a.queries, a.live, a.groups, a.after_d, a.after_i, a.id_base, a.exclude, a.ban, a.n_grp, a.ng, a.nq,
                     a.d, a.depth, a.part_d, a.part_i, a.part_g, a.nonfinite, a.set_size);
  return blocks;
}
// The one place a call's arguments choose an instantiation: the tile of its query count, MASKED by `live`, and the mode by which of the
// groups, the cursor, the excluded keys and the ban bitmap it has.  Returns the grid's x.
// SET: the tile of the set's size, a.nq / a.set_size sets of its tiles each; the four modes without a cursor or a ban.
template <typename G, bool SET>
int launch_scan_of(const ScanArgs &a, hipStream_t stream) {
  const TilePlan p = tile_plan(SET ? a.set_size : a.nq);
  const int tiles = SET ? a.nq / a.set_size * p.tiles : p.tiles;
  auto mode = [&](auto grouped, auto after, auto excl) {
    return with_tile(p, [&](auto tq, auto tr) {
      constexpr int NQ = decltype(tq)::value, NR = decltype(tr)::value;
      constexpr bool GROUPED = decltype(grouped)::value, AFTER = decltype(after)::value, EXCL = decltype(excl)::value;
      return a.live ? launch_scan<G, NQ, NR, true, GROUPED, AFTER, EXCL, SET>(a, tiles, stream)
                    : launch_scan<G, NQ, NR, false, GROUPED, AFTER, EXCL, SET>(a, tiles, stream);
    });
  };
  constexpr std::true_type yes{};
  constexpr std::false_type no{};
  if constexpr (!SET) {
    if (a.ban) return mode(yes, yes, yes);                         // the page scan
  }
  if (a.groups) return a.exclude ? mode(yes, no, yes) : mode(yes, no, no);
  if (a.exclude) return mode(no, yes, yes);                        // the cursor scan with an excluded row; a.after_d may be null
  if constexpr (!SET) {
    if (a.after_d) return mode(no, yes, no);
  }
  return mode(no, no, no);
}
// The mark pass runs the scan's grid without its occupancy question: no lists depend on the number of workgroups, and a workgroup that is
// not resident at once only starts later.
template <typename G>
void launch_mark_of(const ScanArgs &a, unsigned *ban, hipStream_t stream) {
  const TilePlan p = tile_plan(a.nq);
  with_tile(p, [&](auto tq, auto tr) {
    constexpr int NQ = decltype(tq)::value, NR = decltype(tr)::value;
    const long long n_steps = ((long long)a.ng + NR - 1) / NR;
    const int blocks = (int)std::min<long long>(std::min(search_max_lists(a.ng), 4 * vtcgemm::num_cus()), (n_steps + 3) / 4);
    const size_t lds = (size_t)NQ * a.d * sizeof(float);
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(blocks, p.tiles), dim3(256), lds, stream, static_cast<const G *>(a.gallery), a.queries, a.live, a.groups,
                         a.after_d, a.after_i, a.id_base, a.n_grp, a.ng, a.nq, a.d, ban);
    };
    if (a.live) launch(mark_kernel<G, NQ, NR, true>);
    else launch(mark_kernel<G, NQ, NR, false>);
    return 0;
  });
}

// The checks every entry over a gallery window makes, in this order; `name` is what the entry calls itself in its messages.
// max_q = 0: any number of queries.  n_groups / depth null: the entry has none.  sets: {n_sets, set_size} of an entry whose queries are
// the members of sets, max_q together.
int check_shape(const char *name, int ng, int nq, int max_q, const char *nq_hint, const int *n_groups, const int *depth, int d, int64_t id_base,
                const int *sets = nullptr) {
  VTC_CHECK(ng >= 1, "%s: n_gallery=%d must be at least 1", name, ng);
  if (sets)
    VTC_CHECK(sets[0] >= 1 && sets[1] >= 1 && (long long)sets[0] * sets[1] <= max_q,
              "%s: n_sets=%d and set_size=%d must be at least 1, n_sets * set_size at most %d", name, sets[0], sets[1], max_q);
  else if (max_q) VTC_CHECK(nq >= 1 && nq <= max_q, "%s: n_queries=%d must be in [1, %d]%s", name, nq, max_q, nq_hint);
  else VTC_CHECK(nq >= 1, "%s: n_queries=%d must be at least 1", name, nq);
  if (n_groups) VTC_CHECK(*n_groups >= 1, "%s: n_groups=%d must be in [1, 2^31)", name, *n_groups);
  if (depth)
    VTC_CHECK(*depth >= 1 && *depth <= SEARCH_MAX_DEPTH && *depth <= ng, "%s: depth=%d must be in [1, min(%d, n_gallery)]", name, *depth,
              SEARCH_MAX_DEPTH);
  VTC_CHECK(d >= 64 && d <= SEARCH_MAX_D && d % 64 == 0, "%s: d=%d must be a multiple of 64 in [64, %d]", name, d, SEARCH_MAX_D);
  VTC_CHECK(id_base >= 0 && id_base <= INT64_MAX - ng, "%s: id_base=%lld must be non-negative (and id_base + n_gallery an int64)", name,
            (long long)id_base);
  return 0;
}

// vtc_l2_group_mark_before and vtc_l2_pair_dists64 over a gallery of G: the entries (search.hip, search_q8.hip) only choose G.
template <typename G>
int mark_before(const void *gallery, const float *queries, const uint32_t *live, const int32_t *groups, int n_groups, const double *after_d,
                const int64_t *after_i, int ng, int nq, int d, int64_t id_base, uint32_t *ban, void *stream) {
  const char *name = "l2_group_mark_before (the grouped search's cursor)";
  VTC_CHECK(gallery && queries && groups && after_d && after_i && ban, "%s: null argument", name);
  if (check_shape(name, ng, nq, SEARCH_MAX_Q, "", &n_groups, nullptr, d, id_base)) return 1;
  const ScanArgs a{gallery, queries, live, groups, after_d, after_i, id_base, nullptr, nullptr, n_groups, ng, nq, d, 0, nullptr, nullptr, nullptr, nullptr};
  launch_mark_of<G>(a, ban, (hipStream_t)stream);
  VTC_LAUNCH_CHECK("l2_group_mark_before");
  return 0;
}
template <typename G>
int pair_dists64(const void *gallery, const float *queries, const int64_t *rows, int ng, int nq, int d, int64_t id_base, double *out, void *stream) {
  const char *name = "l2_pair_dists64 (the search's cursor distances)";
  VTC_CHECK(gallery && queries && rows && out, "%s: null argument", name);
  if (check_shape(name, ng, nq, 0, "", nullptr, nullptr, d, id_base)) return 1;
  hipLaunchKernelGGL(pair_dists64_kernel<G>, dim3(cdiv(nq, 4)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const G *>(gallery), queries, rows,
                     ng, nq, d, id_base, out);
  VTC_LAUNCH_CHECK("l2_pair_dists64");
  return 0;
}

// A scan-plus-merge call, as the extern "C" entries fill it.  Null: live (no mask), groups (the ungrouped search; out_groups is then not
// looked at), after_d / after_i (no cursor), exclude, ban (not the page scan: n_groups is then not looked at), dists, nonfinite.
struct SearchCall {
  const void *gallery;
  bool half;                      // the gallery's rows are IEEE binary16
  const float *queries;
  const uint32_t *live;
  const int32_t *groups;
  const double *after_d;
  const int64_t *after_i;
  const int64_t *exclude;
  const uint32_t *ban;
  int n_groups;
  int ng, nq, d, depth;
  int64_t id_base;
  int64_t *ids;
  int32_t *out_groups;
  float *dists;
  int *nonfinite;
  void *ws;
  size_t ws_bytes;
  void *stream;
  bool given;                     // the pointers this entry requires beyond the gallery, the queries and ids are there
  const char *nq_hint = "";       // appended to the message that refuses the number of queries
  bool sets = false;              // the queries are n_sets sets of set_size members; nq is their product (0 where that is no int)
  int n_sets = 0, set_size = 0;
};
// the tiles of a set, each with lists of its own in the workspace
int set_tiles(const SearchCall &c) { return c.sets ? tile_plan(c.set_size).tiles : 1; }
int check_search_call(const char *name, const SearchCall &c) {
  VTC_CHECK(c.gallery && c.queries && c.ids && (!c.groups || c.out_groups) && c.given, "%s: null argument", name);
  VTC_CHECK(!c.after_d == !c.after_i, "%s: after_d and after_i are given together or not at all", name);
  VTC_CHECK(!(c.groups && c.after_d) || c.ban, "%s: the grouped search has no cursor (after_d / after_i with groups)", name);
  const int set_shape[2] = {c.n_sets, c.set_size};
  if (check_shape(name, c.ng, c.nq, SEARCH_MAX_Q, c.nq_hint, c.ban ? &c.n_groups : nullptr, &c.depth, c.d, c.id_base, c.sets ? set_shape : nullptr))
    return 1;
  const size_t need = search_ws(nullptr, c.ng, c.sets ? c.n_sets : c.nq, c.depth, c.groups != nullptr, set_tiles(c)).total;
  VTC_CHECK(c.ws && c.ws_bytes >= need, "%s: workspace too small (%zu < %zu)", name, c.ws_bytes, need);
  return 0;
}
// The scan of the call's mode, then the merge of the workgroups' lists -- grouped when the call is.
// SET: ONE merge per set over the lists of all its tiles' workgroups -- ScanLists with "query" = set.  Ungrouped, a set of several tiles
// is merged through ScanRowLists, which takes out a row that more than one tile has listed.
template <typename G, bool SET>
int run_search(const char *name, const SearchCall &c) {
  hipStream_t stream = (hipStream_t)c.stream;
  const int nout = SET ? c.n_sets : c.nq, tiles = set_tiles(c);
  const SearchWs s = search_ws(c.ws, c.ng, nout, c.depth, c.groups != nullptr, tiles);
  const ScanArgs a{c.gallery, c.queries, c.live, c.groups, c.after_d, c.after_i, c.id_base, c.exclude, c.ban, c.n_groups, c.ng,
                   c.nq,      c.d,       c.depth, s.part_d, s.part_i,  s.part_g,  c.nonfinite, c.set_size};
  const int blocks = launch_scan_of<G, SET>(a, stream);
  VTC_LAUNCH_CHECK2(name, "scan");
  const int nlists = blocks * tiles;
  const ScanLists lists{s.part_d, s.part_i, s.part_g, nlists, c.depth, 0};
  auto merge = [&](auto kernel, auto src, int32_t *out_groups) {
    hipLaunchKernelGGL(kernel, dim3(nout), dim3(256), 0, stream, src, nlists, c.depth, c.id_base, c.ids, out_groups, c.dists, s.dists64);
  };
  if (c.groups) {
    merge(merge_kernel<ScanLists, true>, lists, c.out_groups);
  } else if (SET && tiles > 1) {                           // a row that several tiles have listed comes out once
    if constexpr (SET) merge(merge_kernel<ScanRowLists, true>, ScanRowLists{lists}, nullptr);
  } else {
    merge(merge_kernel<ScanLists, false>, lists, nullptr);
  }
  VTC_LAUNCH_CHECK2(name, "merge");
  return 0;
}
// the entry of a file whose galleries are all of G (search_q8.hip, search_sets_q8.hip: SearchCall::half is not looked at)
template <typename G, bool SET = false>
int search_entry_of(const char *name, const SearchCall &c) {
  if (check_search_call(name, c)) return 1;
  return run_search<G, SET>(name, c);
}
template <bool SET = false>
int search_entry(const char *name, const SearchCall &c) {
  if (check_search_call(name, c)) return 1;
  return c.half ? run_search<_Float16, SET>(name, c) : run_search<float, SET>(name, c);
}
}  // namespace
