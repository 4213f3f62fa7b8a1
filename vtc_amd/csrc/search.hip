// search.hip -- query-time search: the exact top-`depth` of a FEW queries (1 .. 64) over a stored gallery.  The N x N sweeps
// (sweep_topk.hip) split the gallery into bf16 operand planes, run a distance GEMM, select, and settle the result in fp64; at a handful
// of queries all of that is overhead.  Here the gallery is streamed ONCE per tile of queries and the fp64 distances of sweep_common.h are
// formed directly: exact by construction, so there are no candidate lists, error bounds or certification, and nothing of the gallery is
// written.  Every search is two launches:
//
//   scan_kernel<G, NQ, NR, MASKED, GROUPED, AFTER, EXCL>
//                      a grid of persistent workgroups; the tile of NQ queries lives in the LDS for the whole scan; each wave takes steps
//                      of NR gallery rows round-robin (search_walk.h; NQ x NR distances per step, all their loads in flight together)
//                      and keeps one sorted (fp64 distance, row) list per query, an entry per lane.  The list's last key is held in
//                      scalar registers: a row that is not closer than the current depth-th costs ONE COMPARE, whatever the mode --
//                      every mode's own test is asked after it, on the insertion path.  The four waves' lists are merged in the LDS;
//                      a workgroup writes ONE list per query to the workspace.
//   merge_kernel<Src, GROUPED>
//                      one workgroup per query merges the workgroups' lists (Src = ScanLists) or the caller's partial lists over
//                      disjoint gallery windows (Src = PartLists, vtc_l2_search_merge*): the lists are sorted, so a lane follows one
//                      list and leaves at its first entry that does not beat the current depth-th.
//
// G is the gallery's element type.  _Float16 (rows stored as IEEE binary16) differs in the row loader alone (sweep_common.h, row_piece):
// a lane loads 8 bytes a piece where the fp32 scan loads 16, widens them exactly and forms the distance with the same statements in the
// same order -- the fp64 bits of the fp32 scan over the widened rows.  The workspace, the lists and the merges do not know how the
// gallery is stored.  (NQ, NR) is the tile shape of the call's query count (search_walk.h, tile_plan).  The mode flags, and what each
// costs a row that HAS beaten the depth-th (a row that has not pays for none of them):
//
//   MASKED    only the rows whose bit of `live` is set take part (a deleted row, a query that searches a subset).  Costs nothing per
//             row: a step reads its mask word a step ahead, and a step with no live row issues no gallery load (search_walk.h).
//   GROUPED   several rows per video, and the `depth` nearest distinct VIDEOS come back.  Every row has a group id (int32, any value,
//             rows of a group anywhere).  Take the complete list of live rows with a finite distance, sorted by (distance, row); delete
//             every row that is not the first of its group in that order; the first `depth` of what remains are the result.  The
//             de-duplication happens INSIDE the lists (SortedList): one more int per entry, one more ballot per insertion.  The row's
//             group is loaded eagerly, before the step's gallery rows (below), so the insertion never waits for memory of its own.
//   AFTER     query u has a cursor (D*, row*) of the search order and is offered only the rows whose key lies strictly after it -- the
//             next page of a search, to any depth, by chaining each page's last key.  One scalar compare pair.  The cursor's distance
//             has to carry the bits the scan compares: it is the fp64 value of an earlier search's workspace, or vtc_l2_pair_dists64's.
//   EXCL      query u names one key it is never offered: ungrouped a row ("more like this" without the row itself), grouped a group
//             (hard negatives without the text's own video).  One scalar compare, after the cursor's.
//
// Six combinations exist (launch_scan_of): plain; GROUPED; AFTER; AFTER + EXCL, the excluded row, where a null cursor is -inf, so one
// kernel serves the excluding search with and without a cursor; GROUPED + EXCL, the excluded group; and GROUPED + AFTER + EXCL, the PAGE
// scan of vtc_l2_search_grouped_after.  The grouped order has no cursor a row could be asked about by itself: a row after the cursor
// belongs on the page only if NO admissible row of its group lies at or before the cursor, and such a row may be in any wave's share.
// So mark_kernel (vtc_l2_group_mark_before) first walks the gallery as the scan does and ORs bit groups[row] of ban[q] for every live
// row with a finite distance at or before q's cursor -- no lists, no merge -- and the page scan drops a row whose group's bit is set:
// one ordinary load of the word, on the insertion path only, after the cursor and the excluded group (nullable there).  The groups of
// these two entries are DENSE, [0, n_groups): the bitmap is indexed by them.
//
// Deleting a row -- or every row of a group, BEFORE the lists de-duplicate -- from the candidates is deleting it from the order: the
// cursor, the excluded key and the ban only decide which rows are offered, and the lists, both merges and the window merges do not
// care which were.
//
// Why merging de-duplicated lists is exact, for the waves' lists in the LDS, the workgroups' lists and the caller's windows alike: a
// group of the union's first `depth` has its overall nearest row in some part.  In that part fewer than `depth` groups have a smaller
// local minimum (a local minimum is not below the overall one of its group, and fewer than `depth` groups are nearer overall), so that
// part's list holds the entry.  The stale, worse entries of the same group from other parts are absorbed by the insertion: whichever
// comes first, the better one stays.  The early exit of merge_lists stays valid -- the depth-th key only falls, so a lane may leave its
// sorted list at the first entry that does not beat it; an entry that beats it but whose group a better entry holds is dropped and the
// lane goes on.
#include "search_walk.h"

#include <algorithm>
#include <type_traits>

namespace {
using namespace vtcsweep;

constexpr int SEARCH_MAX_Q = 64, SEARCH_MAX_DEPTH = 64, SEARCH_MAX_D = 2048, SEARCH_MAX_PARTS = 64;
constexpr int SEARCH_MAX_BLOCKS = 1024;       // workgroups of a scan (4 per CU on a 256-CU part): the number of lists per query in the workspace
constexpr int EMPTY_ROW = 0x7fffffff;         // index of an empty list slot (distance +inf)
constexpr long long EMPTY_ID = 0x7fffffffffffffffll;

// A sorted list of (fp64 distance, index) keys, one entry per lane, ascending; the first `depth` lanes are the list, (tau, tau_i) its last
// key, wave-uniform.  Empty slots hold (+inf, EMPTY).  Ungrouped, the insertion is exact_fallback_kernel's `offer` (sweep_topk.hip).
//
// GROUPED: every entry carries the group id of its row (bg), and over all 64 lanes -- not only the first `depth` -- no two non-empty
// entries share a group.  An empty slot is known by its index (EMPTY), never by bg: every int is a legal group id.  A candidate that has
// passed `beats` meets the lane p_old that holds its group, if any (one more ballot):
//   that entry is before the candidate         -> the candidate is dropped;
//   otherwise, with pos the candidate's place  -> the lanes (pos, p_old] take their left neighbour's entry, lane pos the candidate, the
//                                                 lanes above p_old keep theirs: the group's old entry is the one that leaves;
//   no lane holds the group                    -> p_old = 63, the ungrouped shift of everything above pos.
// Entries only ever move towards higher lanes, so what lies past the depth-th never comes back: a row that does not beat the depth-th
// changes nothing of the first `depth`, whether its group is held (by an entry that is then not worse than the depth-th, or by one
// past it) or not -- `beats` is the ungrouped list's one compare.  A group no lane holds has no row so far that was before the depth-th
// key of its time (it would still be held, or has left over lane 63 behind 64 closer groups), and that key only falls: inserting is right.
template <bool GROUPED>
struct EntryGroup {
  int bg;
};
template <>
struct EntryGroup<false> {};
template <typename I, I EMPTY, bool GROUPED>
struct SortedList : EntryGroup<GROUPED> {
  static constexpr bool grouped = GROUPED;
  double bd, tau;
  I bi, tau_i;
  __device__ __forceinline__ void init() {
    bd = tau = INFINITY;
    bi = tau_i = EMPTY;
    if constexpr (GROUPED) this->bg = 0;
  }
  // wave-uniform candidate: is it finite and before the depth-th entry?
  __device__ __forceinline__ bool beats(double cv, I ci) const { return cv < INFINITY && (cv < tau || (cv == tau && ci < tau_i)); }
  // cg: the candidate's group, not looked at without GROUPED
  __device__ __forceinline__ void insert(double cv, I ci, int cg, int lane, int depth) {
    const bool less = bd < cv || (bd == cv && bi < ci);
    const int pos = __popcll(__ballot(less));              // <= depth - 1: the candidate is before the depth-th
    if constexpr (GROUPED) {
      const unsigned long long held = __ballot(bi != EMPTY && this->bg == cg);
      const int p_old = held ? __ffsll((long long)held) - 1 : 63;
      if (p_old < pos) return;                             // the lanes below pos are the entries before the candidate (wave-uniform)
      const double ud = __shfl_up(bd, 1, 64);
      const I ui = __shfl_up(bi, 1, 64);
      const int ug = __shfl_up(this->bg, 1, 64);
      if (lane > pos && lane <= p_old) { bd = ud; bi = ui; this->bg = ug; }
      if (lane == pos) { bd = cv; bi = ci; this->bg = cg; }
    } else {
      const double ud = __shfl_up(bd, 1, 64);
      const I ui = __shfl_up(bi, 1, 64);
      if (lane > pos) { bd = ud; bi = ui; }
      if (lane == pos) { bd = cv; bi = ci; }
    }
    tau = uniform_f64(__shfl(bd, depth - 1, 64));
    tau_i = uniform_of(__shfl(bi, depth - 1, 64));
  }
  __device__ __forceinline__ void offer(double cv, I ci, int cg, int lane, int depth) {
    if (beats(cv, ci)) insert(cv, ci, cg, lane, depth);
  }
};

// Merges the sorted lists list0, list0 + stride, ... < nlists into wl, 64 lists at a time: lane l follows list l0 + l entry by entry
// (src.get<grouped>(list, e, cv, ci, cg): the entry, cv = +inf for an empty one, cg its group for a grouped list) and drops out at the
// first entry that does not beat the current depth-th -- the rest of a sorted list cannot either.  The entries that do are offered one
// by one; an entry that beats the depth-th but whose group a better entry holds is dropped by the insertion and the lane goes on.
template <typename List, typename Src>
__device__ __forceinline__ void merge_lists(List &wl, Src src, int nlists, int list0, int stride, int depth, int lane) {
  for (int l0 = list0; l0 < nlists; l0 += stride) {       // wave-uniform
    const int l = l0 + lane;
    bool alive = l < nlists;
    for (int e = 0; e < depth; ++e) {
      double cv = INFINITY;
      long long ci = EMPTY_ID;
      int cg = 0;
      if (alive) src.template get<List::grouped>(l, e, cv, ci, cg);
      alive = alive && wl.beats(cv, ci);
      unsigned long long m = __ballot(alive);
      if (!m) break;
      while (m) {
        const int from = __ffsll((long long)m) - 1;
        m &= m - 1;
        if constexpr (List::grouped) wl.offer(__shfl(cv, from, 64), __shfl(ci, from, 64), __shfl(cg, from, 64), lane, depth);
        else wl.offer(__shfl(cv, from, 64), __shfl(ci, from, 64), 0, lane, depth);
      }
    }
  }
}

// The three places lists are read from.  Each carries the entries' groups (g / sg), which only get<true> reads.
// the lists the scan's workgroups wrote: [query][entry][list], so that the 64 lanes of a merge step read neighbours
struct ScanLists {
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
// the caller's partial lists [part][query][depth]; an entry with a negative id is empty
struct PartLists {
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
// the four waves' lists of a workgroup in the LDS: sd / si / sg [4][64].  I: how the index is kept there (below).
template <typename I>
struct LdsLists {
  const double *sd;
  const I *si;
  const int *sg;
  template <bool GROUPED>
  __device__ __forceinline__ void get(int l, int e, double &cv, long long &ci, int &cg) const {
    cv = sd[l * 64 + e];
    ci = si[l * 64 + e];                                   // an empty entry's distance is +inf: it is never offered
    if constexpr (GROUPED) cg = sg[l * 64 + e];
  }
};

// LDS of the scan: the query tile, then (re-used) the waves' lists of the tile's queries, 16 bytes an entry
constexpr size_t scan_lds_bytes(int nq_tile, int d) {
  const size_t tile = (size_t)nq_tile * d * sizeof(float), lists = (size_t)nq_tile * 4 * 64 * (sizeof(double) + sizeof(long long));
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
template <typename G, int NQ, int NR, bool MASKED, bool GROUPED, bool AFTER, bool EXCL>
__global__ __launch_bounds__(256) void scan_kernel(const G *__restrict__ gallery, const float *__restrict__ queries, const unsigned *__restrict__ live,
                                                   const int *__restrict__ groups, const double *__restrict__ after_d,
                                                   const int64_t *__restrict__ after_i, int64_t id_base, const int64_t *__restrict__ exclude,
                                                   const unsigned *__restrict__ ban, int n_grp, int ng, int nq, int d, int depth,
                                                   double *__restrict__ part_d, int *__restrict__ part_i, int *__restrict__ part_g,
                                                   int *__restrict__ nonfinite) {
  static_assert(!(AFTER && GROUPED) || EXCL, "the grouped scan with a cursor is the page scan: it carries the (nullable) excluded group");
  static_assert(!EXCL || AFTER || GROUPED, "the excluding scans: the cursor scan, the grouped scan, or both (the page scan)");
  constexpr bool PAGE = GROUPED && AFTER;
  extern __shared__ float4 smem4[];
  const float *qt = reinterpret_cast<const float *>(smem4);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q0 = blockIdx.y * NQ;
  const unsigned dead = load_query_tile<NQ>(queries, q0, nq, d, smem4, nonfinite);      // bit u: query q0 + u takes no candidates

  SortedList<int, EMPTY_ROW, GROUPED> wl[NQ];
#pragma unroll
  for (int u = 0; u < NQ; ++u) wl[u].init();
  bool gallery_bad = false;
  [[maybe_unused]] double cd[NQ];                          // the cursors of the tile's queries (AFTER)
  [[maybe_unused]] int cr[NQ];
  if constexpr (AFTER) load_cursors<NQ, EXCL>(after_d, after_i, id_base, ng, q0, nq, cd, cr);
  [[maybe_unused]] std::conditional_t<GROUPED, long long, int> ex[NQ];      // the excluded group / local row of the tile's queries (EXCL)
  if constexpr (EXCL) {
#pragma unroll
    for (int u = 0; u < NQ; ++u) {
      long long e;
      if constexpr (PAGE) e = exclude ? uniform_of((long long)exclude[min(q0 + u, nq - 1)]) : INT64_MIN;      // null: no group
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
        for (int u = 0; u < NQ; ++u) {
          const double cv = dist[u * NR + r];
          if (!(cv < INFINITY)) gallery_bad = true;
          else if (!((dead >> u) & 1) && wl[u].beats(cv, jj[r])) {
            if constexpr (AFTER) {
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
  double *sd = reinterpret_cast<double *>(smem4);          // [NQ][4][64]
  LdsIndex *si = reinterpret_cast<LdsIndex *>(sd + NQ * 4 * 64);
  [[maybe_unused]] int *sg = reinterpret_cast<int *>(si) + NQ * 4 * 64;      // GROUPED: after the int rows
#pragma unroll
  for (int u = 0; u < NQ; ++u) {
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
  const int nlists = gridDim.x;
  for (int u = wave; u < NQ; u += 4) {
    if (q0 + u >= nq) break;
    SortedList<long long, EMPTY_ID, GROUPED> m;
    m.init();
    merge_lists(m, LdsLists<LdsIndex>{sd + u * 4 * 64, si + u * 4 * 64, GROUPED ? sg + u * 4 * 64 : nullptr}, 4, 0, 64, depth, lane);
    if (lane < depth) {
      const size_t o = ((size_t)(q0 + u) * depth + lane) * nlists + blockIdx.x;
      part_d[o] = m.bd;
      part_i[o] = m.bi == EMPTY_ID ? EMPTY_ROW : (int)m.bi;
      if constexpr (GROUPED) part_g[o] = m.bg;
    }
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
  if (lane < depth) {
    const size_t o = (size_t)q * depth + lane;
    const bool empty = wl.bi == EMPTY_ID;
    ids[o] = empty ? -1 : id_base + wl.bi;
    if constexpr (GROUPED) out_groups[o] = empty ? -1 : wl.bg;
    if (dists) dists[o] = empty ? INFINITY : (float)wl.bd;
    if (dists64) dists64[o] = empty ? (double)INFINITY : wl.bd;
  }
}

// words[w] bit b = (flags[32 w + b] != 0) & and_mask[w] bit b: a thread per row, a ballot per wave -- 64 rows, two words, written by
// two lanes.  A row past n_rows votes 0, so the tail bits are 0.
__global__ __launch_bounds__(256) void row_mask_pack_kernel(const uint8_t *__restrict__ flags, int n_rows, const unsigned *__restrict__ and_mask,
                                                            unsigned *__restrict__ words) {
  const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const unsigned long long m = __ballot(row < n_rows && flags[row] != 0);
  const long long w = (row >> 6) * 2 + lane;               // lanes 0 and 1: the wave's two words
  if (lane < 2 && w < ((long long)n_rows + 31) / 32) {
    unsigned v = (unsigned)(m >> (32 * lane));
    if (and_mask) v &= and_mask[w];
    words[w] = v;
  }
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
SearchWs search_ws(void *ws, int ng, int nq, int depth, bool grouped) {
  Bump b(ws);
  SearchWs s;
  const size_t entries = (size_t)nq * depth;
  s.dists64 = (double *)b.take(entries * sizeof(double));            // FIRST: the documented region of the header
  s.part_d = (double *)b.take(entries * search_max_lists(ng) * sizeof(double));
  s.part_i = (int *)b.take(entries * search_max_lists(ng) * sizeof(int));
  s.part_g = grouped ? (int *)b.take(entries * search_max_lists(ng) * sizeof(int)) : nullptr;
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
template <typename G, int NQ, int NR, bool MASKED, bool GROUPED, bool AFTER, bool EXCL>
int launch_scan(const ScanArgs &a, int tiles, hipStream_t stream) {
  // resident workgroups per CU: a property of the instantiation, its LDS (d / 64 = 1 .. 32) and the device -- asked once, as num_cus() is
  static std::atomic<int> resident[64][SEARCH_MAX_D / 64];
  const size_t lds = scan_lds_bytes(NQ, a.d);
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  std::atomic<int> &slot = resident[dev][a.d / 64 - 1];
  int per_cu = slot.load(std::memory_order_relaxed);
  if (per_cu == 0) {
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, scan_kernel<G, NQ, NR, false, false, false, false>, 256, lds) != hipSuccess || per_cu < 1)
      per_cu = 1;
    if constexpr (MASKED || GROUPED || AFTER || EXCL) {
      int own = per_cu;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&own, scan_kernel<G, NQ, NR, MASKED, GROUPED, AFTER, EXCL>, 256, lds) == hipSuccess && own >= 1)
        per_cu = std::min(per_cu, own);
    }
    slot.store(per_cu, std::memory_order_relaxed);
  }
  const long long n_steps = ((long long)a.ng + NR - 1) / NR;
  const int blocks = (int)std::min<long long>(std::min(search_max_lists(a.ng), std::min(per_cu, 4) * vtcgemm::num_cus()), (n_steps + 3) / 4);
  hipLaunchKernelGGL((scan_kernel<G, NQ, NR, MASKED, GROUPED, AFTER, EXCL>), dim3(blocks, tiles), dim3(256), lds, stream,
                     static_cast<const G *>(a.gallery), a.queries, a.live, a.groups, a.after_d, a.after_i, a.id_base, a.exclude, a.ban, a.n_grp, a.ng, a.nq,
                     a.d, a.depth, a.part_d, a.part_i, a.part_g, a.nonfinite);
  return blocks;
}
// The one place a call's arguments choose an instantiation: the tile of its query count, MASKED by `live`, and the mode by which of the
// groups, the cursor, the excluded keys and the ban bitmap it has.  Returns the grid's x.
template <typename G>
int launch_scan_of(const ScanArgs &a, hipStream_t stream) {
  const TilePlan p = tile_plan(a.nq);
  auto mode = [&](auto grouped, auto after, auto excl) {
    return with_tile(p, [&](auto tq, auto tr) {
      constexpr int NQ = decltype(tq)::value, NR = decltype(tr)::value;
      constexpr bool GROUPED = decltype(grouped)::value, AFTER = decltype(after)::value, EXCL = decltype(excl)::value;
      return a.live ? launch_scan<G, NQ, NR, true, GROUPED, AFTER, EXCL>(a, p.tiles, stream)
                    : launch_scan<G, NQ, NR, false, GROUPED, AFTER, EXCL>(a, p.tiles, stream);
    });
  };
  constexpr std::true_type yes{};
  constexpr std::false_type no{};
  if (a.ban) return mode(yes, yes, yes);                           // the page scan
  if (a.groups) return a.exclude ? mode(yes, no, yes) : mode(yes, no, no);
  if (a.exclude) return mode(no, yes, yes);                        // the cursor scan with an excluded row; a.after_d may be null
  return a.after_d ? mode(no, yes, no) : mode(no, no, no);
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
// max_q = 0: any number of queries.  n_groups / depth null: the entry has none.
int check_shape(const char *name, int ng, int nq, int max_q, const char *nq_hint, const int *n_groups, const int *depth, int d, int64_t id_base) {
  VTC_CHECK(ng >= 1, "%s: n_gallery=%d must be at least 1", name, ng);
  if (max_q) VTC_CHECK(nq >= 1 && nq <= max_q, "%s: n_queries=%d must be in [1, %d]%s", name, nq, max_q, nq_hint);
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
};
int check_search_call(const char *name, const SearchCall &c) {
  VTC_CHECK(c.gallery && c.queries && c.ids && (!c.groups || c.out_groups) && c.given, "%s: null argument", name);
  VTC_CHECK(!c.after_d == !c.after_i, "%s: after_d and after_i are given together or not at all", name);
  VTC_CHECK(!(c.groups && c.after_d) || c.ban, "%s: the grouped search has no cursor (after_d / after_i with groups)", name);
  if (check_shape(name, c.ng, c.nq, SEARCH_MAX_Q, c.nq_hint, c.ban ? &c.n_groups : nullptr, &c.depth, c.d, c.id_base)) return 1;
  const size_t need = search_ws(nullptr, c.ng, c.nq, c.depth, c.groups != nullptr).total;
  VTC_CHECK(c.ws && c.ws_bytes >= need, "%s: workspace too small (%zu < %zu)", name, c.ws_bytes, need);
  return 0;
}
// The scan of the call's mode, then the merge of the workgroups' lists -- grouped when the call is.
template <typename G>
int run_search(const char *name, const SearchCall &c) {
  hipStream_t stream = (hipStream_t)c.stream;
  const SearchWs s = search_ws(c.ws, c.ng, c.nq, c.depth, c.groups != nullptr);
  const ScanArgs a{c.gallery, c.queries, c.live, c.groups, c.after_d, c.after_i, c.id_base, c.exclude, c.ban, c.n_groups,
                   c.ng,      c.nq,      c.d,    c.depth,  s.part_d,  s.part_i,  s.part_g,  c.nonfinite};
  const int blocks = launch_scan_of<G>(a, stream);
  VTC_LAUNCH_CHECK2(name, "scan");
  const ScanLists lists{s.part_d, s.part_i, s.part_g, blocks, c.depth, 0};
  if (c.groups)
    hipLaunchKernelGGL((merge_kernel<ScanLists, true>), dim3(c.nq), dim3(256), 0, stream, lists, blocks, c.depth, c.id_base, c.ids, c.out_groups,
                       c.dists, s.dists64);
  else
    hipLaunchKernelGGL((merge_kernel<ScanLists, false>), dim3(c.nq), dim3(256), 0, stream, lists, blocks, c.depth, c.id_base, c.ids,
                       (int32_t *)nullptr, c.dists, s.dists64);
  VTC_LAUNCH_CHECK2(name, "merge");
  return 0;
}
int search_entry(const char *name, const SearchCall &c) {
  if (check_search_call(name, c)) return 1;
  return c.half ? run_search<_Float16>(name, c) : run_search<float>(name, c);
}

int merge_parts(const char *name, const int64_t *ids_parts, const double *dists_parts, const int32_t *groups_parts, int n_parts, int nq, int depth,
                int64_t *ids, int32_t *out_groups, float *dists, void *stream) {
  VTC_CHECK(n_parts >= 1 && n_parts <= SEARCH_MAX_PARTS, "%s: n_parts=%d must be in [1, %d]", name, n_parts, SEARCH_MAX_PARTS);
  VTC_CHECK(nq >= 1 && nq <= SEARCH_MAX_Q, "%s: n_queries=%d must be in [1, %d]", name, nq, SEARCH_MAX_Q);
  VTC_CHECK(depth >= 1 && depth <= SEARCH_MAX_DEPTH, "%s: depth=%d must be in [1, %d]", name, depth, SEARCH_MAX_DEPTH);
  const PartLists lists{dists_parts, ids_parts, groups_parts, nq, depth, 0};
  if (groups_parts)
    hipLaunchKernelGGL((merge_kernel<PartLists, true>), dim3(nq), dim3(256), 0, (hipStream_t)stream, lists, n_parts, depth, (int64_t)0, ids,
                       out_groups, dists, (double *)nullptr);
  else
    hipLaunchKernelGGL((merge_kernel<PartLists, false>), dim3(nq), dim3(256), 0, (hipStream_t)stream, lists, n_parts, depth, (int64_t)0, ids,
                       (int32_t *)nullptr, dists, (double *)nullptr);
  VTC_LAUNCH_CHECK(name);
  return 0;
}
}  // namespace

extern "C" size_t vtc_l2_search_workspace_bytes(int n_gallery, int n_queries, int d, int depth) {
  if (!search_args_ok(n_gallery, n_queries, d, depth)) return 0;
  return search_ws(nullptr, n_gallery, n_queries, depth, false).total;
}

extern "C" size_t vtc_l2_search_grouped_workspace_bytes(int n_gallery, int n_queries, int d, int depth) {
  if (!search_args_ok(n_gallery, n_queries, d, depth)) return 0;
  return search_ws(nullptr, n_gallery, n_queries, depth, true).total;
}

extern "C" size_t vtc_l2_group_ban_words(int n_queries, int n_groups) {
  if (n_queries < 1 || n_queries > SEARCH_MAX_Q || n_groups < 1) return 0;
  return (size_t)n_queries * (((size_t)n_groups + 31) / 32);
}

extern "C" int vtc_l2_search_masked(const float *gallery, const float *queries, const uint32_t *live, int ng, int nq, int d, int depth,
                                    int64_t id_base, int64_t *ids, float *dists, int *nonfinite, void *ws, size_t ws_bytes, void *stream) {
  return search_entry("l2_search", {gallery, false, queries, live, nullptr, nullptr, nullptr, nullptr, nullptr, 0, ng, nq, d, depth, id_base, ids,
                              nullptr, dists, nonfinite, ws, ws_bytes, stream, true, " (more queries: vtc_l2_topk)"});
}

extern "C" int vtc_l2_search(const float *gallery, const float *queries, int ng, int nq, int d, int depth, int64_t id_base, int64_t *ids,
                             float *dists, int *nonfinite, void *ws, size_t ws_bytes, void *stream) {
  return vtc_l2_search_masked(gallery, queries, nullptr, ng, nq, d, depth, id_base, ids, dists, nonfinite, ws, ws_bytes, stream);
}

extern "C" int vtc_l2_search_grouped(const float *gallery, const float *queries, const uint32_t *live, const int32_t *groups, int ng, int nq, int d,
                                     int depth, int64_t id_base, int64_t *ids, int32_t *out_groups, float *dists, int *nonfinite, void *ws,
                                     size_t ws_bytes, void *stream) {
  return search_entry("l2_search_grouped", {gallery, false, queries, live, groups, nullptr, nullptr, nullptr, nullptr, 0, ng, nq, d, depth, id_base, ids,
                                      out_groups, dists, nonfinite, ws, ws_bytes, stream, groups && out_groups});
}

extern "C" int vtc_l2_search_half(const uint16_t *gallery, const float *queries, const uint32_t *live, const int32_t *groups, int ng, int nq, int d,
                                  int depth, int64_t id_base, int64_t *ids, int32_t *out_groups, float *dists, int *nonfinite, void *ws,
                                  size_t ws_bytes, void *stream) {
  return search_entry("l2_search_half", {gallery, true, queries, live, groups, nullptr, nullptr, nullptr, nullptr, 0, ng, nq, d, depth, id_base, ids,
                                   out_groups, dists, nonfinite, ws, ws_bytes, stream, true});
}

extern "C" int vtc_l2_search_after(const void *gallery, int gallery_is_half, const float *queries, const uint32_t *live, const double *after_d,
                                   const int64_t *after_i, int ng, int nq, int d, int depth, int64_t id_base, int64_t *ids, float *dists,
                                   int *nonfinite, void *ws, size_t ws_bytes, void *stream) {
  return search_entry("l2_search_after", {gallery, gallery_is_half != 0, queries, live, nullptr, after_d, after_i, nullptr, nullptr, 0, ng, nq, d, depth,
                                    id_base, ids, nullptr, dists, nonfinite, ws, ws_bytes, stream, after_d && after_i});
}

extern "C" int vtc_l2_search_excluding(const void *gallery, int gallery_is_half, const float *queries, const uint32_t *live, const int32_t *groups,
                                       const int64_t *exclude, const double *after_d, const int64_t *after_i, int ng, int nq, int d, int depth,
                                       int64_t id_base, int64_t *ids, int32_t *out_groups, float *dists, int *nonfinite, void *ws,
                                       size_t ws_bytes, void *stream) {
  return search_entry("l2_search_excluding", {gallery, gallery_is_half != 0, queries, live, groups, after_d, after_i, exclude, nullptr, 0, ng, nq, d,
                                        depth, id_base, ids, out_groups, dists, nonfinite, ws, ws_bytes, stream, exclude != nullptr});
}

extern "C" int vtc_l2_search_grouped_after(const void *gallery, int gallery_is_half, const float *queries, const uint32_t *live,
                                           const int32_t *groups, int n_groups, const uint32_t *ban, const int64_t *exclude, const double *after_d,
                                           const int64_t *after_i, int ng, int nq, int d, int depth, int64_t id_base, int64_t *ids,
                                           int32_t *out_groups, float *dists, int *nonfinite, void *ws, size_t ws_bytes, void *stream) {
  return search_entry("l2_search_grouped_after",
                {gallery, gallery_is_half != 0, queries, live, groups, after_d, after_i, exclude, ban, n_groups, ng, nq, d, depth, id_base, ids, out_groups,
                 dists, nonfinite, ws, ws_bytes, stream, groups && ban && after_d && after_i && out_groups});
}

extern "C" int vtc_l2_group_mark_before(const void *gallery, int gallery_is_half, const float *queries, const uint32_t *live, const int32_t *groups,
                                        int n_groups, const double *after_d, const int64_t *after_i, int ng, int nq, int d, int64_t id_base,
                                        uint32_t *ban, void *stream) {
  const char *name = "l2_group_mark_before (the grouped search's cursor)";
  VTC_CHECK(gallery && queries && groups && after_d && after_i && ban, "%s: null argument", name);
  if (check_shape(name, ng, nq, SEARCH_MAX_Q, "", &n_groups, nullptr, d, id_base)) return 1;
  const ScanArgs a{gallery, queries, live, groups, after_d, after_i, id_base, nullptr, nullptr, n_groups, ng, nq, d, 0, nullptr, nullptr, nullptr, nullptr};
  if (gallery_is_half) launch_mark_of<_Float16>(a, ban, (hipStream_t)stream);
  else launch_mark_of<float>(a, ban, (hipStream_t)stream);
  VTC_LAUNCH_CHECK("l2_group_mark_before");
  return 0;
}

extern "C" int vtc_l2_pair_dists64(const void *gallery, int gallery_is_half, const float *queries, const int64_t *rows, int ng, int nq, int d,
                                   int64_t id_base, double *out, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const char *name = "l2_pair_dists64 (the search's cursor distances)";
  VTC_CHECK(gallery && queries && rows && out, "%s: null argument", name);
  if (check_shape(name, ng, nq, 0, "", nullptr, nullptr, d, id_base)) return 1;
  if (gallery_is_half)
    hipLaunchKernelGGL(pair_dists64_kernel<_Float16>, dim3(cdiv(nq, 4)), dim3(256), 0, stream, reinterpret_cast<const _Float16 *>(gallery), queries,
                       rows, ng, nq, d, id_base, out);
  else
    hipLaunchKernelGGL(pair_dists64_kernel<float>, dim3(cdiv(nq, 4)), dim3(256), 0, stream, reinterpret_cast<const float *>(gallery), queries, rows,
                       ng, nq, d, id_base, out);
  VTC_LAUNCH_CHECK("l2_pair_dists64");
  return 0;
}

extern "C" int vtc_l2_search_merge(const int64_t *ids_parts, const double *dists_parts, int n_parts, int nq, int depth, int64_t *ids,
                                   float *dists, void *stream) {
  VTC_CHECK(ids_parts && dists_parts && ids, "l2_search_merge: null argument");
  return merge_parts("l2_search_merge", ids_parts, dists_parts, nullptr, n_parts, nq, depth, ids, nullptr, dists, stream);
}

extern "C" int vtc_l2_search_merge_grouped(const int64_t *ids_parts, const double *dists_parts, const int32_t *groups_parts, int n_parts, int nq,
                                           int depth, int64_t *ids, int32_t *out_groups, float *dists, void *stream) {
  VTC_CHECK(ids_parts && dists_parts && groups_parts && ids && out_groups, "l2_search_merge_grouped: null argument");
  return merge_parts("l2_search_merge_grouped", ids_parts, dists_parts, groups_parts, n_parts, nq, depth, ids, out_groups, dists, stream);
}

extern "C" int vtc_row_mask_pack(const uint8_t *flags, int n_rows, const uint32_t *and_mask, uint32_t *words, void *stream) {
  VTC_CHECK(flags && words, "row_mask_pack (the search's row mask): null argument");
  VTC_CHECK(n_rows >= 1, "row_mask_pack (the search's row mask): n_rows=%d must be at least 1", n_rows);
  hipLaunchKernelGGL(row_mask_pack_kernel, dim3(cdiv(n_rows, 256)), dim3(256), 0, (hipStream_t)stream, flags, n_rows, and_mask, words);
  VTC_LAUNCH_CHECK("row_mask_pack");
  return 0;
}
