// search.hip -- query-time search: the exact top-`depth` of a FEW queries (1 .. 64) over a stored gallery, vtc_l2_search, and the merge of
// such lists over disjoint gallery windows, vtc_l2_search_merge; vtc_l2_search_masked is the same scan over the rows whose bit of a row
// mask is set (a deleted row, a query that searches a subset), vtc_row_mask_pack packs such a mask.  The N x N sweeps (sweep_topk.hip) split the gallery into bf16 operand
// planes, run a distance GEMM, select, and settle the result in fp64; at a handful of queries all of that is overhead.  Here the gallery
// is streamed ONCE per tile of queries and the fp64 distances of sweep_common.h are formed directly: exact by construction, so there are
// no candidate lists, error bounds or certification, and nothing of the gallery is written.
//
//   search_scan_kernel<NQ, NR, MASKED>
//                                a grid of persistent workgroups; the tile of NQ queries lives in the LDS for the whole scan; each wave
//                                takes groups of NR gallery rows round-robin (NQ x NR distances per step, all their loads in flight together)
//                                and keeps one sorted (fp64 distance, row) list per query, an entry per lane.  The list's last key is held in
//                                scalar registers: a row that is not closer than the current depth-th costs one compare.  The four waves'
//                                lists are merged in the LDS; a workgroup writes ONE list per query to the workspace.
//   merge_kernel<Src>            one workgroup per query merges the workgroups' lists (Src = ScanLists) or the caller's partial lists
//                                (Src = PartLists): the lists are sorted, so a lane follows one list and leaves at its first entry that
//                                does not beat the current depth-th.
//
// vtc_l2_search_grouped / vtc_l2_search_merge_grouped: several rows per video, and the `depth` nearest distinct VIDEOS come back.  Every
// row has a group id (int32, any value, rows of a group anywhere).  Take the complete list of live rows with a finite distance, sorted by
// (distance, row); delete every row that is not the first of its group in that order; the first `depth` of what remains are the result
// (include/vtc_hip.h) -- the group minimum E(u, v) of the video-unit ranks, at query time.  The de-duplication happens INSIDE the lists:
//
//   search_grouped_scan_kernel<NQ, NR, MASKED>
//                                the same scan (one body, scan_body<NQ, NR, MASKED, GROUPED>; GROUPED = false is search_scan_kernel, whose
//                                name and parameters stay what they were) with GroupLists: one more int per entry, and an insertion that
//                                drops a candidate whose group holds a better entry and otherwise lets the group's old entry be the one
//                                that leaves.  A row that does not beat the depth-th still costs the one compare.  A third part array
//                                (part_g) carries the groups to the merge; the grid is the ungrouped scan's.
//   merge_grouped_kernel<Src>    merge_kernel with GroupLists, for the workgroups' lists (ScanGroupLists) and the caller's (PartGroupLists).
//
// vtc_l2_search_half: the masked / grouped search over a gallery stored as IEEE binary16.  half_scan_kernel / half_scan_grouped_kernel
// are scan_body with the gallery's element type _Float16: the row loader (sweep_common.h, row_piece) reads 8 bytes a lane where the
// fp32 scan reads 16 and widens them exactly, every lane keeps its columns, and the same statements form the same fp64 bits as the
// fp32 scan over the widened rows.  The workspace, the lists and both merges do not know how the gallery is stored.
//
// vtc_l2_search_after: the `depth` nearest rows strictly AFTER a cursor key (D*, row*) of the search order, per query -- the next page of
// a search, to any depth, by chaining each page's last key.  search_after_scan_kernel / half_after_scan_kernel are scan_body with AFTER:
// a row that has passed `beats` is offered only if its key lies after the query's cursor (one compare pair, in scalar registers like the
// depth-th key), so the rejecting path of the steady state is the one compare it was.  The lists and merge_kernel<ScanLists> do not
// care which rows were admitted.  The cursor's distance has to carry the bits the scan compares: it is the fp64 value of an earlier
// search's workspace, or vtc_l2_pair_dists64's (pair_dists64_kernel, one wave per query through the same wave_dist64_core).
//
// vtc_l2_search_excluding: every query names ONE row (ungrouped) or one group (grouped) that it is never offered -- "more like this"
// without the row itself, hard negatives without the text's own video, for a whole tile of queries in the one gallery pass.
// excluding_scan_kernel / excluding_grouped_scan_kernel are scan_body with EXCL: the query's excluded key in scalar registers, compared
// after `beats` (and after the cursor) with the row or with the row's group, so the rejecting path stays the one compare.  Deleting a
// row -- or every row of a group, BEFORE the lists de-duplicate -- from the candidates is deleting it from the order: the lists, both
// merges and the window merges stay what they are.  The ungrouped kernel is the cursor scan with EXCL (a null cursor is -inf, the plain
// search), so an exclusion pages like any search.
//
// vtc_l2_group_mark_before / vtc_l2_search_grouped_after: the next page of the GROUPED order -- the `depth` nearest distinct videos whose
// nearest admissible row lies strictly after a cursor key.  One scan cannot decide that: a row after the cursor counts only if no row of
// its group lies at or before the cursor, and such a row may be in any wave's share.  Two passes and a per-query bitmap of groups can:
// videos_page_mark_kernel walks the gallery as the scan does and ORs bit groups[row] of ban[q] for every live row with a finite distance
// at or before q's cursor (no lists, no merge); videos_page_scan_kernel is scan_body with GROUPED, AFTER and EXCL, which drops a row whose
// group's bit is set -- one more test on the insertion path, after `beats`, the cursor and the excluded group (nullable here).  Banned
// groups are deleted from the candidates before the lists de-duplicate, as an excluded group is, so the argument below holds unchanged.
// The groups of these two entries are DENSE, [0, n_groups): the bitmap is indexed by them.
//
// Why merging de-duplicated lists is exact, for the waves' lists in the LDS, the workgroups' lists and the caller's windows alike: a
// group of the union's first `depth` has its overall nearest row in some part.  In that part fewer than `depth` groups have a smaller
// local minimum (a local minimum is not below the overall one of its group, and fewer than `depth` groups are nearer overall), so that
// part's list holds the entry.  The stale, worse entries of the same group from other parts are absorbed by the insertion: whichever
// comes first, the better one stays.  The early exit of merge_lists stays valid -- the depth-th key only falls, so a lane may leave its
// sorted list at the first entry that does not beat it; an entry that beats it but whose group a better entry holds is dropped and the
// lane goes on.
#include "sweep_common.h"

#include <algorithm>
#include <type_traits>

namespace {
using namespace vtcsweep;

constexpr int SEARCH_MAX_Q = 64, SEARCH_MAX_DEPTH = 64, SEARCH_MAX_D = 2048, SEARCH_MAX_PARTS = 64;
constexpr int SEARCH_MAX_BLOCKS = 1024;       // workgroups of a scan (4 per CU on a 256-CU part): the number of lists per query in the workspace
constexpr int EMPTY_ROW = 0x7fffffff;         // index of an empty list slot (distance +inf)
constexpr long long EMPTY_ID = 0x7fffffffffffffffll;

__device__ __forceinline__ double uniform_f64(double v) {      // a wave-uniform value -> scalar registers
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}
__device__ __forceinline__ int uniform_of(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ long long uniform_of(long long v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(unsigned long long)v);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)v >> 32));
  return (long long)(((unsigned long long)hi << 32) | lo);
}

// A sorted list of (fp64 distance, index) keys, one entry per lane, ascending; the first `depth` lanes are the list, (tau, tau_i) its last
// key, wave-uniform.  Empty slots hold (+inf, EMPTY).  The insertion is exact_fallback_kernel's `offer` (sweep_topk.hip).
template <typename I>
struct WaveList {
  static constexpr bool grouped = false;
  double bd, tau;
  I bi, tau_i;
  __device__ __forceinline__ void init(I empty) {
    bd = tau = INFINITY;
    bi = tau_i = empty;
  }
  // wave-uniform candidate: is it finite and before the depth-th entry?
  __device__ __forceinline__ bool beats(double cv, I ci) const { return cv < INFINITY && (cv < tau || (cv == tau && ci < tau_i)); }
  __device__ __forceinline__ void insert(double cv, I ci, int lane, int depth) {
    const bool less = bd < cv || (bd == cv && bi < ci);
    const int pos = __popcll(__ballot(less));
    const double ud = __shfl_up(bd, 1, 64);
    const I ui = __shfl_up(bi, 1, 64);
    if (lane > pos) { bd = ud; bi = ui; }
    if (lane == pos) { bd = cv; bi = ci; }
    tau = uniform_f64(__shfl(bd, depth - 1, 64));
    tau_i = uniform_of(__shfl(bi, depth - 1, 64));
  }
  __device__ __forceinline__ void offer(double cv, I ci, int lane, int depth) {
    if (beats(cv, ci)) insert(cv, ci, lane, depth);
  }
};

// The list of the GROUPED search: every entry carries the group id of its row (bg), and over all 64 lanes -- not only the first `depth`
// -- no two non-empty entries share a group.  An empty slot is known by its index (EMPTY), never by bg: every int is a legal group id.
// A candidate that has passed `beats` meets the lane p_old that holds its group, if any (one more ballot):
//   that entry is before the candidate         -> the candidate is dropped;
//   otherwise, with pos the candidate's place  -> the lanes (pos, p_old] take their left neighbour's entry, lane pos the candidate, the
//                                                 lanes above p_old keep theirs: the group's old entry is the one that leaves;
//   no lane holds the group                    -> p_old = 63, WaveList's shift of everything above pos.
// Entries only ever move towards higher lanes, so what lies past the depth-th never comes back: a row that does not beat the depth-th
// changes nothing of the first `depth`, whether its group is held (by an entry that is then not worse than the depth-th, or by one
// past it) or not -- `beats` is WaveList's one compare.  A group no lane holds has no row so far that was before the depth-th key of
// its time (it would still be held, or has left over lane 63 behind 64 closer groups), and that key only falls: inserting is right.
template <typename I, I EMPTY>
struct GroupList {
  static constexpr bool grouped = true;
  double bd, tau;
  I bi, tau_i;
  int bg;
  __device__ __forceinline__ void init(I) {
    bd = tau = INFINITY;
    bi = tau_i = EMPTY;
    bg = 0;
  }
  __device__ __forceinline__ bool beats(double cv, I ci) const { return cv < INFINITY && (cv < tau || (cv == tau && ci < tau_i)); }
  __device__ __forceinline__ void insert(double cv, I ci, int cg, int lane, int depth) {
    const bool less = bd < cv || (bd == cv && bi < ci);
    const int pos = __popcll(__ballot(less));              // <= depth - 1: the candidate is before the depth-th
    const unsigned long long held = __ballot(bi != EMPTY && bg == cg);
    const int p_old = held ? __ffsll((long long)held) - 1 : 63;
    if (p_old < pos) return;                               // the lanes below pos are the entries before the candidate (wave-uniform)
    const double ud = __shfl_up(bd, 1, 64);
    const I ui = __shfl_up(bi, 1, 64);
    const int ug = __shfl_up(bg, 1, 64);
    if (lane > pos && lane <= p_old) { bd = ud; bi = ui; bg = ug; }
    if (lane == pos) { bd = cv; bi = ci; bg = cg; }
    tau = uniform_f64(__shfl(bd, depth - 1, 64));
    tau_i = uniform_of(__shfl(bi, depth - 1, 64));
  }
  __device__ __forceinline__ void offer(double cv, I ci, int cg, int lane, int depth) {
    if (beats(cv, ci)) insert(cv, ci, cg, lane, depth);
  }
};

// Merges the sorted lists list0, list0 + stride, ... < nlists into wl, 64 lists at a time: lane l follows list l0 + l entry by entry
// (src(list, e, cv, ci): the entry, cv = +inf for an empty one) and drops out at the first entry that does not beat the current
// depth-th -- the rest of a sorted list cannot either.  The entries that do are offered one by one.  For a GroupList the source gives
// the entry's group too (src(list, e, cv, ci, cg)); an entry that beats the depth-th but whose group a better entry holds is dropped
// by the insertion and the lane goes on.
template <typename List, typename Src>
__device__ __forceinline__ void merge_lists(List &wl, Src src, int nlists, int list0, int stride, int depth, int lane) {
  for (int l0 = list0; l0 < nlists; l0 += stride) {       // wave-uniform
    const int l = l0 + lane;
    bool alive = l < nlists;
    for (int e = 0; e < depth; ++e) {
      double cv = INFINITY;
      long long ci = EMPTY_ID;
      [[maybe_unused]] int cg = 0;
      if constexpr (List::grouped) {
        if (alive) src(l, e, cv, ci, cg);
      } else {
        if (alive) src(l, e, cv, ci);
      }
      alive = alive && wl.beats(cv, ci);
      unsigned long long m = __ballot(alive);
      if (!m) break;
      while (m) {
        const int from = __ffsll((long long)m) - 1;
        m &= m - 1;
        if constexpr (List::grouped) wl.offer(__shfl(cv, from, 64), __shfl(ci, from, 64), __shfl(cg, from, 64), lane, depth);
        else wl.offer(__shfl(cv, from, 64), __shfl(ci, from, 64), lane, depth);
      }
    }
  }
}

// the lists the scan's workgroups wrote: [query][entry][list], so that the 64 lanes of a merge step read neighbours
struct ScanLists {
  const double *d;
  const int *i;
  int nlists, depth, q;
  __device__ __forceinline__ void operator()(int l, int e, double &cv, long long &ci) const {
    const size_t o = ((size_t)q * depth + e) * nlists + l;
    cv = d[o];
    ci = i[o];
  }
};
// the caller's partial lists [part][query][depth]; an entry with a negative id is empty
struct PartLists {
  const double *d;
  const int64_t *i;
  int nq, depth, q;
  __device__ __forceinline__ void operator()(int l, int e, double &cv, long long &ci) const {
    const size_t o = ((size_t)l * nq + q) * depth + e;
    ci = i[o];
    cv = ci < 0 ? INFINITY : d[o];
  }
};
// the four waves' lists of a workgroup in the LDS: sd / si [4][64]
struct LdsLists {
  const double *sd;
  const long long *si;
  __device__ __forceinline__ void operator()(int l, int e, double &cv, long long &ci) const {
    cv = sd[l * 64 + e];
    ci = si[l * 64 + e];
  }
};

// the grouped forms of the three: the same places plus the entry's group.  The scan's LDS lists keep the ROW as an int there, so an
// entry takes the 16 bytes it takes without groups and the LDS of a workgroup -- with it the resident workgroups per CU -- is unchanged.
struct ScanGroupLists {
  const double *d;
  const int *i, *g;
  int nlists, depth, q;
  __device__ __forceinline__ void operator()(int l, int e, double &cv, long long &ci, int &cg) const {
    const size_t o = ((size_t)q * depth + e) * nlists + l;
    cv = d[o];
    ci = i[o];
    cg = g[o];
  }
};
struct PartGroupLists {
  const double *d;
  const int64_t *i;
  const int32_t *g;
  int nq, depth, q;
  __device__ __forceinline__ void operator()(int l, int e, double &cv, long long &ci, int &cg) const {
    const size_t o = ((size_t)l * nq + q) * depth + e;
    ci = i[o];
    cv = ci < 0 ? INFINITY : d[o];
    cg = g[o];
  }
};
template <typename I>
struct LdsGroupLists {
  const double *sd;
  const I *si;
  const int *sg;
  __device__ __forceinline__ void operator()(int l, int e, double &cv, long long &ci, int &cg) const {
    cv = sd[l * 64 + e];
    ci = si[l * 64 + e];                                   // an empty entry's distance is +inf: it is never offered
    cg = sg[l * 64 + e];
  }
};

// LDS of the scan: the query tile, then (re-used) the waves' lists of the tile's queries
constexpr size_t scan_lds_bytes(int nq_tile, int d) {
  const size_t tile = (size_t)nq_tile * d * sizeof(float), lists = (size_t)nq_tile * 4 * 64 * (sizeof(double) + sizeof(long long));
  return tile > lists ? tile : lists;
}

// MASKED: only the rows whose bit of `live` is set take part (vtc_l2_search_masked).  A step's NR rows start at a multiple of NR, which
// divides 32: their bits lie in ONE word, and the step -- so the word -- is wave-uniform.  The wave reads the word of its NEXT step while
// it works on this one; a step with no live row issues no gallery load, and in a partly live one a dead slot is pointed at a live row of
// the same step and its results are dropped, exactly as a slot past the gallery is: a dead row's memory is never read.  The mask is only
// read.  Without MASKED `live` is not looked at and the kernel is the scan of vtc_l2_search.
//
// GROUPED: the lists are GroupLists and the workgroup's list of a query goes out with its groups (part_g).  The fast path is the
// ungrouped one: a row's group is needed only once some query's `beats` is true.  It is loaded EAGERLY all the same, every lane reading
// the one address groups[row] with an ordinary load issued BEFORE the step's gallery loads, and moved to a scalar register only inside
// the insertion.  Loads return in order, so when the row's distances are there -- which every step waits for anyway -- the group has
// arrived: the rejecting path never waits on it, and the insertion never pays a memory round trip of its own, which a lazy load would
// cost exactly while a wave fills its lists and every row is inserted.  The price is NR load instructions and NR registers a step.
//
// G: the gallery's element type.  float is the scan of vtc_l2_search*; _Float16 that of vtc_l2_search_half, over rows stored as IEEE
// binary16.  Nothing but the row loader differs (sweep_common.h, row_piece): lane l still keeps the columns 4 l .. 4 l + 3 (+ 256 i),
// loads 8 bytes a piece where the fp32 scan loads 16, widens them exactly and forms the distance with the same statements in the same
// order -- the same fp64 bits as the fp32 scan over the widened rows.  The mask, the groups and the queries in the LDS are untouched.
//
// AFTER: query u of the tile has a cursor (cd[u], cr[u]) -- the fp64 distance after_d[q] and the cursor row after_i[q] as a LOCAL row,
// clamp(after_i[q] - id_base, -1, ng): a cursor row in an earlier window is before every row of this one at an equal distance (-1), one
// in a later window after them (ng).  Both are wave-uniform and live in scalar registers as (tau, tau_i) do.  A row is offered to query
// u only if cv > cd[u] || (cv == cd[u] && row > cr[u]), asked AFTER `beats`: a row that does not beat the depth-th still costs one
// compare.  A NaN cd[u] admits nothing, -inf everything (the plain search), +inf nothing.  Without AFTER the three arguments are not
// looked at and not a statement of the cursor is compiled.
//
// EXCL: query u of the tile has one key it is never offered (vtc_l2_search_excluding) -- ungrouped the LOCAL row ex[u] (exclude[q] -
// id_base inside the window, else -1, which no row is), grouped the group ex[u] as an int64 (a value outside int32 is no group: every
// int32, -1 included, is a legal one).  Wave-uniform, in scalar registers like the cursor, and asked after `beats` and after the cursor:
// the rejecting path of the steady state stays the one compare.  The ungrouped excluding scan is always a cursor scan (AFTER): a null
// after_d is the cursor -inf, the plain search, so there is one excluding kernel where the plain and the cursor scan are two.  Without
// EXCL `exclude` is not looked at and not a statement of it is compiled.
//
// GROUPED && AFTER (with EXCL): the PAGE scan of vtc_l2_search_grouped_after.  The grouped order has no cursor a row could be asked
// about by itself: a row after the cursor belongs on the page only if NO admissible row of its group lies at or before the cursor, and
// such a row can be in any wave's share.  So a pass before this one (videos_page_mark_kernel) has set bit g of ban[q] for every group g
// with such a row, and a row that has passed `beats`, the cursor compare and the excluded group is dropped when its group's bit is set
// -- one ordinary load of the word on the insertion path only, every lane the one address -- or when its group is outside [0, n_grp),
// which has no bit.  The cursor compare stays although a complete ban implies it: it is scalar and saves the load.  `exclude` may be
// null here (no group: a value outside int32), so there is one page scan where the grouped scan and its excluding form are two.  A
// banned group's rows are deleted from the candidates BEFORE the lists de-duplicate, as an excluded group's are: the lists, the LDS
// layout, the merges and the workspace are what they were.
template <int NQ, int NR, bool MASKED, bool GROUPED, bool AFTER = false, bool EXCL = false, typename G>
__device__ __forceinline__ void scan_body(const G *__restrict__ gallery, const float *__restrict__ queries, const unsigned *__restrict__ live,
                                          const int *__restrict__ groups, int ng, int nq, int d, int depth, double *__restrict__ part_d,
                                          int *__restrict__ part_i, int *__restrict__ part_g, int *__restrict__ nonfinite,
                                          const double *__restrict__ after_d = nullptr, const int64_t *__restrict__ after_i = nullptr,
                                          int64_t id_base = 0, const int64_t *__restrict__ exclude = nullptr,
                                          const unsigned *__restrict__ ban = nullptr, int n_grp = 0) {
  static_assert(!(AFTER && GROUPED) || EXCL, "the grouped scan with a cursor is the page scan: it carries the (nullable) excluded group");
  static_assert(!EXCL || AFTER || GROUPED, "the excluding scans: the cursor scan, the grouped scan, or both (the page scan)");
  extern __shared__ float4 smem4[];
  float *qt = reinterpret_cast<float *>(smem4);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q0 = blockIdx.y * NQ;
  // ---- the query tile -> LDS; a query with a NaN / inf (and a slot past the last query) becomes a row of zeros that is never offered
  // to: every distance formed below then has finite query terms, so it is non-finite exactly when the GALLERY row holds a NaN / inf.
  const int d4 = d >> 2;
  unsigned bad_bits = 0;
  for (int x = tid; x < NQ * d4; x += 256) {
    const int u = x / d4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (q0 + u < nq) v = reinterpret_cast<const float4 *>(queries + (size_t)(q0 + u) * d)[x - u * d4];
    if (!(isfinite(v.x) && isfinite(v.y) && isfinite(v.z) && isfinite(v.w))) bad_bits |= 1u << u;
    smem4[x] = v;
  }
  unsigned dead = 0;                                       // bit u: query q0 + u takes no candidates (uniform for the workgroup)
#pragma unroll
  for (int u = 0; u < NQ; ++u) {
    const int bad = __syncthreads_or((bad_bits >> u) & 1);
    if (bad || q0 + u >= nq) dead |= 1u << u;
    if (bad) {
      for (int x = tid; x < d4; x += 256) smem4[u * d4 + x] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (nonfinite && blockIdx.x == 0 && tid == 0) atomicOr(nonfinite, 2);
    }
  }
  __syncthreads();

  // ---- the scan: wave gw of GW takes the row groups gw, gw + GW, ...: ascending rows, so exact ties keep (distance, row) order
  std::conditional_t<GROUPED, GroupList<int, EMPTY_ROW>, WaveList<int>> wl[NQ];
#pragma unroll
  for (int u = 0; u < NQ; ++u) wl[u].init(EMPTY_ROW);
  bool gallery_bad = false;
  [[maybe_unused]] double cd[NQ];                          // the cursors of the tile's queries (AFTER)
  [[maybe_unused]] int cr[NQ];
  if constexpr (AFTER) {
#pragma unroll
    for (int u = 0; u < NQ; ++u) {
      const int q = min(q0 + u, nq - 1);                   // a slot past the last query is dead: its cursor is never asked
      if constexpr (EXCL) {
        if (!after_d) {                                    // no cursor (uniform for the grid): -inf, the plain search
          cd[u] = -INFINITY;
          cr[u] = -1;
          continue;
        }
      }
      const long long a = after_i[q];
      cd[u] = uniform_f64(after_d[q]);
      cr[u] = uniform_of(a < id_base ? -1 : (int)min(a - id_base, (long long)ng));
    }
  }
  [[maybe_unused]] std::conditional_t<GROUPED, long long, int> ex[NQ];      // the excluded group / local row of the tile's queries (EXCL)
  if constexpr (EXCL) {
#pragma unroll
    for (int u = 0; u < NQ; ++u) {
      long long e;
      if constexpr (GROUPED && AFTER) e = exclude ? uniform_of((long long)exclude[min(q0 + u, nq - 1)]) : INT64_MIN;      // null: no group
      else e = uniform_of((long long)exclude[min(q0 + u, nq - 1)]);
      if constexpr (GROUPED) ex[u] = e;
      else ex[u] = e >= id_base && e - id_base < ng ? (int)(e - id_base) : -1;      // jj[r] is a row of the window: never -1
    }
  }
  [[maybe_unused]] const size_t ban_words = ((size_t)(unsigned)n_grp + 31) >> 5;      // words of a query's row of `ban` (PAGE)
  const long long n_groups = ((long long)ng + NR - 1) / NR, GW = (long long)gridDim.x * 4;
  // The mask word of step s's rows, as loaded: every lane reads the same address with an ordinary (vector) load, which returns in order
  // -- requested a step ahead, before that step's gallery rows, it has arrived by the time they have and is never waited for on its own.
  auto live_word = [&](long long s) -> unsigned { return live[(s * NR) >> 5]; };
  // bit r: row s * NR + r is live and inside the gallery (wave-uniform, moved to a scalar register only here, where it is used)
  auto live_bits = [&](long long s, unsigned word) -> unsigned {
    const int j0 = (int)(s * NR), left = ng - j0;          // s < n_groups: j0 < ng, left >= 1
    const unsigned inside = NR == 1 || left >= NR ? (1u << NR) - 1 : (1u << left) - 1;
    return (unsigned)uniform_of((int)((word >> (j0 & 31)) & inside));
  };
  long long s = (long long)blockIdx.x * 4 + wave;
  unsigned next_word = 0;
  if constexpr (MASKED) {
    if (s < n_groups) next_word = live_word(s);
  }
  for (; s < n_groups; s += GW) {
    unsigned bits = 0;
    if constexpr (MASKED) {
      bits = live_bits(s, next_word);
      if (s + GW < n_groups) next_word = live_word(s + GW);
      if (!bits) continue;                                 // nothing live in this step: no gallery load
    }
    int jj[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      if constexpr (MASKED) jj[r] = (int)(s * NR) + (NR == 1 || ((bits >> r) & 1) ? r : __ffs((int)bits) - 1);      // a dead slot: a live row of the step
      else jj[r] = (int)min(s * NR + r, (long long)ng - 1);                                           // a slot past the gallery: clamped
    }                                                                                                 // (the results of both are dropped)
    [[maybe_unused]] int gv[NR];                           // the rows' groups, as loaded (see above): jj[r] is a row of the gallery
    if constexpr (GROUPED) {
#pragma unroll
      for (int r = 0; r < NR; ++r) gv[r] = groups[jj[r]];
    }
    double dist[NQ * NR];
    wave_dist64_queries<NQ, NR>(qt, gallery, jj, d, lane, dist);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      if (MASKED ? (bits >> r) & 1 : s * NR + r < ng) {
#pragma unroll
        for (int u = 0; u < NQ; ++u) {
          const double cv = dist[u * NR + r];
          if (!(cv < INFINITY)) gallery_bad = true;
          else if (!((dead >> u) & 1) && wl[u].beats(cv, jj[r])) {
            if constexpr (AFTER) {
              if (!(cv > cd[u] || (cv == cd[u] && jj[r] > cr[u]))) continue;      // at or before the cursor (or a NaN cursor)
            }
            if constexpr (EXCL && GROUPED) {
              const int cg = uniform_of(gv[r]);
              if ((long long)cg == ex[u]) continue;        // a row of the query's excluded group
              if constexpr (AFTER) {                       // PAGE: a group outside [0, n_grp) has no bit, a banned one a row at or before the cursor
                if ((unsigned)cg >= (unsigned)n_grp) continue;
                const unsigned bw = ban[(size_t)(q0 + u) * ban_words + ((unsigned)cg >> 5)];      // q0 + u < nq: the query is not dead
                if ((uniform_of((int)bw) >> (cg & 31)) & 1) continue;
              }
              wl[u].insert(cv, jj[r], cg, lane, depth);
            } else if constexpr (EXCL) {
              if (jj[r] == ex[u]) continue;                // the query's excluded row
              wl[u].insert(cv, jj[r], lane, depth);
            } else if constexpr (GROUPED) wl[u].insert(cv, jj[r], uniform_of(gv[r]), lane, depth);
            else wl[u].insert(cv, jj[r], lane, depth);
          }
        }
      }
    }
  }
  if (nonfinite && gallery_bad && lane == 0) atomicOr(nonfinite, 1);

  // ---- the workgroup's four lists of a query -> one: wave w merges the queries w, w + 4, ...
  __syncthreads();                                         // every wave is done with the query tile
  double *sd = reinterpret_cast<double *>(smem4);          // [NQ][4][64]
  if constexpr (GROUPED) {
    int *si = reinterpret_cast<int *>(sd + NQ * 4 * 64), *sg = si + NQ * 4 * 64;      // rows as ints + groups: 16 bytes an entry, as below
#pragma unroll
    for (int u = 0; u < NQ; ++u) {
      sd[(u * 4 + wave) * 64 + lane] = wl[u].bd;
      si[(u * 4 + wave) * 64 + lane] = wl[u].bi;
      sg[(u * 4 + wave) * 64 + lane] = wl[u].bg;
    }
    __syncthreads();
    const int nlists = gridDim.x;
    for (int u = wave; u < NQ; u += 4) {
      if (q0 + u >= nq) break;
      GroupList<long long, EMPTY_ID> m;
      m.init(EMPTY_ID);
      merge_lists(m, LdsGroupLists<int>{sd + u * 4 * 64, si + u * 4 * 64, sg + u * 4 * 64}, 4, 0, 64, depth, lane);
      if (lane < depth) {
        const size_t o = ((size_t)(q0 + u) * depth + lane) * nlists + blockIdx.x;
        part_d[o] = m.bd;
        part_i[o] = m.bi == EMPTY_ID ? EMPTY_ROW : (int)m.bi;
        part_g[o] = m.bg;
      }
    }
  } else {
    long long *si = reinterpret_cast<long long *>(sd + NQ * 4 * 64);      // 64-bit indices: what merge_lists reads
#pragma unroll
    for (int u = 0; u < NQ; ++u) {
      sd[(u * 4 + wave) * 64 + lane] = wl[u].bd;
      si[(u * 4 + wave) * 64 + lane] = wl[u].bi == EMPTY_ROW ? EMPTY_ID : (long long)wl[u].bi;
    }
    __syncthreads();
    const int nlists = gridDim.x;
    for (int u = wave; u < NQ; u += 4) {
      if (q0 + u >= nq) break;
      WaveList<long long> m;
      m.init(EMPTY_ID);
      merge_lists(m, LdsLists{sd + u * 4 * 64, si + u * 4 * 64}, 4, 0, 64, depth, lane);
      if (lane < depth) {
        const size_t o = ((size_t)(q0 + u) * depth + lane) * nlists + blockIdx.x;
        part_d[o] = m.bd;
        part_i[o] = m.bi == EMPTY_ID ? EMPTY_ROW : (int)m.bi;
      }
    }
  }
}

// The two kernels of the body.  search_scan_kernel<NQ, NR, MASKED> keeps its name, its parameters and its statements (GROUPED = false
// compiles every line of the grouping away), so the eight ungrouped instantiations compute what they did, bit for bit, in the same
// registers (within 2) and without scratch; the compiler's output for the inlined body is not byte-identical to the one it gave the
// body written in the kernel, and profiles/search_grouped.md has their time before and after (within 1 - 3 %).  The grouped scan
// is a kernel of its own name with the two extra pointers.
template <int NQ, int NR, bool MASKED>
__global__ __launch_bounds__(256) void search_scan_kernel(const float *__restrict__ gallery, const float *__restrict__ queries,
                                                          const unsigned *__restrict__ live, int ng, int nq, int d, int depth,
                                                          double *__restrict__ part_d, int *__restrict__ part_i, int *__restrict__ nonfinite) {
  scan_body<NQ, NR, MASKED, false>(gallery, queries, live, nullptr, ng, nq, d, depth, part_d, part_i, nullptr, nonfinite);
}
// The half gallery's two kernels: the same body with G = _Float16, under names of their own.
template <int NQ, int NR, bool MASKED>
__global__ __launch_bounds__(256) void half_scan_kernel(const _Float16 *__restrict__ gallery, const float *__restrict__ queries,
                                                        const unsigned *__restrict__ live, int ng, int nq, int d, int depth,
                                                        double *__restrict__ part_d, int *__restrict__ part_i, int *__restrict__ nonfinite) {
  scan_body<NQ, NR, MASKED, false>(gallery, queries, live, nullptr, ng, nq, d, depth, part_d, part_i, nullptr, nonfinite);
}
// The cursor scans (vtc_l2_search_after): the same body with AFTER, under names of their own, with the cursors and the window's id_base.
template <int NQ, int NR, bool MASKED>
__global__ __launch_bounds__(256) void search_after_scan_kernel(const float *__restrict__ gallery, const float *__restrict__ queries,
                                                                const unsigned *__restrict__ live, const double *__restrict__ after_d,
                                                                const int64_t *__restrict__ after_i, int64_t id_base, int ng, int nq, int d,
                                                                int depth, double *__restrict__ part_d, int *__restrict__ part_i,
                                                                int *__restrict__ nonfinite) {
  scan_body<NQ, NR, MASKED, false, true>(gallery, queries, live, nullptr, ng, nq, d, depth, part_d, part_i, nullptr, nonfinite, after_d, after_i,
                                         id_base);
}
template <int NQ, int NR, bool MASKED>
__global__ __launch_bounds__(256) void half_after_scan_kernel(const _Float16 *__restrict__ gallery, const float *__restrict__ queries,
                                                              const unsigned *__restrict__ live, const double *__restrict__ after_d,
                                                              const int64_t *__restrict__ after_i, int64_t id_base, int ng, int nq, int d,
                                                              int depth, double *__restrict__ part_d, int *__restrict__ part_i,
                                                              int *__restrict__ nonfinite) {
  scan_body<NQ, NR, MASKED, false, true>(gallery, queries, live, nullptr, ng, nq, d, depth, part_d, part_i, nullptr, nonfinite, after_d, after_i,
                                         id_base);
}
// The excluding scans (vtc_l2_search_excluding): the same body with EXCL, under names of their own, the gallery's element type a
// template argument.  excluding_scan_kernel is the cursor scan plus the excluded row (a null after_d: no cursor);
// excluding_grouped_scan_kernel the grouped scan plus the excluded group.
template <typename G, int NQ, int NR, bool MASKED>
__global__ __launch_bounds__(256) void excluding_scan_kernel(const G *__restrict__ gallery, const float *__restrict__ queries,
                                                             const unsigned *__restrict__ live, const double *__restrict__ after_d,
                                                             const int64_t *__restrict__ after_i, const int64_t *__restrict__ exclude,
                                                             int64_t id_base, int ng, int nq, int d, int depth, double *__restrict__ part_d,
                                                             int *__restrict__ part_i, int *__restrict__ nonfinite) {
  scan_body<NQ, NR, MASKED, false, true, true>(gallery, queries, live, nullptr, ng, nq, d, depth, part_d, part_i, nullptr, nonfinite, after_d,
                                               after_i, id_base, exclude);
}
template <typename G, int NQ, int NR, bool MASKED>
__global__ __launch_bounds__(256) void excluding_grouped_scan_kernel(const G *__restrict__ gallery, const float *__restrict__ queries,
                                                                     const unsigned *__restrict__ live, const int *__restrict__ groups,
                                                                     const int64_t *__restrict__ exclude, int ng, int nq, int d, int depth,
                                                                     double *__restrict__ part_d, int *__restrict__ part_i,
                                                                     int *__restrict__ part_g, int *__restrict__ nonfinite) {
  scan_body<NQ, NR, MASKED, true, false, true>(gallery, queries, live, groups, ng, nq, d, depth, part_d, part_i, part_g, nonfinite, nullptr, nullptr,
                                               0, exclude);
}
// The page scan (vtc_l2_search_grouped_after): the same body with GROUPED, AFTER and EXCL -- the cursor, the ban bitmap of the mark
// pass and the excluded group, which may be null.
template <typename G, int NQ, int NR, bool MASKED>
__global__ __launch_bounds__(256) void videos_page_scan_kernel(const G *__restrict__ gallery, const float *__restrict__ queries,
                                                               const unsigned *__restrict__ live, const int *__restrict__ groups, int n_grp,
                                                               const unsigned *__restrict__ ban, const int64_t *__restrict__ exclude,
                                                               const double *__restrict__ after_d, const int64_t *__restrict__ after_i,
                                                               int64_t id_base, int ng, int nq, int d, int depth, double *__restrict__ part_d,
                                                               int *__restrict__ part_i, int *__restrict__ part_g, int *__restrict__ nonfinite) {
  scan_body<NQ, NR, MASKED, true, true, true>(gallery, queries, live, groups, ng, nq, d, depth, part_d, part_i, part_g, nonfinite, after_d, after_i,
                                              id_base, exclude, ban, n_grp);
}
// The mark pass (vtc_l2_group_mark_before): the scan's walk -- the query tile in the LDS, a non-finite query a row of zeros that takes
// no part, the tile shapes, the mask word of the next step read ahead, a step without a live row issuing no load, the groups loaded
// before the step's gallery rows -- with the distances of wave_dist64_queries, so the bits the page scan compares.  A live row with a
// finite distance that lies AT OR BEFORE query u's cursor, the exact negation of the scan's test, sets bit groups[row] of ban[q0 + u]:
// an atomicOr from one lane, no lists, no merge.  A NaN cursor therefore marks every such row (and admits nothing in the scan), -inf
// none.  A group outside [0, n_grp) marks nothing: it is checked before the address is formed.  The pass only ORs.
template <typename G, int NQ, int NR, bool MASKED>
__global__ __launch_bounds__(256) void videos_page_mark_kernel(const G *__restrict__ gallery, const float *__restrict__ queries,
                                                               const unsigned *__restrict__ live, const int *__restrict__ groups, int n_grp,
                                                               const double *__restrict__ after_d, const int64_t *__restrict__ after_i,
                                                               int64_t id_base, int ng, int nq, int d, unsigned *__restrict__ ban) {
  extern __shared__ float4 smem4[];
  float *qt = reinterpret_cast<float *>(smem4);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q0 = blockIdx.y * NQ;
  const int d4 = d >> 2;
  unsigned bad_bits = 0;
  for (int x = tid; x < NQ * d4; x += 256) {
    const int u = x / d4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (q0 + u < nq) v = reinterpret_cast<const float4 *>(queries + (size_t)(q0 + u) * d)[x - u * d4];
    if (!(isfinite(v.x) && isfinite(v.y) && isfinite(v.z) && isfinite(v.w))) bad_bits |= 1u << u;
    smem4[x] = v;
  }
  unsigned dead = 0;                                       // bit u: query q0 + u marks nothing (uniform for the workgroup)
#pragma unroll
  for (int u = 0; u < NQ; ++u) {
    const int bad = __syncthreads_or((bad_bits >> u) & 1);
    if (bad || q0 + u >= nq) dead |= 1u << u;
    if (bad) {
      for (int x = tid; x < d4; x += 256) smem4[u * d4 + x] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  __syncthreads();
  double cd[NQ];                                           // the cursors, as the scan holds them
  int cr[NQ];
#pragma unroll
  for (int u = 0; u < NQ; ++u) {
    const int q = min(q0 + u, nq - 1);
    const long long a = after_i[q];
    cd[u] = uniform_f64(after_d[q]);
    cr[u] = uniform_of(a < id_base ? -1 : (int)min(a - id_base, (long long)ng));
  }
  const size_t ban_words = ((size_t)(unsigned)n_grp + 31) >> 5;
  const long long n_steps = ((long long)ng + NR - 1) / NR, GW = (long long)gridDim.x * 4;
  auto live_word = [&](long long s) -> unsigned { return live[(s * NR) >> 5]; };
  auto live_bits = [&](long long s, unsigned word) -> unsigned {
    const int j0 = (int)(s * NR), left = ng - j0;          // s < n_steps: j0 < ng, left >= 1
    const unsigned inside = NR == 1 || left >= NR ? (1u << NR) - 1 : (1u << left) - 1;
    return (unsigned)uniform_of((int)((word >> (j0 & 31)) & inside));
  };
  long long s = (long long)blockIdx.x * 4 + wave;
  unsigned next_word = 0;
  if constexpr (MASKED) {
    if (s < n_steps) next_word = live_word(s);
  }
  for (; s < n_steps; s += GW) {
    unsigned bits = 0;
    if constexpr (MASKED) {
      bits = live_bits(s, next_word);
      if (s + GW < n_steps) next_word = live_word(s + GW);
      if (!bits) continue;                                 // nothing live in this step: no gallery load
    }
    int jj[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      if constexpr (MASKED) jj[r] = (int)(s * NR) + (NR == 1 || ((bits >> r) & 1) ? r : __ffs((int)bits) - 1);      // a dead slot: a live row of the step
      else jj[r] = (int)min(s * NR + r, (long long)ng - 1);                                           // a slot past the gallery: clamped
    }
    int gv[NR];                                            // jj[r] is a row of the gallery
#pragma unroll
    for (int r = 0; r < NR; ++r) gv[r] = groups[jj[r]];
    double dist[NQ * NR];
    wave_dist64_queries<NQ, NR>(qt, gallery, jj, d, lane, dist);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      if (MASKED ? (bits >> r) & 1 : s * NR + r < ng) {
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
template <int NQ, int NR, bool MASKED>
__global__ __launch_bounds__(256) void half_scan_grouped_kernel(const _Float16 *__restrict__ gallery, const float *__restrict__ queries,
                                                                const unsigned *__restrict__ live, const int *__restrict__ groups, int ng,
                                                                int nq, int d, int depth, double *__restrict__ part_d,
                                                                int *__restrict__ part_i, int *__restrict__ part_g,
                                                                int *__restrict__ nonfinite) {
  scan_body<NQ, NR, MASKED, true>(gallery, queries, live, groups, ng, nq, d, depth, part_d, part_i, part_g, nonfinite);
}
template <int NQ, int NR, bool MASKED>
__global__ __launch_bounds__(256) void search_grouped_scan_kernel(const float *__restrict__ gallery, const float *__restrict__ queries,
                                                                  const unsigned *__restrict__ live, const int *__restrict__ groups, int ng,
                                                                  int nq, int d, int depth, double *__restrict__ part_d,
                                                                  int *__restrict__ part_i, int *__restrict__ part_g,
                                                                  int *__restrict__ nonfinite) {
  scan_body<NQ, NR, MASKED, true>(gallery, queries, live, groups, ng, nq, d, depth, part_d, part_i, part_g, nonfinite);
}

// One workgroup per query: the first `depth` of the union of the lists by (distance, index).
template <typename Src>
__global__ __launch_bounds__(256) void merge_kernel(Src src, int nlists, int depth, int64_t id_base, int64_t *__restrict__ ids,
                                                    float *__restrict__ dists, double *__restrict__ dists64) {
  __shared__ double sd[4][64];
  __shared__ long long si[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = blockIdx.x;
  src.q = q;
  WaveList<long long> wl;
  wl.init(EMPTY_ID);
  merge_lists(wl, src, nlists, wave * 64, 256, depth, lane);
  sd[wave][lane] = wl.bd;
  si[wave][lane] = wl.bi;
  __syncthreads();
  if (wave != 0) return;
  merge_lists(wl, LdsLists{&sd[1][0], &si[1][0]}, 3, 0, 64, depth, lane);
  if (lane < depth) {
    const size_t o = (size_t)q * depth + lane;
    const bool empty = wl.bi == EMPTY_ID;
    ids[o] = empty ? -1 : id_base + wl.bi;
    if (dists) dists[o] = empty ? INFINITY : (float)wl.bd;
    if (dists64) dists64[o] = empty ? (double)INFINITY : wl.bd;
  }
}

// The grouped merge: the same walk with GroupLists, so a group's stale, worse entries from other lists are absorbed by the insertion.
template <typename Src>
__global__ __launch_bounds__(256) void merge_grouped_kernel(Src src, int nlists, int depth, int64_t id_base, int64_t *__restrict__ ids,
                                                            int32_t *__restrict__ out_groups, float *__restrict__ dists,
                                                            double *__restrict__ dists64) {
  __shared__ double sd[4][64];
  __shared__ long long si[4][64];
  __shared__ int sg[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = blockIdx.x;
  src.q = q;
  GroupList<long long, EMPTY_ID> wl;
  wl.init(EMPTY_ID);
  merge_lists(wl, src, nlists, wave * 64, 256, depth, lane);
  sd[wave][lane] = wl.bd;
  si[wave][lane] = wl.bi;
  sg[wave][lane] = wl.bg;
  __syncthreads();
  if (wave != 0) return;
  merge_lists(wl, LdsGroupLists<long long>{&sd[1][0], &si[1][0], &sg[1][0]}, 3, 0, 64, depth, lane);
  if (lane < depth) {
    const size_t o = (size_t)q * depth + lane;
    const bool empty = wl.bi == EMPTY_ID;
    ids[o] = empty ? -1 : id_base + wl.bi;
    out_groups[o] = empty ? -1 : wl.bg;
    if (dists) dists[o] = empty ? INFINITY : (float)wl.bd;
    if (dists64) dists64[o] = empty ? (double)INFINITY : wl.bd;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
struct SearchPlan {
  int tile_q, tile_r;       // queries of a tile (a gallery pass each), gallery rows of a step
  int tiles;
};
SearchPlan search_plan(int nq) {
  SearchPlan p;
  if (nq == 1) p.tile_q = 1, p.tile_r = 4;
  else if (nq == 2) p.tile_q = 2, p.tile_r = 4;
  else if (nq <= 4) p.tile_q = 4, p.tile_r = 2;
  else p.tile_q = 8, p.tile_r = 1;
  p.tiles = cdiv(nq, p.tile_q);
  return p;
}
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
SearchWs search_ws(void *ws, int ng, int nq, int depth, bool grouped = false) {
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
// G = _Float16: the half gallery's kernels, by the same rule among themselves.  AFTER: the cursor scan, `after` its three arguments.
// EXCL: the excluding scans, `after.exclude` the excluded keys (and after.d / after.i null where there is no cursor).
struct AfterArgs {
  const double *d;
  const int64_t *i;
  int64_t id_base;
  const int64_t *exclude = nullptr;
  const unsigned *ban = nullptr;      // the page scan's bitmap of banned groups and the number of groups it is indexed by
  int n_grp = 0;
};
template <int NQ, int NR, bool MASKED, bool GROUPED, bool AFTER = false, bool EXCL = false, typename G>
int launch_scan(const G *gallery, const float *queries, const unsigned *live, const int *groups, int ng, int nq, int d, int depth,
                const SearchWs &s, int tiles, int *nonfinite, hipStream_t stream, const AfterArgs &after = {}) {
  // resident workgroups per CU: a property of the instantiation, its LDS (d / 64 = 1 .. 32) and the device -- asked once, as num_cus() is
  static std::atomic<int> resident[64][SEARCH_MAX_D / 64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  std::atomic<int> &slot = resident[dev][d / 64 - 1];
  int per_cu = slot.load(std::memory_order_relaxed);
  if (per_cu == 0) {
    constexpr bool HALF = std::is_same_v<G, _Float16>;
    auto resident_of = [&](int &n, auto kernel) { return hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, 256, scan_lds_bytes(NQ, d)); };
    hipError_t e;
    if constexpr (HALF) e = resident_of(per_cu, half_scan_kernel<NQ, NR, false>);
    else e = resident_of(per_cu, search_scan_kernel<NQ, NR, false>);
    if (e != hipSuccess || per_cu < 1) per_cu = 1;
    // The masked scan runs the unmasked scan's grid (never more than is resident of its own), so both leave the same number of lists.
    // The 8 x 1 tile takes fewer registers with the mask and would fit a fourth workgroup per CU; every wave fills lists of its own
    // before it starts rejecting rows, and with all rows live at 10^5 rows the fourth workgroup put the masked scan 4.5 - 5.8 % behind
    // the unmasked one instead of 3.4 - 3.6 %.  It was 2.5 % faster at 10^6 rows and 4 - 12 % on partly live masks there: the trade is
    // written down in profiles/search_masked.md.
    // The grouped scan follows the same rule: the unmasked, ungrouped scan's grid, never more than is resident of its own.
    // The cursor scan too, masked or not, the excluding scans and the page scan.
    int own = per_cu;
    if constexpr (GROUPED && AFTER) {
      e = resident_of(own, videos_page_scan_kernel<G, NQ, NR, MASKED>);
      if (e == hipSuccess && own >= 1) per_cu = std::min(per_cu, own);
    } else if constexpr (EXCL) {
      if constexpr (GROUPED) e = resident_of(own, excluding_grouped_scan_kernel<G, NQ, NR, MASKED>);
      else e = resident_of(own, excluding_scan_kernel<G, NQ, NR, MASKED>);
      if (e == hipSuccess && own >= 1) per_cu = std::min(per_cu, own);
    } else if constexpr (AFTER) {
      if constexpr (HALF) e = resident_of(own, half_after_scan_kernel<NQ, NR, MASKED>);
      else e = resident_of(own, search_after_scan_kernel<NQ, NR, MASKED>);
      if (e == hipSuccess && own >= 1) per_cu = std::min(per_cu, own);
    } else if constexpr (GROUPED) {
      if constexpr (HALF) e = resident_of(own, half_scan_grouped_kernel<NQ, NR, MASKED>);
      else e = resident_of(own, search_grouped_scan_kernel<NQ, NR, MASKED>);
      if (e == hipSuccess && own >= 1) per_cu = std::min(per_cu, own);
    } else if constexpr (MASKED) {
      if constexpr (HALF) e = resident_of(own, half_scan_kernel<NQ, NR, true>);
      else e = resident_of(own, search_scan_kernel<NQ, NR, true>);
      if (e == hipSuccess && own >= 1) per_cu = std::min(per_cu, own);
    }
    slot.store(per_cu, std::memory_order_relaxed);
  }
  const long long n_groups = ((long long)ng + NR - 1) / NR;
  const int blocks = (int)std::min<long long>(std::min(search_max_lists(ng), std::min(per_cu, 4) * vtcgemm::num_cus()), (n_groups + 3) / 4);
  if constexpr (GROUPED && AFTER) {
    hipLaunchKernelGGL((videos_page_scan_kernel<G, NQ, NR, MASKED>), dim3(blocks, tiles), dim3(256), scan_lds_bytes(NQ, d), stream, gallery, queries, live,
                       groups, after.n_grp, after.ban, after.exclude, after.d, after.i, after.id_base, ng, nq, d, depth, s.part_d, s.part_i, s.part_g,
                       nonfinite);
  } else if constexpr (EXCL) {
    if constexpr (GROUPED)
      hipLaunchKernelGGL((excluding_grouped_scan_kernel<G, NQ, NR, MASKED>), dim3(blocks, tiles), dim3(256), scan_lds_bytes(NQ, d), stream, gallery,
                         queries, live, groups, after.exclude, ng, nq, d, depth, s.part_d, s.part_i, s.part_g, nonfinite);
    else
      hipLaunchKernelGGL((excluding_scan_kernel<G, NQ, NR, MASKED>), dim3(blocks, tiles), dim3(256), scan_lds_bytes(NQ, d), stream, gallery, queries,
                         live, after.d, after.i, after.exclude, after.id_base, ng, nq, d, depth, s.part_d, s.part_i, nonfinite);
  } else if constexpr (AFTER) {
    if constexpr (std::is_same_v<G, _Float16>)
      hipLaunchKernelGGL((half_after_scan_kernel<NQ, NR, MASKED>), dim3(blocks, tiles), dim3(256), scan_lds_bytes(NQ, d), stream, gallery, queries, live,
                         after.d, after.i, after.id_base, ng, nq, d, depth, s.part_d, s.part_i, nonfinite);
    else
      hipLaunchKernelGGL((search_after_scan_kernel<NQ, NR, MASKED>), dim3(blocks, tiles), dim3(256), scan_lds_bytes(NQ, d), stream, gallery, queries,
                         live, after.d, after.i, after.id_base, ng, nq, d, depth, s.part_d, s.part_i, nonfinite);
  } else if constexpr (std::is_same_v<G, _Float16>) {
    if constexpr (GROUPED)
      hipLaunchKernelGGL((half_scan_grouped_kernel<NQ, NR, MASKED>), dim3(blocks, tiles), dim3(256), scan_lds_bytes(NQ, d), stream, gallery, queries,
                         live, groups, ng, nq, d, depth, s.part_d, s.part_i, s.part_g, nonfinite);
    else
      hipLaunchKernelGGL((half_scan_kernel<NQ, NR, MASKED>), dim3(blocks, tiles), dim3(256), scan_lds_bytes(NQ, d), stream, gallery, queries, live, ng,
                         nq, d, depth, s.part_d, s.part_i, nonfinite);
  } else if constexpr (GROUPED)
    hipLaunchKernelGGL((search_grouped_scan_kernel<NQ, NR, MASKED>), dim3(blocks, tiles), dim3(256), scan_lds_bytes(NQ, d), stream, gallery, queries,
                       live, groups, ng, nq, d, depth, s.part_d, s.part_i, s.part_g, nonfinite);
  else
    hipLaunchKernelGGL((search_scan_kernel<NQ, NR, MASKED>), dim3(blocks, tiles), dim3(256), scan_lds_bytes(NQ, d), stream, gallery, queries, live, ng,
                       nq, d, depth, s.part_d, s.part_i, nonfinite);
  return blocks;
}
// the instantiation of the plan's tile shape.  The half scan keeps the fp32 scan's shapes: 8 gallery rows a step for its one- and
// two-query tiles (a piece of a half row is 8 bytes a lane, so a step has half the bytes in flight) were measured and lost
// (profiles/search_half.md).
template <bool MASKED, bool GROUPED = false, bool AFTER = false, bool EXCL = false, typename G>
int launch_scan_tile(const SearchPlan &p, const G *gallery, const float *queries, const unsigned *live, const int *groups, int ng, int nq, int d,
                     int depth, const SearchWs &s, int *nonfinite, hipStream_t stream, const AfterArgs &after = {}) {
  if (p.tile_q == 1)
    return launch_scan<1, 4, MASKED, GROUPED, AFTER, EXCL>(gallery, queries, live, groups, ng, nq, d, depth, s, p.tiles, nonfinite, stream, after);
  if (p.tile_q == 2)
    return launch_scan<2, 4, MASKED, GROUPED, AFTER, EXCL>(gallery, queries, live, groups, ng, nq, d, depth, s, p.tiles, nonfinite, stream, after);
  if (p.tile_q == 4)
    return launch_scan<4, 2, MASKED, GROUPED, AFTER, EXCL>(gallery, queries, live, groups, ng, nq, d, depth, s, p.tiles, nonfinite, stream, after);
  return launch_scan<8, 1, MASKED, GROUPED, AFTER, EXCL>(gallery, queries, live, groups, ng, nq, d, depth, s, p.tiles, nonfinite, stream, after);
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
}  // namespace

extern "C" size_t vtc_l2_search_workspace_bytes(int n_gallery, int n_queries, int d, int depth) {
  if (!search_args_ok(n_gallery, n_queries, d, depth)) return 0;
  return search_ws(nullptr, n_gallery, n_queries, depth).total;
}

extern "C" int vtc_l2_search_masked(const float *gallery, const float *queries, const uint32_t *live, int ng, int nq, int d, int depth,
                                    int64_t id_base, int64_t *ids, float *dists, int *nonfinite, void *ws, size_t ws_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  VTC_CHECK(gallery && queries && ids, "l2_search: null argument");
  VTC_CHECK(ng >= 1, "l2_search: n_gallery=%d must be at least 1", ng);
  VTC_CHECK(nq >= 1 && nq <= SEARCH_MAX_Q, "l2_search: n_queries=%d must be in [1, %d] (more queries: vtc_l2_topk)", nq, SEARCH_MAX_Q);
  VTC_CHECK(depth >= 1 && depth <= SEARCH_MAX_DEPTH && depth <= ng, "l2_search: depth=%d must be in [1, min(%d, n_gallery)]", depth, SEARCH_MAX_DEPTH);
  VTC_CHECK(d >= 64 && d <= SEARCH_MAX_D && d % 64 == 0, "l2_search: d=%d must be a multiple of 64 in [64, %d]", d, SEARCH_MAX_D);
  VTC_CHECK(id_base >= 0 && id_base <= INT64_MAX - ng, "l2_search: id_base=%lld must be non-negative (and id_base + n_gallery an int64)",
            (long long)id_base);
  const SearchWs s = search_ws(ws, ng, nq, depth);
  VTC_CHECK(ws && ws_bytes >= s.total, "l2_search: workspace too small (%zu < %zu)", ws_bytes, s.total);
  const SearchPlan p = search_plan(nq);
  const int blocks = live ? launch_scan_tile<true>(p, gallery, queries, live, nullptr, ng, nq, d, depth, s, nonfinite, stream)
                          : launch_scan_tile<false>(p, gallery, queries, nullptr, nullptr, ng, nq, d, depth, s, nonfinite, stream);
  VTC_LAUNCH_CHECK2("l2_search", "scan");
  hipLaunchKernelGGL(merge_kernel<ScanLists>, dim3(nq), dim3(256), 0, stream, ScanLists{s.part_d, s.part_i, blocks, depth, 0}, blocks, depth, id_base,
                     ids, dists, s.dists64);
  VTC_LAUNCH_CHECK2("l2_search", "merge");
  return 0;
}

extern "C" int vtc_l2_search(const float *gallery, const float *queries, int ng, int nq, int d, int depth, int64_t id_base, int64_t *ids,
                             float *dists, int *nonfinite, void *ws, size_t ws_bytes, void *stream) {
  return vtc_l2_search_masked(gallery, queries, nullptr, ng, nq, d, depth, id_base, ids, dists, nonfinite, ws, ws_bytes, stream);
}

extern "C" int vtc_row_mask_pack(const uint8_t *flags, int n_rows, const uint32_t *and_mask, uint32_t *words, void *stream) {
  VTC_CHECK(flags && words, "row_mask_pack (the search's row mask): null argument");
  VTC_CHECK(n_rows >= 1, "row_mask_pack (the search's row mask): n_rows=%d must be at least 1", n_rows);
  hipLaunchKernelGGL(row_mask_pack_kernel, dim3(cdiv(n_rows, 256)), dim3(256), 0, (hipStream_t)stream, flags, n_rows, and_mask, words);
  VTC_LAUNCH_CHECK("row_mask_pack");
  return 0;
}

extern "C" int vtc_l2_search_merge(const int64_t *ids_parts, const double *dists_parts, int n_parts, int nq, int depth, int64_t *ids,
                                   float *dists, void *stream) {
  VTC_CHECK(ids_parts && dists_parts && ids, "l2_search_merge: null argument");
  VTC_CHECK(n_parts >= 1 && n_parts <= SEARCH_MAX_PARTS, "l2_search_merge: n_parts=%d must be in [1, %d]", n_parts, SEARCH_MAX_PARTS);
  VTC_CHECK(nq >= 1 && nq <= SEARCH_MAX_Q, "l2_search_merge: n_queries=%d must be in [1, %d]", nq, SEARCH_MAX_Q);
  VTC_CHECK(depth >= 1 && depth <= SEARCH_MAX_DEPTH, "l2_search_merge: depth=%d must be in [1, %d]", depth, SEARCH_MAX_DEPTH);
  hipLaunchKernelGGL(merge_kernel<PartLists>, dim3(nq), dim3(256), 0, (hipStream_t)stream, PartLists{dists_parts, ids_parts, nq, depth, 0}, n_parts,
                     depth, (int64_t)0, ids, dists, (double *)nullptr);
  VTC_LAUNCH_CHECK("l2_search_merge");
  return 0;
}

extern "C" size_t vtc_l2_search_grouped_workspace_bytes(int n_gallery, int n_queries, int d, int depth) {
  if (!search_args_ok(n_gallery, n_queries, d, depth)) return 0;
  return search_ws(nullptr, n_gallery, n_queries, depth, true).total;
}

extern "C" int vtc_l2_search_grouped(const float *gallery, const float *queries, const uint32_t *live, const int32_t *groups, int ng, int nq, int d,
                                     int depth, int64_t id_base, int64_t *ids, int32_t *out_groups, float *dists, int *nonfinite, void *ws,
                                     size_t ws_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  VTC_CHECK(gallery && queries && groups && ids && out_groups, "l2_search_grouped: null argument");
  VTC_CHECK(ng >= 1, "l2_search_grouped: n_gallery=%d must be at least 1", ng);
  VTC_CHECK(nq >= 1 && nq <= SEARCH_MAX_Q, "l2_search_grouped: n_queries=%d must be in [1, %d]", nq, SEARCH_MAX_Q);
  VTC_CHECK(depth >= 1 && depth <= SEARCH_MAX_DEPTH && depth <= ng, "l2_search_grouped: depth=%d must be in [1, min(%d, n_gallery)]", depth,
            SEARCH_MAX_DEPTH);
  VTC_CHECK(d >= 64 && d <= SEARCH_MAX_D && d % 64 == 0, "l2_search_grouped: d=%d must be a multiple of 64 in [64, %d]", d, SEARCH_MAX_D);
  VTC_CHECK(id_base >= 0 && id_base <= INT64_MAX - ng, "l2_search_grouped: id_base=%lld must be non-negative (and id_base + n_gallery an int64)",
            (long long)id_base);
  const SearchWs s = search_ws(ws, ng, nq, depth, true);
  VTC_CHECK(ws && ws_bytes >= s.total, "l2_search_grouped: workspace too small (%zu < %zu)", ws_bytes, s.total);
  const SearchPlan p = search_plan(nq);
  const int blocks = live ? launch_scan_tile<true, true>(p, gallery, queries, live, groups, ng, nq, d, depth, s, nonfinite, stream)
                          : launch_scan_tile<false, true>(p, gallery, queries, nullptr, groups, ng, nq, d, depth, s, nonfinite, stream);
  VTC_LAUNCH_CHECK2("l2_search_grouped", "scan");
  hipLaunchKernelGGL(merge_grouped_kernel<ScanGroupLists>, dim3(nq), dim3(256), 0, stream, ScanGroupLists{s.part_d, s.part_i, s.part_g, blocks, depth, 0},
                     blocks, depth, id_base, ids, out_groups, dists, s.dists64);
  VTC_LAUNCH_CHECK2("l2_search_grouped", "merge");
  return 0;
}

extern "C" int vtc_l2_search_merge_grouped(const int64_t *ids_parts, const double *dists_parts, const int32_t *groups_parts, int n_parts, int nq,
                                           int depth, int64_t *ids, int32_t *out_groups, float *dists, void *stream) {
  VTC_CHECK(ids_parts && dists_parts && groups_parts && ids && out_groups, "l2_search_merge_grouped: null argument");
  VTC_CHECK(n_parts >= 1 && n_parts <= SEARCH_MAX_PARTS, "l2_search_merge_grouped: n_parts=%d must be in [1, %d]", n_parts, SEARCH_MAX_PARTS);
  VTC_CHECK(nq >= 1 && nq <= SEARCH_MAX_Q, "l2_search_merge_grouped: n_queries=%d must be in [1, %d]", nq, SEARCH_MAX_Q);
  VTC_CHECK(depth >= 1 && depth <= SEARCH_MAX_DEPTH, "l2_search_merge_grouped: depth=%d must be in [1, %d]", depth, SEARCH_MAX_DEPTH);
  hipLaunchKernelGGL(merge_grouped_kernel<PartGroupLists>, dim3(nq), dim3(256), 0, (hipStream_t)stream,
                     PartGroupLists{dists_parts, ids_parts, groups_parts, nq, depth, 0}, n_parts, depth, (int64_t)0, ids, out_groups, dists,
                     (double *)nullptr);
  VTC_LAUNCH_CHECK("l2_search_merge_grouped");
  return 0;
}

extern "C" int vtc_l2_search_half(const uint16_t *gallery_, const float *queries, const uint32_t *live, const int32_t *groups, int ng, int nq, int d,
                                  int depth, int64_t id_base, int64_t *ids, int32_t *out_groups, float *dists, int *nonfinite, void *ws,
                                  size_t ws_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const _Float16 *gallery = reinterpret_cast<const _Float16 *>(gallery_);
  VTC_CHECK(gallery && queries && ids && (!groups || out_groups), "l2_search_half: null argument");
  VTC_CHECK(ng >= 1, "l2_search_half: n_gallery=%d must be at least 1", ng);
  VTC_CHECK(nq >= 1 && nq <= SEARCH_MAX_Q, "l2_search_half: n_queries=%d must be in [1, %d]", nq, SEARCH_MAX_Q);
  VTC_CHECK(depth >= 1 && depth <= SEARCH_MAX_DEPTH && depth <= ng, "l2_search_half: depth=%d must be in [1, min(%d, n_gallery)]", depth,
            SEARCH_MAX_DEPTH);
  VTC_CHECK(d >= 64 && d <= SEARCH_MAX_D && d % 64 == 0, "l2_search_half: d=%d must be a multiple of 64 in [64, %d]", d, SEARCH_MAX_D);
  VTC_CHECK(id_base >= 0 && id_base <= INT64_MAX - ng, "l2_search_half: id_base=%lld must be non-negative (and id_base + n_gallery an int64)",
            (long long)id_base);
  const SearchWs s = search_ws(ws, ng, nq, depth, groups != nullptr);
  VTC_CHECK(ws && ws_bytes >= s.total, "l2_search_half: workspace too small (%zu < %zu)", ws_bytes, s.total);
  const SearchPlan p = search_plan(nq);
  int blocks;
  if (groups)
    blocks = live ? launch_scan_tile<true, true>(p, gallery, queries, live, groups, ng, nq, d, depth, s, nonfinite, stream)
                  : launch_scan_tile<false, true>(p, gallery, queries, nullptr, groups, ng, nq, d, depth, s, nonfinite, stream);
  else
    blocks = live ? launch_scan_tile<true, false>(p, gallery, queries, live, nullptr, ng, nq, d, depth, s, nonfinite, stream)
                  : launch_scan_tile<false, false>(p, gallery, queries, nullptr, nullptr, ng, nq, d, depth, s, nonfinite, stream);
  VTC_LAUNCH_CHECK2("l2_search_half", "scan");
  if (groups)
    hipLaunchKernelGGL(merge_grouped_kernel<ScanGroupLists>, dim3(nq), dim3(256), 0, stream, ScanGroupLists{s.part_d, s.part_i, s.part_g, blocks, depth, 0},
                       blocks, depth, id_base, ids, out_groups, dists, s.dists64);
  else
    hipLaunchKernelGGL(merge_kernel<ScanLists>, dim3(nq), dim3(256), 0, stream, ScanLists{s.part_d, s.part_i, blocks, depth, 0}, blocks, depth, id_base,
                       ids, dists, s.dists64);
  VTC_LAUNCH_CHECK2("l2_search_half", "merge");
  return 0;
}

// The cursor search of either storage: the scan of vtc_l2_search_masked / vtc_l2_search_half with AFTER, then the merge every search runs.
template <typename G>
static int search_after(const G *gallery, const float *queries, const uint32_t *live, const AfterArgs &after, int ng, int nq, int d, int depth,
                        int64_t *ids, float *dists, int *nonfinite, const SearchWs &s, hipStream_t stream) {
  const SearchPlan p = search_plan(nq);
  const int blocks = live ? launch_scan_tile<true, false, true>(p, gallery, queries, live, nullptr, ng, nq, d, depth, s, nonfinite, stream, after)
                          : launch_scan_tile<false, false, true>(p, gallery, queries, nullptr, nullptr, ng, nq, d, depth, s, nonfinite, stream, after);
  VTC_LAUNCH_CHECK2("l2_search_after", "scan");
  hipLaunchKernelGGL(merge_kernel<ScanLists>, dim3(nq), dim3(256), 0, stream, ScanLists{s.part_d, s.part_i, blocks, depth, 0}, blocks, depth,
                     after.id_base, ids, dists, s.dists64);
  VTC_LAUNCH_CHECK2("l2_search_after", "merge");
  return 0;
}

extern "C" int vtc_l2_search_after(const void *gallery, int gallery_is_half, const float *queries, const uint32_t *live, const double *after_d,
                                   const int64_t *after_i, int ng, int nq, int d, int depth, int64_t id_base, int64_t *ids, float *dists,
                                   int *nonfinite, void *ws, size_t ws_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  VTC_CHECK(gallery && queries && ids && after_d && after_i, "l2_search_after: null argument");
  VTC_CHECK(ng >= 1, "l2_search_after: n_gallery=%d must be at least 1", ng);
  VTC_CHECK(nq >= 1 && nq <= SEARCH_MAX_Q, "l2_search_after: n_queries=%d must be in [1, %d]", nq, SEARCH_MAX_Q);
  VTC_CHECK(depth >= 1 && depth <= SEARCH_MAX_DEPTH && depth <= ng, "l2_search_after: depth=%d must be in [1, min(%d, n_gallery)]", depth,
            SEARCH_MAX_DEPTH);
  VTC_CHECK(d >= 64 && d <= SEARCH_MAX_D && d % 64 == 0, "l2_search_after: d=%d must be a multiple of 64 in [64, %d]", d, SEARCH_MAX_D);
  VTC_CHECK(id_base >= 0 && id_base <= INT64_MAX - ng, "l2_search_after: id_base=%lld must be non-negative (and id_base + n_gallery an int64)",
            (long long)id_base);
  const SearchWs s = search_ws(ws, ng, nq, depth);
  VTC_CHECK(ws && ws_bytes >= s.total, "l2_search_after: workspace too small (%zu < %zu)", ws_bytes, s.total);
  const AfterArgs after{after_d, after_i, id_base};
  if (gallery_is_half)
    return search_after(reinterpret_cast<const _Float16 *>(gallery), queries, live, after, ng, nq, d, depth, ids, dists, nonfinite, s, stream);
  return search_after(reinterpret_cast<const float *>(gallery), queries, live, after, ng, nq, d, depth, ids, dists, nonfinite, s, stream);
}

extern "C" int vtc_l2_pair_dists64(const void *gallery, int gallery_is_half, const float *queries, const int64_t *rows, int ng, int nq, int d,
                                   int64_t id_base, double *out, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  VTC_CHECK(gallery && queries && rows && out, "l2_pair_dists64 (the search's cursor distances): null argument");
  VTC_CHECK(ng >= 1, "l2_pair_dists64 (the search's cursor distances): n_gallery=%d must be at least 1", ng);
  VTC_CHECK(nq >= 1, "l2_pair_dists64 (the search's cursor distances): n_queries=%d must be at least 1", nq);
  VTC_CHECK(d >= 64 && d <= SEARCH_MAX_D && d % 64 == 0, "l2_pair_dists64 (the search's cursor distances): d=%d must be a multiple of 64 in [64, %d]",
            d, SEARCH_MAX_D);
  VTC_CHECK(id_base >= 0 && id_base <= INT64_MAX - ng,
            "l2_pair_dists64 (the search's cursor distances): id_base=%lld must be non-negative (and id_base + n_gallery an int64)", (long long)id_base);
  if (gallery_is_half)
    hipLaunchKernelGGL(pair_dists64_kernel<_Float16>, dim3(cdiv(nq, 4)), dim3(256), 0, stream, reinterpret_cast<const _Float16 *>(gallery), queries,
                       rows, ng, nq, d, id_base, out);
  else
    hipLaunchKernelGGL(pair_dists64_kernel<float>, dim3(cdiv(nq, 4)), dim3(256), 0, stream, reinterpret_cast<const float *>(gallery), queries, rows,
                       ng, nq, d, id_base, out);
  VTC_LAUNCH_CHECK("l2_pair_dists64");
  return 0;
}

// The excluding search of either storage: the cursor scan (ungrouped; no cursor is the cursor -inf) or the grouped scan with EXCL, then
// the merge every search runs -- the lists do not know which rows were admitted.
template <typename G>
static int search_excluding(const G *gallery, const float *queries, const uint32_t *live, const int32_t *groups, const AfterArgs &args, int ng,
                            int nq, int d, int depth, int64_t *ids, int32_t *out_groups, float *dists, int *nonfinite, const SearchWs &s,
                            hipStream_t stream) {
  const SearchPlan p = search_plan(nq);
  int blocks;
  if (groups)
    blocks = live ? launch_scan_tile<true, true, false, true>(p, gallery, queries, live, groups, ng, nq, d, depth, s, nonfinite, stream, args)
                  : launch_scan_tile<false, true, false, true>(p, gallery, queries, nullptr, groups, ng, nq, d, depth, s, nonfinite, stream, args);
  else
    blocks = live ? launch_scan_tile<true, false, true, true>(p, gallery, queries, live, nullptr, ng, nq, d, depth, s, nonfinite, stream, args)
                  : launch_scan_tile<false, false, true, true>(p, gallery, queries, nullptr, nullptr, ng, nq, d, depth, s, nonfinite, stream, args);
  VTC_LAUNCH_CHECK2("l2_search_excluding", "scan");
  if (groups)
    hipLaunchKernelGGL(merge_grouped_kernel<ScanGroupLists>, dim3(nq), dim3(256), 0, stream, ScanGroupLists{s.part_d, s.part_i, s.part_g, blocks, depth, 0},
                       blocks, depth, args.id_base, ids, out_groups, dists, s.dists64);
  else
    hipLaunchKernelGGL(merge_kernel<ScanLists>, dim3(nq), dim3(256), 0, stream, ScanLists{s.part_d, s.part_i, blocks, depth, 0}, blocks, depth,
                       args.id_base, ids, dists, s.dists64);
  VTC_LAUNCH_CHECK2("l2_search_excluding", "merge");
  return 0;
}

extern "C" int vtc_l2_search_excluding(const void *gallery, int gallery_is_half, const float *queries, const uint32_t *live, const int32_t *groups,
                                       const int64_t *exclude, const double *after_d, const int64_t *after_i, int ng, int nq, int d, int depth,
                                       int64_t id_base, int64_t *ids, int32_t *out_groups, float *dists, int *nonfinite, void *ws,
                                       size_t ws_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  VTC_CHECK(gallery && queries && ids && exclude && (!groups || out_groups), "l2_search_excluding: null argument");
  VTC_CHECK(!after_d == !after_i, "l2_search_excluding: after_d and after_i are given together or not at all");
  VTC_CHECK(!(groups && after_d), "l2_search_excluding: the grouped search has no cursor (after_d / after_i with groups)");
  VTC_CHECK(ng >= 1, "l2_search_excluding: n_gallery=%d must be at least 1", ng);
  VTC_CHECK(nq >= 1 && nq <= SEARCH_MAX_Q, "l2_search_excluding: n_queries=%d must be in [1, %d]", nq, SEARCH_MAX_Q);
  VTC_CHECK(depth >= 1 && depth <= SEARCH_MAX_DEPTH && depth <= ng, "l2_search_excluding: depth=%d must be in [1, min(%d, n_gallery)]", depth,
            SEARCH_MAX_DEPTH);
  VTC_CHECK(d >= 64 && d <= SEARCH_MAX_D && d % 64 == 0, "l2_search_excluding: d=%d must be a multiple of 64 in [64, %d]", d, SEARCH_MAX_D);
  VTC_CHECK(id_base >= 0 && id_base <= INT64_MAX - ng, "l2_search_excluding: id_base=%lld must be non-negative (and id_base + n_gallery an int64)",
            (long long)id_base);
  const SearchWs s = search_ws(ws, ng, nq, depth, groups != nullptr);
  VTC_CHECK(ws && ws_bytes >= s.total, "l2_search_excluding: workspace too small (%zu < %zu)", ws_bytes, s.total);
  const AfterArgs args{after_d, after_i, id_base, exclude};
  if (gallery_is_half)
    return search_excluding(reinterpret_cast<const _Float16 *>(gallery), queries, live, groups, args, ng, nq, d, depth, ids, out_groups, dists,
                            nonfinite, s, stream);
  return search_excluding(reinterpret_cast<const float *>(gallery), queries, live, groups, args, ng, nq, d, depth, ids, out_groups, dists, nonfinite,
                          s, stream);
}

// ---- pages of distinct videos: the mark pass and the page scan ---------------------------------------------------------------------------
namespace {
template <typename G, int NQ, int NR>
void launch_mark(const G *gallery, const float *queries, const unsigned *live, const int *groups, int n_grp, const AfterArgs &after, int ng, int nq,
                 int d, int tiles, unsigned *ban, hipStream_t stream) {
  // the scan's grid without its occupancy question: no lists depend on the number of workgroups, and a workgroup that is not resident
  // at once only starts later
  const long long n_steps = ((long long)ng + NR - 1) / NR;
  const int blocks = (int)std::min<long long>(std::min(search_max_lists(ng), 4 * vtcgemm::num_cus()), (n_steps + 3) / 4);
  const size_t lds = (size_t)NQ * d * sizeof(float);
  if (live)
    hipLaunchKernelGGL((videos_page_mark_kernel<G, NQ, NR, true>), dim3(blocks, tiles), dim3(256), lds, stream, gallery, queries, live, groups, n_grp,
                       after.d, after.i, after.id_base, ng, nq, d, ban);
  else
    hipLaunchKernelGGL((videos_page_mark_kernel<G, NQ, NR, false>), dim3(blocks, tiles), dim3(256), lds, stream, gallery, queries, live, groups, n_grp,
                       after.d, after.i, after.id_base, ng, nq, d, ban);
}
template <typename G>
void launch_mark_tile(const SearchPlan &p, const G *gallery, const float *queries, const unsigned *live, const int *groups, int n_grp,
                      const AfterArgs &after, int ng, int nq, int d, unsigned *ban, hipStream_t stream) {
  if (p.tile_q == 1) return launch_mark<G, 1, 4>(gallery, queries, live, groups, n_grp, after, ng, nq, d, p.tiles, ban, stream);
  if (p.tile_q == 2) return launch_mark<G, 2, 4>(gallery, queries, live, groups, n_grp, after, ng, nq, d, p.tiles, ban, stream);
  if (p.tile_q == 4) return launch_mark<G, 4, 2>(gallery, queries, live, groups, n_grp, after, ng, nq, d, p.tiles, ban, stream);
  return launch_mark<G, 8, 1>(gallery, queries, live, groups, n_grp, after, ng, nq, d, p.tiles, ban, stream);
}
// The page scan of either storage, then the grouped merge every grouped search runs.
template <typename G>
int search_grouped_after(const G *gallery, const float *queries, const uint32_t *live, const int32_t *groups, const AfterArgs &args, int ng, int nq,
                         int d, int depth, int64_t *ids, int32_t *out_groups, float *dists, int *nonfinite, const SearchWs &s, hipStream_t stream) {
  const SearchPlan p = search_plan(nq);
  const int blocks = live ? launch_scan_tile<true, true, true, true>(p, gallery, queries, live, groups, ng, nq, d, depth, s, nonfinite, stream, args)
                          : launch_scan_tile<false, true, true, true>(p, gallery, queries, nullptr, groups, ng, nq, d, depth, s, nonfinite, stream, args);
  VTC_LAUNCH_CHECK2("l2_search_grouped_after", "scan");
  hipLaunchKernelGGL(merge_grouped_kernel<ScanGroupLists>, dim3(nq), dim3(256), 0, stream, ScanGroupLists{s.part_d, s.part_i, s.part_g, blocks, depth, 0},
                     blocks, depth, args.id_base, ids, out_groups, dists, s.dists64);
  VTC_LAUNCH_CHECK2("l2_search_grouped_after", "merge");
  return 0;
}
}  // namespace

extern "C" size_t vtc_l2_group_ban_words(int n_queries, int n_groups) {
  if (n_queries < 1 || n_queries > SEARCH_MAX_Q || n_groups < 1) return 0;
  return (size_t)n_queries * (((size_t)n_groups + 31) / 32);
}

extern "C" int vtc_l2_group_mark_before(const void *gallery, int gallery_is_half, const float *queries, const uint32_t *live, const int32_t *groups,
                                        int n_groups, const double *after_d, const int64_t *after_i, int ng, int nq, int d, int64_t id_base,
                                        uint32_t *ban, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  VTC_CHECK(gallery && queries && groups && after_d && after_i && ban, "l2_group_mark_before (the grouped search's cursor): null argument");
  VTC_CHECK(ng >= 1, "l2_group_mark_before (the grouped search's cursor): n_gallery=%d must be at least 1", ng);
  VTC_CHECK(nq >= 1 && nq <= SEARCH_MAX_Q, "l2_group_mark_before (the grouped search's cursor): n_queries=%d must be in [1, %d]", nq, SEARCH_MAX_Q);
  VTC_CHECK(n_groups >= 1, "l2_group_mark_before (the grouped search's cursor): n_groups=%d must be in [1, 2^31)", n_groups);
  VTC_CHECK(d >= 64 && d <= SEARCH_MAX_D && d % 64 == 0,
            "l2_group_mark_before (the grouped search's cursor): d=%d must be a multiple of 64 in [64, %d]", d, SEARCH_MAX_D);
  VTC_CHECK(id_base >= 0 && id_base <= INT64_MAX - ng,
            "l2_group_mark_before (the grouped search's cursor): id_base=%lld must be non-negative (and id_base + n_gallery an int64)",
            (long long)id_base);
  const AfterArgs args{after_d, after_i, id_base};
  const SearchPlan p = search_plan(nq);
  if (gallery_is_half) launch_mark_tile(p, reinterpret_cast<const _Float16 *>(gallery), queries, live, groups, n_groups, args, ng, nq, d, ban, stream);
  else launch_mark_tile(p, reinterpret_cast<const float *>(gallery), queries, live, groups, n_groups, args, ng, nq, d, ban, stream);
  VTC_LAUNCH_CHECK("l2_group_mark_before");
  return 0;
}

extern "C" int vtc_l2_search_grouped_after(const void *gallery, int gallery_is_half, const float *queries, const uint32_t *live,
                                           const int32_t *groups, int n_groups, const uint32_t *ban, const int64_t *exclude, const double *after_d,
                                           const int64_t *after_i, int ng, int nq, int d, int depth, int64_t id_base, int64_t *ids,
                                           int32_t *out_groups, float *dists, int *nonfinite, void *ws, size_t ws_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  VTC_CHECK(gallery && queries && groups && ban && after_d && after_i && ids && out_groups, "l2_search_grouped_after: null argument");
  VTC_CHECK(ng >= 1, "l2_search_grouped_after: n_gallery=%d must be at least 1", ng);
  VTC_CHECK(nq >= 1 && nq <= SEARCH_MAX_Q, "l2_search_grouped_after: n_queries=%d must be in [1, %d]", nq, SEARCH_MAX_Q);
  VTC_CHECK(n_groups >= 1, "l2_search_grouped_after: n_groups=%d must be in [1, 2^31)", n_groups);
  VTC_CHECK(depth >= 1 && depth <= SEARCH_MAX_DEPTH && depth <= ng, "l2_search_grouped_after: depth=%d must be in [1, min(%d, n_gallery)]", depth,
            SEARCH_MAX_DEPTH);
  VTC_CHECK(d >= 64 && d <= SEARCH_MAX_D && d % 64 == 0, "l2_search_grouped_after: d=%d must be a multiple of 64 in [64, %d]", d, SEARCH_MAX_D);
  VTC_CHECK(id_base >= 0 && id_base <= INT64_MAX - ng,
            "l2_search_grouped_after: id_base=%lld must be non-negative (and id_base + n_gallery an int64)", (long long)id_base);
  const SearchWs s = search_ws(ws, ng, nq, depth, true);
  VTC_CHECK(ws && ws_bytes >= s.total, "l2_search_grouped_after: workspace too small (%zu < %zu)", ws_bytes, s.total);
  const AfterArgs args{after_d, after_i, id_base, exclude, ban, n_groups};
  if (gallery_is_half)
    return search_grouped_after(reinterpret_cast<const _Float16 *>(gallery), queries, live, groups, args, ng, nq, d, depth, ids, out_groups, dists,
                                nonfinite, s, stream);
  return search_grouped_after(reinterpret_cast<const float *>(gallery), queries, live, groups, args, ng, nq, d, depth, ids, out_groups, dists,
                              nonfinite, s, stream);
}
