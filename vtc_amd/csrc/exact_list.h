// exact_list.h -- the exact finish, shared by everything that makes an approximate candidate list exact again or ranks rows in fp64:
// the sorted fp64 (distance, index) list with one entry per lane and its merge (the scan and merge of search_scan.h, the fallbacks and
// the rescan), the brute-force scan of one query over a gallery (exact_fallback_kernel of sweep_topk.hip, many_fallback_kernel of
// search_many.hip), and the fp64 re-rank of the candidates a wave holds one per lane (exact_rerank_kernel, many_finish_kernel).  One
// copy: every user forms the same doubles (sweep_common.h) and orders them by the same compare, so their results agree bit for bit.
#pragma once
#include "search_walk.h"

#include <algorithm>

namespace {
using namespace vtcsweep;

constexpr int EMPTY_ROW = 0x7fffffff;         // index of an empty list slot (distance +inf)
constexpr long long EMPTY_ID = 0x7fffffffffffffffll;

// A sorted list of (fp64 distance, index) keys, one entry per lane, ascending; the first `depth` lanes are the list, (tau, tau_i) its last
// key, wave-uniform.  Empty slots hold (+inf, EMPTY).  Ungrouped, this is the list of the sweeps' fallback and rescan too (sweep_topk.hip),
// which ask `precedes` where the scans ask `beats`.
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
  // the same without the finiteness clause: a row at +inf (a gallery row holding an inf) is a row and takes an empty slot, which the
  // sweeps' contract asks for and the scans' forbids
  __device__ __forceinline__ bool precedes(double cv, I ci) const { return cv < tau || (cv == tau && ci < tau_i); }
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
  // FINITE: `beats` decides, else `precedes`
  template <bool FINITE = true>
  __device__ __forceinline__ void offer(double cv, I ci, int cg, int lane, int depth) {
    if (FINITE ? beats(cv, ci) : precedes(cv, ci)) insert(cv, ci, cg, lane, depth);
  }
};

// Merges the sorted lists list0, list0 + stride, ... < nlists into wl, 64 lists at a time: lane l follows list l0 + l entry by entry
// (src.get<grouped>(list, e, cv, ci, cg): the entry, cv = +inf for an empty one, cg its group for a grouped list) and drops out at the
// first entry that does not beat the current depth-th -- the rest of a sorted list cannot either.  The entries that do are offered one
// by one; an entry that beats the depth-th but whose group a better entry holds is dropped by the insertion and the lane goes on.
// FINITE = false: `precedes` in the place of `beats`, for lists that hold rows at +inf (an empty entry precedes nothing either way).
template <bool FINITE = true, typename List, typename Src>
__device__ __forceinline__ void merge_lists(List &wl, Src src, int nlists, int list0, int stride, int depth, int lane) {
  for (int l0 = list0; l0 < nlists; l0 += stride) {       // wave-uniform
    const int l = l0 + lane;
    bool alive = l < nlists;
    for (int e = 0; e < depth; ++e) {
      double cv = INFINITY;
      long long ci = EMPTY_ID;
      int cg = 0;
      if (alive) src.template get<List::grouped>(l, e, cv, ci, cg);
      alive = alive && (FINITE ? wl.beats(cv, ci) : wl.precedes(cv, ci));
      unsigned long long m = __ballot(alive);
      if (!m) break;
      while (m) {
        const int from = __ffsll((long long)m) - 1;
        m &= m - 1;
        if constexpr (List::grouped) wl.template offer<FINITE>(__shfl(cv, from, 64), __shfl(ci, from, 64), __shfl(cg, from, 64), lane, depth);
        else wl.template offer<FINITE>(__shfl(cv, from, 64), __shfl(ci, from, 64), 0, lane, depth);
      }
    }
  }
}

// the waves' lists of a workgroup in the LDS: sd / si / sg [waves][64].  I: how the index is kept there (search_scan.h).
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

// The first `depth` lanes write their entry of result row `row`: the id (id_base + index), the fp32 and the fp64 distance (both nullable);
// an empty slot is -1 / +inf.
template <typename I, I EMPTY, bool GROUPED>
__device__ __forceinline__ void write_result_row(const SortedList<I, EMPTY, GROUPED> &wl, size_t row, int depth, int lane, int64_t id_base,
                                                 int64_t *__restrict__ ids, float *__restrict__ dists, double *__restrict__ dists64) {
  if (lane >= depth) return;
  const size_t o = row * depth + lane;
  const bool empty = wl.bi == EMPTY;
  ids[o] = empty ? -1 : id_base + wl.bi;
  if (dists) dists[o] = empty ? INFINITY : (float)wl.bd;
  if (dists64) dists64[o] = empty ? (double)INFINITY : wl.bd;
}

// The brute force behind an uncertified list: query row `qrow` against every row of the gallery (of G: float or _Float16) whose bit of
// `live` is set (null: every row), in fp64, by a workgroup of NW waves.  Wave w takes the steps w, w + NW, ... of four rows through
// wave_dist64_queries<1, 4>; a dead slot of a step, or one past the gallery, is pointed at a live row of the step and its result dropped,
// as step_rows does (search_walk.h), so a dead row's memory is never read.  The waves' lists go through sd / si [NW][64] in the LDS and
// wave 0 returns their merge, the first `depth` rows by (distance, row); the other waves return an empty list.  FINITE: a row with a
// non-finite distance is rejected (the scan's contract); without it a row at +inf is listed behind the finite ones (the sweep's).
// The caller puts a barrier before sd / si are written again.
template <bool FINITE, int NW, typename G>
__device__ __forceinline__ SortedList<long long, EMPTY_ID, false> fallback_scan(const float *__restrict__ qrow, const G *__restrict__ gallery,
                                                                                const unsigned *__restrict__ live, int ng, int d, int depth,
                                                                                double *sd, long long *si) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  SortedList<int, EMPTY_ROW, false> wl;
  wl.init();
  for (long long j0 = (long long)wave * 4; j0 < ng; j0 += NW * 4) {
    unsigned bits = ng - j0 >= 4 ? 0xfu : (1u << (ng - j0)) - 1;
    if (live) bits &= (unsigned)uniform_of((int)(live[j0 >> 5] >> (j0 & 31)));
    if (!bits) continue;
    int jj[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) jj[r] = (int)j0 + (((bits >> r) & 1) ? r : __ffs((int)bits) - 1);
    double dist[4];
    wave_dist64_queries<1, 4>(qrow, gallery, jj, d, lane, dist);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if ((bits >> r) & 1) wl.template offer<FINITE>(dist[r], jj[r], 0, lane, depth);
  }
  sd[wave * 64 + lane] = wl.bd;
  si[wave * 64 + lane] = wl.bi == EMPTY_ROW ? EMPTY_ID : (long long)wl.bi;
  __syncthreads();
  SortedList<long long, EMPTY_ID, false> m;
  m.init();
  if (wave == 0) merge_lists<FINITE>(m, LdsLists<long long>{sd, si, nullptr}, NW, 0, 64, depth, lane);
  return m;
}

// The fp64 re-rank of the candidates a wave holds one per lane: `my` is the lane's gallery row (negative: absent; Idx is int where the
// rows are, as a 64-bit shuffle is two), the lanes [0, n_loop) -- wave-uniform -- are looked at.  Eight candidates a step (one at a time
// the loop is a chain of dependent gather latencies), by the one distance loop of sweep_common.h: the fallbacks and the scans form the
// same doubles.  An absent slot reads row 0; its result is dropped.
// md: the lane's distance to query row q, +inf when absent.  Returns the lane's rank among the present candidates by (distance, row).
template <typename G, typename Idx>
__device__ __forceinline__ int rerank64(const float *__restrict__ q, const G *__restrict__ gallery, Idx my, int n_loop, int d, int lane, double &md) {
  md = INFINITY;
  constexpr int NB = 8;                                    // candidates per step
  for (int c0 = 0; c0 < n_loop; c0 += NB) {
    Idx jj[NB], rows[NB];
    double sacc[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      jj[u] = c0 + u < n_loop ? __shfl(my, c0 + u, 64) : -1;      // wave-uniform
      rows[u] = jj[u] < 0 ? 0 : jj[u];
    }
    wave_dist64_core<NB>([&](int) { return q; }, [&](int u) { return gallery + (size_t)rows[u] * d; }, d, lane, sacc);
#pragma unroll
    for (int u = 0; u < NB; ++u)
      if (jj[u] >= 0 && lane == c0 + u) md = sacc[u];
  }
  int rank = 0;                                            // absent slots sort last
  for (int c = 0; c < n_loop; ++c) {
    const double od = __shfl(md, c, 64);
    const Idx oi = __shfl(my, c, 64);
    if (oi >= 0 && (od < md || (od == md && oi < my))) ++rank;
  }
  return rank;
}

// candidate list depth of an exact finish: 21 spare ranks behind the requested ones, at least 32, at most 64 / n_gallery
inline int exact_cdepth(int depth, int ng) { return std::min(std::min(64, ng), std::max(32, depth + 21)); }

}  // namespace
