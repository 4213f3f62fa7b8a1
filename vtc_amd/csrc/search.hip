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
// The scan, the merge, their lists, the mark pass, the pair distances and the host driver are in search_scan.h, which search_sets.hip and
// the q8 files (search_q8.hip, search_sets_q8.hip) share; this file holds the mask packer and the entries -- and, through the entries,
// every non-SET instantiation over float and _Float16 galleries.
//
// G is the gallery's element type.  q8_t (8-bit codes and a scale a row) is search_q8.hip's.  _Float16 (rows stored as IEEE binary16) differs in the row loader alone (sweep_common.h, row_piece):
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
//   SET       the NQ queries of a tile are the MEMBERS of one set query, whose distance to a row is the minimum over them (include/vtc_hip.h,
//             vtc_l2_search_sets): the tile keeps ONE list, a row's candidate is the fmin over the tile's live members of distances the
//             step has formed anyway, and it meets `beats` once -- NQ - 1 fmin a row, one compare on the rejecting path instead of NQ,
//             the insertion path as it is.  The flag rides on G (scan_kernel<SetOf<G>, ...>, search_scan.h) and its instantiations --
//             plain, GROUPED, GROUPED + EXCL and the excluding scan without its cursor -- are search_sets.hip's.
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
//
// A SET of more than one tile (9 .. 64 members) is the same argument with "part" read as "the members of one tile": every tile scans the
// whole gallery for the minimum over ITS members, and one merge per set runs over the lists of all its tiles' workgroups.  A row (group)
// of the set's first `depth` has its minimum in some tile.  In that tile fewer than `depth` rows (groups) are nearer, since a tile's
// minimum is never below the set's: that tile's list holds the entry, at the set's distance.  Ungrouped, the same row can now sit in
// the lists of different tiles at different distances, which no other search's parts can; it must come out once, with the smaller one.
// The grouped list does exactly that when a row's group is the row itself (ScanRowLists), and the stale, worse entries are absorbed
// by the insertion as a group's are.  Grouped, merge_kernel<ScanLists, true> is used unchanged.  This is also why a set search has no
// cursor: a tile could only test a row against its own minimum, not the set's.
#include "search_scan.h"

namespace {
using namespace vtcsweep;

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
  return gallery_is_half ? mark_before<_Float16>(gallery, queries, live, groups, n_groups, after_d, after_i, ng, nq, d, id_base, ban, stream)
                         : mark_before<float>(gallery, queries, live, groups, n_groups, after_d, after_i, ng, nq, d, id_base, ban, stream);
}

extern "C" int vtc_l2_pair_dists64(const void *gallery, int gallery_is_half, const float *queries, const int64_t *rows, int ng, int nq, int d,
                                   int64_t id_base, double *out, void *stream) {
  return gallery_is_half ? pair_dists64<_Float16>(gallery, queries, rows, ng, nq, d, id_base, out, stream)
                         : pair_dists64<float>(gallery, queries, rows, ng, nq, d, id_base, out, stream);
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
