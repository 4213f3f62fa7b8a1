// search_sets.hip -- SET QUERIES of the query-time search: several vectors as one query, the minimum over them (include/vtc_hip.h,
// vtc_l2_search_sets).  The scan, the merge and the driver are search.hip's (search_scan.h), instantiated with SET: a tile's NQ queries
// are members of one set, the tile keeps one list, and a set of several tiles is merged once over all its tiles' lists.  This file holds
// the entries and, through them, the SET instantiations: plain, GROUPED, GROUPED + EXCL and the ungrouped excluding scan, each with and
// without MASKED, for float and _Float16 galleries, in every tile shape.
#include "search_scan.h"

extern "C" size_t vtc_l2_search_sets_workspace_bytes(int n_gallery, int n_sets, int set_size, int d, int depth, int grouped) {
  if (n_sets < 1 || set_size < 1 || (long long)n_sets * set_size > SEARCH_MAX_Q || !search_args_ok(n_gallery, n_sets * set_size, d, depth)) return 0;
  return search_ws(nullptr, n_gallery, n_sets, depth, grouped != 0, tile_plan(set_size).tiles).total;
}

extern "C" int vtc_l2_search_sets(const void *gallery, int gallery_is_half, const float *queries, const uint32_t *live, const int32_t *groups,
                                  const int64_t *exclude, int ng, int n_sets, int set_size, int d, int depth, int64_t id_base, int64_t *ids,
                                  int32_t *out_groups, float *dists, int *nonfinite, void *ws, size_t ws_bytes, void *stream) {
  const bool shape_ok = n_sets >= 1 && set_size >= 1 && (long long)n_sets * set_size <= SEARCH_MAX_Q;
  SearchCall c{gallery, gallery_is_half != 0, queries, live, groups, nullptr, nullptr, exclude, nullptr, 0, ng, shape_ok ? n_sets * set_size : 0, d,
               depth, id_base, ids, out_groups, dists, nonfinite, ws, ws_bytes, stream, true};
  c.sets = true;
  c.n_sets = n_sets;
  c.set_size = set_size;
  return search_entry<true>("l2_search_sets", c);
}
