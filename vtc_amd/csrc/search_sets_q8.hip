// search_sets_q8.hip -- SET QUERIES over a q8 gallery (include/vtc_hip.h, vtc_l2_search_sets_q8): search_sets.hip's table with q8_t as
// the gallery's element type -- the SET scans plain, GROUPED, GROUPED + EXCL and the ungrouped excluding scan, each with and without
// MASKED, in every tile shape -- and the entry.  The workspace is vtc_l2_search_sets_workspace_bytes: it does not know how rows are stored.
#include "search_scan.h"

extern "C" int vtc_l2_search_sets_q8(const void *gallery, const float *queries, const uint32_t *live, const int32_t *groups, const int64_t *exclude,
                                     int ng, int n_sets, int set_size, int d, int depth, int64_t id_base, int64_t *ids, int32_t *out_groups,
                                     float *dists, int *nonfinite, void *ws, size_t ws_bytes, void *stream) {
  const bool shape_ok = n_sets >= 1 && set_size >= 1 && (long long)n_sets * set_size <= SEARCH_MAX_Q;
  SearchCall c{gallery, false, queries, live, groups, nullptr, nullptr, exclude, nullptr, 0, ng, shape_ok ? n_sets * set_size : 0, d,
               depth, id_base, ids, out_groups, dists, nonfinite, ws, ws_bytes, stream, true};
  c.sets = true;
  c.n_sets = n_sets;
  c.set_size = set_size;
  return search_entry_of<vtcsweep::q8_t, true>("l2_search_sets", c);
}
