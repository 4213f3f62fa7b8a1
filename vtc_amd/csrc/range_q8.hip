// range_q8.hip -- the range search over a q8 gallery (include/vtc_hip.h, vtc_l2_range_count_q8 / vtc_l2_range_fill_q8): range.hip's two
// passes (range_common.h) with q8_t as the gallery's element type -- the 8 count passes and the fill pass -- and their entries.  The
// workspace is vtc_l2_range_workspace_bytes, the hit words and lims are range.hip's: the passes differ in the row loader alone.
#include "range_common.h"

extern "C" int vtc_l2_range_count_q8(const void *gallery, const float *queries, const uint32_t *live, const double *radius2, int ng, int nq, int d,
                                     int64_t *lims, int *nonfinite, void *ws, size_t ws_bytes, void *stream) {
  return range_count<vtcsweep::q8_t>(gallery, queries, live, radius2, ng, nq, d, lims, nonfinite, ws, ws_bytes, stream);
}

extern "C" int vtc_l2_range_fill_q8(const void *gallery, const float *queries, int ng, int nq, int d, const int64_t *lims, int64_t capacity,
                                    int64_t id_base, int64_t *ids, float *dists, double *dists64, void *ws, size_t ws_bytes, void *stream) {
  return range_fill<vtcsweep::q8_t>(gallery, queries, ng, nq, d, lims, capacity, id_base, ids, dists, dists64, ws, ws_bytes, stream);
}
