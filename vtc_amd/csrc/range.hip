// range.hip -- range search: EVERY row of a stored gallery within a squared-distance threshold of a few queries (1 .. 64), exact, however
// many rows that is.  search.hip answers "the nearest k, k <= 64" with one list entry per lane; here the output's size depends on the data,
// so the work is split in two calls around the one number the host has to know before it can allocate:
//
//   vtc_l2_range_count   one pass over the gallery (the scan's structure: the query tile in the LDS, search.hip's tile shapes, the mask
//                        word of the next unit read ahead, dead steps that issue no load, G = float or _Float16), the fp64 distances
//                        formed by sweep_common.h's wave_dist64_queries and compared with the query's radius IN FP64.  Leaves one bit
//                        per (query, row) -- the HIT WORDS, vtc_row_mask_pack's format -- and lims, the prefix sum of the hit counts.
//   vtc_l2_range_fill    walks the non-zero hit words, forms the distances of the hits again through the same function (the same bits)
//                        and writes ids / dists at positions that come from counts and prefix sums alone.
//
//   range_count_kernel<NQ, NR, MASKED, G>
//                        a grid of persistent workgroups.  A wave's unit of work is ONE hit word: the 32 rows 32 w .. 32 w + 31, 32 / NR
//                        steps of NR rows; wave gw of GW takes the words gw, gw + GW, ...  It owns the word of each of its tile's
//                        queries -- builds it in a register, writes it with a plain store, zero words included (the workspace is not
//                        cleared) -- and adds the popcounts into per-workgroup counts, one slot per (query, workgroup): no atomics.
//   range_prefix_kernel  (range_common.h: it follows range_many.hip's count pass too) one workgroup per query: lims[q + 1] = the sum of the counts of the queries 0 .. q, and the CHUNK BASES of its
//                        own words: the number of hits before every chunk of 16 words (512 rows).
//   range_fill_kernel<G> a wave per (query, chunk): 16 words in 16 lanes, nothing else is read when all are zero.  The hits are taken in
//                        ascending row order, four rows a step; position = lims[q] + chunk base + hits so far.  Stores are bounded by
//                        `capacity` and the rows by n_gallery whatever the workspace holds.
//
// No atomic decides a position and every word has one writer, so the result does not depend on the grid.  Not here: a grouped
// (distinct-video) range search, sharding over several devices, more than 64 queries a call.
// The kernels and the two calls are templates over G in range_common.h, which range_q8.hip shares; this file holds the entries and,
// through them, the float and _Float16 instantiations.
#include "range_common.h"      // also the limits, the workspace's head and range_prefix_kernel: range_many.hip's pass is followed by them too

extern "C" size_t vtc_l2_range_workspace_bytes(int n_gallery, int n_queries, int d) {
  if (!range_args_ok(n_gallery, n_queries, d)) return 0;
  return range_ws(nullptr, n_gallery, n_queries).total;
}

extern "C" int vtc_l2_range_count(const void *gallery, int gallery_is_half, const float *queries, const uint32_t *live, const double *radius2,
                                  int ng, int nq, int d, int64_t *lims, int *nonfinite, void *ws, size_t ws_bytes, void *stream) {
  return gallery_is_half ? range_count<_Float16>(gallery, queries, live, radius2, ng, nq, d, lims, nonfinite, ws, ws_bytes, stream)
                         : range_count<float>(gallery, queries, live, radius2, ng, nq, d, lims, nonfinite, ws, ws_bytes, stream);
}

extern "C" int vtc_l2_range_fill(const void *gallery, int gallery_is_half, const float *queries, int ng, int nq, int d, const int64_t *lims,
                                 int64_t capacity, int64_t id_base, int64_t *ids, float *dists, double *dists64, void *ws, size_t ws_bytes,
                                 void *stream) {
  return gallery_is_half ? range_fill<_Float16>(gallery, queries, ng, nq, d, lims, capacity, id_base, ids, dists, dists64, ws, ws_bytes, stream)
                         : range_fill<float>(gallery, queries, ng, nq, d, lims, capacity, id_base, ids, dists, dists64, ws, ws_bytes, stream);
}
