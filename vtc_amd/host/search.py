"""Query-time search: a stored gallery of video embeddings and the nearest videos of a few text queries.

Every other retrieval entry point of the package is an evaluation -- N paired rows in, a recall figure or N ranks out.  ``VideoIndex``
is what a retrieval model is for:

    index = VideoIndex(512)
    index.add(video_embeddings)                       # [n, 512] fp32, any number of times
    ids, scores = index.search_text(model, title_tokens, k=10)

The search is exact: fp64 squared distances of the stored fp32 rows, ties to the earlier row (libvtc_hip.so, vtc_l2_search for up to
``ROUTE_TOPK_MIN_QUERIES - 1`` queries, vtc_l2_topk(EXACT) above; both return the same ids by construction).  No CPU path.

Rows can go away and a query can search part of the gallery; both are one bit per row that the scan reads (vtc_l2_search_masked):

    index.remove([17, 42])                            # ids are never reused, nothing is renumbered or compacted
    cats = index.subset(subreddit_of_row == 3)        # bool [ntotal] or ids; reusable across queries
    ids, scores = index.search_text(model, title_tokens, k=10, subset=cats)

A video can own several rows -- a title and its comments, many captions, the chunks of a long video -- and then the k nearest distinct
VIDEOS are what a query wants, each by its nearest row (vtc_l2_search_grouped: the de-duplication happens inside the scan, exactly):

    index.add(caption_embeddings, video_ids=video_of_caption)      # int [n] in [0, 2^31); a video's rows in any number of calls
    videos, rows, scores = index.search_videos(queries, k=10)
    index.remove_videos([7, 9])

The rows can be stored as IEEE half, half the memory and half the bytes a one-query search streams (vtc_l2_search_half):

    index = VideoIndex(512, storage=torch.float16)    # or: index = fp32_index.converted(torch.float16)

A stored row is then the unit row rounded to nearest-even to the 11 significant bits of binary16 per component.  The search stays exact
over the rows AS STORED: the fp64 distances of the fp32 queries and the widened half rows, bit for bit what an fp32 index holding those
widened rows returns.

Or as 8-bit codes with one fp32 scale a row, the scalar quantiser of every vector-search library (vtc_quantize_rows_q8 / vtc_l2_search_q8):

    index = VideoIndex(512, storage=torch.int8)       # or: index = fp32_index.converted(torch.int8)

A stored row is then ``width`` signed bytes and its scale, width + 16 bytes: (width + 16) / (4 width) of fp32, 0.258 at 512 columns.  The
loss happens once, at ``add``; every search stays exact over the rows AS STORED, bit for bit what an fp32 index holding the dequantised
rows returns.  It saves memory, not time (profiles/search_q8.md: one query over 10^6 rows takes 385 us, the fp32 scan 390, the half scan
271; from 8 queries on the three are equal within 1 %).

Every search above returns the nearest k, k <= 64.  The other question -- WHICH rows score at least s, however many -- is the range
search (vtc_l2_range_count / vtc_l2_range_fill: the same fp64 distances, compared with the threshold in fp64):

    lims, ids, scores = index.range_search(queries, min_score=0.9)     # query i's hits: ids[lims[i]:lims[i + 1]], nearest first
    counts = index.range_count(queries, min_score=0.9)                 # how many, without fetching them: no host sync
    near = index.range_subset(query, min_score=0.8)                    # the hits of one query as a RowSubset: filters chain

The range search has a batch form too, for the workloads that ask many range questions at once -- near-duplicate and repost detection,
which asks of every stored row which other rows score at least s, and thresholded retrieval for a batch of texts.  On a half index 64
queries are ONE pass of the stored rows through the matrix cores, and only the pairs the pass's error bound cannot decide are taken in
fp64 (vtc_l2_range_count_many_half); the result is ``range_search``'s, bit for bit:

    lims, ids, scores = index.range_search_many(queries, min_score=0.9)  # and range_count_many: range_search / range_count for a batch
    lims, ids, scores = index.similar_within(row_ids, min_score=0.9)     # the range form of ``similar``: stored rows, each without itself
    pairs, scores = index.near_duplicates(min_score=0.9)                 # every pair a < b of live rows that score at least 0.9

Between the two lies "the next page", and a ranking deeper than 64 -- a re-ranker, a hard-negative miner, recall at 100 or 1000.  The
search order is a total order on (fp64 distance, row), so "the k nearest rows after row r" is well defined and needs no state
(vtc_l2_search_after: a cursor in the scan):

    ids2, scores2 = index.search(queries, 10, after=ids[:, -1])        # the next 10 of every query; chain as long as needed
    ids, scores = index.search_deep(queries, 500)                      # the exact 500 nearest: pages of 64, concatenated

And a query can name ONE row, or one video, that it must not be given -- the row it was taken from ("more like this"), the video a
training text belongs to (hard negatives).  A per-query compare in the scan, for a whole batch in one gallery pass per tile of 8
(vtc_l2_search_excluding; a ``subset`` holds for the whole batch and cannot say this):

    ids, scores = index.similar(row_ids, 10)                           # the nearest rows of STORED rows, each without itself
    videos, rows, scores = index.similar_videos(row_ids, 10)           # grouped: the nearest other videos of a row's video
    videos, rows, scores = index.search_videos(text_queries, 10, exclude_videos=video_of_text)      # hard negatives

The grouped order pages too -- recall at 100 or 1000 over videos with several captions, hard negatives below rank 64, a re-ranker's
few hundred candidate videos.  "The videos after row r" cannot be asked of a row by itself: a row after the cursor counts only if no row
of its video lies at or before it, anywhere in the gallery.  So a page is two gallery passes, one that marks the videos already behind
the cursor in a per-query bitmap and the scan that skips them (vtc_l2_group_mark_before / vtc_l2_search_grouped_after), still exact and
stateless:

    videos2, rows2, scores2 = index.search_videos(queries, 10, after=rows[:, -1])     # the next 10 distinct videos of every query
    videos, rows, scores = index.search_videos_deep(queries, 300)                      # the exact 300 nearest videos: pages of 64

A query can also be SEVERAL vectors, any of which may match -- a title and its comments, the captions or chunks of a whole video,
paraphrases.  The set's distance to a row is the minimum over its members, taken inside the scan on distances it forms anyway
(vtc_l2_search_sets), so nothing is merged, sorted or de-duplicated on the host:

    ids, scores = index.search_any(query_sets, 10)                                     # [S, M, dim]: S queries of M members each
    videos, rows, scores = index.search_videos_any(query_sets, 10, sizes=[3, 9, 1])    # ragged sets, distinct videos
    videos, rows, scores = index.similar_to_video(video_ids, 10)                       # the videos nearest to a video, by any of its rows
"""
from __future__ import annotations

import torch

from .. import _lib as L
from .. import ops

__all__ = ["VideoIndex", "RowSubset"]


def _video_id_tensor(video_ids, n, device, what):
    """An integer [n] sequence or tensor with values in [0, 2^31) -> int32 [n] on ``device``; anything else raises ValueError (a
    device-to-host read when n > 0)."""
    v = torch.as_tensor(video_ids)
    if v.numel() == 0 and not n:                               # an empty list has no dtype to speak of
        return torch.empty(0, dtype=torch.int32, device=device)
    if v.dtype == torch.bool or v.is_floating_point() or v.is_complex():
        raise ValueError(f"VideoIndex.{what}: video_ids must be integers, got {v.dtype}")
    if n is not None and tuple(v.shape) != (n,):
        raise ValueError(f"VideoIndex.{what}: video_ids must be [{n}], one per row, got {tuple(v.shape)}")
    v = v.to(device=device).reshape(-1)
    if v.numel() and (int(v.min()) < 0 or int(v.max()) >= 2 ** 31):
        raise ValueError(f"VideoIndex.{what}: video_ids must be in [0, 2^31), got {int(v.min())} .. {int(v.max())}")
    return v.to(torch.int32)


def _id_tensor(ids, ntotal, device, what):
    """An int64 id sequence or tensor -> int64 [m] on ``device``; an id outside [0, ntotal) raises ValueError (a device-to-host read)."""
    ids = torch.as_tensor(ids)
    if ids.numel() == 0:
        return torch.empty(0, dtype=torch.int64, device=device)
    if ids.dtype == torch.bool or ids.is_floating_point() or ids.is_complex():
        raise ValueError(f"VideoIndex.{what}: ids must be integers, got {ids.dtype}")
    ids = ids.to(device=device, dtype=torch.int64).reshape(-1)
    if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= ntotal):
        raise ValueError(f"VideoIndex.{what}: ids must be in [0, ntotal = {ntotal}), got {int(ids.min())} .. {int(ids.max())}")
    return ids


class RowSubset:
    """The rows of one VideoIndex a query may return (``VideoIndex.subset``): built once, passed to any number of searches.  Rows added
    to the index afterwards are not members.  It keeps its packed words ANDed with the index's live rows and packs them again (one
    launch, vtc_row_mask_pack) only when the index has changed since -- a query with an unchanged subset adds no launch and no host sync
    over an unmasked one."""

    def __init__(self, index, flags):
        self.index = index
        self._flags = flags                 # uint8 [ntotal when built or last refreshed]
        self._words = None
        self._generation = -1

    def words(self):
        index = self.index
        if self._generation != index._generation:
            n = index.ntotal
            if self._flags.shape[0] > n:
                raise ValueError(f"RowSubset: built for {self._flags.shape[0]} rows, the index now holds {n} (its state was reloaded)")
            if self._flags.shape[0] < n:
                self._flags = torch.nn.functional.pad(self._flags, (0, n - self._flags.shape[0]))
            self._words = ops.row_mask_pack(self._flags, and_mask=index._live_words())
            self._generation = index._generation
        return self._words


class VideoIndex:
    """A gallery of fp32 rows on the GPU with exact nearest-row search.  Ids are positions in insertion order and are never reused:
    ``ntotal`` counts the rows ever added, ``len(index)`` the live ones, ``remove`` only clears a row's bit (no compaction, no
    renumbering; the memory stays).  With nothing removed and no ``subset`` a search is routed as the constants below say; otherwise it
    is the masked scan (vtc_l2_search_masked) for any number of queries, in slices of 64 -- vtc_l2_topk has no mask.
    ``storage=torch.float16`` keeps the rows as IEEE half (``index.storage``): ``add`` normalises in fp32 and rounds to nearest-even, so
    a stored row is the unit row rounded to 11 significant bits per component, and every search is exact over those stored rows (scores
    are 1 - D/2 of them).  A half index ALWAYS searches with the scan (vtc_l2_search_half), in slices of 64 queries and by the masked
    route's rules: vtc_l2_topk reads fp32 rows, so ROUTE_TOPK_MIN_QUERIES does not apply, and many-query batches are slower than on
    an fp32 index (profiles/search.md: the scan takes 4.5 x vtc_l2_topk's time at 64 queries) -- through ``search``.  ``search_many``
    is the batch form: the same result, and on a half index with k <= 32 one pass of the stored rows through the matrix cores per 64
    queries with an exact fp64 finish (vtc_l2_search_many_half, profiles/search_many.md).  ``converted`` moves an index over.
    ``range_search_many`` / ``range_count_many`` are the batch forms of the range search: the same result, and on a half index from
    ROUTE_RANGE_MANY_MIN_QUERIES queries on one pass of the stored rows through the matrix cores per 64 queries, the pairs inside the
    error band decided in fp64 (vtc_l2_range_count_many_half, profiles/range_many.md); ``similar_within`` (the range form of
    ``similar``) and ``near_duplicates`` (every pair of live rows above a score) are built on them and run through the scan on an fp32
    index.
    ``storage=torch.int8`` keeps every row as ``width`` signed 8-bit codes and one fp32 scale (``index.rows`` is int8 [ntotal, width + 16]:
    the codes, the scale at byte ``width``, 12 zero bytes): ``add`` normalises in fp32 and quantises with one kernel launch
    (ops.quantize_rows_q8: scale = max |x| / 127 rounded up to 16 significant bits, code = the quotient rounded to nearest even, so
    |x - scale * code| <= 0.5 (1 + 2^-15) scale), and every search is exact over the stored values scale * code -- bit for bit the search
    of an fp32 index holding ``ops.dequantize_rows_q8(index.rows)``.  An int8 index searches by the half index's rules (always the scan,
    vtc_l2_search_q8 and its siblings, slices of 64 queries, only enqueued); ``search_many`` / ``range_search_many`` /
    ``range_count_many`` ARE the scan on it, the matrix-core passes read half rows only.  The memory is (width + 16) / (4 width) of an
    fp32 index's.  The time is not less (profiles/search_q8.md, d = 512, depth 11): one query over 10^6 rows takes 385 us against the
    fp32 scan's 390 and the half scan's 271 (1.42 x half), over 10^5 rows 91 against 87 and 82; at 8 and 64 queries all three storages
    take the same time within 1 %.  On that file's synthetic rows the int8 index returned 97.2 - 100 % of the fp32 index's top 10 and
    moved no score by more than 1.6e-3.
    ``exclude`` / ``exclude_videos`` (one row or one video per query that it is never given), ``similar`` and ``similar_videos`` (the
    neighbours of a stored row without itself / without its own video) are the excluding scan (vtc_l2_search_excluding), by the same
    rules: any number of queries in slices of 64, only enqueued.  ``search_videos(after=)`` and ``search_videos_deep`` page the grouped
    order (vtc_l2_group_mark_before + vtc_l2_search_grouped_after, two gallery passes a page)."""
    #: queries per call from which search() goes through ops.l2_topk(precision=SWEEP_EXACT) instead of ops.l2_search (which takes up to
    #: 64 per call; an instance that sets the constant above that gets the scan in slices, as every masked search does).  Measured, profiles/search.md (d = 512, depth 11, medians of 30 alternating calls; us at 10^5 / 10^6 gallery rows, scan vs
    #: vtc_l2_topk): the scan's time grows with the number of queries (one gallery pass per started tile of 8), vtc_l2_topk's does not.
    #:    8 queries   244.4 vs 275.6 (1.13 x)   1 468.9 vs 2 229.0 (1.52 x)   scan faster
    #:    9           358.8 vs 386.6 (1.08 x)   2 818.6 vs 3 768.7 (1.34 x)   scan faster
    #:   10           366.8 vs 384.2 (1.05 x)   2 840.9 vs 3 759.1 (1.32 x)   scan faster at 10^6, within 5 % at 10^5
    #:   11           373.0 vs 383.1 (1.03 x)   2 883.2 vs 3 744.5 (1.30 x)   scan faster at 10^6, within 5 % at 10^5
    #:   12           381.7 vs 265.2 (0.69 x)   2 714.8 vs 2 198.2 (0.81 x)   vtc_l2_topk faster, and at 16, 32, 64 (4.5 - 5 x there)
    #: 12 is the first count at which vtc_l2_topk wins by more than 5 %.  (vtc_l2_topk takes 40 - 70 % longer at 9, 10 and 11 queries,
    #: as at 1 and 2, than at 8 and 12: unexplained, that entry is not changed here.  13 - 15 queries were not measured.)
    ROUTE_TOPK_MIN_QUERIES = 12
    #: queries per call from which search_many() on a HALF index goes through ops.l2_search_many (k <= 32) instead of the scan.
    #: Measured, profiles/search_many.md (d = 512, depth 11, medians of 30 alternating calls; us at 10^5 / 10^6 half rows, new entry vs
    #: the scan over the same rows; in brackets under a random 50 % mask):
    #:    8 queries   209.0 vs 242.8 (1.16 x) [188.4 vs 186.8, 0.99 x]       386.1 vs  1 454.5 (3.77 x) [2.45 x]   level at 10^5 masked
    #:    9           221.1 vs 362.8 (1.64 x) [199.5 vs 264.6, 1.33 x]       420.5 vs  2 595.3 (6.17 x) [3.86 x]   new entry faster
    #:   12           252.5 vs 381.6 (1.51 x) [223.4 vs 274.4, 1.23 x]       482.6 vs  2 639.5 (5.47 x) [3.48 x]   new entry faster
    #:   16           298.4 vs 415.4 (1.39 x) [1.19 x]                       579.2 vs  2 740.7 (4.73 x) [3.09 x]   new entry faster
    #:   32           355.4 vs 746.6 (2.10 x) [1.72 x]                       717.3 vs  5 197.7 (7.25 x) [4.62 x]   new entry faster
    #:   64           400.1 vs 1 408.0 (3.52 x) [2.67 x]                     882.8 vs 10 088.7 (11.4 x) [7.05 x]   new entry faster
    #: 9 is the first count from which the new entry wins by more than 5 % at both sizes, masked or not (9 is from the tool's second
    #: run, --queries 8,9,10,11,12, where 10 and 11 won as well): the scan starts its second gallery pass there.
    ROUTE_MANY_MIN_QUERIES = 9
    #: queries per call from which range_search_many() / range_count_many() / similar_within() on a HALF index go through
    #: ops.l2_range_count_many instead of the scan's count pass (a call of more than 64 queries counts as 64, so 65 means never).
    #: Measured, profiles/range_many.md (d = 512, a radius about 10 rows of a query pass, medians of 30 alternating calls; us at
    #: 10^5 / 10^6 half rows, new count vs the scan's count over the same rows; in brackets under a random 50 % mask; a radius that
    #: 1 % of the rows pass moves no figure by more than 5 %):
    #:    8 queries    58.8 vs 193.7 (3.30 x) [ 60.6 vs 131.6, 2.17 x]       240.2 vs 1 288.0 ( 5.36 x) [3.69 x]   new entry faster
    #:    9            61.0 vs 306.6 (5.03 x) [ 64.4 vs 187.6, 2.92 x]       244.0 vs 2 386.7 ( 9.78 x) [6.63 x]   new entry faster
    #:   12            62.6 vs 306.8 (4.90 x) [ 65.3 vs 189.8, 2.91 x]       247.4 vs 2 383.0 ( 9.63 x) [6.52 x]   new entry faster
    #:   16            66.2 vs 311.9 (4.71 x) [ 68.4 vs 194.2, 2.84 x]       260.7 vs 2 406.9 ( 9.23 x) [6.41 x]   new entry faster
    #:   32            79.7 vs 537.5 (6.74 x) [ 83.7 vs 320.8, 3.83 x]       366.6 vs 4 567.3 (12.5 x)  [7.74 x]   new entry faster
    #:   64           105.2 vs 998.6 (9.49 x) [109.2 vs 573.7, 5.25 x]       570.1 vs 8 949.5 (15.7 x)  [9.22 x]   new entry faster
    #: 8 is the first MEASURED count, and the new entry wins there by more than 5 % at both sizes, masked or not.  Fewer than 8 queries
    #: were not measured: the scan runs them as one tile, in one gallery pass.
    ROUTE_RANGE_MANY_MIN_QUERIES = 8
    MAX_K = 64                # one list entry per lane of a wavefront, as everywhere in the sweeps
    STORAGE = {"float32": torch.float32, "float16": torch.float16, "int8": torch.int8}      # the state dict's names of the storage dtypes

    def __init__(self, dim, device="cuda", normalized=False, storage=torch.float32):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"vtc_amd VideoIndex: the index lives on the GPU (got {device}); this package has no CPU path")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if int(dim) < 1:
            raise ValueError(f"VideoIndex: dim={dim}")
        self.dim = int(dim)
        self.width = self.dim + -self.dim % 64          # zero-padded to the sweep's granule of 64 columns (host/metric.py pads alike)
        self.device = device
        self.normalized = bool(normalized)
        if storage not in self.STORAGE.values():
            raise ValueError(f"VideoIndex: storage={storage} must be torch.float32, torch.float16 or torch.int8")
        self.storage = storage
        self.row_width = self.width + (ops.Q8_TAIL if storage == torch.int8 else 0)      # columns of a stored row: a q8 row ends in its scale
        self._rows = torch.empty(0, self.row_width, dtype=storage, device=device)   # capacity rows; the first _n are the index
        self._n = 0
        self._ws = None
        self._live = None                   # bool [ntotal] on the device once a row was removed; None: every row is live
        self._n_live = 0
        self._generation = 0                # bumped by add / remove / load_state_dict: what a RowSubset's cached words are valid for
        self._words = None                  # (generation, packed words of _live)
        self._video_ids = None              # int32 [capacity] on the device once the first non-empty add passed video_ids: a GROUPED index
        self._dense = None                  # (sorted distinct video ids int64 [V], slot of every row int32 [ntotal], V): the paged searches
        self._by_video = None               # (generation, video ids sorted int64 [ntotal], the rows in that order): similar_to_video

    def __len__(self):
        """The number of live rows."""
        return self._n_live

    @property
    def ntotal(self):
        """The number of rows ever added: one more than the largest id."""
        return self._n

    @property
    def live_mask(self):
        """bool [ntotal] on the device (a copy): False for a removed row."""
        return torch.ones(self._n, dtype=torch.bool, device=self.device) if self._live is None else self._live.clone()

    @property
    def grouped(self):
        """True once the first non-empty ``add`` passed ``video_ids``: every row then has a video id and ``search_videos`` works."""
        return self._video_ids is not None

    @property
    def video_ids(self):
        """int32 [ntotal] on the device (a copy): the video of every row of a grouped index; None for an ungrouped one."""
        return None if self._video_ids is None else self._video_ids[:self._n].clone()

    # ---- rows ----------------------------------------------------------------------------------
    def _prepared(self, x, what, check=True, stored=False):
        """fp32 [n, dim] on the index's device -> unit rows (unless the index was built as ``normalized``), zero-padded to ``width``;
        with ``check``, NaN / inf rows are rejected as the eval entry points reject them (ops.nonfinite_bits: a 4-byte device-to-host
        read, so a host sync).  ``stored``: the rows as the index keeps them -- for half storage rounded to nearest-even AFTER the fp32
        normalisation and BEFORE the check, which then sees what the rounding made of them (a component above 65504 of a
        ``normalized`` index's row has become inf).  For int8 storage the padded fp32 rows are quantised (ops.quantize_rows_q8: the
        padding is codes of 0) and the check sees the dequantised rows; the q8 rows [n, width + 16] come back."""
        x = torch.as_tensor(x)
        if x.dim() != 2 or x.shape[1] != self.dim:
            raise ValueError(f"VideoIndex: {what} must be [n, {self.dim}], got {tuple(x.shape)}")
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        if x.shape[0] == 0:
            return x.new_zeros(0, self.row_width, dtype=self.storage) if stored else x.new_zeros(0, self.width)
        if not self.normalized:
            x = ops.normalize_rows(x)
        if stored and self.storage == torch.int8:
            rows = ops.quantize_rows_q8(torch.nn.functional.pad(x, (0, self.width - self.dim)) if self.width != self.dim else x)
            x = ops.dequantize_rows_q8(rows)                   # a NaN scale (a non-finite row) makes the whole row NaN
            if check and ops.nonfinite_bits(x, x):
                raise ValueError("VideoIndex: non-finite values in the " + what + ("" if self.normalized else " (after normalisation: a NaN, "
                                 "an inf or an all-zero row)") + " -- such a row has no distance to anything")
            return rows
        if stored and self.storage != torch.float32:
            x = x.to(self.storage).float()                     # rounded; widened again (exactly) for the check and the padding
        if check and ops.nonfinite_bits(x, x):
            raise ValueError(f"VideoIndex: non-finite values in the {what}" + ("" if self.normalized else " (after normalisation: a NaN, an inf "
                             "or an all-zero row)") + " -- such a row has no distance to anything")
        if self.width != self.dim:
            x = torch.nn.functional.pad(x, (0, self.width - self.dim))
        return x.to(self.storage) if stored else x

    def add(self, embeddings, video_ids=None):
        """Appends [n, dim] fp32 rows; their ids are their positions in insertion order (removed ids are not reused).  Returns the id of
        the first one, which is ``ntotal`` before the call.  A half index normalises in fp32 as an fp32 one does and then rounds to
        nearest-even (``.to(torch.float16)``); the non-finite check runs on the rounded rows.  An int8 index normalises in fp32 too, pads
        to ``width`` and quantises every row to 8-bit codes and one scale with the kernel (ops.quantize_rows_q8, one launch); the check
        runs on the dequantised rows.
        ``video_ids`` (an integer [n] tensor or sequence, values in [0, 2^31)) names the video of every row; one video's rows may come in
        different calls.  An index is GROUPED iff its first non-empty add passed them, and every later add must do the same as the first:
        mixing the two forms raises ValueError and changes nothing."""
        x = self._prepared(embeddings, "embeddings", stored=True)
        first, n = self._n, x.shape[0]
        vids = None if video_ids is None else _video_id_tensor(video_ids, n, self.device, "add")
        if n and first and (vids is not None) != self.grouped:
            raise ValueError("VideoIndex.add: this index " + ("has a video id for every row: pass video_ids" if self.grouped else
                             "was started without video_ids: its rows have none, so later rows cannot either"))
        if first + n > self._rows.shape[0]:                 # amortised doubling
            grown = torch.empty(max(first + n, 2 * self._rows.shape[0], 1024), self.row_width, dtype=self.storage, device=self.device)
            grown[:first] = self._rows[:first]
            self._rows = grown
        self._rows[first:first + n] = x
        if n and vids is not None:
            if self._video_ids is None or self._video_ids.shape[0] < self._rows.shape[0]:
                grown = torch.zeros(self._rows.shape[0], dtype=torch.int32, device=self.device)
                if self._video_ids is not None:
                    grown[:first] = self._video_ids[:first]
                self._video_ids = grown
            self._video_ids[first:first + n] = vids
            self._dense = None
        self._n = first + n
        if n:
            self._n_live += n
            if self._live is not None:
                self._live = torch.cat([self._live, torch.ones(n, dtype=torch.bool, device=self.device)])
            self._generation += 1
        return first

    def remove(self, ids):
        """Removes the rows with these ids (an int64 sequence or tensor) from every later search; returns how many were live until now.
        Duplicates and ids already removed are ignored; an id outside [0, ntotal) raises ValueError and changes nothing.  Reads the count
        back from the device (a host sync): removal is not the query path."""
        ids = _id_tensor(ids, self._n, self.device, "remove")
        if ids.numel() == 0:
            return 0
        live = torch.ones(self._n, dtype=torch.bool, device=self.device) if self._live is None else self._live
        ids = torch.unique(ids)
        newly = int(live[ids].sum())
        if newly:
            live[ids] = False
            self._live = live
            self._n_live -= newly
            self._generation += 1
        return newly

    def remove_videos(self, video_ids):
        """Removes every live row of these videos (an integer sequence or tensor) and returns how many rows that were.  A video the index
        does not hold removes nothing.  Reads the count back from the device (a host sync): removal is not the query path."""
        if not self.grouped:
            raise ValueError("VideoIndex.remove_videos: the index has no video ids (add(embeddings, video_ids=...))")
        vids = _video_id_tensor(video_ids, None, self.device, "remove_videos")
        if vids.numel() == 0 or self._n == 0:
            return 0
        rows = torch.nonzero(torch.isin(self._video_ids[:self._n], vids)).reshape(-1)
        return self.remove(rows)

    def subset(self, members):
        """The rows a search may return, as a reusable ``RowSubset``: ``members`` is a bool [ntotal] tensor or int64 ids (a sequence or a
        tensor; an id outside [0, ntotal) raises ValueError).  Removed rows stay out whatever ``members`` says."""
        m = torch.as_tensor(members)
        if m.dtype == torch.bool:
            if tuple(m.shape) != (self._n,):
                raise ValueError(f"VideoIndex.subset: a bool mask must be [ntotal = {self._n}], got {tuple(m.shape)}")
            flags = m.to(self.device).contiguous().view(torch.uint8).clone()
        else:
            ids = _id_tensor(m, self._n, self.device, "subset")
            flags = torch.zeros(self._n, dtype=torch.uint8, device=self.device)
            flags[ids] = 1
        return RowSubset(self, flags)

    def _live_words(self):
        """The packed words of the live rows (None while nothing was removed), packed once per generation."""
        if self._live is None:
            return None
        if self._words is None or self._words[0] != self._generation:
            self._words = (self._generation, ops.row_mask_pack(self._live))
        return self._words[1]

    @property
    def rows(self):
        """The stored rows [ntotal, width] (a view) in the storage dtype, removed ones included; of an int8 index the q8 rows
        [ntotal, width + 16]: ``width`` codes, the row's fp32 scale, 12 zero bytes (``ops.dequantize_rows_q8`` gives their values)."""
        return self._rows[:self._n]

    def _widened(self, rows):
        """Stored rows (any selection of ``self.rows``) as the fp32 values they hold [m, width]: exact for every storage."""
        return ops.dequantize_rows_q8(rows) if self.storage == torch.int8 else rows.float()

    def state_dict(self):
        """The rows in the storage dtype; a half index writes "storage": "float16" beside them.  An fp32 index's state has the keys it
        always had -- a state without "storage" IS fp32 (``load_state_dict`` also takes an explicit "float32").  An int8 index writes
        "storage": "int8", its codes [n, dim] as "rows" and the rows' fp32 "scales" [n]."""
        state = {"rows": self.rows[:, :self.dim].clone(), "count": self._n, "dim": self.dim, "normalized": self.normalized}
        if self.storage != torch.float32:
            state["storage"] = {v: k for k, v in self.STORAGE.items()}[self.storage]
        if self.storage == torch.int8:
            state["scales"] = ops.q8_scales(self.rows)
        if self._live is not None:
            state["live"] = self._live.clone()
        if self.grouped:
            state["video_ids"] = self.video_ids
        return state

    def load_state_dict(self, state):
        """A state whose storage differs from the index's raises ValueError (``converted`` changes the storage); rows are taken bit
        for bit, never rounded or normalised again.  An int8 state's "scales" must be finite fp32 [count] with their low 8 mantissa bits
        clear -- the quantiser's 16 significant bits, with which every stored value is an exact product."""
        storage = state.get("storage", "float32")
        if self.STORAGE.get(storage) != self.storage:
            raise ValueError(f"VideoIndex.load_state_dict: the state's storage is {storage}, the index's {self.storage} "
                             "(load it into an index of that storage; converted() changes it)")
        rows = torch.as_tensor(state["rows"])
        if storage != "float32" and rows.dtype != self.storage:
            raise ValueError(f"VideoIndex.load_state_dict: a {storage} state holds {rows.dtype} rows")
        if int(state.get("dim", self.dim)) != self.dim or rows.dim() != 2 or rows.shape[1] != self.dim or int(state["count"]) != rows.shape[0]:
            raise ValueError(f"VideoIndex.load_state_dict: rows {tuple(rows.shape)}, count {state.get('count')} do not fit dim {self.dim}")
        rows = rows.to(device=self.device, dtype=self.storage)
        if storage == "int8":
            scales = state.get("scales")
            scales = None if scales is None else torch.as_tensor(scales)
            if scales is None or scales.dtype != torch.float32 or tuple(scales.shape) != (rows.shape[0],):
                raise ValueError(f"VideoIndex.load_state_dict: an int8 state holds float32 scales [{rows.shape[0]}], one per row")
            scales = scales.to(self.device).contiguous()
            if rows.shape[0] and (not bool(torch.isfinite(scales).all()) or bool((scales.view(torch.int32) & 0xFF).any())):
                raise ValueError("VideoIndex.load_state_dict: an int8 state's scales must be finite with their low 8 mantissa bits clear "
                                 "(16 significant bits: every stored value is then an exact product)")
            self._rows = ops.q8_rows(torch.nn.functional.pad(rows, (0, self.width - self.dim)), scales)
        else:
            wide = rows.float().contiguous()
            if rows.shape[0] and ops.nonfinite_bits(wide, wide):
                raise ValueError("VideoIndex.load_state_dict: non-finite values in the stored rows")
            self._rows = torch.nn.functional.pad(rows, (0, self.width - self.dim)).contiguous()     # stored rows are final: not normalised again
        live = state.get("live")
        if live is not None:
            live = torch.as_tensor(live)
            if live.dtype != torch.bool or tuple(live.shape) != (rows.shape[0],):
                raise ValueError(f"VideoIndex.load_state_dict: live must be bool [{rows.shape[0]}], got {live.dtype} {tuple(live.shape)}")
            live = live.to(self.device).clone()
        vids = state.get("video_ids")
        if vids is not None:
            vids = torch.as_tensor(vids)
            if vids.dtype != torch.int32 or tuple(vids.shape) != (rows.shape[0],):
                raise ValueError(f"VideoIndex.load_state_dict: video_ids must be int32 [{rows.shape[0]}], got {vids.dtype} {tuple(vids.shape)}")
            vids = _video_id_tensor(vids, rows.shape[0], self.device, "load_state_dict").clone()
        self._video_ids = vids
        self._dense = None
        self._n = rows.shape[0]
        self._live = live
        self._n_live = self._n if live is None else int(live.sum())
        self._generation += 1

    def converted(self, storage):
        """A new index of ``storage`` (torch.float32, torch.float16 or torch.int8) with the same ids, ``ntotal``, live mask and video
        ids: fp32 -> half rounds every stored row to nearest-even, half -> fp32 widens exactly, the same storage gives a copy.  To
        int8: the stored rows, widened to fp32, are quantised (ops.quantize_rows_q8) -- never normalised again.  From int8: the rows
        are dequantised, which is exact, and for half then rounded as an fp32 -> half conversion rounds.  This index is not changed;
        RowSubsets belong to the index they were built on."""
        other = VideoIndex(self.dim, device=self.device, normalized=self.normalized, storage=storage)
        if other.storage == self.storage:
            rows = self.rows
        elif other.storage == torch.int8:
            rows = ops.quantize_rows_q8(self.rows.float()) if self._n else self.rows.new_zeros(0, other.row_width, dtype=torch.int8)
        else:
            rows = self._widened(self.rows).to(other.storage)
        if other.storage != self.storage and self._n and other.storage != torch.int8:
            wide = rows.float().contiguous()                   # fp32 -> half can only overflow for a ``normalized`` index's rows
            if ops.nonfinite_bits(wide, wide):
                raise ValueError(f"VideoIndex.converted: a stored row has a component that {storage} cannot hold")
        other._rows = rows.clone() if rows.data_ptr() == self._rows.data_ptr() else rows.contiguous()
        other._n, other._n_live = self._n, self._n_live
        other._live = None if self._live is None else self._live.clone()
        other._video_ids = None if self._video_ids is None else self._video_ids[:self._n].clone()
        other._generation += 1
        return other

    # ---- search --------------------------------------------------------------------------------
    def _workspace(self, nbytes):
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = None
            self._ws = ops.workspace(nbytes, self.device)
        return self._ws

    def search(self, queries, k, subset=None, after=None, exclude=None):
        """(ids [Q, k] int64, scores [Q, k] fp32), both on the device: the k nearest stored rows of every query, nearest first, and
        score = 1 - |q - g|^2 / 2, the cosine for unit rows.  1 <= k <= min(64, len(index)), len being the live rows.
        Fewer than ROUTE_TOPK_MIN_QUERIES queries -- batch 1 is the design point -- are only enqueued: no device-to-host read, no host
        sync.  A query with a NaN / inf (or an all-zero row, which has no direction) is not rejected there; the scan gives it a row of
        ids -1 and scores -inf.  From ROUTE_TOPK_MIN_QUERIES queries on the queries are checked first, as add() checks its rows, and a
        non-finite one raises ValueError: vtc_l2_topk has no defined answer for such a row.
        After a ``remove``, or with a ``subset`` (a RowSubset of this index), only the live members are searched: the masked scan for any
        number of queries, 64 per call, with the few-query rule for a non-finite query (a row of -1 / -inf, no raise, no read) and no host
        sync.  A subset with fewer than k live members gives rows that end in -1 / -inf.
        A half index (``storage=torch.float16``) takes that route for EVERY search -- the scan over the stored half rows
        (vtc_l2_search_half), 64 queries per call, only enqueued, a non-finite query a row of -1 / -inf -- whatever the number of
        queries: vtc_l2_topk reads fp32 rows.  Batches of many queries are therefore slower than on an fp32 index
        (profiles/search.md: 4.5 x at 64 queries).  The scores are 1 - D/2 over the stored rows, each the unit row rounded to
        binary16's 11 significant bits per component.  An int8 index (``storage=torch.int8``) takes the same route by the same rules
        (vtc_l2_search_q8); its scores are 1 - D/2 over the stored values scale * code.
        ``after`` (an int64 [Q] tensor of row ids, typically ``ids[:, -1]`` of the previous page): the k nearest rows that come AFTER
        that row in the query's search order -- by (fp64 distance, row), the order every search returns -- so the pages chained by their
        last ids are, concatenated, the exact ranking to any depth, without repeats or gaps.  Stateless: the cursor's distance is formed
        again from the stored row (vtc_l2_pair_dists64, the bits the scan compares), then the cursor scan runs (vtc_l2_search_after) for
        any number of queries, 64 per call, by the masked route's rules: only enqueued, no host sync, a non-finite query a row of
        -1 / -inf.  So an id cannot be validated: -1 (the previous page was not full: there is nothing after it) or an id outside
        [0, ntotal) gives that query a row of -1 / -inf and leaves the others alone -- chaining past the end returns empty pages, it
        never starts over.  The cursor row need not be live nor a member of ``subset``: a page token survives a ``remove``.  Each page
        costs a gallery pass per started tile of 8 queries, however deep the cursor is.  ``after=None`` changes nothing above.
        ``exclude`` (an int64 [Q] tensor of row ids): query q is never given row ``exclude[q]`` -- its search order with that row
        deleted, then cut (vtc_l2_search_excluding).  -1, or an id outside [0, ntotal), excludes nothing.  The call is then always the
        scan, by the masked route's rules: slices of 64 queries, only enqueued, no host sync, a non-finite query a row of -1 / -inf.  It
        composes with ``subset``, removed rows, half storage and ``after`` (the cursor may be the excluded row).  A query with fewer
        than k admissible rows ends in -1 / -inf.  ``exclude=None`` changes nothing above."""
        k = self._checked_k(k, "search")
        plain = after is None and exclude is None and subset is None and self._live is None and self.storage == torch.float32
        if not (plain and len(queries) >= self.ROUTE_TOPK_MIN_QUERIES):
            return self._scan(queries, k, subset, after, exclude, "search")      # nothing is read back: no sync
        q = self._prepared(queries, "queries")
        if q.shape[0] == 0:
            raise ValueError("VideoIndex.search: no queries")
        ws = self._workspace(L.lib().vtc_l2_topk_workspace_bytes(self._n, q.shape[0], self.width, L.SWEEP_EXACT, 0))
        ids, dists = ops.l2_topk(self.rows, q, k, precision=L.SWEEP_EXACT, ws=ws)
        return ids, 1.0 - dists / 2.0

    def search_many(self, queries, k, subset=None):
        """``search(queries, k, subset)`` for a BATCH: the same (ids [Q, k], scores [Q, k]), bit for bit, on every index.  On a half
        index with k <= 32 and at least ROUTE_MANY_MIN_QUERIES queries the slices of 64 go through vtc_l2_search_many_half -- one
        pass of the stored half rows through the matrix cores per slice and an exact fp64 finish, where ``search`` scans the gallery
        once per 8 queries -- by the masked route's rules: removed rows and ``subset`` honoured, only enqueued, no host sync, a
        non-finite query a row of -1 / -inf.  In every other case (an fp32 index, k above 32, fewer queries) the call IS ``search``."""
        k = self._checked_k(k, "search_many")
        if self.storage != torch.float16 or k > ops.SEARCH_MANY_MAX_DEPTH or len(queries) < self.ROUTE_MANY_MIN_QUERIES:
            return self.search(queries, k, subset=subset)
        self._check_subset(subset, "search_many")
        q = self._prepared(queries, "queries", check=False)
        words = self._live_words() if subset is None else subset.words()
        # the last slice may need MORE than a full one: fewer queries a workgroup, more workgroups, more lists
        sizes = {min(q.shape[0], ops.SEARCH_MAX_QUERIES), q.shape[0] % ops.SEARCH_MAX_QUERIES} - {0}
        ws = self._workspace(max(ops.l2_search_many_workspace_bytes(self._n, s, self.width, k) for s in sizes))
        out = [ops.l2_search_many(self.rows, qs, k, live=words, ws=ws)[:2] for (qs,) in self._sliced(q)]
        ids, dists = out[0] if len(out) == 1 else [torch.cat(column) for column in zip(*out)]
        return ids, 1.0 - dists / 2.0

    def _checked_k(self, k, what, deep=False):
        """int(k), which must be in [1, min(64, len(index))] -- ``deep``, the paged searches: in [1, len(index)] -- or ValueError."""
        k = int(k)
        if not 1 <= k <= (self._n_live if deep else min(self.MAX_K, self._n_live)):
            most = f"len(index) = {self._n_live}"
            raise ValueError(f"VideoIndex.{what}: k={k} must be in [1, {most if deep else f'min({self.MAX_K}, {most})'}]")
        return k

    def _check_subset(self, subset, what):
        if subset is not None and (not isinstance(subset, RowSubset) or subset.index is not self):
            raise ValueError(f"VideoIndex.{what}: the subset belongs to another index (build it with this index's subset())")

    def _per_query_ids(self, ids, n_queries, name, what, row_ids=False):
        """An int64 tensor with one entry per query (``n_queries`` None: any number >= 1) -> on the index's device, contiguous; anything
        else raises ValueError.  ``row_ids`` (the cursor of ``search``): whatever ``torch.as_tensor`` makes such a tensor of.  The VALUES
        are not read: no host sync."""
        if row_ids:
            ids = torch.as_tensor(ids)
        ok = isinstance(ids, torch.Tensor) and ids.dtype == torch.int64 and ids.dim() == 1
        if not ok or (ids.shape[0] < 1 if n_queries is None else ids.shape[0] != n_queries):
            got = f"{ids.dtype} {tuple(ids.shape)}" if isinstance(ids, torch.Tensor) else type(ids).__name__
            raise ValueError(f"VideoIndex.{what}: {name} must be an int64 [{n_queries or 'Q >= 1'}] tensor{' of row ids' * row_ids}, one per "
                             f"query, got {got}")
        return ids.to(self.device).contiguous()

    @staticmethod
    def _sliced(queries, *per_query, step=ops.SEARCH_MAX_QUERIES):
        """[(queries, *per_query) of one library call]: slices of at most ``ops.SEARCH_MAX_QUERIES`` queries, each with the entries of
        the same queries of every per-query sequence (None stays None).  THE place where a call's arguments are cut; up to 64 queries
        are the arguments themselves.  ``step``: set queries [S, M, width] are cut into calls of 64 // M sets."""
        n, whole = queries.shape[0], (queries, *per_query)
        if n <= step:
            return [whole]
        return [tuple(None if t is None else t[lo:lo + step] for t in whole) for lo in range(0, n, step)]

    def _scan(self, queries, k, subset, after, exclude, what, grouped=False, stored=False, sets=False):
        """The scan behind every top-k search of rows (``ops.l2_search``) and, ``grouped``, of distinct videos
        (``ops.l2_search_grouped``): any number of queries in slices of 64, only enqueued.  ``after`` / ``exclude``: one row id (grouped:
        one row id / one video id) per query or None.  ``stored``: the queries are stored rows [Q, width] widened to fp32 (``similar``)
        and are searched as they are.  ``sets``: the queries are prepared SET queries [S, M, width] (``_set_queries``), a query being a
        set: ``ops.l2_search_sets`` in slices of 64 // M sets, ``exclude`` one key per set, no ``after``.  Returns (ids, scores), grouped
        (videos, rows, scores).  ``what`` names the caller in the messages."""
        self._check_subset(subset, what)
        q = queries if stored else self._prepared(queries, "queries", check=False)
        if q.shape[0] == 0:
            raise ValueError(f"VideoIndex.{what}: no queries")
        if exclude is not None:
            exclude = self._per_query_ids(exclude, q.shape[0], "exclude_videos" if grouped else "exclude", what)
        words = self._live_words() if subset is None else subset.words()      # None with every row live: no mask
        step = ops.SEARCH_MAX_QUERIES // q.shape[1] if sets else ops.SEARCH_MAX_QUERIES
        if sets:
            ws = self._workspace(ops.l2_search_sets_workspace_bytes(self._n, min(q.shape[0], step), q.shape[1], self.width, k, grouped))
        else:
            ws_bytes = ops.l2_search_grouped_workspace_bytes if grouped else ops.l2_search_workspace_bytes
            ws = self._workspace(ws_bytes(self._n, min(q.shape[0], step), self.width, k))
        if after is not None:
            after = self._per_query_ids(after, q.shape[0], "after", what, row_ids=not grouped)
        uniq = n_videos = None
        if grouped and after is None:
            groups = self._video_ids[:self._n]
        elif grouped:                                              # a page: the videos by their dense slots, which index its bitmap
            uniq, groups, n_videos = self._dense_videos()
            if exclude is not None:                                # the excluded VIDEO as its slot; one the index does not hold is no group
                at = torch.searchsorted(uniq, exclude).clamp(max=n_videos - 1)
                exclude = torch.where(uniq[at] == exclude, at, torch.full_like(at, 1 << 40))
        g, out = self.rows, []
        # What the call does not have stays None, every argument's default: each slice reaches the library entry of exactly the
        # arguments that are set (ops: the narrowest entry that takes the call).
        for qs, cursor, ex in self._sliced(q, after, exclude, step=step):
            if cursor is not None:
                cursor = (ops.l2_pair_dists64(g, qs, cursor), cursor)          # +inf for an id that is no row: nothing comes after it
            if sets:
                found = ops.l2_search_sets(g, qs, k, groups=groups if grouped else None, live=words, exclude=ex, ws=ws)
                out.append(found[:3] if grouped else (found[0], found[2]))
            elif grouped:
                out.append(ops.l2_search_grouped(g, qs, groups, k, ws=ws, live=words, exclude=ex, after=cursor, n_groups=n_videos)[:3])
            else:
                out.append(ops.l2_search(g, qs, k, ws=ws, live=words, after=cursor, exclude=ex)[:2])
        *found, dists = out[0] if len(out) == 1 else [torch.cat(column) for column in zip(*out)]
        if grouped:                                                # (rows, their videos -- of a page: their slots)
            rows, videos = found
            videos = videos.to(torch.int64) if uniq is None else uniq[videos.clamp(min=0).to(torch.int64)]
            found = torch.where(rows >= 0, videos, rows), rows
        return (*found, 1.0 - dists / 2.0)

    def search_deep(self, queries, k, subset=None, exclude=None):
        """``search`` without the limit of 64: (ids [Q, k] int64, scores [Q, k] fp32) for any 1 <= k <= len(index), the exact k nearest
        live rows (of ``subset``) of every query, nearest first.  Page 1 is ``search(queries, min(k, 64), subset)`` by whatever route
        that takes, with its rules for non-finite queries and host syncs; every further page of 64 is
        ``search(..., after=ids[:, -1])`` of the page before, only enqueued, and the pages are concatenated.  Fewer than k members
        give rows that end in -1 / -inf.
        THE COST: one gallery pass per 64 results per started tile of 8 queries -- k = 1024 for 8 queries is 16 passes over the
        gallery, for 64 queries 128.  That is right for a few hundred neighbours of a few queries.  For thousands of results, or
        whenever a score threshold is known, ``range_search`` is the tool: ONE pass per tile of queries however many rows come back,
        at the price of one host sync, a sort of the hits and a result whose size the data decides.  Measured
        (profiles/search_after.md, d = 512, one query over 10^6 rows): k = 256 takes 1.84 ms and k = 1024 7.3 ms, ``range_search`` at
        the k-th neighbour's score 0.58 and 0.59 ms -- it is the better tool from k = 256 on whenever a threshold is known.
        From ROUTE_TOPK_MIN_QUERIES queries on, page 1 of an fp32 index with every row live is ``search``'s vtc_l2_topk call, whose
        routing was measured at depth 11; at k = 64 it takes 29 ms over 10^5 rows and 290 ms over 10^6 (the scan: 2 and 14 ms) and
        dominates the call.  For deep rankings of many queries pass fewer than that per call.
        ``exclude``: ``search``'s, passed on every page -- the ranking without that row, what a hard-negative miner asks for; every
        page, the first included, is then the scan."""
        return self._paged(lambda n, after: self.search(queries, n, subset=subset, after=after, exclude=exclude), 0, k, "search_deep")

    def _paged(self, page, cursor_column, k, what):
        """The pager of ``search_deep`` and ``search_videos_deep``: ``page(n, after)`` is one page of n <= 64 results (after=None: the
        first), and the last entry of every query in output ``cursor_column`` -- the row ids -- is the cursor of the next."""
        k = self._checked_k(k, what, deep=True)
        pages = [page(min(k, self.MAX_K), None)]
        got = pages[0][0].shape[1]
        while got < k:
            pages.append(page(min(k - got, self.MAX_K), pages[-1][cursor_column][:, -1]))
            got += pages[-1][0].shape[1]
        return pages[0] if len(pages) == 1 else tuple(torch.cat(column, dim=1) for column in zip(*pages))

    def _dense_videos(self):
        """(uniq int64 [V] sorted, slot int32 [ntotal], V): the videos of the index numbered densely, what the paged grouped search
        indexes its bitmap by -- video ids themselves stay arbitrary.  Built at the first paged call after an ``add`` or a
        ``load_state_dict`` (``torch.unique`` reads V back: ONE host sync) and kept until the next; a ``remove`` does not touch it."""
        if self._dense is None:
            uniq, slot = torch.unique(self._video_ids[:self._n], return_inverse=True)
            self._dense = (uniq.to(torch.int64), slot.to(torch.int32).contiguous(), int(uniq.shape[0]))
        return self._dense

    def search_videos(self, queries, k, subset=None, exclude_videos=None, after=None):
        """(video_ids [Q, k] int64, row_ids [Q, k] int64, scores [Q, k] fp32) of a GROUPED index: the k nearest distinct videos of every
        query, nearest first, each with its nearest live row (the best-matching caption, comment or chunk) and that row's score as
        ``search`` gives it.  Ties go to the lower row.  Always the scan (vtc_l2_search_grouped; vtc_l2_topk has no grouping), 64 queries
        per call, with the few-query rules of the masked route: only enqueued, no host sync, and a non-finite query gets a row of
        -1 / -1 / -inf.  A half index searches its stored half rows the same way (vtc_l2_search_half).  1 <= k <= min(64, len(index)), len counting live ROWS; fewer than k distinct live videos (in the ``subset``, if
        one is given) give rows that end in -1 / -1 / -inf.  On an ungrouped index it raises ValueError.
        ``exclude_videos`` (an int64 [Q] tensor of video ids): query q is never given a row of the video ``exclude_videos[q]`` -- the
        nearest OTHER videos, the hard negatives of a (text, video) pair (vtc_l2_search_excluding).  -1, or a video the index does not
        hold, excludes nothing.  ``None`` changes nothing above.
        ``after`` (an int64 [Q] tensor of ROW ids, typically ``rows[:, -1]`` of the previous page): the k nearest distinct videos that
        come AFTER that row in the query's grouped order -- the videos (with a live row, of ``subset``, not excluded) sorted by the key
        (fp64 distance, row) of their nearest such row -- so the pages chained by their last rows are, concatenated, that order to any
        depth, bit for bit, without repeats or gaps.  Stateless and exact: the cursor's distance is formed again from the stored row
        (vtc_l2_pair_dists64), one gallery pass marks the videos with a row at or before the cursor in a per-query bitmap
        (vtc_l2_group_mark_before) and the scan skips them (vtc_l2_search_grouped_after): TWO gallery passes per started tile of 8
        queries, 64 queries per call, only enqueued, a non-finite query a row of -1 / -1 / -inf.  -1 (the previous page was not
        full) or an id outside [0, ntotal) gives that query an empty page and leaves the others alone.  The cursor row need not be
        live, nor a member of ``subset``, and may belong to the excluded video.  It composes with ``subset``, removed rows, half
        storage and ``exclude_videos``.  The bitmap is indexed by a dense numbering of the videos that the index builds at the first
        paged call after an ``add`` (or ``load_state_dict``) with ``torch.unique``, which reads the number of videos back: ONE host
        sync then, none at the paged calls after it.  ``after=None`` changes nothing above."""
        return self._search_videos(queries, k, subset, exclude_videos, "search_videos", after=after)

    def _search_videos(self, queries, k, subset, exclude, what, stored=False, after=None):
        if not self.grouped:
            raise ValueError(f"VideoIndex.{what}: the index has no video ids (add(embeddings, video_ids=...)); search() returns rows")
        return self._scan(queries, self._checked_k(k, what), subset, after, exclude, what, grouped=True, stored=stored)

    def search_videos_deep(self, queries, k, subset=None, exclude_videos=None):
        """``search_videos`` without the limit of 64: (video_ids [Q, k] int64, row_ids [Q, k] int64, scores [Q, k] fp32) for any
        1 <= k <= len(index) (len counting live ROWS, as the grouped bounds do), the exact k nearest distinct videos of every query.
        Page 1 is ``search_videos(queries, min(k, 64))``; every further page of 64 is ``search_videos(..., after=rows[:, -1])`` of the
        page before, only enqueued (after the one host sync of the first paged call since an ``add``), and the pages are concatenated.
        Fewer than k videos give rows that end in -1 / -1 / -inf.
        THE COST: TWO gallery passes per page per started tile of 8 queries from page 2 on (one that marks the videos behind the
        cursor, one that scans; page 1 is one pass) -- k = 1024 for 8 queries is 31 passes over the gallery.  That is right for a few
        hundred videos of a few queries (profiles/search_grouped_after.md).  For thousands of results, or whenever a score threshold
        is known, ``range_search`` is the tool: one pass per tile of queries however many rows come back; its hits are rows, which the
        caller reduces to videos."""
        return self._paged(lambda n, after: self.search_videos(queries, n, subset=subset, exclude_videos=exclude_videos, after=after), 1, k,
                           "search_videos_deep")

    def search_videos_text(self, model, title_tokens, k, comments=None, subset=None, exclude_videos=None, after=None):
        """``search_text`` for a grouped index: the k nearest distinct videos of text queries given as token ids, as ``search_videos``
        returns them.  ``exclude_videos`` and ``after`` (the next page): ``search_videos``'s."""
        return self.search_videos(self._text_queries(model, title_tokens, comments, "search_videos_text"), k, subset=subset,
                                  exclude_videos=exclude_videos, after=after)

    # ---- more like this --------------------------------------------------------------------------
    def _stored_queries(self, ids, what):
        """(ids int64 [Q] on the device, the STORED rows ids[q] widened to fp32 [Q, width]).  The gather is clamped into the index and the
        query of an id outside [0, ntotal) becomes a row of NaN -- which every search answers with -1 / -inf -- without a host read."""
        ids = self._per_query_ids(ids, None, "ids", what)
        if self._n == 0:
            raise ValueError(f"VideoIndex.{what}: the index is empty")
        inside = (ids >= 0) & (ids < self._n)
        q = self._widened(self.rows[ids.clamp(0, self._n - 1)])          # half -> fp32 and scale * code are exact, the zero padding included
        return ids, torch.where(inside[:, None], q, q.new_full((), float("nan"))).contiguous()

    def similar(self, ids, k, subset=None, after=None):
        """MORE LIKE THIS: (ids [Q, k] int64, scores [Q, k] fp32), the k nearest rows of the STORED row ``ids[q]`` (an int64 [Q]
        tensor of row ids), that row itself left out -- ``search`` with the stored row as the query and ``exclude=ids``.  The query is
        the row as the index keeps it, never normalised again: a half index's row widened exactly, an int8 index's dequantised exactly, zero
        padding included.  So a
        bit-equal duplicate of the row scores exactly 1 and IS returned: it is another row.  The query row need not be live nor a
        member of ``subset`` (the neighbours are).  ``after``: ``search``'s cursor, the next page.  An id outside [0, ntotal) (-1
        included) cannot be validated without a host read: that query comes back as -1 / -inf and the others are left alone.  Any
        number of queries, 64 per call, only enqueued.  1 <= k <= min(64, len(index)); fewer than k other rows end in -1 / -inf."""
        k = self._checked_k(k, "similar")
        ids, q = self._stored_queries(ids, "similar")
        return self._scan(q, k, subset, after, ids, "search", stored=True)      # its messages say VideoIndex.search

    def similar_videos(self, ids, k, subset=None, after=None):
        """(video_ids [Q, k] int64, row_ids [Q, k] int64, scores [Q, k] fp32) of a GROUPED index: the k nearest distinct videos of the
        STORED row ``ids[q]`` -- ROW ids, for example the ``rows`` a ``search_videos`` call returned -- with every row of that row's
        own video left out; otherwise ``search_videos`` with the stored row as the query (as ``similar`` takes it).  An id outside
        [0, ntotal) gives -1 / -1 / -inf.  On an ungrouped index it raises ValueError.  ``after``: ``search_videos``'s cursor, the next
        page of other videos (the ``rows[:, -1]`` of the page before), to any depth by chaining.  A query given as a whole VIDEO, all
        of its rows merged into one ranking, is ``similar_to_video``."""
        if not self.grouped:
            raise ValueError("VideoIndex.similar_videos: the index has no video ids (add(embeddings, video_ids=...)); similar() returns rows")
        ids, q = self._stored_queries(ids, "similar_videos")
        own = self._video_ids[:self._n][ids.clamp(0, self._n - 1)].to(torch.int64)
        return self._search_videos(q, k, subset, own, "similar_videos", stored=True, after=after)

    # ---- set queries: several vectors as one query ---------------------------------------------------
    MAX_SET = ops.SEARCH_MAX_QUERIES      # members of a set query: one library call takes 64 vectors

    def _set_queries(self, query_sets, sizes, what):
        """[S, M, dim] -> the prepared members [S, M, width] (as ``search`` prepares queries, no check: a non-finite member takes no
        part).  ``sizes``: a HOST sequence of S ints in [1, M], never read from a device; the members at or past ``sizes[s]`` are
        replaced by member 0 of their set, which changes no output bit (a repeated member is no new candidate)."""
        x = torch.as_tensor(query_sets)
        if x.dim() != 3 or x.shape[2] != self.dim or not 1 <= x.shape[1] <= self.MAX_SET:
            raise ValueError(f"VideoIndex.{what}: query_sets must be [S, M, {self.dim}] with 1 <= M <= {self.MAX_SET} members a set, got "
                             f"{tuple(x.shape)}")
        n_sets, m = x.shape[:2]
        if n_sets == 0:
            raise ValueError(f"VideoIndex.{what}: no queries")
        q = self._prepared(x.reshape(n_sets * m, self.dim), "query_sets", check=False).view(n_sets, m, self.width)
        if sizes is not None:
            if isinstance(sizes, torch.Tensor) and sizes.is_cuda:
                raise ValueError(f"VideoIndex.{what}: sizes must be a host sequence of {n_sets} ints (it is not read from a device)")
            sizes = [int(s) for s in sizes]
            if len(sizes) != n_sets or not all(1 <= s <= m for s in sizes):
                raise ValueError(f"VideoIndex.{what}: sizes must be {n_sets} ints in [1, M = {m}], one per set, got {sizes}")
            if min(sizes) < m:
                keep = torch.tensor([[j < s for j in range(m)] for s in sizes], device=self.device)
                q = torch.where(keep[:, :, None], q, q[:, :1]).contiguous()
        return q

    def _attaining_members(self, q, rows):
        """int64 [S, k]: for every returned row the LOWEST member of its set that attains E -- the fp64 argmin, over the members, of
        the pair distances with the scan's bits (ops.l2_pair_dists64; a non-finite member counts as +inf), -1 where the row is -1.
        One launch over S * k * M pairs (their member vectors are gathered: S * k * M * width floats) plus torch ops, no host sync."""
        (n_sets, m, width), k = q.shape, rows.shape[1]
        pairs = ops.l2_pair_dists64(self.rows, q[:, None].expand(n_sets, k, m, width).reshape(-1, width),
                                    rows[:, :, None].expand(n_sets, k, m).reshape(-1)).view(n_sets, k, m)
        pairs = torch.where(torch.isfinite(pairs), pairs, pairs.new_full((), float("inf")))
        return torch.where(rows >= 0, torch.argmin(pairs, dim=2), rows)

    def _search_sets(self, q, k, subset, exclude, what, grouped, return_members):
        if q.shape[1] == 1:      # a set of one member IS the plain search, bit for bit, and that scan is 1 - 4 % faster (profiles/search_sets.md)
            out = self._scan(q[:, 0], k, subset, None, exclude, what, grouped=grouped, stored=True)
        else:
            out = self._scan(q, k, subset, None, exclude, what, grouped=grouped, stored=True, sets=True)
        return (*out, self._attaining_members(q, out[1] if grouped else out[0])) if return_members else out

    def search_any(self, query_sets, k, sizes=None, subset=None, exclude=None, return_members=False):
        """SET QUERIES: (ids [S, k] int64, scores [S, k] fp32) for ``query_sets`` [S, M, dim], 1 <= M <= 64 -- S queries, each a SET of
        M member vectors, any of which may match: a title and its comments, the captions or chunks of a video, paraphrases.  A set's
        distance to a row is E = the MINIMUM over its members of the fp64 squared distance ``search`` forms, the result the k live
        rows (of ``subset``) with the smallest (E, row), and score = 1 - E / 2: the best score any member reaches.  The minimum is
        taken inside the scan (vtc_l2_search_sets), not merged on the host: no sync, no sort, every row once.  The members are
        prepared as ``search`` prepares queries; a non-finite one takes no part, a set of only such members is a row of -1 / -inf.
        ``sizes``: a host sequence of S ints in [1, M] for ragged sets -- set s is its first ``sizes[s]`` members (the rest are
        overwritten by member 0, which changes nothing).  ``exclude``: an int64 [S] device tensor, ONE row per set that it is never
        given.  ``return_members=True`` appends an int64 [S, k] tensor: the member that attains E for the returned row (the lowest
        on a tie), -1 where the row is -1; one more small launch (vtc_l2_pair_dists64), no sync.
        Sets are cut into calls of 64 // M sets, only enqueued.  THE COST: one gallery pass per started tile of 8 members per set
        -- what M separate queries cost, less their lists.  1 <= k <= min(64, len(index)).
        THERE IS NO ``after=`` and no deep form.  A set of more than 8 members is scanned as several tiles and a tile knows only its
        own members' minimum: a row an earlier page returned on one tile's distance would pass a cursor test against another tile's
        larger one and come back.  Paging needs the cursor test on the set-wide E, which the scan does not have."""
        k = self._checked_k(k, "search_any")
        return self._search_sets(self._set_queries(query_sets, sizes, "search_any"), k, subset, exclude, "search_any", False, return_members)

    def search_videos_any(self, query_sets, k, sizes=None, subset=None, exclude_videos=None, return_members=False):
        """``search_any`` of a GROUPED index: (video_ids [S, k] int64, row_ids [S, k] int64, scores [S, k] fp32), the k nearest distinct
        videos of every set, each by the row and the member that are nearest, as ``search_videos`` returns them.
        ``exclude_videos``: an int64 [S] device tensor, one VIDEO per set none of whose rows it is given.  ``sizes``,
        ``return_members`` (the member that attains the returned row's distance), the cost and the missing ``after=``:
        ``search_any``'s.  On an ungrouped index it raises ValueError."""
        if not self.grouped:
            raise ValueError("VideoIndex.search_videos_any: the index has no video ids (add(embeddings, video_ids=...)); search_any() returns rows")
        k = self._checked_k(k, "search_videos_any")
        return self._search_sets(self._set_queries(query_sets, sizes, "search_videos_any"), k, subset, exclude_videos, "search_videos_any", True,
                                 return_members)

    def _rows_by_video(self):
        """(the video ids of the rows, sorted, int64 [ntotal]; the rows in that order, int64 [ntotal]): a video's LIVE rows are one run,
        in ascending row order (a stable sort), and the dead rows lie behind every video id.  O(ntotal) memory whatever the number of
        videos asked for; sorted once per ``add`` / ``remove`` / ``load_state_dict`` and kept; no host sync."""
        if self._by_video is None or self._by_video[0] != self._generation:
            vid = self._video_ids[:self._n].to(torch.int64)
            if self._live is not None:
                vid = torch.where(self._live, vid, vid.new_full((), 1 << 40))
            self._by_video = (self._generation, *torch.sort(vid, stable=True))
        return self._by_video[1:]

    def similar_to_video(self, video_ids, k, subset=None, return_members=False):
        """THE VIDEOS NEAREST TO A VIDEO, by any of its rows: (video_ids [V, k] int64, row_ids [V, k] int64, scores [V, k] fp32) of a
        GROUPED index.  For every entry of ``video_ids`` (an integer [V] sequence or tensor) the query SET is the video's LIVE stored
        rows as the index keeps them -- a half index's rows widened exactly, nothing normalised again -- in ascending row order, and
        every row of that video is left out: ``search_videos_any`` with ``exclude_videos=video_ids``.  A video the index does not hold,
        or one with no live row, gives -1 / -1 / -inf and leaves the others alone.  A video with more than 64 live rows raises
        ValueError.  ``return_members`` appends the position, among the video's live rows, of the row that attains the distance.
        Finding the videos' rows is a binary search in the rows sorted by video -- sorted once per ``add`` / ``remove`` and kept,
        O(ntotal) memory whatever V is -- and reads the largest count back: ONE host sync per call; the searches are only enqueued,
        64 // (that count) videos a call.  No ``after=``: see ``search_any``."""
        if not self.grouped:
            raise ValueError("VideoIndex.similar_to_video: the index has no video ids (add(embeddings, video_ids=...)); similar() returns rows")
        k = self._checked_k(k, "similar_to_video")
        v = torch.as_tensor(video_ids)
        if v.dtype == torch.bool or v.is_floating_point() or v.is_complex() or v.dim() != 1 or v.shape[0] < 1:
            raise ValueError(f"VideoIndex.similar_to_video: video_ids must be an integer [V >= 1] sequence or tensor, got {v.dtype} {tuple(v.shape)}")
        v = v.to(device=self.device, dtype=torch.int64)
        n = self._n
        by_video, order = self._rows_by_video()
        lo, hi = torch.searchsorted(by_video, v), torch.searchsorted(by_video, v, right=True)
        count = torch.where((v >= 0) & (v < 2 ** 31), hi - lo, torch.zeros_like(lo))   # what is no video id has no rows
        most = int(count.max())                                                          # the one host sync
        if most > self.MAX_SET:
            raise ValueError(f"VideoIndex.similar_to_video: a video has {most} live rows, a set query takes at most {self.MAX_SET} members")
        m = max(most, 1)
        rows = order[(lo[:, None] + torch.arange(m, device=self.device)[None]).clamp(max=n - 1)]      # [V, m]; past the count: replaced below
        member = torch.arange(m, device=self.device)[None] < count[:, None]
        rows = torch.where(member, rows, rows[:, :1])                                    # padded by member 0, as ``sizes`` pads
        q = self._widened(self.rows[rows.reshape(-1)]).view(v.shape[0], m, self.width)    # half -> fp32 and scale * code are exact
        q = torch.where((count > 0)[:, None, None], q, q.new_full((), float("nan"))).contiguous()      # no live row: no member
        return self._search_sets(q, k, subset, v, "similar_to_video", True, return_members)

    def search_any_text(self, model, tokens, k, **kw):
        """``search_any`` of text given as token ids [S, M, ctx] -- a title and its comments as separate vectors, any of which may
        match: model.encode_text on the flattened tokens, normalisation, the set search.  ``**kw``: ``search_any``'s."""
        return self.search_any(self._text_sets(model, tokens, "search_any_text"), k, **kw)

    def search_videos_any_text(self, model, tokens, k, **kw):
        """``search_videos_any`` of text given as token ids [S, M, ctx] -- a title and its comments as separate vectors, any of which may
        match -- on a grouped index.  ``**kw``: ``search_videos_any``'s."""
        return self.search_videos_any(self._text_sets(model, tokens, "search_videos_any_text"), k, **kw)

    def _text_sets(self, model, tokens, what):
        if tokens.dim() != 3:
            raise ValueError(f"VideoIndex.{what}: tokens must be [S, M, ctx], got {tuple(tokens.shape)}")
        n_sets, m, ctx = tokens.shape
        return self._text_queries(model, tokens.reshape(n_sets * m, ctx), None, what).view(n_sets, m, -1)

    def search_text(self, model, title_tokens, k, comments=None, subset=None, after=None, exclude=None):
        """The k nearest videos of text queries given as token ids [Q, ctx]: model.encode_text + normalisation + search.  For a
        ``*_finaltf`` model that adapts the text branch (branch_to_adapt_val == "text"), ``comments`` [Q, n_comments, ctx] adapts the
        query through the Context Adapter Module as the wrapper's eval forward does.  ``after``: the cursor of ``search``, the next page.
        ``exclude``: ``search``'s, a row per query that it is never given."""
        return self.search(self._text_queries(model, title_tokens, comments, "search_text"), k, subset=subset, after=after, exclude=exclude)

    # ---- range search ----------------------------------------------------------------------------
    def _range_setup(self, queries, min_score, subset, what, many=False, stored=False):
        """([(the prepared queries [<= 64, width] of a slice, their radius2 as Python doubles)], the packed words of the rows that take
        part or None, the workspace of a slice's call).  ``many``: the slices go through the many-query count pass, whose workspace is
        larger.  ``stored``: the queries are stored rows [Q, width] widened to fp32 (``similar_within``), taken as they are."""
        self._check_subset(subset, what)
        if self._n == 0:
            raise ValueError(f"VideoIndex.{what}: the index is empty")
        q = queries if stored else self._prepared(queries, "queries", check=False)
        if q.shape[0] == 0:
            raise ValueError(f"VideoIndex.{what}: no queries")
        if isinstance(min_score, torch.Tensor):
            min_score = min_score.detach().cpu().double().reshape(-1).tolist() if min_score.dim() else float(min_score)
        if isinstance(min_score, (int, float)):
            scores = [float(min_score)] * q.shape[0]
        else:
            scores = [float(s) for s in min_score]
            if len(scores) != q.shape[0]:
                raise ValueError(f"VideoIndex.{what}: min_score must be a float or one per query ({q.shape[0]}), got {len(scores)}")
        radius2 = [2.0 * (1.0 - s) for s in scores]             # score = 1 - D / 2, in Python doubles
        words = self._live_words() if subset is None else subset.words()
        ws_bytes = ops.l2_range_many_workspace_bytes if many else ops.l2_range_workspace_bytes
        ws = self._workspace(ws_bytes(self._n, min(q.shape[0], ops.SEARCH_MAX_QUERIES), self.width))
        return q, radius2, words, ws

    def _range_many_route(self, n_queries):
        """Whether a range call of ``n_queries`` goes through vtc_l2_range_count_many_half."""
        return self.storage == torch.float16 and min(n_queries, ops.SEARCH_MAX_QUERIES) >= self.ROUTE_RANGE_MANY_MIN_QUERIES

    def range_search(self, queries, min_score, subset=None, sort=True, max_results=1 << 22):
        """EVERY live row that scores at least ``min_score`` against a query, however many: (lims [Q + 1] int64, ids [total] int64,
        scores [total] fp32) on the device, query i's hits being [lims[i], lims[i + 1]).  ``min_score``: a float, or one per query; a row
        is a hit iff its fp64 squared distance D <= 2 (1 - min_score) (computed in Python doubles, compared in fp64 on the device), and
        scores = 1 - D / 2 as ``search`` returns them.  ``sort=True`` orders every query's hits nearest first, by (fp64 distance, row);
        ``sort=False`` leaves them in ascending row order.  Exact (vtc_l2_range_count / vtc_l2_range_fill): the distances are the bits
        ``search`` compares, over the stored rows of a half index.  Removed rows and ``subset`` are honoured as in ``search``; any number
        of queries, 64 per call.  A non-finite query has no hits.
        One host sync per 64 queries: the number of hits is read back before the result is allocated, and more than ``max_results`` in
        total raise ValueError before that allocation (``range_count`` tells the size without fetching)."""
        return self._range_search(queries, min_score, subset, sort, max_results, "range_search", False)

    def _range_search(self, queries, min_score, subset, sort, max_results, what, many, stored=False, exclude=None):
        """``range_search`` and what is built on it: ``many`` chooses the count pass of every slice, ``stored`` takes the queries as they
        are, ``exclude`` (int64 [Q] row ids) is a row per query that it is never given."""
        q, radius2, words, ws = self._range_setup(queries, min_score, subset, what, many, stored)
        search = ops.l2_range_search_many if many else ops.l2_range_search
        lims, ids, dists, total = [torch.zeros(1, dtype=torch.int64, device=self.device)], [], [], 0
        for qs, r2, ex in self._sliced(q, radius2, exclude):
            l, i, d32, d64 = search(self.rows, qs, r2, live=words, max_results=int(max_results) - total, return_dists64=True, ws=ws, exclude=ex)
            if sort and i.numel():
                n_q = l.shape[0] - 1
                seg = torch.repeat_interleave(torch.arange(n_q, device=self.device), l[1:] - l[:-1], output_size=i.numel())
                order = torch.argsort(d64, stable=True)         # rows ascend inside a segment: stable sorts keep (distance, row)
                order = order[torch.argsort(seg[order], stable=True)]
                i, d32 = i[order], d32[order]
            lims.append(l[1:] + total)
            ids.append(i)
            dists.append(d32)
            total += i.numel()
        return torch.cat(lims), torch.cat(ids), 1.0 - torch.cat(dists) / 2.0

    def range_count(self, queries, min_score, subset=None):
        """int64 [Q] on the device: how many live rows (of the ``subset``) score at least ``min_score`` against every query -- the sizes
        of ``range_search``'s segments without fetching them.  Only enqueued: no host sync."""
        return self._range_count(queries, min_score, subset, "range_count", False)

    def _range_count(self, queries, min_score, subset, what, many):
        q, radius2, words, ws = self._range_setup(queries, min_score, subset, what, many)
        count = ops.l2_range_count_many if many else ops.l2_range_count
        out = []
        for qs, r2 in self._sliced(q, radius2):
            l = count(self.rows, qs, r2, live=words, ws=ws)
            out.append(l[1:] - l[:-1])
        return out[0] if len(out) == 1 else torch.cat(out)

    def range_search_many(self, queries, min_score, subset=None, sort=True, max_results=1 << 22):
        """``range_search(queries, min_score, subset, sort, max_results)`` for a BATCH: the same (lims, ids, scores), bit for bit, on
        every index.  On a half index with at least ROUTE_RANGE_MANY_MIN_QUERIES queries the count pass of every slice of 64 is
        vtc_l2_range_count_many_half -- one pass of the stored half rows through the matrix cores, only the pairs its error bound
        cannot decide taken in fp64, where ``range_search`` forms every distance in fp64, a gallery pass per 8 queries -- and the
        fill is ``range_search``'s.  The masked route's rules hold: removed rows and ``subset`` honoured, a non-finite query has no
        hits, one host sync per 64 queries.  In every other case (an fp32 index, fewer queries) the call IS ``range_search``.
        Not here: a grouped (distinct-video) range, more than 64 queries a library call, an MFMA pass over fp32 rows."""
        if not self._range_many_route(len(queries)):
            return self.range_search(queries, min_score, subset=subset, sort=sort, max_results=max_results)
        return self._range_search(queries, min_score, subset, sort, max_results, "range_search_many", True)

    def range_count_many(self, queries, min_score, subset=None):
        """``range_count(queries, min_score, subset)`` for a BATCH: the same int64 [Q], bit for bit, on every index; routed as
        ``range_search_many`` is (vtc_l2_range_count_many_half on a half index from ROUTE_RANGE_MANY_MIN_QUERIES queries on, otherwise
        the call IS ``range_count``).  Only enqueued: no host sync.  Not here: a grouped (distinct-video) range, more than 64 queries
        a library call, an MFMA pass over fp32 rows."""
        if not self._range_many_route(len(queries)):
            return self.range_count(queries, min_score, subset=subset)
        return self._range_count(queries, min_score, subset, "range_count_many", True)

    def similar_within(self, ids, min_score, subset=None, sort=True, max_results=1 << 22):
        """THE RANGE FORM OF ``similar``: (lims [Q + 1] int64, ids [total] int64, scores [total] fp32), every live row (of ``subset``)
        that scores at least ``min_score`` against the STORED row ``ids[q]`` (an int64 [Q] tensor of row ids), that row itself left
        out -- ``range_search_many`` with the stored rows as the queries (as ``similar`` takes them: never normalised again, a half
        index's row widened exactly) and routed as it is, so on a half index the slices of 64 go through the matrix cores.  A bit-equal
        duplicate of the row scores exactly 1 and IS returned: it is another row.  The query row need not be live nor a member of
        ``subset`` (the hits are).  An id outside [0, ntotal) cannot be validated without a host read: its segment is empty and the
        others are left alone.  ``min_score``, ``sort``, ``max_results`` and the one host sync per 64 queries: ``range_search``'s; the
        own row is dropped with torch ops whose sizes come back in that same read, no further sync.  On an fp32 index the call runs
        through the scan (vtc_l2_range_count).  Not here: a grouped (distinct-video) range, more than 64 queries a library call, an
        MFMA pass over fp32 rows."""
        ids, q = self._stored_queries(ids, "similar_within")
        return self._range_search(q, min_score, subset, sort, max_results, "similar_within", self._range_many_route(q.shape[0]), stored=True,
                                  exclude=ids)

    NEAR_DUPLICATES_SLICE = 16 * ops.SEARCH_MAX_QUERIES      # stored rows a ``similar_within`` call of ``near_duplicates``

    def near_duplicates(self, min_score, subset=None, max_results=1 << 22):
        """(pairs int64 [P, 2], scores fp32 [P]) on the device: EVERY unordered pair a < b of live rows (of ``subset``) whose stored rows
        score at least ``min_score`` against each other, ascending by (a, b) -- near-duplicate and repost detection over the whole
        gallery.  A loop of ``similar_within(sort=False)`` over the live rows in slices of NEAR_DUPLICATES_SLICE that keeps the hits
        above the own id; a pair's score is that of row b against the stored row a as the query.  On a half index every 64 rows are
        one pass of the gallery through the matrix cores (profiles/range_many.md); on an fp32 index the call runs through the scan, a
        gallery pass per 8 rows.  More than ``max_results`` pairs in total raise ValueError.  Host syncs: one to list the live rows,
        one per 64 rows (``range_search``'s) and one per slice.  Not here: restricting a slice's gallery to the rows above it (every
        pair is found from both ends and one is dropped), a grouped (distinct-video) range, more than 64 queries a library call, an
        MFMA pass over fp32 rows."""
        self._check_subset(subset, "near_duplicates")
        if self._n == 0:
            raise ValueError("VideoIndex.near_duplicates: the index is empty")
        words = self._live_words() if subset is None else subset.words()
        if words is None:
            rows = torch.arange(self._n, dtype=torch.int64, device=self.device)
        else:
            shifts = torch.arange(32, dtype=torch.int32, device=self.device)
            rows = torch.nonzero(((words[:, None] >> shifts[None]) & 1).reshape(-1)[:self._n]).reshape(-1)
        pairs, scores, total = [], [], 0
        for lo in range(0, rows.shape[0], self.NEAR_DUPLICATES_SLICE):
            own = rows[lo:lo + self.NEAR_DUPLICATES_SLICE]
            # an unordered pair is a hit from both of its ends: twice max_results hits in a slice are more than max_results pairs
            lims, hit, score = self.similar_within(own, min_score, subset=subset, sort=False, max_results=2 * int(max_results))
            a = torch.repeat_interleave(own, lims[1:] - lims[:-1], output_size=hit.numel())
            above = hit > a
            pairs.append(torch.stack([a[above], hit[above]], dim=1))
            scores.append(score[above])
            total += pairs[-1].shape[0]
            if total > int(max_results):
                raise ValueError(f"VideoIndex.near_duplicates: more than max_results={int(max_results)} pairs score at least {min_score} "
                                 "(raise it or the score)")
        if not pairs:
            return torch.empty(0, 2, dtype=torch.int64, device=self.device), torch.empty(0, dtype=torch.float32, device=self.device)
        return torch.cat(pairs), torch.cat(scores)

    def range_search_text(self, model, title_tokens, min_score, comments=None, **kw):
        """``range_search`` of text queries given as token ids, encoded as ``search_text`` encodes them."""
        return self.range_search(self._text_queries(model, title_tokens, comments, "range_search_text"), min_score, **kw)

    def range_subset(self, query, min_score, subset=None):
        """The live rows (of ``subset``) that score at least ``min_score`` against ONE query ([dim] or [1, dim]), as a ``RowSubset`` of
        this index built from the count pass's hit words: ``search(q, k, subset=index.range_subset(q, s))`` is the nearest k among the
        rows scoring at least s, and subsets chain.  Only enqueued: no host sync."""
        query = torch.as_tensor(query)
        if query.dim() == 1:
            query = query[None]
        if query.dim() != 2 or query.shape[0] != 1:
            raise ValueError(f"VideoIndex.range_subset: one query ([{self.dim}] or [1, {self.dim}]), got {tuple(query.shape)}")
        q, radius2, words, ws = self._range_setup(query, min_score, subset, "range_subset")
        ops.l2_range_count(self.rows, q, radius2, live=words, ws=ws)
        hit = ops.range_hit_words(ws, self._n, 1)[0].clone()
        shifts = torch.arange(32, dtype=torch.int32, device=self.device)
        flags = ((hit[:, None] >> shifts[None]) & 1).reshape(-1)[:self._n].to(torch.uint8).contiguous()
        out = RowSubset(self, flags)
        out._words, out._generation = hit, self._generation     # the hit words ARE the packed flags, dead rows already out
        return out

    def _text_queries(self, model, title_tokens, comments, what):
        if not title_tokens.is_cuda:
            raise RuntimeError(f"vtc_amd VideoIndex.{what}: token ids must be on the GPU (no CPU fallback)")
        if comments is not None and getattr(model, "branch_to_adapt_val", None) != "text":
            raise ValueError(f"VideoIndex.{what}: comments adapt the query only for a *_finaltf model with branch_to_adapt_val == 'text'")
        feats = model.encode_text(title_tokens)
        if comments is not None:
            b, ncomms, ntoks = comments.shape
            feats_comm = model.encode_text(comments.reshape(b * ncomms, ntoks))
            feats = model._pack()["cam"].forward(feats, feats_comm, comments)
        return ops.normalize_rows(feats.float().contiguous())
