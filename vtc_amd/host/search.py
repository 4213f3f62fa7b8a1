"""Query-time search: a stored gallery of video embeddings and the nearest videos of a few text queries.

Every other retrieval entry point of the package is an evaluation -- N paired rows in, a recall figure or N ranks out.  ``VideoIndex``
is what a retrieval model is for:

    index = VideoIndex(512)
    index.add(video_embeddings)                       # [n, 512] fp32, any number of times
    ids, scores = index.search_text(model, title_tokens, k=10)

The search is exact: fp64 squared distances of the stored fp32 rows, ties to the earlier row (libvtc_hip.so, vtc_l2_search for up to
``ROUTE_TOPK_MIN_QUERIES - 1`` queries, vtc_l2_topk(EXACT) above; both return the same ids by construction).  No CPU path.
"""
from __future__ import annotations

import torch

from .. import _lib as L
from .. import ops

__all__ = ["VideoIndex"]


class VideoIndex:
    #: queries per call from which search() goes through ops.l2_topk(precision=SWEEP_EXACT) instead of ops.l2_search (which takes up to
    #: 64).  Measured, profiles/search.md (d = 512, depth 11, medians of 30 alternating calls; us at 10^5 / 10^6 gallery rows, scan vs
    #: vtc_l2_topk): the scan's time grows with the number of queries (one gallery pass per started tile of 8), vtc_l2_topk's does not.
    #:    8 queries   244.4 vs 275.6 (1.13 x)   1 468.9 vs 2 229.0 (1.52 x)   scan faster
    #:    9           358.8 vs 386.6 (1.08 x)   2 818.6 vs 3 768.7 (1.34 x)   scan faster
    #:   10           366.8 vs 384.2 (1.05 x)   2 840.9 vs 3 759.1 (1.32 x)   scan faster at 10^6, within 5 % at 10^5
    #:   11           373.0 vs 383.1 (1.03 x)   2 883.2 vs 3 744.5 (1.30 x)   scan faster at 10^6, within 5 % at 10^5
    #:   12           381.7 vs 265.2 (0.69 x)   2 714.8 vs 2 198.2 (0.81 x)   vtc_l2_topk faster, and at 16, 32, 64 (4.5 - 5 x there)
    #: 12 is the first count at which vtc_l2_topk wins by more than 5 %.  (vtc_l2_topk takes 40 - 70 % longer at 9, 10 and 11 queries,
    #: as at 1 and 2, than at 8 and 12: unexplained, that entry is not changed here.  13 - 15 queries were not measured.)
    ROUTE_TOPK_MIN_QUERIES = 12
    MAX_K = 64                # one list entry per lane of a wavefront, as everywhere in the sweeps

    def __init__(self, dim, device="cuda", normalized=False):
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
        self._rows = torch.empty(0, self.width, dtype=torch.float32, device=device)       # capacity rows; the first _n are the index
        self._n = 0
        self._ws = None

    def __len__(self):
        return self._n

    # ---- rows ----------------------------------------------------------------------------------
    def _prepared(self, x, what, check=True):
        """fp32 [n, dim] on the index's device -> unit rows (unless the index was built as ``normalized``), zero-padded to ``width``;
        with ``check``, NaN / inf rows are rejected as the eval entry points reject them (ops.nonfinite_bits: a 4-byte device-to-host
        read, so a host sync)."""
        x = torch.as_tensor(x)
        if x.dim() != 2 or x.shape[1] != self.dim:
            raise ValueError(f"VideoIndex: {what} must be [n, {self.dim}], got {tuple(x.shape)}")
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        if x.shape[0] == 0:
            return x.new_zeros(0, self.width)
        if not self.normalized:
            x = ops.normalize_rows(x)
        if check and ops.nonfinite_bits(x, x):
            raise ValueError(f"VideoIndex: non-finite values in the {what}" + ("" if self.normalized else " (after normalisation: a NaN, an inf "
                             "or an all-zero row)") + " -- such a row has no distance to anything")
        if self.width != self.dim:
            x = torch.nn.functional.pad(x, (0, self.width - self.dim))
        return x

    def add(self, embeddings):
        """Appends [n, dim] fp32 rows; their ids are their positions in insertion order.  Returns the id of the first one."""
        x = self._prepared(embeddings, "embeddings")
        first, n = self._n, x.shape[0]
        if first + n > self._rows.shape[0]:                 # amortised doubling
            grown = torch.empty(max(first + n, 2 * self._rows.shape[0], 1024), self.width, dtype=torch.float32, device=self.device)
            grown[:first] = self._rows[:first]
            self._rows = grown
        self._rows[first:first + n] = x
        self._n = first + n
        return first

    @property
    def rows(self):
        """The stored rows [len, width] (a view)."""
        return self._rows[:self._n]

    def state_dict(self):
        return {"rows": self.rows[:, :self.dim].clone(), "count": self._n, "dim": self.dim, "normalized": self.normalized}

    def load_state_dict(self, state):
        rows = torch.as_tensor(state["rows"])
        if int(state.get("dim", self.dim)) != self.dim or rows.dim() != 2 or rows.shape[1] != self.dim or int(state["count"]) != rows.shape[0]:
            raise ValueError(f"VideoIndex.load_state_dict: rows {tuple(rows.shape)}, count {state.get('count')} do not fit dim {self.dim}")
        rows = rows.to(device=self.device, dtype=torch.float32)
        if rows.shape[0] and ops.nonfinite_bits(rows.contiguous(), rows.contiguous()):
            raise ValueError("VideoIndex.load_state_dict: non-finite values in the stored rows")
        self._rows = torch.nn.functional.pad(rows, (0, self.width - self.dim)).contiguous()     # stored rows are final: not normalised again
        self._n = rows.shape[0]

    # ---- search --------------------------------------------------------------------------------
    def _workspace(self, nbytes):
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = None
            self._ws = ops.workspace(nbytes, self.device)
        return self._ws

    def search(self, queries, k):
        """(ids [Q, k] int64, scores [Q, k] fp32), both on the device: the k nearest stored rows of every query, nearest first, and
        score = 1 - |q - g|^2 / 2, the cosine for unit rows.  1 <= k <= min(64, len(index)).
        Fewer than ROUTE_TOPK_MIN_QUERIES queries -- batch 1 is the design point -- are only enqueued: no device-to-host read, no host
        sync.  A query with a NaN / inf (or an all-zero row, which has no direction) is not rejected there; the scan gives it a row of
        ids -1 and scores -inf.  From ROUTE_TOPK_MIN_QUERIES queries on the queries are checked first, as add() checks its rows, and a
        non-finite one raises ValueError: vtc_l2_topk has no defined answer for such a row."""
        k = int(k)
        if not 1 <= k <= min(self.MAX_K, self._n):
            raise ValueError(f"VideoIndex.search: k={k} must be in [1, min({self.MAX_K}, len(index) = {self._n})]")
        scan = 0 < len(queries) < min(self.ROUTE_TOPK_MIN_QUERIES, ops.SEARCH_MAX_QUERIES + 1)
        q = self._prepared(queries, "queries", check=not scan)
        if q.shape[0] == 0:
            raise ValueError("VideoIndex.search: no queries")
        g = self.rows
        if scan:
            ws = self._workspace(ops.l2_search_workspace_bytes(self._n, q.shape[0], self.width, k))
            ids, dists, _ = ops.l2_search(g, q, k, ws=ws)         # the word is not read: no sync (a bad query's row is -1 / +inf)
        else:
            ws = self._workspace(L.lib().vtc_l2_topk_workspace_bytes(self._n, q.shape[0], self.width, L.SWEEP_EXACT, 0))
            ids, dists = ops.l2_topk(g, q, k, precision=L.SWEEP_EXACT, ws=ws)
        return ids, 1.0 - dists / 2.0

    def search_text(self, model, title_tokens, k, comments=None):
        """The k nearest videos of text queries given as token ids [Q, ctx]: model.encode_text + normalisation + search.  For a
        ``*_finaltf`` model that adapts the text branch (branch_to_adapt_val == "text"), ``comments`` [Q, n_comments, ctx] adapts the
        query through the Context Adapter Module as the wrapper's eval forward does."""
        if not title_tokens.is_cuda:
            raise RuntimeError("vtc_amd VideoIndex.search_text: token ids must be on the GPU (no CPU fallback)")
        if comments is not None and getattr(model, "branch_to_adapt_val", None) != "text":
            raise ValueError("VideoIndex.search_text: comments adapt the query only for a *_finaltf model with branch_to_adapt_val == 'text'")
        feats = model.encode_text(title_tokens)
        if comments is not None:
            b, ncomms, ntoks = comments.shape
            feats_comm = model.encode_text(comments.reshape(b * ncomms, ntoks))
            feats = model._pack()["cam"].forward(feats, feats_comm, comments)
        return self.search(ops.normalize_rows(feats.float().contiguous()), k)
