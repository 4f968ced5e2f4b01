"""``EmbeddingIndex`` -- a gallery of embeddings resident on one GPU, searched with the fused
top-k kernels (``clipgpu_index_*``, include/clipgpu.h): what the reference's README asks of its users
("store the image embeddings, search with the text embedding", README.md:76-82; examples/search.rs)
without the [queries x gallery] score matrix or a host sort."""
from __future__ import annotations

import ctypes
from ctypes import c_void_p
from typing import NamedTuple, Tuple

import numpy as np

from ._lib import check, lib

TOPK_MAX = 128  # CLIPGPU_TOPK_MAX
RANGE_MAX = 1 << 28  # most records of a range search or a self-join (include/clipgpu.h)
MAX_CENTROIDS = 1 << 16  # most centroids of assign and kmeans (include/clipgpu.h)
CODES_MAX_E = 1024  # the widest rows enable_codes takes (include/clipgpu.h)
DTYPES = {"f32": 0, "f16": 1, "bf16": 2}  # enum clipgpu_index_dtype
PROB_ACTIVATIONS = {"softmax": 0, "sigmoid": 1}  # CLIPGPU_SIM_SOFTMAX, CLIPGPU_SIM_SIGMOID


def pack_allow(allowed) -> np.ndarray:
    """A bool array [n] as the ``allow`` bitmap of ``clipgpu_index_search_filtered``: ceil(n / 32)
    ``np.uint32`` words, row i at bit ``i & 31`` of word ``i >> 5``, zero-padded -- the words that
    ``np.packbits(allowed, bitorder="little")`` gives when read as little-endian ``uint32``."""
    a = np.asarray(allowed)
    if a.dtype != np.bool_ or a.ndim != 1:
        raise TypeError(f"allow must be a 1-d bool array, got dtype {a.dtype} with {a.ndim} dimensions")
    words = (a.size + 31) // 32
    bits = np.zeros(words * 32, np.uint64)
    bits[:a.size] = a
    return (bits.reshape(words, 32) << np.arange(32, dtype=np.uint64)).sum(axis=1, dtype=np.uint64).astype(np.uint32)


class KMeansResult(NamedTuple):
    """What ``EmbeddingIndex.kmeans`` returns."""
    centroids: np.ndarray  # f32 [C, E]
    labels: np.ndarray     # int64 [len(index)]: exactly assign(centroids); -1 for a dead or not allowed row
    scores: np.ndarray     # f32 [len(index)]: the cosine to the row's centroid; -inf where the label is -1
    counts: np.ndarray     # int64 [C]: the rows with each label
    moved: np.ndarray      # int64 [iters]: per iteration, the rows whose label changed (the first: all of them)
    iters: int             # assignments compared: <= max_iter; moved[-1] == 0 means converged


class EmbeddingIndex:
    """``E``-dimensional rows (E % 16 == 0), at most ``capacity`` of them (fixed: the device
    memory is allocated here), on GPU ``device``.  Rows keep the order they were added in; a search
    returns their positions in that order.  ``dtype`` is the storage type: "f32", or "f16" / "bf16"
    at half the memory (the search is only slightly faster for one query, 0.43 against 0.47 ms over
    a million 512-d rows, and no faster from 16 queries on: its kernels are not bound by reading the
    gallery).  Rows are always given as f32; a 16-bit
    index rounds them to nearest even on the device, and a search returns exactly what an f32 index
    of the rounded rows returns (include/clipgpu.h has the bound on a logit's change).  ``remove``
    marks rows dead without moving the others, ``set_rows`` overwrites rows in place (and revives
    them), and ``search(..., allow=)`` searches a subset, exactly.  ``search_probs`` is the same search
    with the softmax (over all searched rows) or sigmoid probabilities of the k results.  ``range_search``
    returns every row at or above a score threshold instead of the k best, and ``duplicates`` joins the
    gallery against itself at a threshold; neither builds the score matrix.  ``assign`` gives every row its
    nearest of C centroids and ``kmeans`` puts the rows into groups, reproducibly.  ``partition`` cuts the
    gallery into inverted lists by nearest centroid and ``search_probed`` searches only the ``nprobe`` lists
    closest to each query: approximate in which rows it looks at, exact in what it returns for them.
    ``enable_codes`` adds an int8 copy of the gallery and ``search_coded`` scans that copy for ``refine``
    candidates per query, which it re-ranks exactly: approximate in the candidates alone."""

    def __init__(self, E: int, capacity: int, device: int = 0, dtype: str = "f32"):
        self._h = None
        if dtype not in DTYPES:
            raise ValueError(f"dtype must be one of {sorted(DTYPES)}, got {dtype!r}")
        h = c_void_p()
        check(lib().clipgpu_index_create_ex(int(device), int(E), int(capacity), DTYPES[dtype], ctypes.byref(h)))
        self._h = h
        self.dtype = dtype
        self.E = int(E)
        self.capacity = int(capacity)
        self.device = int(device)

    @property
    def handle(self):
        if self._h is None:
            raise RuntimeError("index destroyed")
        return self._h

    def close(self) -> None:
        if getattr(self, "_h", None) is not None:
            lib().clipgpu_index_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self) -> "EmbeddingIndex":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __len__(self) -> int:
        return int(lib().clipgpu_index_size(self.handle))

    def clear(self) -> None:
        check(lib().clipgpu_index_clear(self.handle))

    def _rows(self, a, what: str) -> np.ndarray:
        x = np.ascontiguousarray(a, dtype=np.float32)
        if x.ndim == 1:
            x = x[None]
        if x.ndim != 2 or x.shape[1] != self.E:
            from .error import ShapeError
            raise ShapeError(f"Shape error: {what} must be [n, {self.E}], got {x.shape}")
        return x

    def _ids(self, ids) -> np.ndarray:
        x = np.atleast_1d(np.asarray(ids))
        if x.ndim != 1 or (x.size and not np.issubdtype(x.dtype, np.integer)):
            raise TypeError("ids must be a 1-d array of integers")
        return np.ascontiguousarray(x, dtype=np.int64)

    def remove(self, ids) -> None:
        """Marks the rows at ``ids`` dead: they never appear in a result again; all other rows keep
        their positions and ``len(self)`` is unchanged (it counts slots; ``live`` counts rows).
        Removing a dead row is a no-op and ids may repeat; an id outside [0, len(self)) raises and
        changes nothing."""
        x = self._ids(ids)
        check(lib().clipgpu_index_remove(self.handle, x.ctypes.data, x.size))

    @property
    def live(self) -> int:
        """The number of live rows."""
        return int(lib().clipgpu_index_live(self.handle))

    def is_live(self) -> np.ndarray:
        """A bool array [len(self)]: True where the row is live."""
        out = np.empty(len(self), np.uint8)
        if out.size:
            check(lib().clipgpu_index_get_live(self.handle, 0, out.size, out.ctypes.data))
        return out.astype(bool)

    def set_rows(self, ids, rows) -> None:
        """Overwrites the rows at ``ids`` (each < len(self), none twice) with ``rows`` [n, E] and marks
        them live: how the slot of a removed row is used again.  A 16-bit index rounds the rows as
        ``add`` does.  A bad or repeated id raises and changes nothing."""
        x = self._ids(ids)
        r = self._rows(rows, "rows")
        if r.shape[0] != x.size:
            from .error import ShapeError
            raise ShapeError(f"Shape error: {x.size} ids for {r.shape[0]} rows")
        check(lib().clipgpu_index_set_rows(self.handle, x.ctypes.data, r.ctypes.data, x.size))

    def add(self, rows) -> None:
        """Appends host rows [n, E]; raises "index full" (and adds nothing) beyond the capacity."""
        x = self._rows(rows, "rows")
        check(lib().clipgpu_index_add(self.handle, x.ctypes.data, x.shape[0]))

    def rows(self, first: int = 0, n=None) -> np.ndarray:
        """Rows [first, first + n) as stored, widened to f32 [n, E] (n = None: to the end): an export
        of the index; for a 16-bit index, the rounded rows."""
        n = len(self) - int(first) if n is None else int(n)
        out = np.empty((max(n, 0), self.E), np.float32)
        check(lib().clipgpu_index_get_rows(self.handle, int(first), n, out.ctypes.data))
        return out

    def add_device(self, d_rows: int, n: int, stream: int = 0) -> None:
        """Appends n rows from the device pointer ``d_rows`` (f32 [n, E] on this index's GPU), ordered
        on ``stream`` (a hipStream_t; 0 = the legacy default stream).  Does not synchronise.  A 16-bit
        index reads the rows four at a time: ``d_rows`` must then be 16-byte aligned."""
        check(lib().clipgpu_index_add_device(self.handle, c_void_p(d_rows), int(n), c_void_p(stream or None)))

    def _allow_words(self, allow):
        """The bitmap words of ``allow`` (None = no filter), checked before any native call."""
        if allow is None:
            return None
        a = np.asarray(allow)
        if a.dtype != np.bool_ or a.ndim != 1:
            raise TypeError(f"allow must be a 1-d bool array, got dtype {a.dtype} with {a.ndim} dimensions")
        if a.size != len(self):
            from .error import ShapeError
            raise ShapeError(f"Shape error: allow must have len(index) = {len(self)} entries, got {a.size}")
        return pack_allow(a)

    def search(self, queries, k: int, logit_scale: float = 1.0, logit_bias: float = 0.0, allow=None
               ) -> Tuple[np.ndarray, np.ndarray]:
        """The k best rows per query, best first: (indices int64 [nq, k], scores f32 [nq, k]) with
        score = dot(query, row).mul_add(logit_scale, logit_bias), bit-identical to
        ``similarity(..., "logits")``; equal scores come out by ascending index.  Removed rows never
        appear; ``allow`` (a bool array [len(self)], one for all queries) restricts the search to the
        rows where it is True, exactly: the result is that of an index holding only those rows.  Slots
        beyond min(k, live allowed rows) hold (-1, -inf).  1 <= k <= 128."""
        words = self._allow_words(allow)
        q = self._rows(queries, "queries")
        idx = np.empty((q.shape[0], int(k)), np.int64)
        score = np.empty((q.shape[0], int(k)), np.float32)
        check(lib().clipgpu_index_search_filtered(self.handle, q.ctypes.data, q.shape[0], int(k), float(logit_scale),
                                                  float(logit_bias), None if words is None else words.ctypes.data,
                                                  idx.ctypes.data, score.ctypes.data))
        return idx, score

    def search_device(self, d_queries: int, nq: int, k: int, d_idx: int, d_score: int, logit_scale: float = 1.0,
                      logit_bias: float = 0.0, stream: int = 0, d_allow: int = 0) -> None:
        """``search`` on device pointers (queries f32 [nq, E] in; int64 [nq, k] and f32 [nq, k] out),
        ordered on ``stream``; returns without synchronising.  ``d_allow``: a device pointer to the
        ``pack_allow`` words of an allow array (0 = none); it is read on ``stream``."""
        check(lib().clipgpu_index_search_filtered_device(self.handle, c_void_p(d_queries), int(nq), int(k),
                                                         float(logit_scale), float(logit_bias),
                                                         c_void_p(d_allow or None), c_void_p(d_idx), c_void_p(d_score),
                                                         c_void_p(stream or None)))

    @staticmethod
    def _range_args(threshold, limit, what: str) -> Tuple[float, int]:
        """(threshold, the result limit), checked before any native call."""
        thr = float(threshold)
        if thr != thr:
            raise ValueError("threshold must not be NaN")
        if isinstance(limit, bool) or not isinstance(limit, (int, np.integer)):
            raise TypeError(f"{what} must be an integer, got {type(limit).__name__}")
        if not 1 <= int(limit) <= RANGE_MAX:
            raise ValueError(f"{what} must be in 1..{RANGE_MAX} (2^28), got {int(limit)}")
        return thr, int(limit)

    @staticmethod
    def _check_range(rc: int, total: int, limit: int, what: str) -> None:
        """``check`` for the range forms: an overflow becomes ``ResultOverflow`` with the needed size."""
        if rc != 0 and total > limit:
            from .error import ResultOverflow
            msg = lib().clipgpu_last_error().decode("utf-8", "replace")
            raise ResultOverflow(f"{msg}: pass {what}={total}", total)
        check(rc)

    def range_search(self, queries, threshold: float, logit_scale: float = 1.0, logit_bias: float = 0.0, allow=None,
                     max_results: int = 1 << 20) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """EVERY live (and allowed) row whose score is >= ``threshold``, per query, for a caller who knows a
        score and not a k: (lims int64 [nq + 1], idx int64 [total], scores f32 [total]); query q's rows are
        ``idx[lims[q]:lims[q + 1]]``, best first, in ``search``'s order and with ``search``'s scores, bit for
        bit.  The comparison is f32 ``score >= threshold``; a NaN score never passes.  ``max_results``
        bounds the device buffer the results pass through (12 bytes each); more results than that raise
        ``ResultOverflow``, whose ``needed`` is the exact total to retry with."""
        thr, cap = self._range_args(threshold, max_results, "max_results")
        words = self._allow_words(allow)
        q = self._rows(queries, "queries")
        lims = np.zeros(q.shape[0] + 1, np.int64)
        idx = np.empty(cap, np.int64)
        score = np.empty(cap, np.float32)
        total = ctypes.c_int64(-1)
        rc = lib().clipgpu_index_range_search(self.handle, q.ctypes.data, q.shape[0], thr, float(logit_scale),
                                              float(logit_bias), None if words is None else words.ctypes.data, cap,
                                              lims.ctypes.data, idx.ctypes.data, score.ctypes.data,
                                              ctypes.addressof(total))
        self._check_range(rc, total.value, cap, "max_results")
        return lims, idx[:total.value].copy(), score[:total.value].copy()

    def range_search_device(self, d_queries: int, nq: int, threshold: float, capacity: int, d_out_query: int,
                            d_out_row: int, d_out_score: int, d_out_total: int, logit_scale: float = 1.0,
                            logit_bias: float = 0.0, stream: int = 0, d_allow: int = 0) -> None:
        """``range_search`` on device pointers, unsorted: records (query int32, row int32, score f32) go to
        three device arrays of ``capacity`` entries in no particular order, and the uint64 at ``d_out_total``
        (8-byte aligned; zeroed by this call on ``stream``) counts every hit, past the capacity too --
        min(total, capacity) records are valid, the complete set if total <= capacity.  Ordered on ``stream``;
        returns without synchronising."""
        thr, cap = self._range_args(threshold, capacity, "capacity")
        check(lib().clipgpu_index_range_search_device(self.handle, c_void_p(d_queries), int(nq), thr,
                                                      float(logit_scale), float(logit_bias), c_void_p(d_allow or None),
                                                      cap, c_void_p(d_out_query), c_void_p(d_out_row),
                                                      c_void_p(d_out_score), c_void_p(d_out_total),
                                                      c_void_p(stream or None)))

    def duplicates(self, threshold: float, logit_scale: float = 1.0, logit_bias: float = 0.0, allow=None,
                   max_pairs: int = 1 << 20) -> Tuple[np.ndarray, np.ndarray]:
        """The gallery joined against itself: every pair i < j of live (and allowed) rows with
        score(i, j) >= ``threshold``, as (pairs int64 [n, 2] sorted by (i, j), scores f32 [n]).  With the
        default scale 1 and bias 0 on unit rows the threshold is a cosine.  A score is exactly
        ``similarity(rows(), rows())[i, j]``.  Overflow as in ``range_search``."""
        thr, cap = self._range_args(threshold, max_pairs, "max_pairs")
        words = self._allow_words(allow)
        oi = np.empty(cap, np.int64)
        oj = np.empty(cap, np.int64)
        score = np.empty(cap, np.float32)
        total = ctypes.c_int64(-1)
        rc = lib().clipgpu_index_self_join(self.handle, thr, float(logit_scale), float(logit_bias),
                                           None if words is None else words.ctypes.data, cap, oi.ctypes.data,
                                           oj.ctypes.data, score.ctypes.data, ctypes.addressof(total))
        self._check_range(rc, total.value, cap, "max_pairs")
        n = total.value
        return np.stack([oi[:n], oj[:n]], axis=1), score[:n].copy()

    def rows_at(self, ids) -> np.ndarray:
        """The rows at ``ids`` as stored, widened to f32 [n, E], in the order of ``ids``; dead rows and
        repeated ids are allowed, an id outside [0, len(self)) raises."""
        x = self._ids(ids)
        out = np.empty((x.size, self.E), np.float32)
        check(lib().clipgpu_index_get_rows_at(self.handle, x.ctypes.data, x.size, out.ctypes.data))
        return out

    def _centroids(self, a, what: str) -> np.ndarray:
        """``a`` as f32 [C, E] with 1 <= C <= MAX_CENTROIDS, checked before any native call."""
        c = self._rows(a, what)
        if not 1 <= c.shape[0] <= MAX_CENTROIDS:
            raise ValueError(f"the number of centroids must be in 1..{MAX_CENTROIDS}, got {c.shape[0]}")
        return c

    def assign(self, centroids, logit_scale: float = 1.0, logit_bias: float = 0.0, allow=None
               ) -> Tuple[np.ndarray, np.ndarray]:
        """The nearest of ``centroids`` [C, E] for every row: (labels int64 [len(self)], scores f32
        [len(self)]).  ``labels[j]`` is what ``search(row j, 1)`` of an index holding the centroids returns
        (highest score, equal scores to the lower centroid, a NaN below -inf) and ``scores[j]`` has the bits
        of ``similarity(centroids, rows(), "logits")[labels[j], j]``; a row that is dead or not allowed by
        ``allow`` (as in ``search``) gets (-1, -inf).  1 <= C <= 65536."""
        words = self._allow_words(allow)
        c = self._centroids(centroids, "centroids")
        labels = np.empty(len(self), np.int64)
        scores = np.empty(len(self), np.float32)
        check(lib().clipgpu_index_assign(self.handle, c.ctypes.data, c.shape[0], float(logit_scale), float(logit_bias),
                                         None if words is None else words.ctypes.data, labels.ctypes.data,
                                         scores.ctypes.data))
        return labels, scores

    def assign_device(self, d_centroids: int, C: int, d_label: int, d_score: int, logit_scale: float = 1.0,
                      logit_bias: float = 0.0, stream: int = 0, d_allow: int = 0) -> None:
        """``assign`` on device pointers (centroids f32 [C, E], 16-byte aligned, in; labels int32
        [len(self)] and scores f32 [len(self)] out), ordered on ``stream``; returns without synchronising."""
        check(lib().clipgpu_index_assign_device(self.handle, c_void_p(d_centroids), int(C), float(logit_scale),
                                                float(logit_bias), c_void_p(d_allow or None), c_void_p(d_label),
                                                c_void_p(d_score), c_void_p(stream or None)))

    def kmeans(self, n_clusters=None, init=None, max_iter: int = 25, seed: int = 0, allow=None) -> "KMeansResult":
        """Spherical k-means over the live (and allowed) rows: Lloyd iterations of ``assign`` (scale 1, bias
        0) and an update whose sums are 64-bit integers (include/clipgpu.h has the arithmetic), so the result
        does not depend on the order of the rows: a repeated run and a permuted gallery give the same bits.
        ``init`` [C, E] is the start, used as given; with ``init=None`` the start is the stored rows at
        ``np.sort(np.random.default_rng(seed).choice(live allowed ids, n_clusters, replace=False))``.  Stops
        when no label changes or after ``max_iter`` assignments-and-updates; either way ``labels`` and
        ``scores`` are exactly ``assign(centroids)``.  An empty cluster keeps its centroid (``counts`` says
        which): re-seeding is the caller's business.  Returns a ``KMeansResult``."""
        if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)):
            raise TypeError(f"max_iter must be an integer, got {type(max_iter).__name__}")
        if int(max_iter) < 1:
            raise ValueError(f"max_iter must be at least 1, got {int(max_iter)}")
        words = self._allow_words(allow)
        if init is not None:
            cen = self._centroids(init, "init").copy()
            if n_clusters is not None and int(n_clusters) != cen.shape[0]:
                raise ValueError(f"n_clusters is {int(n_clusters)} but init has {cen.shape[0]} rows")
        else:
            if n_clusters is None:
                raise ValueError("n_clusters is required when init is None")
            if isinstance(n_clusters, bool) or not isinstance(n_clusters, (int, np.integer)):
                raise TypeError(f"n_clusters must be an integer, got {type(n_clusters).__name__}")
            if not 1 <= int(n_clusters) <= MAX_CENTROIDS:
                raise ValueError(f"n_clusters must be in 1..{MAX_CENTROIDS}, got {int(n_clusters)}")
            ok = self.is_live()
            if allow is not None:
                ok &= np.asarray(allow)
            ids = np.flatnonzero(ok)
            if int(n_clusters) > ids.size:
                raise ValueError(f"n_clusters is {int(n_clusters)} but only {ids.size} rows are live and allowed")
            cen = self.rows_at(np.sort(np.random.default_rng(seed).choice(ids, int(n_clusters), replace=False)))
        C = cen.shape[0]
        labels = np.empty(len(self), np.int64)
        scores = np.empty(len(self), np.float32)
        counts = np.empty(C, np.int64)
        moved = np.empty(int(max_iter), np.int64)
        iters = ctypes.c_int64(0)
        check(lib().clipgpu_index_kmeans(self.handle, C, cen.ctypes.data, int(max_iter),
                                         None if words is None else words.ctypes.data, labels.ctypes.data,
                                         scores.ctypes.data, counts.ctypes.data, moved.ctypes.data,
                                         ctypes.addressof(iters)))
        return KMeansResult(cen, labels, scores, counts, moved[:iters.value].copy(), int(iters.value))

    @staticmethod
    def _prob_args(k, activation) -> Tuple[int, int]:
        """(k, the activation's enum value), checked before any native call."""
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise TypeError(f"k must be an integer, got {type(k).__name__}")
        if not 1 <= int(k) <= TOPK_MAX:
            raise ValueError(f"k must be in 1..{TOPK_MAX}, got {int(k)}")
        if activation not in PROB_ACTIVATIONS:
            raise ValueError(f"activation must be one of {sorted(PROB_ACTIVATIONS)}, got {activation!r} "
                             "(logits alone: search)")
        return int(k), PROB_ACTIVATIONS[activation]

    def search_probs(self, queries, k: int, logit_scale: float = 1.0, logit_bias: float = 0.0,
                     activation: str = "softmax", allow=None, return_norm: bool = False):
        """``search`` with the probabilities of the k results: (indices, logits, probs f32 [nq, k]); the
        first two are exactly what ``search(..., allow=allow)`` returns.  "softmax": exp(l - M) / sum
        exp(l_i - M) over ALL live allowed rows (not only the k returned), M their largest logit -- what
        ``similarity(..., "softmax")`` gives over those rows, without the score matrix; "sigmoid":
        1 / (1 + exp(-l)), bit-identical to ``similarity(..., "sigmoid")``.  Empty slots hold probability
        0.  ``return_norm=True`` adds a fourth array f32 [nq, 2], (M, S = sum exp(l_i - M)) per query, so
        that any row's probability is exp(l - M) / S; for "sigmoid" it is NaN (there is no normaliser)."""
        k, act = self._prob_args(k, activation)
        words = self._allow_words(allow)
        q = self._rows(queries, "queries")
        idx = np.empty((q.shape[0], k), np.int64)
        score = np.empty((q.shape[0], k), np.float32)
        prob = np.empty((q.shape[0], k), np.float32)
        norm = np.full((q.shape[0], 2), np.nan, np.float32) if return_norm else None
        check(lib().clipgpu_index_search_probs(self.handle, q.ctypes.data, q.shape[0], k, float(logit_scale),
                                               float(logit_bias), act, None if words is None else words.ctypes.data,
                                               idx.ctypes.data, score.ctypes.data, prob.ctypes.data,
                                               None if norm is None else norm.ctypes.data))
        return (idx, score, prob, norm) if return_norm else (idx, score, prob)

    def search_probs_device(self, d_queries: int, nq: int, k: int, d_idx: int, d_score: int, d_prob: int,
                            logit_scale: float = 1.0, logit_bias: float = 0.0, activation: str = "softmax",
                            stream: int = 0, d_allow: int = 0, d_norm: int = 0) -> None:
        """``search_probs`` on device pointers (as ``search_device``; probs f32 [nq, k] out, ``d_norm`` f32
        [nq, 2] out or 0 = not wanted, written for "softmax" only), ordered on ``stream``; returns without
        synchronising."""
        k, act = self._prob_args(k, activation)
        check(lib().clipgpu_index_search_probs_device(self.handle, c_void_p(d_queries), int(nq), k, float(logit_scale),
                                                      float(logit_bias), act, c_void_p(d_allow or None),
                                                      c_void_p(d_idx), c_void_p(d_score), c_void_p(d_prob),
                                                      c_void_p(d_norm or None), c_void_p(stream or None)))

    # ---- inverted lists and the probed search ----------------------------------------------------------
    def partition(self, centroids) -> np.ndarray:
        """Cuts the gallery into ``C`` inverted lists: list c holds the live rows whose ``assign(centroids)``
        label is c, ids ascending; a row dead now is in no list.  ``centroids`` [C, E] (1 <= C <= 65536) are
        copied into the index.  Returns the list lengths, int64 [C].  ``remove`` keeps the partition valid;
        ``add``, ``add_device``, ``set_rows`` and ``clear`` make it stale (``n_lists == -1``) until
        ``partition`` is called again, which costs an ``assign`` plus a few milliseconds."""
        c = self._centroids(centroids, "centroids")
        counts = np.empty(c.shape[0], np.int64)
        check(lib().clipgpu_index_partition(self.handle, c.ctypes.data, c.shape[0], counts.ctypes.data))
        return counts

    def partition_kmeans(self, n_lists: int, max_iter: int = 25, seed: int = 0) -> "KMeansResult":
        """``kmeans(n_lists, max_iter=max_iter, seed=seed)`` followed by ``partition`` of its centroids;
        returns the ``KMeansResult`` (its ``counts`` are the list lengths)."""
        km = self.kmeans(n_lists, max_iter=max_iter, seed=seed)
        self.partition(km.centroids)
        return km

    @property
    def n_lists(self) -> int:
        """The number of lists of the partition, 0 if there is none, -1 if it is stale."""
        return int(lib().clipgpu_index_partition_lists(self.handle))

    def lists(self) -> Tuple[np.ndarray, np.ndarray]:
        """The partition as CSR: (offsets int64 [C + 1], ids int64 [offsets[C]]); list c is
        ``ids[offsets[c]:offsets[c + 1]]``, ascending."""
        offsets = np.zeros(max(self.n_lists, 0) + 1, np.int64)
        ids = np.empty(len(self), np.int64)
        check(lib().clipgpu_index_get_lists(self.handle, offsets.ctypes.data, ids.ctypes.data))
        return offsets, ids[:offsets[-1]].copy()

    def drop_partition(self) -> None:
        check(lib().clipgpu_index_drop_partition(self.handle))

    @staticmethod
    def _probe_args(k, nprobe) -> Tuple[int, int]:
        """(k, nprobe), checked before any native call."""
        for name, v in (("k", k), ("nprobe", nprobe)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"{name} must be an integer, got {type(v).__name__}")
            if not 1 <= int(v) <= TOPK_MAX:
                raise ValueError(f"{name} must be in 1..{TOPK_MAX}, got {int(v)}")
        return int(k), int(nprobe)

    def search_probed(self, queries, k: int, nprobe: int, logit_scale: float = 1.0, logit_bias: float = 0.0,
                      allow=None, return_probes: bool = False):
        """``search`` over the ``nprobe`` lists whose centroids are closest to each query (by the dot product,
        equal ones to the lower list): per query exactly -- ids, order and score bits -- what
        ``search(query, k, ..., allow=mask)`` returns with ``mask`` = the rows of those lists that are live and
        allowed.  A row outside the probed lists is never found: that is the whole approximation.
        ``nprobe >= n_lists`` is ``search`` itself.  1 <= nprobe <= 128.  ``return_probes=True`` adds the probed
        lists, int64 [nq, nprobe], best first, -1 past ``n_lists``.  Raises if there is no partition or it is
        stale."""
        k, nprobe = self._probe_args(k, nprobe)
        words = self._allow_words(allow)
        q = self._rows(queries, "queries")
        idx = np.empty((q.shape[0], k), np.int64)
        score = np.empty((q.shape[0], k), np.float32)
        probes = np.empty((q.shape[0], nprobe), np.int64) if return_probes else None
        check(lib().clipgpu_index_search_probed(self.handle, q.ctypes.data, q.shape[0], k, nprobe, float(logit_scale),
                                                float(logit_bias), None if words is None else words.ctypes.data,
                                                idx.ctypes.data, score.ctypes.data,
                                                None if probes is None else probes.ctypes.data))
        return (idx, score, probes) if return_probes else (idx, score)

    def search_probed_device(self, d_queries: int, nq: int, k: int, nprobe: int, d_idx: int, d_score: int,
                             logit_scale: float = 1.0, logit_bias: float = 0.0, stream: int = 0, d_allow: int = 0,
                             d_probes: int = 0) -> None:
        """``search_probed`` on device pointers (as ``search_device``; ``d_probes`` int64 [nq, nprobe] out or 0 =
        not wanted), ordered on ``stream``; returns without synchronising."""
        k, nprobe = self._probe_args(k, nprobe)
        check(lib().clipgpu_index_search_probed_device(self.handle, c_void_p(d_queries), int(nq), k, nprobe,
                                                       float(logit_scale), float(logit_bias),
                                                       c_void_p(d_allow or None), c_void_p(d_idx), c_void_p(d_score),
                                                       c_void_p(d_probes or None), c_void_p(stream or None)))

    # ---- int8 codes and the coded search ---------------------------------------------------------------
    def enable_codes(self) -> None:
        """Gives the index int8 codes: a second device array beside the gallery, ``capacity * (Ep + 4)`` bytes
        (Ep = E rounded up to 64; a quarter of an f32 gallery), one int8 per element and one f32 scale per row
        (include/clipgpu.h has the rule).  The rows present are coded now; ``add``, ``add_device`` and
        ``set_rows`` keep the codes current from here on, ``clear`` keeps them enabled.  A second call is a
        no-op.  E <= 1024."""
        if self.E > CODES_MAX_E:
            raise ValueError(f"codes need E <= {CODES_MAX_E}, got {self.E}")
        check(lib().clipgpu_index_enable_codes(self.handle))

    @property
    def has_codes(self) -> bool:
        return bool(lib().clipgpu_index_has_codes(self.handle))

    def drop_codes(self) -> None:
        """Frees the codes; ``search_coded`` raises until ``enable_codes`` is called again."""
        check(lib().clipgpu_index_drop_codes(self.handle))

    def codes(self, first: int = 0, n=None) -> Tuple[np.ndarray, np.ndarray]:
        """The codes of rows [first, first + n) (n = None: to the end): (int8 [n, E], scales f32 [n])."""
        n = len(self) - int(first) if n is None else int(n)
        out = np.empty((max(n, 0), self.E), np.int8)
        scales = np.empty(max(n, 0), np.float32)
        check(lib().clipgpu_index_get_codes(self.handle, int(first), n, out.ctypes.data, scales.ctypes.data))
        return out, scales

    @staticmethod
    def _coded_args(k, refine) -> Tuple[int, int]:
        """(k, refine), checked before any native call; refine None = min(128, max(32, 4 k))."""
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise TypeError(f"k must be an integer, got {type(k).__name__}")
        if not 1 <= int(k) <= TOPK_MAX:
            raise ValueError(f"k must be in 1..{TOPK_MAX}, got {int(k)}")
        if refine is None:
            refine = min(TOPK_MAX, max(32, 4 * int(k)))
        if isinstance(refine, bool) or not isinstance(refine, (int, np.integer)):
            raise TypeError(f"refine must be an integer, got {type(refine).__name__}")
        if not int(k) <= int(refine) <= TOPK_MAX:
            raise ValueError(f"refine must be in k..{TOPK_MAX}, got {int(refine)} with k = {int(k)}")
        return int(k), int(refine)

    def search_coded(self, queries, k: int, refine=None, logit_scale: float = 1.0, logit_bias: float = 0.0,
                     allow=None, return_candidates: bool = False):
        """``search`` in two stages: a coarse scan of the int8 codes picks ``refine`` candidate rows per query
        (by the integer dot product of the codes times the row's scale, equal ones to the lower row), and the
        candidates are re-ranked exactly.  Per query the result is -- ids, order and score bits -- what
        ``search(query, k, ..., allow=mask)`` returns with ``mask`` = its candidates: a row the coarse stage
        misses is never found, and that is the whole approximation.  With at most ``refine`` live allowed rows
        it is ``search`` itself.  1 <= k <= refine <= 128; ``refine=None`` is min(128, max(32, 4 k)).
        ``return_candidates=True`` adds (candidates int64 [nq, refine], -1 padded, and their coarse scores f32
        [nq, refine], -inf padded), best first.  Raises if the index has no codes."""
        k, refine = self._coded_args(k, refine)
        words = self._allow_words(allow)
        q = self._rows(queries, "queries")
        idx = np.empty((q.shape[0], k), np.int64)
        score = np.empty((q.shape[0], k), np.float32)
        cand = np.empty((q.shape[0], refine), np.int64) if return_candidates else None
        coarse = np.empty((q.shape[0], refine), np.float32) if return_candidates else None
        check(lib().clipgpu_index_search_coded(self.handle, q.ctypes.data, q.shape[0], k, refine, float(logit_scale),
                                               float(logit_bias), None if words is None else words.ctypes.data,
                                               idx.ctypes.data, score.ctypes.data,
                                               None if cand is None else cand.ctypes.data,
                                               None if coarse is None else coarse.ctypes.data))
        return (idx, score, cand, coarse) if return_candidates else (idx, score)

    def search_coded_device(self, d_queries: int, nq: int, k: int, d_idx: int, d_score: int, refine=None,
                            logit_scale: float = 1.0, logit_bias: float = 0.0, stream: int = 0, d_allow: int = 0,
                            d_cand: int = 0, d_coarse: int = 0) -> None:
        """``search_coded`` on device pointers (as ``search_device``; ``d_cand`` int64 [nq, refine] and
        ``d_coarse`` f32 [nq, refine] out, or 0 = not wanted), ordered on ``stream``; returns without
        synchronising."""
        k, refine = self._coded_args(k, refine)
        check(lib().clipgpu_index_search_coded_device(self.handle, c_void_p(d_queries), int(nq), k, refine,
                                                      float(logit_scale), float(logit_bias),
                                                      c_void_p(d_allow or None), c_void_p(d_idx), c_void_p(d_score),
                                                      c_void_p(d_cand or None), c_void_p(d_coarse or None),
                                                      c_void_p(stream or None)))
