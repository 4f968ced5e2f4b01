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
DEEP_K_MAX = 4096  # CLIPGPU_DEEP_K_MAX: the largest k of search_deep
COMPOUND_TERMS_MAX = 16  # CLIPGPU_COMPOUND_TERMS_MAX: the most terms of one compound query
COMPOUND_OPS = {"min": 0, "max": 1}  # CLIPGPU_COMPOUND_MIN (all-of), CLIPGPU_COMPOUND_MAX (any-of)
GROUP_MAX = (1 << 31) - 1  # the largest group label of set_groups (include/clipgpu.h)
RANGE_MAX = 1 << 28  # most records of a range search or a self-join (include/clipgpu.h)
MAX_CENTROIDS = 1 << 16  # most centroids of assign and kmeans (include/clipgpu.h)
CLASSIFY_K_MAX = 16  # CLIPGPU_CLASSIFY_K_MAX: the most labels per row of classify
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
    with the softmax (over all searched rows) or sigmoid probabilities of the k results.  ``search_deep`` is
    ``search`` for k up to 4096, as exact.  ``search_compound`` takes queries made of up to 16 terms and scores a
    row by the smallest (all-of) or largest (any-of) of its term logits, in one scan.  ``set_groups`` labels rows
    and ``search_grouped`` returns the k best groups, each by its best row.  ``search_diverse`` re-ranks a pool of
    the best rows for variety (maximal marginal relevance), on the device.  ``neighbors`` returns the k rows
    closest to stored rows and ``knn_graph`` does so for every row, the row itself left out.  ``range_search``
    returns every row at or above a score threshold instead of the k best, and ``duplicates`` joins the
    gallery against itself at a threshold; neither builds the score matrix.  ``duplicate_groups`` gives every row
    the label of its group of near-duplicates (the connected components of ``duplicates``' pairs) without the pair
    list.  ``assign`` gives every row its
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
    def _deep_k(k) -> int:
        """k, checked before any native call."""
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise TypeError(f"k must be an integer, got {type(k).__name__}")
        if not 1 <= int(k) <= DEEP_K_MAX:
            raise ValueError(f"k must be in 1..{DEEP_K_MAX}, got {int(k)}")
        return int(k)

    def search_deep(self, queries, k: int, logit_scale: float = 1.0, logit_bias: float = 0.0, allow=None,
                    return_passes: bool = False):
        """``search`` for 1 <= k <= 4096: exactly the first k live (and allowed) rows per query in ``search``'s
        order, with ``search``'s scores bit for bit and (-1, -inf) beyond the rows there are; for k <= 128 the
        result is ``search``'s.  No score matrix and no k-deep list: a radix select finds each query's k-th key
        in a few scans of the gallery, one more scan emits the rows at or above it and a sort orders them.
        ``return_passes=True`` adds int32 [nq], the selection scans each query needed (1 .. 8; mass ties drive
        it up).  The first call allocates the search's 36 MiB work area, kept until the index is closed."""
        k = self._deep_k(k)
        words = self._allow_words(allow)
        q = self._rows(queries, "queries")
        idx = np.empty((q.shape[0], k), np.int64)
        score = np.empty((q.shape[0], k), np.float32)
        passes = np.empty(q.shape[0], np.int32) if return_passes else None
        check(lib().clipgpu_index_search_deep(self.handle, q.ctypes.data, q.shape[0], k, float(logit_scale),
                                              float(logit_bias), None if words is None else words.ctypes.data,
                                              idx.ctypes.data, score.ctypes.data,
                                              None if passes is None else passes.ctypes.data))
        return (idx, score, passes) if return_passes else (idx, score)

    def search_deep_device(self, d_queries: int, nq: int, k: int, d_idx: int, d_score: int, logit_scale: float = 1.0,
                           logit_bias: float = 0.0, stream: int = 0, d_allow: int = 0, d_passes: int = 0) -> None:
        """``search_deep`` on device pointers (as ``search_device``; ``d_passes`` int32 [nq] out or 0 = not
        wanted), ordered on ``stream``; enqueues a fixed sequence of launches and returns without
        synchronising."""
        check(lib().clipgpu_index_search_deep_device(self.handle, c_void_p(d_queries), int(nq), self._deep_k(k),
                                                     float(logit_scale), float(logit_bias), c_void_p(d_allow or None),
                                                     c_void_p(d_idx), c_void_p(d_score), c_void_p(d_passes or None),
                                                     c_void_p(stream or None)))

    # ---- compound queries ------------------------------------------------------------------------------
    @staticmethod
    def _compound_args(k, op) -> Tuple[int, int]:
        """(k, the op's enum value), checked before any native call."""
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise TypeError(f"k must be an integer, got {type(k).__name__}")
        if not 1 <= int(k) <= TOPK_MAX:
            raise ValueError(f"k must be in 1..{TOPK_MAX}, got {int(k)}")
        if op not in COMPOUND_OPS:
            raise ValueError(f"op must be one of {sorted(COMPOUND_OPS)}, got {op!r}")
        return int(k), COMPOUND_OPS[op]

    def search_compound(self, terms, lims, k: int, op: str, logit_scale: float = 1.0, logit_bias: float = 0.0,
                        allow=None) -> Tuple[np.ndarray, np.ndarray]:
        """``search`` for queries made of several terms.  ``terms`` f32 [T, E]; ``lims`` integers [Q + 1] with
        ``lims[0] == 0`` and ``lims[Q] == T``: compound query q owns ``terms[lims[q]:lims[q + 1]]``, 1 to 16 of
        them, and one call may mix sizes.  A row's score is the smallest (``op="min"``: all-of, "a dog" AND "a
        beach") or the largest (``op="max"``: any-of, a prompt ensemble) of its term logits, each with
        ``similarity``'s bits; it comes back as +0.0 if it is a zero and as the canonical NaN if it is one.  Under
        "min" a NaN term makes the score NaN (ranked last, still an entry); under "max" a NaN term is ignored
        unless all are.  Returns (indices int64 [Q, k], scores f32 [Q, k]): the k best live allowed rows per
        query, best first, equal scores by ascending row, (-1, -inf) beyond the rows there are -- exact and
        bit-reproducible, without the [T, N] matrix.  A one-term query is ``search``.  1 <= k <= 128."""
        k, opv = self._compound_args(k, op)
        words = self._allow_words(allow)
        t = self._rows(terms, "terms")
        l = np.asarray(lims)
        if l.ndim != 1 or l.size < 2 or not np.issubdtype(l.dtype, np.integer):
            raise ValueError("lims must be a 1-d array of at least two integers: [0, ..., T]")
        l = np.ascontiguousarray(l, dtype=np.int64)
        n = np.diff(l)
        if l[0] != 0 or l[-1] != t.shape[0] or (n < 0).any():
            raise ValueError(f"lims must ascend from 0 to the number of terms, {t.shape[0]}")
        if (n < 1).any() or (n > COMPOUND_TERMS_MAX).any():
            raise ValueError(f"a compound query has 1..{COMPOUND_TERMS_MAX} terms, got groups of {int(n.min())} to "
                             f"{int(n.max())}")
        Q = l.size - 1
        idx = np.empty((Q, k), np.int64)
        score = np.empty((Q, k), np.float32)
        check(lib().clipgpu_index_search_compound(self.handle, t.ctypes.data, t.shape[0], l.ctypes.data, Q, k, opv,
                                                  float(logit_scale), float(logit_bias),
                                                  None if words is None else words.ctypes.data, idx.ctypes.data,
                                                  score.ctypes.data))
        return idx, score

    def search_compound_device(self, d_terms: int, n_terms: int, d_lims: int, nq: int, k: int, op: str, d_idx: int,
                               d_score: int, logit_scale: float = 1.0, logit_bias: float = 0.0, stream: int = 0,
                               d_allow: int = 0, max_terms: int = COMPOUND_TERMS_MAX) -> None:
        """``search_compound`` on device pointers (terms f32 [n_terms, E], 16-byte aligned, and lims int32
        [nq + 1] in; int64 [nq, k] and f32 [nq, k] out), ordered on ``stream``; returns without synchronising.
        The offsets cannot be checked without reading them back: ``max_terms`` (1..16) is the caller's bound on
        the size of a group -- 16 is always valid, a tighter bound is faster -- and the device clamps every
        group to 1..max_terms terms inside ``d_terms``."""
        k, opv = self._compound_args(k, op)
        if not 1 <= int(max_terms) <= COMPOUND_TERMS_MAX:
            raise ValueError(f"max_terms must be in 1..{COMPOUND_TERMS_MAX}, got {int(max_terms)}")
        check(lib().clipgpu_index_search_compound_device(self.handle, c_void_p(d_terms), int(n_terms), c_void_p(d_lims),
                                                         int(nq), int(max_terms), k, opv, float(logit_scale),
                                                         float(logit_bias), c_void_p(d_allow or None), c_void_p(d_idx),
                                                         c_void_p(d_score), c_void_p(stream or None)))

    # ---- group labels and the grouped search ------------------------------------------------------------
    def set_groups(self, ids, groups) -> None:
        """Gives the rows at ``ids`` (each < len(self), none twice) the group labels ``groups``: integers in
        [0, 2^31), or -1 to make a row ungrouped again.  A row that never got a label is ungrouped, a group of
        its own.  ``add`` leaves new rows ungrouped; ``set_rows`` and ``remove`` keep a slot's label, so a reused
        slot belongs to its old group until ``set_groups`` says otherwise; ``clear`` resets every label.  A bad
        id or label raises and changes nothing.  The first call allocates 4 bytes per slot of the capacity."""
        x = self._ids(ids)
        g = np.atleast_1d(np.asarray(groups))
        if g.ndim != 1 or (g.size and not np.issubdtype(g.dtype, np.integer)):
            raise TypeError("groups must be a 1-d array of integers")
        if g.size != x.size:
            from .error import ShapeError
            raise ShapeError(f"Shape error: {x.size} ids for {g.size} groups")
        if g.size and (int(g.min()) < -1 or int(g.max()) > GROUP_MAX):
            raise ValueError(f"a group label must be in 0..{GROUP_MAX}, or -1 for no group, got "
                             f"{int(g.min())} to {int(g.max())}")
        g = np.ascontiguousarray(g, dtype=np.int32)
        check(lib().clipgpu_index_set_groups(self.handle, x.ctypes.data, g.ctypes.data, x.size))

    def groups(self) -> np.ndarray:
        """The group labels, int64 [len(self)]: -1 for an ungrouped row."""
        out = np.empty(len(self), np.int32)
        check(lib().clipgpu_index_groups(self.handle, out.ctypes.data))
        return out.astype(np.int64)

    @staticmethod
    def _grouped_k(k) -> int:
        """k, checked before any native call."""
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise TypeError(f"k must be an integer, got {type(k).__name__}")
        if not 1 <= int(k) <= TOPK_MAX:
            raise ValueError(f"k must be in 1..{TOPK_MAX}, got {int(k)}")
        return int(k)

    def search_grouped(self, queries, k: int, logit_scale: float = 1.0, logit_bias: float = 0.0, allow=None,
                       return_groups: bool = False):
        """The k best GROUPS per query, each by its best row (field collapsing, group-by search): over a gallery
        of video frames, the k best videos with the best frame of each, where ``search`` would return k frames of
        one video.  Take the live allowed rows in ``search``'s order; a group's representative is its first row
        in that order, and the result is the first k representatives: (indices int64 [nq, k], scores f32 [nq, k])
        with ``search``'s score bits, (-1, -inf) beyond the groups that have a live allowed row.
        ``return_groups=True`` adds int64 [nq, k], the label of each result, -1 for an ungrouped row or an empty
        slot.  Exact: an index without labels returns what ``search`` returns, and removing or filtering out a
        group's best row makes its next best row the representative.  1 <= k <= 128."""
        k = self._grouped_k(k)
        words = self._allow_words(allow)
        q = self._rows(queries, "queries")
        idx = np.empty((q.shape[0], k), np.int64)
        score = np.empty((q.shape[0], k), np.float32)
        group = np.empty((q.shape[0], k), np.int64) if return_groups else None
        check(lib().clipgpu_index_search_grouped(self.handle, q.ctypes.data, q.shape[0], k, float(logit_scale),
                                                 float(logit_bias), None if words is None else words.ctypes.data,
                                                 idx.ctypes.data, score.ctypes.data,
                                                 None if group is None else group.ctypes.data))
        return (idx, score, group) if return_groups else (idx, score)

    def search_grouped_device(self, d_queries: int, nq: int, k: int, d_idx: int, d_score: int, logit_scale: float = 1.0,
                              logit_bias: float = 0.0, stream: int = 0, d_allow: int = 0, d_group: int = 0) -> None:
        """``search_grouped`` on device pointers (as ``search_device``, queries 16-byte aligned; ``d_group`` int64
        [nq, k] out or 0 = not wanted), ordered on ``stream``; returns without synchronising."""
        check(lib().clipgpu_index_search_grouped_device(self.handle, c_void_p(d_queries), int(nq), self._grouped_k(k),
                                                        float(logit_scale), float(logit_bias),
                                                        c_void_p(d_allow or None), c_void_p(d_idx), c_void_p(d_score),
                                                        c_void_p(d_group or None), c_void_p(stream or None)))

    # ---- the diversified search ---------------------------------------------------------------------------
    @staticmethod
    def _diverse_args(k, pool, diversity) -> Tuple[int, int, float]:
        """(k, pool, diversity), checked before any native call; pool None: min(128, max(32, 4 k))."""
        k = EmbeddingIndex._grouped_k(k)
        if pool is None:
            pool = min(TOPK_MAX, max(32, 4 * k))
        if isinstance(pool, bool) or not isinstance(pool, (int, np.integer)):
            raise TypeError(f"pool must be an integer, got {type(pool).__name__}")
        if not 1 <= int(pool) <= TOPK_MAX:
            raise ValueError(f"pool must be in 1..{TOPK_MAX}, got {int(pool)}")
        if k > int(pool):
            raise ValueError(f"k <= pool is required (pool in 1..{TOPK_MAX}), got k {k}, pool {int(pool)}")
        lam = float(diversity)
        if not 0.0 <= lam <= 1.0:  # a NaN fails both comparisons
            raise ValueError(f"diversity must be in [0, 1], got {lam}")
        return k, int(pool), lam

    def search_diverse(self, queries, k: int, diversity: float = 0.5, pool=None, logit_scale: float = 1.0,
                       logit_bias: float = 0.0, allow=None, return_pool: bool = False):
        """``search`` with variety (maximal marginal relevance): over a library of bursts and re-saved copies, k
        different pictures where ``search`` would return k of one scene.  The candidates are ``search(queries,
        pool, ...)`` (``pool`` None: min(128, max(32, 4 k)); 1 <= k <= pool <= 128).  The first result is the best
        candidate; each further one is the candidate with the best ``(1 - diversity) * logit - diversity * (its
        largest logit-scaled similarity to a result already taken)`` in f32, ties by the position in the pool.
        Returns (indices int64 [nq, k], scores f32 [nq, k]) in the order taken, each score the candidate's own
        ``search`` logit, bit for bit; (-1, -inf) once the candidates are used up.  ``diversity`` 0 is ``search``,
        1 is farthest-first.  ``return_pool=True`` adds (pool_idx [nq, pool], pool_scores [nq, pool]), the
        candidates.  Gather, Gram matrix and selection run on the device (include/clipgpu.h has the exact rule)."""
        k, pool, lam = self._diverse_args(k, pool, diversity)
        words = self._allow_words(allow)
        q = self._rows(queries, "queries")
        idx = np.empty((q.shape[0], k), np.int64)
        score = np.empty((q.shape[0], k), np.float32)
        pidx = np.empty((q.shape[0], pool), np.int64) if return_pool else None
        pscore = np.empty((q.shape[0], pool), np.float32) if return_pool else None
        check(lib().clipgpu_index_search_diverse(self.handle, q.ctypes.data, q.shape[0], k, pool, lam, float(logit_scale),
                                                 float(logit_bias), None if words is None else words.ctypes.data,
                                                 idx.ctypes.data, score.ctypes.data,
                                                 None if pidx is None else pidx.ctypes.data,
                                                 None if pscore is None else pscore.ctypes.data))
        return (idx, score, pidx, pscore) if return_pool else (idx, score)

    def search_diverse_device(self, d_queries: int, nq: int, k: int, d_idx: int, d_score: int, diversity: float = 0.5,
                              pool=None, logit_scale: float = 1.0, logit_bias: float = 0.0, stream: int = 0,
                              d_allow: int = 0, d_pool_idx: int = 0, d_pool_score: int = 0) -> None:
        """``search_diverse`` on device pointers (as ``search_device``; ``d_pool_idx`` int64 and ``d_pool_score``
        f32 [nq, pool] out, both or 0 = not wanted), ordered on ``stream``; returns without synchronising."""
        k, pool, lam = self._diverse_args(k, pool, diversity)
        check(lib().clipgpu_index_search_diverse_device(self.handle, c_void_p(d_queries), int(nq), k, pool, lam,
                                                        float(logit_scale), float(logit_bias), c_void_p(d_allow or None),
                                                        c_void_p(d_idx), c_void_p(d_score), c_void_p(d_pool_idx or None),
                                                        c_void_p(d_pool_score or None), c_void_p(stream or None)))

    # ---- neighbours of stored rows and the k-NN graph ------------------------------------------------------
    def _neighbors(self, ids, n: int, k, logit_scale, logit_bias, allow) -> Tuple[np.ndarray, np.ndarray]:
        k = self._grouped_k(k)
        words = self._allow_words(allow)
        idx = np.empty((n, k), np.int64)
        score = np.empty((n, k), np.float32)
        check(lib().clipgpu_index_neighbors(self.handle, None if ids is None else ids.ctypes.data, n, k,
                                            float(logit_scale), float(logit_bias),
                                            None if words is None else words.ctypes.data, idx.ctypes.data,
                                            score.ctypes.data))
        return idx, score

    def neighbors(self, ids, k: int, logit_scale: float = 1.0, logit_bias: float = 0.0, allow=None
                  ) -> Tuple[np.ndarray, np.ndarray]:
        """The k rows closest to each stored row ``ids[r]`` ("more like this"): (indices int64 [n, k], scores f32
        [n, k]), the k best live allowed rows other than the row itself, in ``search``'s order with ``search``'s
        score bits -- exactly ``search(rows_at([i]), k, ..., allow=allow & ~{i})``, without the rows leaving the
        device.  The row is left out before the selection, so exact duplicates of it are all kept (dropping the
        first hit of ``search(k + 1)`` loses one of them or keeps the row).  ``allow`` filters the candidates only;
        a removed row gets (-1, -inf) throughout, as do the slots beyond the rows there are.  ``ids`` may repeat, in
        any order; one outside [0, len(self)) raises.  1 <= k <= 128."""
        x = self._ids(ids)
        return self._neighbors(x, x.size, k, logit_scale, logit_bias, allow)

    def knn_graph(self, k: int, logit_scale: float = 1.0, logit_bias: float = 0.0, allow=None
                  ) -> Tuple[np.ndarray, np.ndarray]:
        """The k-NN graph of the gallery: ``neighbors(arange(len(self)), k, ...)`` in one pass, as (indices int64
        [len(self), k], scores), except that the graph is over the live allowed rows: a row that is removed or
        not allowed gets (-1, -inf) throughout and costs no work."""
        return self._neighbors(None, len(self), k, logit_scale, logit_bias, allow)

    def neighbors_device(self, d_ids: int, n: int, k: int, d_idx: int, d_score: int, logit_scale: float = 1.0,
                         logit_bias: float = 0.0, stream: int = 0, d_allow: int = 0) -> None:
        """``neighbors`` on device pointers (ids int64 [n] in, 0 = every slot with ``knn_graph``'s rule and n =
        len(self); int64 [n, k] and f32 [n, k] out), ordered on ``stream``; returns without synchronising.  An id
        outside [0, len(self)) gives its row (-1, -inf) throughout."""
        check(lib().clipgpu_index_neighbors_device(self.handle, c_void_p(d_ids or None), int(n), self._grouped_k(k),
                                                   float(logit_scale), float(logit_bias), c_void_p(d_allow or None),
                                                   c_void_p(d_idx), c_void_p(d_score), c_void_p(stream or None)))

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

    def duplicate_groups(self, threshold: float, logit_scale: float = 1.0, logit_bias: float = 0.0, allow=None,
                         set_groups: bool = False) -> Tuple[np.ndarray, int]:
        """The near-duplicates as groups instead of pairs: the connected components of the graph whose vertices
        are the live (and allowed) rows and whose edges are exactly the pairs ``duplicates(threshold, ...)`` lists,
        computed on the device without the pair list (which is quadratic in the size of a cluster and may exceed
        any ``max_pairs``).  Returns (labels int64 [len(self)], n_groups int): ``labels[i]`` is the smallest row id
        of i's component -- a row with no duplicate is its own label -- and -1 for a row that is dead or not
        allowed; ``n_groups`` counts the components, singletons included.  The result is a function of the rows,
        the threshold and the filter alone.  ``set_groups=True`` also makes the labels the group labels, on the
        device: every slot's label is overwritten (a dead or not allowed row becomes ungrouped), after which
        ``search_grouped`` returns one row per duplicate group.  The first call allocates 8 bytes per slot of
        the capacity."""
        thr = float(threshold)
        if thr != thr:
            raise ValueError("threshold must not be NaN")
        words = self._allow_words(allow)
        labels = np.empty(len(self), np.int64)
        count = ctypes.c_int64(0)
        check(lib().clipgpu_index_components(self.handle, thr, float(logit_scale), float(logit_bias),
                                             None if words is None else words.ctypes.data, int(bool(set_groups)),
                                             labels.ctypes.data, ctypes.addressof(count)))
        return labels, int(count.value)

    def duplicate_groups_device(self, threshold: float, d_label: int, d_count: int = 0, logit_scale: float = 1.0,
                                logit_bias: float = 0.0, stream: int = 0, d_allow: int = 0, set_groups: bool = False
                                ) -> None:
        """``duplicate_groups`` on device pointers (labels int32 [len(self)] out, 0 = not wanted, allowed only with
        ``set_groups``; ``d_count`` uint32 out or 0 = not wanted), ordered on ``stream``; enqueues three launches
        and returns without synchronising."""
        thr = float(threshold)
        if thr != thr:
            raise ValueError("threshold must not be NaN")
        check(lib().clipgpu_index_components_device(self.handle, thr, float(logit_scale), float(logit_bias),
                                                    c_void_p(d_allow or None), int(bool(set_groups)),
                                                    c_void_p(d_label or None), c_void_p(d_count or None),
                                                    c_void_p(stream or None)))

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

    def _classify_args(self, k, activation):
        """(k, the activation's enum) of a ``classify`` call, checked before any native call."""
        if not 1 <= int(k) <= CLASSIFY_K_MAX:
            raise ValueError(f"k must be in 1..{CLASSIFY_K_MAX}, got {k}")
        if activation not in PROB_ACTIVATIONS:
            raise ValueError(f"activation must be one of {sorted(PROB_ACTIVATIONS)}, got {activation!r}")
        return int(k), PROB_ACTIVATIONS[activation]

    def classify(self, labels, k: int, logit_scale: float = 1.0, logit_bias: float = 0.0,
                 activation: str = "softmax", allow=None, return_norm: bool = False):
        """The k best of ``labels`` [C, E] for every stored row, best first: (labels int64 [len(self), k],
        logits f32, probs f32).  Row j's entries are what ``search_probs(row j, k)`` of an f32 index holding the
        labels returns, with ``assign``'s scan: the rows are read as stored, one launch covers the gallery.
        "softmax": exp(l - M) / sum exp(l_i - M) over ALL C labels; "sigmoid": 1 / (1 + exp(-l)).  Entries past
        min(k, C) are (-1, -inf, 0), and so is every entry of a row that is dead or not allowed by ``allow`` (as in
        ``search``).  ``return_norm=True`` adds f32 [len(self), 2], (M, S) per row; NaN for "sigmoid".
        1 <= C <= 65536, 1 <= k <= 16; k = 1 is ``assign``, bit for bit."""
        k, act = self._classify_args(k, activation)
        words = self._allow_words(allow)
        c = self._centroids(labels, "labels")
        n = len(self)
        idx = np.empty((n, k), np.int64)
        score = np.empty((n, k), np.float32)
        prob = np.empty((n, k), np.float32)
        norm = np.full((n, 2), np.nan, np.float32) if return_norm else None
        check(lib().clipgpu_index_classify(self.handle, c.ctypes.data, c.shape[0], k, float(logit_scale),
                                           float(logit_bias), act, None if words is None else words.ctypes.data,
                                           idx.ctypes.data, score.ctypes.data, prob.ctypes.data,
                                           None if norm is None else norm.ctypes.data))
        return (idx, score, prob, norm) if return_norm else (idx, score, prob)

    def classify_device(self, d_labels: int, C: int, k: int, d_label: int, d_score: int, d_prob: int,
                        logit_scale: float = 1.0, logit_bias: float = 0.0, activation: str = "softmax",
                        stream: int = 0, d_allow: int = 0, d_norm: int = 0) -> None:
        """``classify`` on device pointers (labels f32 [C, E], 16-byte aligned, in; labels int32, logits and
        probs f32 [len(self), k] out; ``d_norm`` f32 [len(self), 2] out or 0 = not wanted, written for "softmax"
        only), ordered on ``stream``; returns without synchronising."""
        k, act = self._classify_args(k, activation)
        check(lib().clipgpu_index_classify_device(self.handle, c_void_p(d_labels), int(C), k, float(logit_scale),
                                                  float(logit_bias), act, c_void_p(d_allow or None),
                                                  c_void_p(d_label), c_void_p(d_score), c_void_p(d_prob),
                                                  c_void_p(d_norm or None), c_void_p(stream or None)))

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
