"""``EmbeddingIndex`` -- a gallery of embeddings resident on one GPU, searched with the fused
top-k kernels (``clipgpu_index_*``, include/clipgpu.h): what the reference's README asks of its users
("store the image embeddings, search with the text embedding", README.md:76-82; examples/search.rs)
without the [queries x gallery] score matrix or a host sort."""
from __future__ import annotations

import ctypes
from ctypes import c_void_p
from typing import Tuple

import numpy as np

from ._lib import check, lib

TOPK_MAX = 128  # CLIPGPU_TOPK_MAX


class EmbeddingIndex:
    """``E``-dimensional f32 rows (E % 16 == 0), at most ``capacity`` of them (fixed: the device
    memory is allocated here), on GPU ``device``.  Rows keep the order they were added in; a search
    returns their positions in that order."""

    def __init__(self, E: int, capacity: int, device: int = 0):
        self._h = None
        h = c_void_p()
        check(lib().clipgpu_index_create(int(device), int(E), int(capacity), ctypes.byref(h)))
        self._h = h
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

    def add(self, rows) -> None:
        """Appends host rows [n, E]; raises "index full" (and adds nothing) beyond the capacity."""
        x = self._rows(rows, "rows")
        check(lib().clipgpu_index_add(self.handle, x.ctypes.data, x.shape[0]))

    def add_device(self, d_rows: int, n: int, stream: int = 0) -> None:
        """Appends n rows from the device pointer ``d_rows`` (f32 [n, E] on this index's GPU), ordered
        on ``stream`` (a hipStream_t; 0 = the legacy default stream).  Does not synchronise."""
        check(lib().clipgpu_index_add_device(self.handle, c_void_p(d_rows), int(n), c_void_p(stream or None)))

    def search(self, queries, k: int, logit_scale: float = 1.0, logit_bias: float = 0.0
               ) -> Tuple[np.ndarray, np.ndarray]:
        """The k best rows per query, best first: (indices int64 [nq, k], scores f32 [nq, k]) with
        score = dot(query, row).mul_add(logit_scale, logit_bias), bit-identical to
        ``similarity(..., "logits")``; equal scores come out by ascending index.  Slots beyond
        min(k, len(self)) hold (-1, -inf).  1 <= k <= 128."""
        q = self._rows(queries, "queries")
        idx = np.empty((q.shape[0], int(k)), np.int64)
        score = np.empty((q.shape[0], int(k)), np.float32)
        check(lib().clipgpu_index_search(self.handle, q.ctypes.data, q.shape[0], int(k), float(logit_scale),
                                         float(logit_bias), idx.ctypes.data, score.ctypes.data))
        return idx, score

    def search_device(self, d_queries: int, nq: int, k: int, d_idx: int, d_score: int, logit_scale: float = 1.0,
                      logit_bias: float = 0.0, stream: int = 0) -> None:
        """``search`` on device pointers (queries f32 [nq, E] in; int64 [nq, k] and f32 [nq, k] out),
        ordered on ``stream``; returns without synchronising."""
        check(lib().clipgpu_index_search_device(self.handle, c_void_p(d_queries), int(nq), int(k), float(logit_scale),
                                                float(logit_bias), c_void_p(d_idx), c_void_p(d_score),
                                                c_void_p(stream or None)))
