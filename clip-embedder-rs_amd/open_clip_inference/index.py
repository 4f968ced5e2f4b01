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
DTYPES = {"f32": 0, "f16": 1, "bf16": 2}  # enum clipgpu_index_dtype


class EmbeddingIndex:
    """``E``-dimensional rows (E % 16 == 0), at most ``capacity`` of them (fixed: the device
    memory is allocated here), on GPU ``device``.  Rows keep the order they were added in; a search
    returns their positions in that order.  ``dtype`` is the storage type: "f32", or "f16" / "bf16"
    at half the memory (the search is only slightly faster for one query, 0.43 against 0.47 ms over
    a million 512-d rows, and no faster from 16 queries on: its kernels are not bound by reading the
    gallery).  Rows are always given as f32; a 16-bit
    index rounds them to nearest even on the device, and a search returns exactly what an f32 index
    of the rounded rows returns (include/clipgpu.h has the bound on a logit's change)."""

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
