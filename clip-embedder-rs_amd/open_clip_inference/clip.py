"""``Clip`` facade — mirror of src/clip.rs (kept as-is in the north star; restated
here because the reference's Rust cannot be compiled in this image).  The math is
the reference's: dot -> ``mul_add(logit_scale, logit_bias)`` (defaults 1.0 / 0.0)
-> sigmoid or max-subtracted softmax -> sort descending."""
from __future__ import annotations

import math
import os
from typing import List, Sequence, Tuple

import numpy as np

from .config import ModelConfig
from .model_manager import verify_model_dir
from .text import TextEmbedder
from .vision import VisionEmbedder, _Builder


class Clip:
    def __init__(self, vision: VisionEmbedder, text: TextEmbedder, model_dir: str):
        self.vision = vision
        self.text = text
        self.model_dir = model_dir

    @classmethod
    def from_local_dir(cls, model_dir: str) -> _Builder:  # src/clip.rs:48-66
        return _Builder(cls, model_dir=model_dir)

    @classmethod
    def from_local_id(cls, model_id: str) -> _Builder:  # src/clip.rs:35-46
        return _Builder(cls, model_id=model_id)

    @classmethod
    def _build(cls, model_dir, devices, dtype, max_batch, **opts):
        verify_model_dir(model_dir, need_tokenizer=True)
        v = VisionEmbedder._build(model_dir, devices, dtype, max_batch, **opts)
        t = TextEmbedder._build(model_dir, devices, dtype, max_batch)
        return cls(v, t, model_dir)

    def duplicate(self) -> "Clip":  # src/clip.rs:68-73
        return Clip(self.vision.duplicate(), self.text.duplicate(), self.model_dir)

    def get_model_config(self) -> ModelConfig:  # src/clip.rs:75-77
        return self.text.model_config

    def _scale_bias(self):
        mc = self.text.model_config
        scale = 1.0 if mc.logit_scale is None else mc.logit_scale
        bias = 0.0 if mc.logit_bias is None else mc.logit_bias
        return np.float32(scale), np.float32(bias)

    def _activation(self) -> str:
        act = self.text.model_config.activation_function or "softmax"
        return "sigmoid" if act == "sigmoid" else "softmax"

    def _scores(self, embs: np.ndarray, query: np.ndarray, activation: str) -> np.ndarray:
        """logits = embs . query, mul_add(scale, bias), then the activation -- the reference's
        f32 arithmetic bit for bit (clipgpu_facade_scores, csrc/host/facade.cpp)."""
        from ._lib import check_host, host_lib
        from .engine import SIM_ACTIVATIONS
        e = np.ascontiguousarray(embs, dtype=np.float32)
        q = np.ascontiguousarray(query, dtype=np.float32).reshape(-1)
        if e.ndim != 2 or e.shape[1] != q.shape[0]:
            from .error import ShapeError
            raise ShapeError(f"Shape error: {e.shape} . {q.shape}")
        scale, bias = self._scale_bias()
        out = np.empty(e.shape[0], np.float32)
        check_host(host_lib().clipgpu_facade_scores(e.ctypes.data, e.shape[0], q.ctypes.data, e.shape[1],
                                                    float(scale), float(bias), SIM_ACTIVATIONS[activation],
                                                    out.ctypes.data))
        return out

    def compare(self, image, text: str) -> float:  # src/clip.rs:79-90
        v = self.vision.embed_image(image)
        t = self.text.embed_text(text)
        return float(self._scores(v[None], t, "logits")[0])

    def classify(self, image, labels: Sequence[str]) -> List[Tuple[str, float]]:  # src/clip.rs:92-132
        v = self.vision.embed_image(image)
        t = self.text.embed_texts(labels)
        probs = self._scores(t, v, self._activation())
        res = [(str(l), float(p)) for l, p in zip(labels, probs)]
        res.sort(key=lambda x: -x[1])  # stable, descending (sort_by partial_cmp)
        return res

    def rank_images(self, images, text: str) -> List[Tuple[int, float]]:  # src/clip.rs:134-170
        v = self.vision.embed_images(images)
        t = self.text.embed_text(text)
        probs = self._scores(v, t, self._activation())
        res = [(i, float(p)) for i, p in enumerate(probs)]
        res.sort(key=lambda x: -x[1])
        return res

    # -- many images x many labels, math on the GPU -------------------
    def _device_probs(self, img_embs, txt_embs, axis: int) -> np.ndarray:
        from .engine import similarity
        scale, bias = self._scale_bias()
        act = self.text.model_config.activation_function or "softmax"
        return similarity(img_embs, txt_embs, float(scale), float(bias), "sigmoid" if act == "sigmoid" else "softmax",
                          axis, self.vision.session.devices[0])

    def classify_many(self, images, labels: Sequence[str]) -> List[List[Tuple[str, float]]]:
        """classify (src/clip.rs:92-132) for every image of a batch: one image batch, one label
        batch, the [images x labels] probabilities on the GPU; each list sorted descending."""
        probs = self._device_probs(self.vision.embed_images(images), self.text.embed_texts(labels), axis=1)
        out = []
        for row in probs:
            res = [(str(l), float(p)) for l, p in zip(labels, row)]
            res.sort(key=lambda x: -x[1])
            out.append(res)
        return out

    def rank_images_many(self, images, texts: Sequence[str]) -> List[List[Tuple[int, float]]]:
        """rank_images (src/clip.rs:134-170) for every query text: softmax over the images per
        text on the GPU; one descending (image_index, probability) list per text."""
        probs = self._device_probs(self.vision.embed_images(images), self.text.embed_texts(texts), axis=0)
        out = []
        for col in probs.T:
            res = [(i, float(p)) for i, p in enumerate(col)]
            res.sort(key=lambda x: -x[1])
            out.append(res)
        return out

    # -- a gallery resident on the GPU, searched top-k (README.md:76-82, examples/search.rs) ----
    def build_index(self, images, capacity=None, dtype="f32"):
        """Embeds ``images`` and stores them in an ``EmbeddingIndex`` on the vision engine's first
        device (``capacity`` rows, default: as many as there are images; ``dtype`` "f32", "f16" or
        "bf16": the index's storage type); image i is index i."""
        from .index import EmbeddingIndex
        embs = self.vision.embed_images(images)
        index = EmbeddingIndex(embs.shape[1], len(embs) if capacity is None else int(capacity),
                               self.vision.session.devices[0], dtype)
        index.add(embs)
        return index

    def search(self, index, texts: Sequence[str], k: int, allow=None, nprobe=None, refine=None
               ) -> List[List[Tuple[int, float]]]:
        """Semantic search (examples/search.rs; rank_images, src/clip.rs:134-170, cut to its k best):
        per text the k best rows of ``index`` as (gallery index, logit), best first, equal logits by
        ascending index.  The logits use the model's logit_scale / logit_bias (defaults 1.0 / 0.0).
        Logits, not probabilities: ``rank`` returns the probabilities.  Removed rows never appear; ``allow`` (a bool array
        [len(index)]) restricts the search to the rows where it is True, and a text gets fewer than k
        pairs when fewer rows are allowed.  ``nprobe`` (None: every row, as always) searches only the
        ``nprobe`` lists of the index's partition closest to each text (``EmbeddingIndex.search_probed``).
        ``refine`` (None: the exact search, as always) re-ranks the ``refine`` candidates that a scan of the index's
        int8 codes picks per text (``EmbeddingIndex.search_coded``; the index needs ``enable_codes()``).  Giving
        both ``refine`` and ``nprobe`` raises ``ValueError``."""
        if refine is not None and nprobe is not None:
            raise ValueError("give refine (the coded search) or nprobe (the probed search), not both")
        scale, bias = self._scale_bias()
        if refine is not None:
            idx, score = index.search_coded(self.text.embed_texts(texts), k, refine, float(scale), float(bias),
                                            allow=allow)
        elif nprobe is None:
            idx, score = index.search(self.text.embed_texts(texts), k, float(scale), float(bias), allow=allow)
        else:
            idx, score = index.search_probed(self.text.embed_texts(texts), k, nprobe, float(scale), float(bias),
                                             allow=allow)
        return [[(int(i), float(s)) for i, s in zip(ri, rs) if i >= 0] for ri, rs in zip(idx, score)]

    def search_above(self, index, texts: Sequence[str], min_logit: float, allow=None, max_results: int = 1 << 20
                     ) -> List[List[Tuple[int, float]]]:
        """``search`` by score instead of by count: per text EVERY row of ``index`` whose logit (the model's
        logit_scale / logit_bias, as ``search``) is >= ``min_logit``, as (gallery index, logit), best first.
        ``allow`` as in ``search``; more than ``max_results`` results in all raise ``ResultOverflow``
        (``EmbeddingIndex.range_search``)."""
        scale, bias = self._scale_bias()
        lims, idx, score = index.range_search(self.text.embed_texts(texts), min_logit, float(scale), float(bias),
                                              allow=allow, max_results=max_results)
        return [[(int(i), float(s)) for i, s in zip(idx[a:b], score[a:b])] for a, b in zip(lims[:-1], lims[1:])]

    def find_duplicates(self, index, min_cosine: float, allow=None, max_pairs: int = 1 << 20
                        ) -> List[Tuple[int, int, float]]:
        """Near-duplicates in a gallery: every pair i < j of live (and allowed) rows of ``index`` whose cosine
        (the rows are L2-normalised embeddings; scale 1, bias 0) is >= ``min_cosine``, as (i, j, cosine)
        sorted by (i, j) (``EmbeddingIndex.duplicates``)."""
        pairs, score = index.duplicates(min_cosine, 1.0, 0.0, allow=allow, max_pairs=max_pairs)
        return [(int(i), int(j), float(s)) for (i, j), s in zip(pairs, score)]

    def cluster(self, index, n_clusters: int, seed: int = 0, max_iter: int = 25, allow=None
                ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Puts the live (and allowed) rows of ``index`` into ``n_clusters`` groups by cosine (spherical
        k-means from ``n_clusters`` rows drawn with ``seed``; ``EmbeddingIndex.kmeans``): (labels int64
        [len(index)], -1 for a row that is dead or not allowed; counts int64 [n_clusters]; centroids f32
        [n_clusters, E], unit rows).  The same index, seed and arguments give the same bits on every run."""
        km = index.kmeans(n_clusters, max_iter=max_iter, seed=seed, allow=allow)
        return km.labels, km.counts, km.centroids

    def rank(self, index, texts: Sequence[str], k: int, allow=None) -> List[List[Tuple[int, float]]]:
        """rank_images (src/clip.rs:134-170) against a resident gallery, cut to its k best: per text
        [(gallery index, probability)], best first, with the model's activation (softmax over all live
        allowed rows of ``index``, or sigmoid), logit_scale and logit_bias.  The probabilities are
        those of ``rank_images_many`` over the same rows, without the [images x texts] matrix."""
        scale, bias = self._scale_bias()
        idx, _, prob = index.search_probs(self.text.embed_texts(texts), k, float(scale), float(bias),
                                          self._activation(), allow=allow)
        return [[(int(i), float(p)) for i, p in zip(ri, rp) if i >= 0] for ri, rp in zip(idx, prob)]

    def build_label_index(self, labels: Sequence[str], dtype="f32"):
        """Embeds ``labels`` and stores them in an ``EmbeddingIndex`` on the text engine's first device
        (``dtype`` as for ``build_index``); label i is index i.  For ``classify_topk``."""
        from .index import EmbeddingIndex
        embs = self.text.embed_texts(labels)
        index = EmbeddingIndex(embs.shape[1], len(embs), self.text.session.devices[0], dtype)
        index.add(embs)
        return index

    def classify_topk(self, images, label_index, k: int) -> List[List[Tuple[int, float]]]:
        """classify (src/clip.rs:92-132) for many images against a label index (``build_label_index``),
        cut to its k best: per image [(label index, probability)], best first, the probabilities those of
        ``classify_many`` (softmax over all labels of the index, or sigmoid)."""
        scale, bias = self._scale_bias()
        idx, _, prob = label_index.search_probs(self.vision.embed_images(images), k, float(scale), float(bias),
                                                self._activation())
        return [[(int(i), float(p)) for i, p in zip(ri, rp) if i >= 0] for ri, rp in zip(idx, prob)]

    @staticmethod
    def softmax(logits) -> np.ndarray:  # src/clip.rs:172-179 (f32, sequential sum; facade.cpp)
        # host-only library (no HIP / RCCL): usable on a host without ROCm
        from ._lib import check_host, host_lib
        x = np.ascontiguousarray(logits, dtype=np.float32).reshape(-1)
        if x.size == 0:
            return x.copy()
        one = np.ones(1, np.float32)  # logits = x[i] * 1 (exact) .mul_add(1, 0) (exact)
        out = np.empty(x.size, np.float32)
        check_host(host_lib().clipgpu_facade_scores(x.ctypes.data, x.size, one.ctypes.data, 1, 1.0, 0.0, 0,
                                                    out.ctypes.data))
        return out

    @staticmethod
    def sigmoid(logit: float) -> float:  # src/clip.rs:181-185
        from ._lib import check_host, host_lib
        x = np.array([logit], np.float32)
        one = np.ones(1, np.float32)
        out = np.empty(1, np.float32)
        check_host(host_lib().clipgpu_facade_scores(x.ctypes.data, 1, one.ctypes.data, 1, 1.0, 0.0, 1,
                                                    out.ctypes.data))
        return float(out[0])
