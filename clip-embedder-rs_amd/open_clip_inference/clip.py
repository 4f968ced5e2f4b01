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
    def build_index(self, images, capacity=None, dtype="f32", groups=None):
        """Embeds ``images`` and stores them in an ``EmbeddingIndex`` on the vision engine's first
        device (``capacity`` rows, default: as many as there are images; ``dtype`` "f32", "f16" or
        "bf16": the index's storage type); image i is index i.  ``groups`` (None: every row ungrouped) is one
        group label per image, for ``search_grouped``: the video of a frame, the picture of a crop."""
        from .index import EmbeddingIndex
        embs = self.vision.embed_images(images)
        if groups is not None and len(groups) != len(embs):
            raise ValueError(f"{len(groups)} groups for {len(embs)} images")
        index = EmbeddingIndex(embs.shape[1], len(embs) if capacity is None else int(capacity),
                               self.vision.session.devices[0], dtype)
        index.add(embs)
        if groups is not None:
            index.set_groups(np.arange(len(embs)), groups)
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

    def search_deep(self, index, texts: Sequence[str], k: int, allow=None) -> List[List[Tuple[int, float]]]:
        """``search`` for a long result list, 1 <= k <= 4096 (a page that scrolls, a candidate pool): what
        ``search(index, texts, k, allow)`` would return if it took such a k, exactly
        (``EmbeddingIndex.search_deep``)."""
        scale, bias = self._scale_bias()
        idx, score = index.search_deep(self.text.embed_texts(texts), k, float(scale), float(bias), allow=allow)
        return [[(int(i), float(s)) for i, s in zip(ri, rs) if i >= 0] for ri, rs in zip(idx, score)]

    def search_grouped(self, index, texts: Sequence[str], k: int, allow=None) -> List[List[Tuple[int, float, int]]]:
        """``search`` with distinct results per group: per text the k best GROUPS of ``index`` (the labels of
        ``build_index(groups=)`` or ``EmbeddingIndex.set_groups``), each by its best row, as (gallery index,
        logit, group label), best first; the label is -1 for a row without one, which is a group of its own
        (``EmbeddingIndex.search_grouped``)."""
        scale, bias = self._scale_bias()
        idx, score, group = index.search_grouped(self.text.embed_texts(texts), k, float(scale), float(bias), allow=allow,
                                                 return_groups=True)
        return [[(int(i), float(s), int(g)) for i, s, g in zip(ri, rs, rg) if i >= 0]
                for ri, rs, rg in zip(idx, score, group)]

    def search_diverse(self, index, texts: Sequence[str], k: int, diversity: float = 0.5, pool=None, allow=None
                       ) -> List[List[Tuple[int, float]]]:
        """``search`` with variety: per text, k of its ``pool`` best rows (None: min(128, max(32, 4 k))) picked one
        by one by maximal marginal relevance -- each the candidate with the best (1 - diversity) * logit -
        diversity * (its largest similarity, in logit units, to a row already picked) -- as (gallery index, the
        row's own logit) in the order picked (``EmbeddingIndex.search_diverse``)."""
        scale, bias = self._scale_bias()
        idx, score = index.search_diverse(self.text.embed_texts(texts), k, diversity, pool, float(scale), float(bias),
                                          allow=allow)
        return [[(int(i), float(s)) for i, s in zip(ri, rs) if i >= 0] for ri, rs in zip(idx, score)]

    def similar(self, index, ids, k: int, allow=None) -> List[List[Tuple[int, float]]]:
        """More like this: per image ``ids[r]`` of ``index`` its k closest other images as (gallery index,
        cosine), best first (``EmbeddingIndex.neighbors`` at scale 1, bias 0)."""
        idx, score = index.neighbors(ids, k, allow=allow)
        return [[(int(i), float(s)) for i, s in zip(ri, rs) if i >= 0] for ri, rs in zip(idx, score)]

    def knn_graph(self, index, k: int, allow=None) -> Tuple[np.ndarray, np.ndarray]:
        """The k-NN graph of ``index``: (indices int64 [len(index), k], cosines f32), each row's k closest other
        rows, (-1, -inf) where there are none (``EmbeddingIndex.knn_graph`` at scale 1, bias 0)."""
        return index.knn_graph(k, allow=allow)

    def _search_groups(self, index, groups, k: int, op: str, allow) -> List[List[Tuple[int, float]]]:
        groups = [list(g) for g in groups]
        lims = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int64)
        scale, bias = self._scale_bias()
        flat = [t for g in groups for t in g]
        if not flat:
            raise ValueError("Empty batch: no texts")
        idx, score = index.search_compound(self.text.embed_texts(flat), lims, k, op, float(scale), float(bias),
                                           allow=allow)
        return [[(int(i), float(s)) for i, s in zip(ri, rs) if i >= 0] for ri, rs in zip(idx, score)]

    def search_all(self, index, groups: Sequence[Sequence[str]], k: int, allow=None) -> List[List[Tuple[int, float]]]:
        """``search`` for conjunctions: per group of 1 to 16 texts (``["a dog", "a beach"]``) the k best rows by
        the SMALLEST of the group's logits -- rows that match every text -- as (gallery index, that logit), best
        first.  All texts are embedded in one batch and the gallery is scanned once
        (``EmbeddingIndex.search_compound`` with "min")."""
        return self._search_groups(index, groups, k, "min", allow)

    def search_any(self, index, groups: Sequence[Sequence[str]], k: int, allow=None) -> List[List[Tuple[int, float]]]:
        """``search`` for prompt ensembles and synonyms: per group of 1 to 16 texts the k best rows by the
        LARGEST of the group's logits, as (gallery index, that logit), best first
        (``EmbeddingIndex.search_compound`` with "max")."""
        return self._search_groups(index, groups, k, "max", allow)

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

    def group_duplicates(self, index, min_cosine: float, allow=None, apply: bool = False) -> List[List[int]]:
        """Near-duplicates in a gallery as groups: the rows connected by the pairs of ``find_duplicates(index,
        min_cosine, allow)``, without the pair list.  Returns the groups of two or more rows, each ascending,
        ordered by their first row.  ``apply=True`` also makes the groups the index's group labels (every other row
        ungrouped), after which ``search_grouped`` returns one image per duplicate group
        (``EmbeddingIndex.duplicate_groups``)."""
        labels, _ = index.duplicate_groups(min_cosine, 1.0, 0.0, allow=allow, set_groups=apply)
        ids = np.flatnonzero(labels >= 0)
        ids = ids[np.argsort(labels[ids], kind="stable")]  # by label, the smallest row of the group, then by row
        groups = np.split(ids, np.flatnonzero(np.diff(labels[ids])) + 1) if ids.size else []
        return [[int(i) for i in g] for g in groups if len(g) >= 2]

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

    def classify_index(self, index, labels, k: int = 5, allow=None) -> List[List[Tuple[int, float]]]:
        """classify (src/clip.rs:92-132) for every image ``index`` stores: per row [(label index, probability)],
        best first, cut to its k best (k <= 16), with the model's activation (softmax over ALL labels, or
        sigmoid), logit_scale and logit_bias, as ``classify_topk`` takes them.  ``labels`` is a label index
        (``build_label_index``; its rows are used as stored, so an f32 one gives ``classify_topk``'s labels) or
        an array [C, E].  A row that is dead or not allowed by ``allow`` gives an empty list
        (``EmbeddingIndex.classify``)."""
        scale, bias = self._scale_bias()
        rows = labels.rows() if hasattr(labels, "rows") else labels
        idx, _, prob = index.classify(rows, k, float(scale), float(bias), self._activation(), allow=allow)
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
