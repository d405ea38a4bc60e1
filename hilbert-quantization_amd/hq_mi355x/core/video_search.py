"""Level-0 scan over stored frames: the `hierarchical` mode of the
reference's VideoEnhancedSearchEngine (core/video_search.py:215-264, :1316-1328), which compares the
query's index with every stored frame's `hierarchical_indices` at level 0, keeps sim > threshold
(strict), and stable-sorts descending.  Frames are held as one device-resident IndexCorpus."""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

from .. import kernels as K
from .._dev import to_dev, to_np, torch
from .search_engine import IndexCorpus, _idx


class HierarchicalFrameSearch:
    def __init__(self, frame_indices, similarity_threshold: float = 0.1):
        self.corpus = IndexCorpus(frame_indices)
        self.similarity_threshold = similarity_threshold

    def search(self, query_indices, max_results: int) -> List[Tuple[int, float]]:
        # the query keeps its dtype: a float32 index is compared with float32 statistics, as in the reference
        ids, sc = self.corpus.frame_search(_idx(query_indices)[None], max_results, self.similarity_threshold)
        ids, sc = to_np(ids)[0], to_np(sc)[0]
        return [(int(i), float(s)) for i, s in zip(ids, sc) if i >= 0]

    def search_batch(self, queries, max_results: int):
        return self.corpus.frame_search(queries, max_results, self.similarity_threshold)


def _u8_frames(frames, what: str):
    """The dtype check comes before any device work: a float frame is refused, not rounded."""
    if not hasattr(frames, "dtype"):
        frames = np.asarray(frames)
    dt = frames.dtype
    if dt != np.uint8 and str(dt) != "torch.uint8":
        raise TypeError(f"{what} must be uint8 frames, got {dt}")
    return K.vfeat_extract(to_dev(frames))


class VideoFeatureIndex:
    """The `video_features` and `hybrid` modes of the reference's VideoEnhancedSearchEngine on resident frames:
    _build_feature_index (one feature row per frame, extracted once by hq_vfeat_extract and kept on the device),
    _video_feature_search_optimized (:1527: score > threshold, strict, stable descending) and
    _hybrid_search_optimized (:1576: the hierarchical candidates re-scored and blended).  The score is the
    histogram, texture and stats parts of _calculate_feature_similarity (:1499); the ORB part is not computed
    (DESIGN.md §7), `weights` = (histogram, texture, stats) rescales the rest.  Frames are uint8 [N, H, W] with
    sides >= 4 and at most 16768 pixels; queries may have another shape than the corpus."""

    def __init__(self, frames_u8, similarity_threshold: float = 0.1, weights=None):
        self._rows = _u8_frames(frames_u8, "frames_u8")
        self.similarity_threshold = similarity_threshold
        self.weights = weights

    def __len__(self) -> int:
        return len(self._rows)

    def features(self):
        """Device float64 [N, 55]: histogram [0, 32), texture [32, 48), stats [48, 55)."""
        return self._rows.features()

    def scores(self, queries_u8):
        """queries u8 [Q, H, W] (or one frame) -> device float64 [Q, N]."""
        return K.vfeat_scores(_u8_frames(queries_u8, "queries_u8"), self._rows, self.weights)

    def search(self, queries_u8, max_results: int):
        """`video_features`: -> device (ids [Q, max_results] i64, scores f64) of the frames with score >
        similarity_threshold by (score desc, frame asc), -1 / -inf where fewer pass."""
        s, ids, _, _ = K.select_topk(self.scores(queries_u8), int(max_results), self.similarity_threshold, 2)
        return ids, s

    def hybrid(self, queries_u8, ids, hier_scores, max_results: int):
        """`hybrid`: ids int64 [Q, C] (the hierarchical stage's candidates, e.g. HierarchicalFrameSearch.search_batch;
        < 0: a pad) with their scores [Q, C] -> device (ids, combined, video, hierarchical), each [Q, max_results], by
        (combined desc, list position asc), -1 / -inf padded."""
        t = torch()
        q = _u8_frames(queries_u8, "queries_u8")
        il = to_dev(ids).to(t.int64)
        hs = to_dev(hier_scores).to(t.float64)
        video, comb = K.vfeat_scores_listed(q, self._rows, il, hs, self.weights)
        # list_topk ranks list positions (-1 where the entry is a pad); the four outputs are gathered through them
        pos = t.arange(il.shape[1], device=il.device).expand_as(il).masked_fill((il < 0) | (il >= len(self)), -1)
        cs, cp, _ = K.list_topk(comb, pos, int(max_results))
        pad, at = cp < 0, cp.clamp(min=0)
        ninf = float("-inf")
        return (il.gather(1, at).masked_fill(pad, -1), cs, video.gather(1, at).masked_fill(pad, ninf),
                hs.gather(1, at).masked_fill(pad, ninf))


def extract_video_features(frame_u8) -> dict:
    """The reference's _extract_comprehensive_features for one gray uint8 frame, without its ORB entry:
    {'histogram': [32], 'texture': [16], 'stats': [7]} as float64 NumPy arrays (the reference's histogram is
    float32 with the same integer values)."""
    if getattr(frame_u8, "ndim", None) != 2:
        raise ValueError("extract_video_features takes one 2-D grayscale frame")
    f = to_np(_u8_frames(frame_u8, "frame_u8").features())[0]
    return {"histogram": f[:32].copy(), "texture": f[32:48].copy(), "stats": f[48:55].copy()}
