"""Frame ordering of a video store by hierarchical-index similarity (core/video_storage.py).

The reference's VideoModelStorage orders the frames of a video so that neighbours compress well:
`_sort_frames_by_hierarchical_indices` (:1203-1277, start nearest the centroid, then greedily the most similar
remaining frame), `get_frame_ordering_metrics` (:1445-1522) and `_find_optimal_insertion_position` (:1751-1803),
all through one `np.corrcoef` per pair (`_calculate_hierarchical_similarity`, :762-781).  `FrameOrdering` keeps the
prepared index rows of one video on the device and answers all three from libhq_mi355x (csrc/hq_order.hip): one
float64 MFMA contraction for the pair similarities, one resident workgroup for the chain.

Contract: rows are finite float64 of one length 1 <= L <= 256; a row with a NaN or inf is refused.  Rows whose
np.std is non-zero but below 1e-12 |mean| are outside the contract (the reference's value there is rounding noise).
The greedy order takes at most 16384 frames (the N x N matrix; the reference's videos roll over at 10,000).
"""
from __future__ import annotations

from typing import Dict, List, Sequence

import numpy as np

from .. import _lib
from .. import kernels as K
from .._dev import to_dev, to_np, torch

METRIC_KEYS = ("average_neighbor_similarity", "similarity_variance", "temporal_coherence", "ordering_efficiency")


def _rows(x) -> "np.ndarray":
    a = np.asarray(x, dtype=np.float64)
    return a[None] if a.ndim == 1 else a


class FrameOrdering:
    """The index rows [N, L] of one video, prepared once and resident on the device."""

    def __init__(self, index_rows):
        x = index_rows if torch().is_tensor(index_rows) else _rows(index_rows)
        if x.ndim != 2 or x.shape[0] < 1:
            raise ValueError("FrameOrdering needs index rows [N, L] with N >= 1")
        self.rows = self._prepare(x)

    @staticmethod
    def _prepare(x) -> K.OrderRows:
        r = K.order_prepare(to_dev(x))
        bad = np.flatnonzero(to_np(r.flags[:r.N]) & 4)
        if len(bad):
            raise _lib.NativeLibraryError(f"index row {int(bad[0])} holds a NaN or inf (frame ordering needs finite rows)")
        return r

    def __len__(self) -> int:
        return self.rows.N

    def greedy_order(self):
        """(order [N] int64, step_sims [N - 1] float64) on the device: the reference's sorted frame order as
        positions in the stored order, and the similarity of every appended frame to its predecessor."""
        return K.order_greedy(self.rows)

    def metrics(self, order=None) -> Dict[str, float]:
        """The reference's four-key dict for the rows taken in `order` (None = stored order)."""
        if order is not None:
            o = np.asarray(to_np(order), dtype=np.int64)
            if o.shape != (len(self),) or not np.array_equal(np.sort(o), np.arange(len(self))):
                raise ValueError(f"order must be a permutation of the {len(self)} frames")
            order = to_dev(o)
        _, stats = K.order_pairs(self.rows, order)
        return {k: float(v) for k, v in zip(METRIC_KEYS, to_np(stats))}

    def similarities(self, queries):
        """Similarity of every query row against every stored row -> float64 [Q, N] on the device."""
        return K.order_sims(self._prepare(queries if torch().is_tensor(queries) else _rows(queries)), self.rows)

    def insertion_positions(self, queries):
        """(pos [Q] int64, score [Q] float64) on the device: where each query frame goes in the stored order."""
        return K.order_insert(self.similarities(queries))


def _index_rows(frames: Sequence) -> "np.ndarray":
    lens = {len(f.hierarchical_indices) for f in frames}
    if len(lens) != 1 or 0 in lens:
        raise ValueError(f"frames carry index vectors of different lengths {sorted(lens)}")
    return np.stack([np.asarray(f.hierarchical_indices, dtype=np.float64) for f in frames])


def sort_frames_by_hierarchical_indices(frames: Sequence) -> List:
    """`_sort_frames_by_hierarchical_indices` (:1203-1277): a new list in greedy order; `frame_index` of every
    frame is rewritten to its new position, as the reference does (not for a list of one frame or none).
    The start frame is the one nearest the centroid with the sums taken in the kernel's order, not np.mean's and
    np.linalg.norm's: where two distances agree to a few ulps the start can differ from the reference.  That is
    always so for a video of two frames (both are equidistant from their midpoint, and the reference's own choice
    is rounding noise), so a two-frame list may come back in either order."""
    frames = list(frames)
    if len(frames) <= 1:
        return frames
    order, _ = FrameOrdering(_index_rows(frames)).greedy_order()
    out = [frames[int(i)] for i in to_np(order)]
    for i, f in enumerate(out):
        f.frame_index = i
    return out


def frame_ordering_metrics(frames: Sequence) -> Dict[str, float]:
    """`get_frame_ordering_metrics` (:1445-1490) of the frames in their list order."""
    if len(frames) < 2:
        return {"temporal_coherence": 1.0, "average_neighbor_similarity": 1.0, "similarity_variance": 0.0,
                "ordering_efficiency": 1.0}
    return FrameOrdering(_index_rows(frames)).metrics()


def find_optimal_insertion_position(hierarchical_indices, frames: Sequence) -> int:
    """`_find_optimal_insertion_position` (:1751-1803) of a new frame's index vector among `frames`."""
    if not frames:
        return 0
    pos, _ = FrameOrdering(_index_rows(frames)).insertion_positions(_rows(hierarchical_indices))
    return int(to_np(pos)[0])
