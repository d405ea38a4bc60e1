"""RAG scoring functions, reference rag/search/engine.py:134-162, 243-287,
604-714, 1025-1138.

Every score runs on the GPU (hq_cosine_scores / hq_cosine_scores_dt / hq_cos_scores_mfma, hq_cos_topk for
rankings of large float32 problems, hq_cosq_topk / hq_cosqf_topk for u8 / float32 queries against the u8 frame
store, hq_spatial_locality, hq_detect_heights, hq_threshold_select); the level weights and the progressive
thresholds are host-side constants computed with the reference's own Python float expressions.  Inputs
keep their dtype: float64 arrays are scored in float64 (the reference's np.dot / np.linalg.norm run in
the input dtype), float32 ones from float32 values."""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

from .. import _lib
from .. import kernels as K
from .._dev import dtype_code, ptr, stream, to_dev, to_np, torch


def _score_dtype(*arrays) -> np.dtype:
    """NumPy's result dtype of np.dot / np.linalg.norm on these arrays: float32 only if all are float32."""
    return np.dtype(np.float32) if all(np.asarray(a).dtype == np.float32 for a in arrays) else np.dtype(np.float64)


def cosine_scores_batch(a, b):
    """(cos + 1) / 2 of every row of a [Q, K] against every row of b [N, K] -> device f64 [Q, N]
    (float32 rows: the split-f16 MFMA kernel for large problems; float64 rows in float64)."""
    t = torch()
    a2, b2 = to_dev(a), to_dev(b)
    if a2.dtype == t.float64 or b2.dtype == t.float64:
        return K.cosine_scores_dt(a2.to(t.float64), b2.to(t.float64))
    return K.cosine_scores(a2, b2)


def _threshold_mode(threshold):
    """threshold=None keeps every frame; a number keeps the frames scoring >= it."""
    return (0.0, 0) if threshold is None else (float(threshold), 1)


def cosine_topk_batch(a, b, k: int, threshold=None):
    """The k best rows of b [N, K] for every row of a [Q, K] by (score desc, row asc) -> device (scores [Q, k]
    f64, ids [Q, k] i64; -inf / -1 where fewer pass): the ranking select_topk gives on cosine_scores_batch(a, b).
    Large float32 problems never form the [Q, N] matrix (hq_cos_topk); float64 rows and small problems do."""
    t = torch()
    a2, b2 = to_dev(a), to_dev(b)
    thr, mode = _threshold_mode(threshold)
    if a2.dtype == t.float32 and b2.dtype == t.float32:
        ar, br = a2.reshape(a2.shape[0], -1), b2.reshape(b2.shape[0], -1)
        m = min(int(ar.shape[1]), int(br.shape[1]))  # the reference truncates to the common length
        if m > 0 and int(ar.shape[0]) * int(br.shape[0]) * m >= K.MFMA_COS_MIN_WORK:
            return K.cosine_topk(K.cos_prepare(ar[:, :m]), K.cos_prepare(br[:, :m]), int(k), thr, mode)
    s, ids, _, _ = K.select_topk(cosine_scores_batch(a2, b2), int(k), thr, mode)
    return s, ids


class FrameCosineCorpus:
    """Float32 frames [N, ...] prepared once for the matrix-core cosine and kept resident (split-f16 operand
    fragments + inverse norms); search() returns the nearest k frames of every query in one call, with
    memory O(Q k N / 384) instead of the [Q, N] score matrix."""

    def __init__(self, frames):
        x = to_dev(frames)
        if x.dim() < 2:
            raise ValueError("frames must be [N, ...]")
        self.shape = tuple(int(d) for d in x.shape[1:])
        self._rows = K.cos_prepare(x.reshape(x.shape[0], -1))

    @property
    def N(self) -> int:
        return self._rows.N

    @property
    def K(self) -> int:
        return self._rows.K

    def __len__(self) -> int:
        return self._rows.N

    def search(self, queries, k: int = 10, threshold=None):
        """queries [Q, ...] (or one frame) -> device (scores [Q, k] f64, ids [Q, k] i64), (score desc, frame
        asc), -inf / -1 where fewer than k frames pass `threshold` (None: no test; else score >= threshold)."""
        q = to_dev(queries)
        q2 = q.reshape(1, -1) if q.dim() <= len(self.shape) else q.reshape(q.shape[0], -1)
        thr, mode = _threshold_mode(threshold)
        return K.cosine_topk(K.cos_prepare(q2), self._rows, int(k), thr, mode)


class QuantizedFrameCorpus:
    """The store's own u8 frames [N, r, c] with their (min, max) pairs [N, 2], prepared once for the exact
    integer cosine (hq_cosq_prepare) and searched without decoding: only the signed bytes (1 B per value, in
    int8 MFMA operand fragments) and four float64 statistics per frame stay resident.

    The score of a (query, frame) pair is (cos + 1) / 2 of the two dequantised frames, x = mn + (mx - mn) u / 255,
    within a few float64 roundings of the exact value (the contraction is an exact int32 sum); a frame whose
    (mn, mx) is not finite scores 0.0.  `rows` is how many leading rows of every frame are compared: by default
    c when r == c + 1 (the pipeline's frames, index row left out), else r.  rows * c <= 65536.

    Two kinds of query meet the same resident corpus.  u8 frames with their own (min, max): search() takes them
    as they are, search_parameters() quantises float32 parameters with map_index_quantize at the corpus's n first.
    Float32 frames at full precision: search_float() (hq_cosqf_*: the query as three int8 digit planes of its
    24-bit fixed-point row, the same exact integer contraction), search_parameters(quantize_query=False) for
    float32 parameters; those scores are cosines of the query itself to 2^-23 sqrt(K) amax / |q| (below 7e-7 for
    gaussian rows), not of its 8-bit quantisation.  Queries of any other dtype (float64, float16) are out of scope:
    convert them to float32 first."""

    def __init__(self, frames_u8, minmax, rows=None):
        t = torch()
        x = to_dev(frames_u8)
        if x.dim() != 3 or x.dtype != t.uint8:
            raise ValueError("frames_u8 must be uint8 [N, r, c]")
        r, c = int(x.shape[1]), int(x.shape[2])
        if rows is None:
            rows = c if r == c + 1 else r
        self.rows = int(rows)
        self.shape = (r, c)
        self._rows = K.cosq_prepare(x, to_dev(minmax), self.rows)

    @classmethod
    def from_parameters(cls, x, n: int):
        """Float32 parameters [N, d] -> the pipeline's (n + 1) x n u8 frames (map_index_quantize) -> corpus."""
        frames, _, mm = K.map_index_quantize(to_dev(x), int(n), want_idx=False)
        return cls(frames, mm)

    @property
    def N(self) -> int:
        return self._rows.N

    @property
    def K(self) -> int:
        return self._rows.K

    def __len__(self) -> int:
        return self._rows.N

    @property
    def resident_bytes(self) -> int:
        return self._rows.nbytes

    def search(self, query_frames_u8, query_minmax, k: int = 10, threshold=None):
        """u8 query frames [Q, r, c] (or one [r, c]; r >= the corpus's rows, same c) with minmax [Q, 2] -> device
        (scores [Q, k] f64, ids [Q, k] i64), (score desc, frame asc), -inf / -1 where fewer than k frames pass
        `threshold` (None: no test; else score >= threshold)."""
        q = to_dev(query_frames_u8)
        if q.dim() == 2:
            q = q.unsqueeze(0)
        if q.dim() != 3 or int(q.shape[2]) != self.shape[1] or int(q.shape[1]) < self.rows:
            raise ValueError(f"query frames {tuple(q.shape)} do not hold {self.rows} rows of {self.shape[1]}")
        thr, mode = _threshold_mode(threshold)
        return K.cosq_topk(K.cosq_prepare(q, to_dev(query_minmax), self.rows), self._rows, int(k), thr, mode)

    def search_float(self, query_frames_f32, k: int = 10, threshold=None):
        """float32 query frames [Q, r, c] (or one [r, c]; r >= the corpus's rows, same c), or rows [Q, K] with K =
        the corpus's K, kept at full precision -> device (scores [Q, k] f64, ids [Q, k] i64) as search() orders and
        pads them.  A zero row and a row holding a NaN or inf score 0.0 against every frame."""
        t = torch()
        q = to_dev(query_frames_f32)
        if q.dtype != t.float32:
            raise TypeError("search_float expects float32 queries (u8 query frames go through search())")
        thr, mode = _threshold_mode(threshold)
        if q.dim() == 2 and int(q.shape[1]) == self.K and int(q.shape[1]) != self.shape[1]:
            return K.cosqf_topk(K.cosqf_prepare(q), self._rows, int(k), thr, mode)
        if q.dim() == 2:
            q = q.unsqueeze(0)
        if q.dim() != 3 or int(q.shape[2]) != self.shape[1] or int(q.shape[1]) < self.rows:
            raise ValueError(f"query frames {tuple(q.shape)} do not hold {self.rows} rows of {self.shape[1]}")
        return K.cosqf_topk(K.cosqf_prepare(q, self.rows), self._rows, int(k), thr, mode)

    def search_parameters(self, x, k: int = 10, threshold=None, quantize_query: bool = True):
        """Float32 parameters [Q, d]: quantised like the store (map_index_quantize at n = c), then search().
        quantize_query=False keeps the query's precision: the parameters are laid onto n x n along the curve
        (map_to_2d, zero padded as the pipeline pads) and go through search_float()."""
        if not quantize_query:
            t = torch()
            n = self.shape[1]
            p = to_dev(x)
            if p.dtype != t.float32:
                raise TypeError("search_parameters(quantize_query=False) expects float32 parameters")
            p2 = p.reshape(1, -1) if p.dim() == 1 else p
            return self.search_float(K.map_to_2d(p2[:, :n * n], n), k, threshold)
        frames, _, mm = K.map_index_quantize(to_dev(x), self.shape[1], want_idx=False)
        return self.search(frames, mm, k, threshold)


def calculate_embedding_cosine_similarity(embedding1, embedding2) -> float:
    """engine.py:622-660: flatten, truncate to the common length, (cos + 1) / 2, 0 for a zero norm."""
    e1, e2 = np.asarray(embedding1), np.asarray(embedding2)
    if e1.size == 0 or e2.size == 0:
        return 0.0
    m = min(e1.size, e2.size)
    dt = _score_dtype(e1, e2)
    f1 = e1.reshape(-1)[:m].astype(dt, copy=False).reshape(1, -1)
    f2 = e2.reshape(-1)[:m].astype(dt, copy=False).reshape(1, -1)
    return float(to_np(K.cosine_scores_dt(to_dev(f1), to_dev(f2)))[0, 0])


def compare_single_level_indices(query_indices, candidate_indices) -> float:
    """engine.py:1025-1051 (cosine of two 1-D index rows of equal length)."""
    if len(query_indices) == 0 or len(candidate_indices) == 0:
        return 0.0
    return calculate_embedding_cosine_similarity(query_indices, candidate_indices)


def calculate_granularity_weights(num_levels: int) -> np.ndarray:
    """engine.py:1101-1138: 8^(L-i-1), normalised, the first doubled, re-normalised."""
    if num_levels <= 0:
        return np.array([])
    if num_levels == 1:
        return np.array([1.0])
    w = np.array([8.0 ** (num_levels - i - 1) for i in range(num_levels)])
    w = w / np.sum(w)
    w[0] = w[0] * 2.0
    return w / np.sum(w)


def compare_multi_level_indices(query_indices, candidate_indices) -> float:
    """engine.py:1053-1099: weighted mean of the per-level cosines (one launch scores every level pair)."""
    q = np.asarray(query_indices)
    c = np.asarray(candidate_indices)
    levels = q.shape[0]
    if levels == 0:
        return 0.0
    w = calculate_granularity_weights(levels)
    if q.shape[1] == 0 or c.shape[1] == 0:
        return 0.0
    dt = _score_dtype(q, c)
    s = np.diag(to_np(K.cosine_scores_dt(to_dev(q.astype(dt, copy=False)), to_dev(c[:levels].astype(dt, copy=False)))))
    tot, tw = 0.0, 0.0
    for l in range(levels):
        tot += float(s[l]) * w[l]
        tw += w[l]
    return tot / tw if tw else 0.0


def detect_original_embedding_heights(images) -> np.ndarray:
    """engine.py:134-162 for a batch [N, H, W] (or one [H, W] image) -> int heights [N] (hq_detect_heights)."""
    t = torch()
    x = to_dev(images)
    if x.dtype not in (t.float32, t.float64):
        x = x.to(t.float64)
    x3 = (x.unsqueeze(0) if x.dim() == 2 else x).contiguous()
    N, H, W = x3.shape
    out = t.empty(N, dtype=t.int32, device=x3.device)
    _lib.check(_lib.lib().hq_detect_heights(dtype_code(x3.dtype), ptr(x3), N, H, W, ptr(out), stream()))
    return to_np(out).astype(np.int64)


def detect_original_embedding_height(enhanced_embedding) -> int:
    return int(detect_original_embedding_heights(enhanced_embedding)[0])


def extract_original_embedding(enhanced_embedding) -> np.ndarray:
    """engine.py:604-620: a 1-D input as is, else the rows above the detected index rows."""
    e = np.asarray(enhanced_embedding)
    if e.ndim == 1:
        return e
    return e[:detect_original_embedding_height(e), :]


def spatial_locality_scores(queries, images):
    """_calculate_spatial_locality_similarity of every query image [Q, H, W] against every stored
    enhanced image [N, H, W] -> device f64 [Q, N] (hq_spatial_locality: original heights detected on
    both, windowed cosine, NumPy-order mean)."""
    t = torch()
    q, c = to_dev(queries), to_dev(images)
    dt = t.float64 if (q.dtype == t.float64 or c.dtype == t.float64) else t.float32
    q3 = (q.unsqueeze(0) if q.dim() == 2 else q).to(dt).contiguous()
    c3 = (c.unsqueeze(0) if c.dim() == 2 else c).to(dt).contiguous()
    if q3.shape[1:] != c3.shape[1:]:
        raise ValueError(f"image shapes differ: {tuple(q3.shape[1:])} vs {tuple(c3.shape[1:])}")
    Q, H, W = q3.shape
    N = c3.shape[0]
    out = t.empty((Q, N), dtype=t.float64, device=q3.device)
    _lib.check(_lib.lib().hq_spatial_locality(dtype_code(dt), ptr(q3), Q, ptr(c3), N, H, W, ptr(out), stream()))
    return out


def calculate_spatial_locality_similarity(embedding1, embedding2) -> float:
    """engine.py:662-714 on two enhanced (index rows appended) Hilbert images."""
    a, b = np.asarray(embedding1), np.asarray(embedding2)
    if a.shape != b.shape or a.ndim != 2 or a.size == 0:
        return 0.0
    return float(to_np(spatial_locality_scores(a, b))[0, 0])


# ------------------------------------------------------------------ progressive threshold (:243-287)


def progressive_threshold(level: int, n_candidates: int) -> Tuple[float, int]:
    """The level's score threshold and candidate cap, with the reference's Python float arithmetic."""
    base_threshold = 0.3
    level_factor = 0.1
    threshold = base_threshold + (level_factor * (3 - min(level, 3)))
    threshold = min(threshold, 0.8)
    ratio = 0.3 if level == 0 else (0.5 if level == 1 else 0.7)
    return threshold, max(1, int(n_candidates * ratio))


def progressive_threshold_batch(scores, level: int, ids=None):
    """Device form of _apply_progressive_threshold for Q rows of scores [Q, N] in candidate order:
    -> (ids [Q, cap] (-1 padded), count [Q]) with the candidates passing the level's threshold, first
    `cap` in order (ids[q, i] or the position i)."""
    t = torch()
    s = to_dev(scores).to(t.float64)
    s2 = (s.view(1, -1) if s.dim() == 1 else s).contiguous()
    Q, N = s2.shape
    thr, cap = progressive_threshold(level, N)
    idt = None if ids is None else to_dev(ids).to(t.int64).view(Q, N).contiguous()
    out = t.empty((Q, cap), dtype=t.int64, device=s2.device)
    cnt = t.empty(Q, dtype=t.int64, device=s2.device)
    _lib.check(_lib.lib().hq_threshold_select(ptr(s2), ptr(idt), Q, N, float(thr), cap, ptr(out), ptr(cnt), stream()))
    return out, cnt


def apply_progressive_threshold(candidate_scores: Sequence[Tuple[int, float]], level: int) -> List[int]:
    """Drop-in for engine.py:243-287: [(candidate_index, score), ...] -> the passing candidate indices."""
    if not candidate_scores:
        return []
    ids = np.array([int(i) for i, _ in candidate_scores], dtype=np.int64)
    sc = np.array([float(s) for _, s in candidate_scores], dtype=np.float64)
    out, cnt = progressive_threshold_batch(sc[None], level, ids[None])
    n = int(to_np(cnt)[0])
    return [int(x) for x in to_np(out)[0][:n]]
