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
from .._dev import dtype_code, is_tensor, ptr, stream, to_dev, to_np, torch
from .._resident import ResidentRows


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


class QuantizedFrameCorpus(ResidentRows):
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
    convert them to float32 first.

    Mutable, as the stores it models are (add_document_chunk, insert_synchronized_frames, delete_model): `append`
    prepares new frames behind the resident ones (one hq_cosq_append launch, nothing resident moves, the buffers
    grow geometrically; `reserve` sizes them ahead), `replace` overwrites frames in place (hq_cosq_replace),
    `remove`, `insert` and `select` move prepared rows into a second pair of buffers (one hq_cosq_gather launch
    each; nothing is recomputed, so no raw copy of the store is needed).  After any of them the operand is byte
    for byte what a fresh corpus of the resulting frames holds, so results never depend on how a corpus was
    built.  Recovering the raw frames or their (min, max) from the operand is out of scope.

    Positions change on `remove` and `insert`.  A corpus built with `keys` (int64 [N], the caller's stable ids)
    keeps them in a device vector that follows every mutation, and a search with return_keys=True lists keys
    instead of positions (-1 stays -1).  The keys are not counted in resident_bytes.

    Writers (`reserve`, `append`, `append_parameters`, `replace`, `remove`, `insert`) follow IndexCorpus's rule:
    each runs on the calling thread's current stream and records an event that searches issued from another
    stream wait for on the device; the caller must not mutate while another thread's search of the same corpus
    is in flight, nor while a search queued on another stream may still be running.  Every argument is checked
    on the host before anything is launched: ValueError for a shape mismatch, repeated rows in `replace`,
    removing every row and a missing or unexpected `keys`, TypeError for a wrong dtype, IndexError for a row
    outside [0, N)."""

    def __init__(self, frames_u8, minmax, rows=None, keys=None):
        t = torch()
        x = to_dev(frames_u8)
        if x.dim() != 3 or x.dtype != t.uint8:
            raise ValueError("frames_u8 must be uint8 [N, r, c]")
        r, c = int(x.shape[1]), int(x.shape[2])
        if rows is None:
            rows = c if r == c + 1 else r
        self.rows = int(rows)
        self.shape = (r, c)
        host_keys = None if keys is None else self._host_keys(keys, int(x.shape[0]), "QuantizedFrameCorpus")
        self._rows = K.cosq_prepare(x, to_dev(minmax), self.rows)
        self._keys = None if host_keys is None else to_dev(host_keys)
        self._mark_ready()

    @classmethod
    def from_parameters(cls, x, n: int, keys=None):
        """Float32 parameters [N, d] -> the pipeline's (n + 1) x n u8 frames (map_index_quantize) -> corpus."""
        frames, _, mm = K.map_index_quantize(to_dev(x), int(n), want_idx=False)
        return cls(frames, mm, keys=keys)

    @classmethod
    def _of_rows(cls, prepared, shape, rows, keys):
        """A corpus around prepared rows (select; a host-side shell in the tests)."""
        c = object.__new__(cls)
        c._rows, c.shape, c.rows, c._keys = prepared, tuple(shape), int(rows), keys
        c._built_on = c._ready = None
        return c

    # ---- host-side checks (before any launch) ----------------------------------------------------------------
    @staticmethod
    def _host_keys(keys, M: int, what: str):
        a = to_np(keys) if is_tensor(keys) else np.asarray(keys)
        a = a.reshape(-1)
        if a.size and a.dtype.kind not in "iu":
            raise TypeError(f"{what}: keys must be integers")
        if a.size != M:
            raise ValueError(f"{what}: {a.size} keys for {M} frames")
        return np.ascontiguousarray(a.astype(np.int64))

    def _incoming_keys(self, keys, M: int, what: str):
        if self._keys is None:
            if keys is not None:
                raise ValueError(f"QuantizedFrameCorpus.{what}: keys= given, but the corpus has no keys")
            return None
        if keys is None:
            raise ValueError(f"QuantizedFrameCorpus.{what}: the corpus has keys, keys= is required")
        return self._host_keys(keys, M, f"QuantizedFrameCorpus.{what}")

    def _incoming(self, frames_u8, minmax, what: str):
        """Shape and dtype of the u8 frames [M, r, c] (or one [r, c]) and their minmax [M, 2] against the corpus's,
        looked at where they are (host or device): M."""
        if not is_tensor(frames_u8):
            frames_u8 = np.asarray(frames_u8)
        if not is_tensor(minmax):
            minmax = np.asarray(minmax)
        shape = tuple(int(d) for d in frames_u8.shape)
        if "uint8" not in str(frames_u8.dtype):
            raise TypeError(f"QuantizedFrameCorpus.{what} expects uint8 frames, not {frames_u8.dtype}")
        if len(shape) == 2:
            shape = (1,) + shape
        if len(shape) != 3 or shape[1:] != self.shape:
            raise ValueError(f"QuantizedFrameCorpus.{what}: frames {shape} are not [M, {self.shape[0]}, {self.shape[1]}]")
        if str(minmax.dtype).replace("torch.", "") not in ("float32", "float64"):
            raise TypeError(f"QuantizedFrameCorpus.{what} expects float32 (min, max) pairs, not {minmax.dtype}")
        if int(np.prod(minmax.shape)) != 2 * shape[0]:
            raise ValueError(f"QuantizedFrameCorpus.{what}: minmax {tuple(minmax.shape)} for {shape[0]} frames")
        return shape[0]

    def _frames3(self, frames_u8):
        x = to_dev(frames_u8)
        return x.unsqueeze(0) if x.dim() == 2 else x

    # ---- writers ---------------------------------------------------------------------------------------------
    @property
    def capacity(self) -> int:
        """Frames the resident buffers hold without another reallocation (a multiple of 128)."""
        return self._rows.cap

    def reserve(self, capacity: int) -> int:
        """Room for `capacity` frames without another reallocation (device-to-device copies of the resident rows
        when the buffers grow).  A writer.  Returns the capacity."""
        self._wait_ready()
        grown = K.cosq_reserve(self._rows, int(capacity))
        if grown is not self._rows:
            self._rows = grown
            self._mark_ready()
        return self._rows.cap

    def append(self, frames_u8, minmax, keys=None) -> int:
        """Add the u8 frames [M, r, c] (or one [r, c]; the corpus's frame shape) with minmax [M, 2] behind the
        resident ones: appended frame i gets position N + i.  keys: the new frames' keys, when the corpus has keys.
        A writer.  Returns the new N."""
        M = self._incoming(frames_u8, minmax, "append")
        new_keys = self._incoming_keys(keys, M, "append")
        self._wait_ready()
        if M == 0:
            return self.N
        self._rows = K.cosq_append(self._rows, self._frames3(frames_u8), to_dev(minmax), self.rows)
        if new_keys is not None:
            self._keys = torch().cat([self._keys, to_dev(new_keys)])
        self._mark_ready()
        return self.N

    def append_parameters(self, x, keys=None) -> int:
        """Float32 parameters [M, d]: quantised like the store (map_index_quantize at n = c), then append()."""
        p = np.asarray(x) if not is_tensor(x) else x
        new_keys = self._incoming_keys(keys, 1 if len(p.shape) == 1 else int(p.shape[0]), "append_parameters")
        frames, _, mm = K.map_index_quantize(to_dev(x), self.shape[1], want_idx=False)
        return self.append(frames, mm, new_keys)

    def replace(self, rows, frames_u8, minmax) -> int:
        """Overwrite the distinct positions `rows` with the u8 frames [len(rows), r, c] and their minmax in place;
        positions and keys do not change.  One hq_cosq_replace launch.  A writer.  Returns N."""
        sel = self._local_rows(rows, "replace")
        if np.unique(sel).size != sel.size:
            raise ValueError("QuantizedFrameCorpus.replace: repeated row numbers")
        M = self._incoming(frames_u8, minmax, "replace")
        if M != sel.size:
            raise ValueError(f"QuantizedFrameCorpus.replace: {sel.size} row numbers for {M} frames")
        self._wait_ready()
        if M == 0:
            return self.N
        K.cosq_replace(self._rows, sel, self._frames3(frames_u8), to_dev(minmax), self.rows, checked=True)
        self._mark_ready()
        return self.N

    def _regather(self, sel: np.ndarray):
        """The corpus becomes its rows `sel`: one gather into a second pair of buffers of the same capacity."""
        self._wait_ready()
        self._rows = K.cosq_gather(self._rows, sel, checked=True)
        if self._keys is not None:
            self._keys = self._keys[to_dev(sel)]
        self._mark_ready()
        return self.N

    def remove(self, rows) -> int:
        """Drop the positions `rows` (duplicates tolerated).  The survivors keep their order and are renumbered
        consecutively, exactly as a fresh corpus of the surviving frames would be: one hq_cosq_gather launch into
        a second pair of buffers of the same capacity.  A writer.  Returns the new N."""
        sel = self._survivors(self._local_rows(rows, "remove"))
        if sel.size == 0:
            raise ValueError("QuantizedFrameCorpus.remove: no frame would be left")
        if sel.size == self.N:
            return self.N
        return self._regather(sel)

    def insert(self, position: int, frames_u8, minmax, keys=None) -> int:
        """Put the u8 frames [M, r, c] (or one) at positions position .. position + M - 1 (0 <= position <= N); the
        frames behind move up by M.  An append and then one gather with the permutation: the primitive behind
        insert_synchronized_frames.  A writer.  Returns the new N."""
        M = self._incoming(frames_u8, minmax, "insert")
        new_keys = self._incoming_keys(keys, M, "insert")
        pos, N0 = int(position), self.N
        if not 0 <= pos <= N0:
            raise IndexError(f"QuantizedFrameCorpus.insert: position {pos} outside [0, {N0}]")
        self.append(frames_u8, minmax, new_keys)
        if M == 0 or pos == N0:
            return self.N
        return self._regather(np.concatenate([np.arange(pos), np.arange(N0, N0 + M), np.arange(pos, N0)]))

    def select(self, rows) -> "QuantizedFrameCorpus":
        """A new, independent corpus of the positions `rows`, in that order (repeats allowed; keys follow): one
        hq_cosq_gather launch, exactly a fresh corpus of those frames.  This corpus is only read."""
        sel = self._local_rows(rows, "select")
        self._wait_ready()
        prepared = K.cosq_gather(self._rows, sel, cap=max(1, sel.size), checked=True)
        c = self._of_rows(prepared, self.shape, self.rows, None if self._keys is None else self._keys[to_dev(sel)])
        c._mark_ready()
        return c

    def _listed(self, found, return_keys: bool):
        """A search's (scores, ids); with return_keys the ids go through the resident key vector (-1 stays -1)."""
        if not return_keys:
            return found
        if self._keys is None:
            raise ValueError("QuantizedFrameCorpus: return_keys=True, but the corpus has no keys")
        t = torch()
        s, ids = found
        return s, t.where(ids >= 0, self._keys[ids.clamp(min=0)], t.full_like(ids, -1))

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

    def search(self, query_frames_u8, query_minmax, k: int = 10, threshold=None, return_keys: bool = False):
        """u8 query frames [Q, r, c] (or one [r, c]; r >= the corpus's rows, same c) with minmax [Q, 2] -> device
        (scores [Q, k] f64, ids [Q, k] i64), (score desc, frame asc), -inf / -1 where fewer than k frames pass
        `threshold` (None: no test; else score >= threshold).  ids are positions; return_keys=True: the corpus's
        keys."""
        q = to_dev(query_frames_u8)
        if q.dim() == 2:
            q = q.unsqueeze(0)
        if q.dim() != 3 or int(q.shape[2]) != self.shape[1] or int(q.shape[1]) < self.rows:
            raise ValueError(f"query frames {tuple(q.shape)} do not hold {self.rows} rows of {self.shape[1]}")
        thr, mode = _threshold_mode(threshold)
        self._wait_ready()
        return self._listed(K.cosq_topk(K.cosq_prepare(q, to_dev(query_minmax), self.rows), self._rows, int(k), thr,
                                        mode), return_keys)

    def search_float(self, query_frames_f32, k: int = 10, threshold=None, return_keys: bool = False):
        """float32 query frames [Q, r, c] (or one [r, c]; r >= the corpus's rows, same c), or rows [Q, K] with K =
        the corpus's K, kept at full precision -> device (scores [Q, k] f64, ids [Q, k] i64) as search() orders and
        pads them.  A zero row and a row holding a NaN or inf score 0.0 against every frame."""
        t = torch()
        q = to_dev(query_frames_f32)
        if q.dtype != t.float32:
            raise TypeError("search_float expects float32 queries (u8 query frames go through search())")
        thr, mode = _threshold_mode(threshold)
        self._wait_ready()
        if q.dim() == 2 and int(q.shape[1]) == self.K and int(q.shape[1]) != self.shape[1]:
            return self._listed(K.cosqf_topk(K.cosqf_prepare(q), self._rows, int(k), thr, mode), return_keys)
        if q.dim() == 2:
            q = q.unsqueeze(0)
        if q.dim() != 3 or int(q.shape[2]) != self.shape[1] or int(q.shape[1]) < self.rows:
            raise ValueError(f"query frames {tuple(q.shape)} do not hold {self.rows} rows of {self.shape[1]}")
        return self._listed(K.cosqf_topk(K.cosqf_prepare(q, self.rows), self._rows, int(k), thr, mode), return_keys)

    def search_parameters(self, x, k: int = 10, threshold=None, quantize_query: bool = True,
                          return_keys: bool = False):
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
            return self.search_float(K.map_to_2d(p2[:, :n * n], n), k, threshold, return_keys)
        frames, _, mm = K.map_index_quantize(to_dev(x), self.shape[1], want_idx=False)
        return self.search(frames, mm, k, threshold, return_keys)


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


def progressive_level(level: int) -> Tuple[float, float]:
    """The level's score threshold and kept share, with the reference's Python float arithmetic."""
    base_threshold = 0.3
    level_factor = 0.1
    threshold = base_threshold + (level_factor * (3 - min(level, 3)))
    threshold = min(threshold, 0.8)
    ratio = 0.3 if level == 0 else (0.5 if level == 1 else 0.7)
    return threshold, ratio


def progressive_threshold(level: int, n_candidates: int) -> Tuple[float, int]:
    """The level's score threshold and candidate cap, with the reference's Python float arithmetic."""
    threshold, ratio = progressive_level(level)
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


# ------------------------------------------------------------------ comprehensive similarity (:478-727)

_WIDTH_ERROR = "Query and candidate indices must have the same shape"


def similarity_weights() -> dict:
    """engine.py:716-727."""
    return {"hierarchical": 0.5, "embedding": 0.3, "spatial": 0.2}


def _weight_table(max_levels: int) -> np.ndarray:
    """Row m = calculate_granularity_weights(m), zero padded: float64 [max_levels + 1, max_levels]."""
    tab = np.zeros((max_levels + 1, max(max_levels, 1)), dtype=np.float64)
    for m in range(1, max_levels + 1):
        tab[m, :m] = calculate_granularity_weights(m)
    return tab


def _level_coef(levels: int) -> np.ndarray:
    """sqrt(2 a_l), a_l = 0.5 (w_l / sum w) / 2, the sum taken left to right as _compare_multi_level_indices does."""
    w = calculate_granularity_weights(levels)
    tw = 0.0
    for l in range(levels):
        tw += w[l]
    return np.sqrt(0.5 * w / tw) if levels else np.zeros(0)


def _comp_frames(x, dtype=None):
    """Enhanced frames [N, H, W] (or one [H, W]) on the device, float32 or float64 (`dtype` when given)."""
    t = torch()
    f = to_dev(x)
    if f.dim() == 2:
        f = f.unsqueeze(0)
    if f.dim() != 3:
        raise ValueError("enhanced frames must be [N, H, W] or [H, W]")
    if dtype is not None:
        return f.to(dtype).contiguous()
    return (f if f.dtype in (t.float32, t.float64) else f.to(t.float64)).contiguous()


def _check_widths(dq: np.ndarray, dc: np.ndarray):
    """The reference pads each frame's index rows to its own largest trimmed length and raises when a pair with
    index rows on both sides differs in it (engine.py:1013-1014): checked on the host before the scoring launch."""
    wq = set(dq[dq[:, 1] >= 1, 2].tolist())
    wc = set(dc[dc[:, 1] >= 1, 2].tolist())
    if wq and wc and len(wq | wc) > 1:
        raise ValueError(_WIDTH_ERROR)


def _comp_exact(q3, dq_dev, dq, c3, dc_dev, dc, parts: bool = False):
    _check_widths(dq, dc)
    ml = int(max(dq[:, 1].max(initial=0), dc[:, 1].max(initial=0)))
    return K.comp_scores(q3, dq_dev, c3, dc_dev, _weight_table(ml), parts)


def _index_widths(desc: np.ndarray) -> frozenset:
    """The index widths of the frames that have index rows (host descriptors [N, 4])."""
    return frozenset(desc[desc[:, 1] >= 1, 2].tolist())


def _windows_host(head: np.ndarray, N: int, window: int) -> np.ndarray:
    """hq_list_windows' rule for one host list (the per-query route of lists beyond the kernel's 1024 entries)."""
    half, seen, out = window // 2, set(), []
    for f in head.tolist():
        start = max(0, f - half)
        for x in range(start, min(start + window, f + half + 1, N)):
            if x not in seen:
                seen.add(x)
                out.append(x)
    return np.array(out, dtype=np.int64)


def _comp_listed(q3, dq_dev, dq, c3, dc_dev, ml_c: int, widths_c: frozenset, ids, parts: bool = False):
    """The exact scores of the listed frames (hq_comp_scores_listed, the frames read in place), the weight table
    sized by the larger of the store's and the batch's level count (row M does not depend on the number of
    columns).  The width error of _check_widths, for the listed pairs only: when the queries and the whole store
    share one index width nothing can differ and nothing is read back; otherwise the listed frames' descriptors
    are gathered on the device and one flag is read."""
    wq = _index_widths(dq)
    if wq and widths_c and len(wq | widths_c) > 1:
        N = int(c3.shape[0])
        d = dc_dev[ids.clamp(0, N - 1)]
        qd = dq_dev.unsqueeze(1)
        differ = ((ids >= 0) & (ids < N) & (d[..., 1] >= 1) & (qd[..., 1] >= 1) & (d[..., 2] != qd[..., 2])).any()
        if bool(to_np(differ)):
            raise ValueError(_WIDTH_ERROR)
    ml = max(int(ml_c), int(dq[:, 1].max(initial=0)))
    return K.comp_scores_listed(q3, dq_dev, c3, dc_dev, ids, _weight_table(ml), parts)


def comprehensive_scores_listed(queries, frames, ids, parts: bool = False):
    """comprehensive_scores through an id list: ids int64 [Q, C] -> device f64 [Q, C], entry (a, j) bit for bit the
    dense score of (query a, frame ids[a, j]); an id < 0 or >= N is a pad (-inf, parts 0.0).  The stored frames are
    read in place, one scoring launch.  ValueError with the reference's message when a listed pair whose frames
    both have index rows differs in index width."""
    t = torch()
    q3, c3 = _comp_frames(queries), _comp_frames(frames)
    if q3.dtype != c3.dtype:
        q3, c3 = q3.to(t.float64), c3.to(t.float64)
    if q3.shape[1:] != c3.shape[1:]:
        raise ValueError(f"frame shapes differ: {tuple(q3.shape[1:])} vs {tuple(c3.shape[1:])}")
    dq_dev, dc_dev = K.comp_describe(q3), K.comp_describe(c3)
    dc = to_np(dc_dev)
    return _comp_listed(q3, dq_dev, to_np(dq_dev), c3, dc_dev, dc[:, 1].max(initial=0), _index_widths(dc),
                        to_dev(ids, t.int64), parts)


def comprehensive_scores(queries, frames, parts: bool = False):
    """_calculate_comprehensive_similarity (engine.py:516-575) of every query frame [Q, H, W] against every stored
    enhanced frame [N, H, W] -> device f64 [Q, N]; parts=True adds the components [Q, N, 3] (hierarchical,
    embedding, spatial).  The exact route (hq_comp_describe + hq_comp_scores): float64 frames in float64, float32
    frames from their float32 values.  ValueError with the reference's message when a pair whose frames both have
    index rows differs in index width."""
    t = torch()
    q3, c3 = _comp_frames(queries), _comp_frames(frames)
    if q3.dtype != c3.dtype:
        q3, c3 = q3.to(t.float64), c3.to(t.float64)
    if q3.shape[1:] != c3.shape[1:]:
        raise ValueError(f"frame shapes differ: {tuple(q3.shape[1:])} vs {tuple(c3.shape[1:])}")
    dq_dev, dc_dev = K.comp_describe(q3), K.comp_describe(c3)
    return _comp_exact(q3, dq_dev, to_np(dq_dev), c3, dc_dev, to_np(dc_dev), parts)


def calculate_comprehensive_similarity(query, query_indices, candidate_frame, frame_number=None) -> float:
    """Drop-in for engine.py:516-575 on two enhanced frames; query_indices and frame_number are accepted and
    ignored (the index rows are read from the query frame itself, as the reference's caller extracts them)."""
    a, b = np.asarray(query), np.asarray(candidate_frame)
    if a.ndim != 2 or a.shape != b.shape or a.size == 0:
        raise ValueError("calculate_comprehensive_similarity expects two enhanced frames of one shape [H, W]")
    return float(to_np(comprehensive_scores(a, b))[0, 0])


def calculate_embedding_similarity(query_embedding, cached_frames: dict) -> List[Tuple[int, float]]:
    """Drop-in for engine.py:478-514: [(frame_number, score), ...] over the cached frames, stable-sorted by score
    descending (ties keep the dict's order) — one batched launch instead of a Python loop per frame."""
    q = np.asarray(query_embedding)
    if q.size == 0 or not cached_frames:
        return []
    keys = list(cached_frames.keys())
    stack = np.stack([np.asarray(cached_frames[k]) for k in keys])
    sc = comprehensive_scores(q, stack)
    s, ids, _, _ = K.select_topk(sc, len(keys))  # (score desc, position asc) = the reference's stable sort
    s, ids = to_np(s)[0], to_np(ids)[0]
    return [(keys[int(i)], float(v)) for v, i in zip(s, ids)]


class ComprehensiveFrameCorpus:
    """Enhanced frames [N, H, W] kept resident for the RAG engine's comprehensive ranking
    (calculate_embedding_similarity, engine.py:478-575).

    The store is described once (hq_comp_describe).  A float32 store written by one generator — every frame the
    same detected height h < H, every index row non-zero, one index width — is `fused`: its frames become
    "composite" rows (hq_comp_prepare: level-normalised index rows, normalised original block and windows, validity
    indicators, one constant column) whose dot product with a query's composite row is an affine
    function of the comprehensive score, and only that operand stays resident (`K` halves x 2 per frame,
    `resident_bytes`; about 82 KB for a 67 x 64 frame against 17 KB raw — the price of a search that is one matrix
    core contraction with the top-k in its epilogue).  keep_frames=True keeps the raw frames as well, so that
    queries off the profile (another height, a dropped index row) can take the exact route; without them such a
    query raises ValueError.  Any other store keeps the frames and their descriptors and is searched by the exact
    route (hq_comp_scores + hq_select_topk).

    A profile is fused only while hq_comp_prepare can stage it: 16 frames x (L + 1 + n_windows) section coefficients
    in 160 KiB of LDS, i.e. at most 1280 - L - 1 windows (67 x 64 frames have 961; the generator's 131 x 128 frames
    have 3969 and are not fused).  Such a store takes the exact route, and where that cannot stage a frame either
    (hq_comp_scores: 5 max_windows + H W values in 160 KiB, which 131 x 128 exceeds) scores() and search() raise the
    library's HQ_E_UNSUPPORTED message; nothing is computed another way.

    Fused scores are within 1e-5 of the exact ones (profiles/comp_error_bounds.txt has the measured error) and
    the lists equal select_topk of the fused dense scores bit for bit.  Appending, replacing and removing frames
    are out of scope: build a new corpus."""

    def __init__(self, frames, keep_frames: bool = False):
        t = torch()
        x = _comp_frames(frames)
        self.N, self.H, self.W = (int(d) for d in x.shape)
        self.dtype = x.dtype
        self._desc_dev = K.comp_describe(x)
        self._desc = to_np(self._desc_dev)
        self.profile = None
        self._rows = None
        d = self._desc
        if self.N and x.dtype == t.float32:
            h, L, width = int(d[0, 0]), int(d[0, 1]), int(d[0, 2])
            if h < self.H and L == self.H - h and bool((d == d[0]).all()) and K.comp_prepare_fits(self.H, self.W, h):
                self.profile = (h, L, width)
                self._coef = _level_coef(L)
                self._rows = K.comp_prepare(x, h, 1, self._coef)
        self._frames = x if (self._rows is None or keep_frames) else None
        if self._frames is None:
            self._desc_dev = None

    @property
    def fused(self) -> bool:
        return self._rows is not None

    @property
    def K(self):
        """Composite row length (None for a store that is not fused)."""
        return self._rows.K if self._rows is not None else None

    def __len__(self) -> int:
        return self.N

    @property
    def resident_bytes(self) -> int:
        n = 0
        if self._rows is not None:
            n += self._rows.X16.numel() * 2 + self._rows.inv.numel() * 8
        if self._frames is not None:
            n += self._frames.numel() * self._frames.element_size() + self.N * 16
        return n

    def _route(self, queries):
        """(query frames, their descriptors on the device and the host, bool [Q]: on the fused profile)."""
        q3 = _comp_frames(queries)
        if tuple(q3.shape[1:]) != (self.H, self.W):
            raise ValueError(f"query frames {tuple(q3.shape[1:])} are not [{self.H}, {self.W}]")
        if q3.dtype != self.dtype:
            q3 = q3.to(self.dtype)
        dq_dev = K.comp_describe(q3)
        dq = to_np(dq_dev)
        on = np.zeros(len(dq), dtype=bool)
        if self.fused:
            h, L, width = self.profile
            on = (dq[:, 0] == h) & (dq[:, 1] == L) & (dq[:, 2] == width)
        if not on.all() and self._frames is None:
            raise ValueError("a query is off the fused profile and the corpus was built without keep_frames=True")
        return q3, dq_dev, dq, on

    def _split(self, queries, fused_fn, exact_fn, empty):
        """Each query through its own route, results back in query order."""
        t = torch()
        q3, dq_dev, dq, on = self._route(queries)
        if not len(on) or not self.N:  # nothing to score: the padded lists / the empty matrix, no launch
            return empty(len(on), q3.device)
        if on.all():
            return fused_fn(K.comp_prepare(q3, self.profile[0], 0, self._coef))
        if not on.any():
            return exact_fn(q3, dq_dev, dq)
        out = empty(len(on), q3.device)
        i_on = t.as_tensor(np.flatnonzero(on), device=q3.device)
        i_off = t.as_tensor(np.flatnonzero(~on), device=q3.device)
        got_on = fused_fn(K.comp_prepare(q3[i_on], self.profile[0], 0, self._coef))
        got_off = exact_fn(q3[i_off].contiguous(), dq_dev[i_off].contiguous(), dq[~on])
        for o, a, b in zip(out, got_on, got_off):
            o[i_on], o[i_off] = a, b
        return out

    def scores(self, queries):
        """The dense comprehensive scores [Q, N] (device f64): composite operands on the matrix cores for queries on
        a fused store's profile, hq_comp_scores for the others."""
        t = torch()
        return self._split(
            queries,
            lambda rows: (K.cosine_scores_mfma(rows, self._rows),),
            lambda q3, dq_dev, dq: (_comp_exact(q3, dq_dev, dq, self._frames, self._desc_dev, self._desc),),
            lambda Q, dev: (t.empty((Q, self.N), dtype=t.float64, device=dev),))[0]

    def search(self, queries, k: int = 10, threshold=None):
        """queries [Q, H, W] (or one frame) -> device (scores [Q, k] f64, ids [Q, k] i64), (score desc, frame asc),
        -inf / -1 where fewer than k frames pass `threshold` (None: no test; else score >= threshold).  Queries on
        the profile of a fused store: hq_comp_prepare + hq_cos_topk (k > 64: the dense fused scores and
        hq_select_topk); the others: hq_comp_scores + hq_select_topk."""
        t = torch()
        k = int(k)
        if k < 1:
            raise ValueError(f"k = {k}")
        thr, mode = _threshold_mode(threshold)

        def exact(q3, dq_dev, dq):
            s, ids, _, _ = K.select_topk(_comp_exact(q3, dq_dev, dq, self._frames, self._desc_dev, self._desc), k, thr,
                                         mode)
            return s, ids

        return self._split(
            queries, lambda rows: K.cosine_topk(rows, self._rows, k, thr, mode), exact,
            lambda Q, dev: (t.full((Q, k), float("-inf"), dtype=t.float64, device=dev),
                            t.full((Q, k), -1, dtype=t.int64, device=dev)))

    def rescore(self, queries, ids):
        """The exact scores of the listed frames: ids int64 [Q, C] (the list of a fused search, say) -> device f64
        [Q, C], bit for bit comprehensive_scores' values for those pairs, -inf where the id is < 0 or >= N
        (hq_comp_scores_listed: one launch, the frames read in place).  Needs the raw frames: a store that is not
        fused, or keep_frames=True."""
        t = torch()
        if self._frames is None:
            raise ValueError("rescore needs the raw frames and the corpus was built without keep_frames=True")
        q3 = _comp_frames(queries)
        if tuple(q3.shape[1:]) != (self.H, self.W):
            raise ValueError(f"query frames {tuple(q3.shape[1:])} are not [{self.H}, {self.W}]")
        if q3.dtype != self.dtype:
            q3 = q3.to(self.dtype)
        dq_dev = K.comp_describe(q3)
        return _comp_listed(q3, dq_dev, to_np(dq_dev), self._frames, self._desc_dev, self._desc[:, 1].max(initial=0),
                            _index_widths(self._desc), to_dev(ids, t.int64))


# ------------------------------------------------------------------ progressive hierarchical search (:51-95)


class HierarchicalFrameCorpus:
    """Enhanced frames [N, H, W] (float32 or float64) prepared once for the engine's progressive hierarchical
    search (progressive_hierarchical_search, engine.py:51-95, 178-287): the candidate cascade that runs before the
    comprehensive score.  The store is described (hq_comp_describe) and its index rows are packed (hq_hier_prepare:
    compacted, trimmed, float64) and kept resident, max_levels x W x 8 bytes per frame plus the lengths
    (`resident_bytes`); keep_frames=True (the default) keeps the raw frames too, which search() needs for the
    comprehensive re-rank: search() is the engine's whole workflow (cascade, neighbour windows, exact scores of the
    list, threshold and cut) for a query batch, on the device.

    The cascade: level l orders the survivors by (s_l desc, s_{l-1} desc, ..., s_0 desc, id asc) and
    keeps the first max(1, int(n_prev ratio_l)) of those with s_l >= thr_l (progressive_threshold's tables).  It runs
    on the device for a whole query batch, no host round trip between levels (hq_hier_filter).  A store with a frame
    of more than 8 levels is refused with the library's message.  Appending and removing frames, u8 stores and
    sharding are out of scope: build a new corpus."""

    def __init__(self, frames, keep_frames: bool = True):
        x = _comp_frames(frames)
        self.N, self.H, self.W = (int(d) for d in x.shape)
        self.dtype = x.dtype
        desc_dev = K.comp_describe(x)
        self._rows = K.hier_prepare(x, desc_dev)
        self.max_levels = self._rows.max_levels
        lv = [progressive_level(l) for l in range(self.max_levels)]
        self._thr = np.array([v[0] for v in lv], dtype=np.float64)
        self._ratio = np.array([v[1] for v in lv], dtype=np.float64)
        self._frames = x if keep_frames else None
        self._desc_dev = desc_dev if keep_frames else None
        self._desc = to_np(desc_dev) if keep_frames else None
        if keep_frames:  # what the listed re-rank needs of the whole store: its level count and index widths
            self._ml = int(self._desc[:, 1].max(initial=0))
            self._widths = _index_widths(self._desc)

    def __len__(self) -> int:
        return self.N

    @property
    def resident_bytes(self) -> int:
        n = self._rows.nbytes
        if self._frames is not None:
            n += self._frames.numel() * self._frames.element_size() + self.N * 16
        return n

    def _queries(self, queries):
        """(query frames [Q, H, W], their descriptors on the device, their packed rows at the corpus's max_levels)."""
        q3 = _comp_frames(queries)
        if tuple(q3.shape[1:]) != (self.H, self.W):
            raise ValueError(f"query frames {tuple(q3.shape[1:])} are not [{self.H}, {self.W}]")
        dq_dev = K.comp_describe(q3)
        return q3, dq_dev, K.hier_prepare(q3, dq_dev, self.max_levels, clamp=True)

    def filter(self, queries, kout: int = 20, workspace_bytes: int = 1 << 30):
        """queries [Q, H, W] (or one frame) -> device (top_ids [Q, kout] i64, -1 padded: the first kout candidates of
        every query in the cascade's order; top_scores [Q, kout, max_levels] f64: their level scores; counts
        [Q, max_levels] i64: the survivors after each level, 0 for the levels a query does not have or never
        reached).  kout <= 64.  The level scores of a query block live in a workspace of max_levels * Qb * N * 8
        bytes; the batch is split so that it stays under workspace_bytes."""
        _, _, qr = self._queries(queries)
        counts, ids, sc, _ = K.hier_filter(qr, self._rows, self._thr, self._ratio, kout, False, workspace_bytes)
        return ids, sc, counts

    def _candidates(self, qr, a: int) -> np.ndarray:
        """The whole ordered candidate list of prepared query a (host int64): the alive mask and the level scores of
        the survivors from the device, then one lexsort over the survivors only."""
        t = torch()
        one = K.HierRows(qr.rows[a:a + 1], qr.lens[a:a + 1], qr.L[a:a + 1], qr.levels[a:a + 1], 1, qr.W, qr.max_levels)
        Lq = int(qr.levels[a])
        if Lq == 0 or Lq > self.max_levels or self.N == 0:
            return np.zeros(0, dtype=np.int64)
        _, _, _, alive, S = K.hier_filter(one, self._rows, self._thr, self._ratio, 0, True, want_scores=True)
        idx = t.nonzero(alive[0] == Lq).view(-1)
        ids, s = to_np(idx), to_np(S[:Lq, 0][:, idx])
        # np.lexsort: the last key is the primary one
        return ids[np.lexsort((ids,) + tuple(-s[l] for l in range(Lq)))].astype(np.int64)

    def candidates(self, query) -> List[int]:
        """One query frame [H, W] -> the reference's progressive_hierarchical_search list (every survivor, in order)."""
        _, _, qr = self._queries(query)
        if qr.N != 1:
            raise ValueError("candidates() takes one query frame [H, W]")
        return [int(i) for i in self._candidates(qr, 0)]

    def _search_inputs(self, queries, k):
        """(k, query frames in the store's dtype, their descriptors on the device and the host, their packed rows)."""
        k = int(k)
        if k < 1:
            raise ValueError(f"k = {k}")
        if self._frames is None:
            raise ValueError("HierarchicalFrameCorpus.search needs the raw frames for the comprehensive re-rank: "
                             "build the corpus with keep_frames=True")
        q3, dq_dev, qr = self._queries(queries)
        if q3.dtype != self.dtype:
            q3 = q3.to(self.dtype)
            dq_dev = K.comp_describe(q3)
        return k, q3, dq_dev, to_np(dq_dev), qr

    def _search_per_query(self, queries, k: int = 10, threshold: float = 0.1, window: int = 0):
        """search() with a host loop over the queries: the list heads copied to the host, then per query the raw
        frames of its list gathered, one hq_comp_scores launch and a NumPy stable sort.  The route of lists beyond
        hq_list_topk's 1024 entries, and the yardstick search() is tested against."""
        t = torch()
        k, q3, dq_dev, dq, qr = self._search_inputs(queries, k)
        Q = qr.N
        out_s = np.full((Q, k), -np.inf)
        out_i = np.full((Q, k), -1, dtype=np.int64)
        if 2 * k <= K.HIER_MAX_K:
            _, ids, _, _ = K.hier_filter(qr, self._rows, self._thr, self._ratio, 2 * k)
            heads = [r[r >= 0] for r in to_np(ids)]
        else:
            heads = [self._candidates(qr, a)[:2 * k] for a in range(Q)]
        if window:
            heads = [_windows_host(h, self.N, int(window)) for h in heads]
        for a, head in enumerate(heads):
            if not len(head):
                continue
            sel = t.as_tensor(head, device=q3.device)
            sc = to_np(_comp_exact(q3[a:a + 1], dq_dev[a:a + 1].contiguous(), dq[a:a + 1], self._frames[sel],
                                   self._desc_dev[sel].contiguous(), self._desc[head]))[0]
            order = np.argsort(-sc, kind="stable")
            order = order[sc[order] >= threshold][:k]
            out_s[a, :len(order)], out_i[a, :len(order)] = sc[order], head[order]
        return to_dev(out_s), to_dev(out_i)

    def search(self, queries, k: int = 10, threshold: float = 0.1, window: int = 0):
        """The engine's search workflow (search_similar_documents_with_caching, engine.py:754-781, steps 2 - 5) for
        queries [Q, H, W] (or one frame): the first 2 k candidates of the cascade (hq_hier_filter); window = w >= 1
        (step 3, 10 in the engine): every candidate widened to its window of w consecutive frames, first appearances
        kept in order (hq_list_windows), window = 0: the candidates themselves; the comprehensive scores of that
        list by the exact route, the resident frames read through the list (hq_comp_scores_listed); a stable order
        by score descending (ties keep the list's order), score >= threshold, the first k (hq_list_topk) -> device
        (scores [Q, k] f64, ids [Q, k] i64), -inf / -1 padded.  The batch stays on the device: the number of
        launches and of copies to the host does not grow with Q.  A list of more than 1024 entries (2 k w) takes a
        host loop over the queries instead.  ValueError with the reference's message when a query and a listed
        frame with index rows differ in index width."""
        window = int(window)
        if not 0 <= window <= 64:
            raise ValueError(f"window = {window} (0 .. 64)")
        if 2 * int(k) * max(window, 1) > K.LIST_MAX:
            return self._search_per_query(queries, k, threshold, window)
        k, q3, dq_dev, dq, qr = self._search_inputs(queries, k)
        if 2 * k <= K.HIER_MAX_K:
            _, lst, _, _ = K.hier_filter(qr, self._rows, self._thr, self._ratio, 2 * k)
        else:  # the cascade kernel lists at most 64: longer heads are built per query on the host, then batched
            head = np.full((qr.N, 2 * k), -1, dtype=np.int64)
            for a in range(qr.N):
                h = self._candidates(qr, a)[:2 * k]
                head[a, :len(h)] = h
            lst = to_dev(head)
        if window:
            lst, _ = K.list_windows(lst, self.N, window)
        sc = _comp_listed(q3, dq_dev, dq, self._frames, self._desc_dev, self._ml, self._widths, lst)
        s, ids, _ = K.list_topk(sc, lst, k, float(threshold), 1)
        return s, ids


def progressive_hierarchical_search(query_embedding, candidate_embeddings) -> List[int]:
    """Drop-in for engine.py:51-95 with the store passed in (the reference reads it from
    _get_all_candidate_embeddings): the candidate frame numbers after the progressive cascade, in its order.  An
    empty or 1-D query and an empty store return [] as the reference does."""
    q = np.asarray(query_embedding)
    if q.size == 0 or q.ndim != 2 or len(candidate_embeddings) == 0:
        return []
    c = np.stack([np.asarray(x) for x in candidate_embeddings])
    if c.ndim != 3 or c.shape[1:] != q.shape:
        raise ValueError(f"candidate frames {c.shape[1:]} are not the query's {q.shape}")
    return HierarchicalFrameCorpus(c, keep_frames=False).candidates(q)
