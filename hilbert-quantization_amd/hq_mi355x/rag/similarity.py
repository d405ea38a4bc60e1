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

    # ---- the writer rule ------------------------------------------------------------------------------------
    def _mark_ready(self):
        self._built_on = K.stream()
        self._ready = torch().cuda.Event()
        self._ready.record()

    def _wait_ready(self):
        """Entry of every search and writer: ordered after the last writer (an event wait queued on the device)."""
        if self._ready is not None and K.stream() != self._built_on:
            torch().cuda.current_stream().wait_event(self._ready)

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

    def _local_rows(self, rows, what: str) -> np.ndarray:
        """Row numbers (sequence, NumPy array or device tensor) as a host int64 array, every one in [0, N)."""
        a = to_np(rows) if is_tensor(rows) else np.asarray(rows)
        a = a.reshape(-1)
        if a.size and a.dtype.kind not in "iu":
            raise TypeError(f"QuantizedFrameCorpus.{what}: row numbers must be integers")
        a = a.astype(np.int64)
        if a.size and (a.min() < 0 or a.max() >= self.N):
            bad = int(a.min()) if a.min() < 0 else int(a.max())
            raise IndexError(f"QuantizedFrameCorpus.{what}: row {bad} outside [0, {self.N})")
        return a

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
        drop = self._local_rows(rows, "remove")
        keep = np.ones(self.N, dtype=bool)
        keep[drop] = False
        sel = np.flatnonzero(keep)
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
