"""Inputs of the fused frame-cosine top-k tests (hq_cos_topk): seeded, NumPy only.

The kernel works on 128-query x 384-frame tiles, 48 frames per wave, and maps workgroup -> frame tile as
nt = xcd + 8 (slot / qtiles); the shapes below are the smallest at which each of those can go wrong:
N around one wave's columns (47, 48, 49), around one tile (383, 384, 385), two tiles and a ragged third (769),
nine tiles (3100: the XCD map wraps); Q of one row, one row short of a tile and one past it; K of a one-step, a
two-step, a ragged and the benchmark's K loop; k of 1, 10 and 64, k > N included."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

NS = (1, 47, 48, 49, 383, 384, 385, 769, 3100)
QS = (1, 127, 129)
KS = (32, 64, 1000, 4096)
TOPKS = (1, 10, 64)

# kind: how the rows are planted (build()); thr_mode / thr_at: the threshold test and the (query, frame) pair
# whose score is the threshold (an actual score of the matrix, so >= and > differ); thr: a fixed threshold
Case = namedtuple("Case", "name Q N K k seed kind thr_mode thr_at thr")

TIE_PAIRS = ((47, 48), (383, 384), (5, 3072 + 5))  # wave boundary, workgroup boundary, XCD wrap (tile 0 and 8)
ZERO_FROM = 40                                     # zeros_run: frames [40, N) are zero rows
ZERO_QUERY = 3
LATE_N, LATE_K, LATE_TILE0 = 5000, 5, 13 * 384     # the last 384-frame tile of 5000 frames starts at 4992
FEW_PASS = 3


def _c(name, Q, N, K, k, seed, kind="plain", thr_mode=0, thr_at=None, thr=0.0):
    return Case(name, Q, N, K, k, seed, kind, thr_mode, thr_at, thr)


def _grid():
    out = []
    for i, N in enumerate(NS):
        for j, k in enumerate(TOPKS):
            Q, K = QS[(i + j) % 3], KS[(i + 2 * j + 1) % 4]
            out.append(_c(f"grid-N{N}-Q{Q}-K{K}-k{k}", Q, N, K, k, 100 + 10 * i + j))
    return out


def _special():
    out = [
        # every (Q, K) pair appears at a multi-tile N with a ragged last tile
        *[_c(f"qk-Q{Q}-K{K}", Q, 769, K, 10, 300 + 4 * a + b) for a, Q in enumerate(QS) for b, K in enumerate(KS)],
        _c("ties", 129, 3100, 64, 10, 400, kind="ties"),
        _c("ties-k1", 127, 3100, 32, 1, 401, kind="ties"),
        _c("zeros-run", 127, 450, 64, 64, 410, kind="zeros"),
        _c("zeros-run-k10", 129, 450, 1000, 10, 411, kind="zeros"),
        _c("few-passers", 129, 769, 64, 10, 420, kind="few", thr_mode=1, thr=0.9),
        _c("late-winners", 129, LATE_N, 64, LATE_K, 430, kind="late"),
        _c("late-winners-K4096", 1, LATE_N, 4096, LATE_K, 431, kind="late"),
    ]
    # threshold sweep: the threshold is the score of query tq's r-th best frame, modes 1 and 2
    # (rank < k: the frame at the threshold is inside the list in mode 1 and outside it in mode 2)
    for N, Q, K, k, r in ((385, 127, 64, 10, 2), (769, 129, 1000, 10, 3), (3100, 1, 32, 64, 4), (384, 129, 64, 1, 0)):
        for mode in (1, 2):
            out.append(_c(f"thr-N{N}-mode{mode}-rank{r}", Q, N, K, k, 440 + r, kind="thr", thr_mode=mode,
                          thr_at=(Q // 2, r)))
    return out


CASES = tuple(_grid() + _special())


@lru_cache(maxsize=None)
def build(case):
    """(A [Q, K], B [N, K]) float32, read-only."""
    rng = np.random.default_rng(case.seed)
    Q, N, K = case.Q, case.N, case.K
    A = rng.standard_normal((Q, K)).astype(np.float32)
    B = rng.standard_normal((N, K)).astype(np.float32)
    # every query has a few near frames spread over the corpus, so the lists are not noise
    for q in range(Q):
        for j in range(3):
            B[(7 * q + 131 * j + 3) % N] += np.float32(1.5 - 0.4 * j) * A[q]
    if case.kind == "ties":
        for t, (i, j) in enumerate(TIE_PAIRS):
            B[i] = A[t % Q] * np.float32(2.0) + rng.standard_normal(K).astype(np.float32) * np.float32(0.25)
            B[j] = B[i]
    elif case.kind == "zeros":
        B[ZERO_FROM:] = 0.0
        A[ZERO_QUERY] = 0.0
    elif case.kind == "few":
        # FEW_PASS frames nearly parallel to query 0 (score > 0.9), nothing else comes close
        for j in range(FEW_PASS):
            B[100 + 300 * j] = A[0] + rng.standard_normal(K).astype(np.float32) * np.float32(0.05)
    elif case.kind == "late":
        # all queries near one direction; the frames nearest to it are the last eight, in the last tile
        base = rng.standard_normal(K).astype(np.float32)
        A = (base + np.float32(0.3) * A).astype(np.float32)
        B = rng.standard_normal((N, K)).astype(np.float32)
        B[N // 3] = base + np.float32(0.8) * B[N // 3]  # an early good frame: the hint rises in tile 4
        for j in range(8):
            B[N - 1 - j] = base + np.float32(0.02 * (j + 1)) * rng.standard_normal(K).astype(np.float32)
    A.setflags(write=False)
    B.setflags(write=False)
    return A, B


def exact_scores(A, B):
    """NumPy float64 (cos + 1) / 2, 0.0 where a norm is 0 (rag/search/engine.py:622-660 in float64)."""
    a, b = np.asarray(A, np.float64), np.asarray(B, np.float64)
    na, nb = np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = ((a @ b.T) / np.outer(na, nb) + 1.0) / 2.0
    s[na == 0, :] = 0.0
    s[:, nb == 0] = 0.0
    return s


def exact_columns(A, B, cols):
    """exact_scores of the frames `cols` with one fixed summation order per pair (no BLAS blocking), so equal
    rows give equal bits."""
    a, b = np.asarray(A, np.float64), np.asarray(B, np.float64)[list(cols)]
    dot = np.stack([(a * b[j]).sum(axis=1) for j in range(len(b))], axis=1)
    na, nb = np.sqrt((a * a).sum(axis=1)), np.sqrt((b * b).sum(axis=1))
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (dot / np.outer(na, nb) + 1.0) / 2.0
    s[na == 0, :] = 0.0
    s[:, nb == 0] = 0.0
    return s


def threshold_of(case, scores):
    """The case's threshold given a [Q, N] score matrix: fixed, or the score of query tq's r-th best frame
    (rank 0 = best) in that matrix."""
    if case.thr_at is None:
        return float(case.thr)
    tq, r = case.thr_at
    row = np.asarray(scores[tq], np.float64)
    order = np.lexsort((np.arange(len(row)), -row))
    return float(row[order[min(r, len(row) - 1)]])


def reference_topk(scores, k, thr, mode, id_base=0):
    """hq_select_topk's rule in NumPy: passing frames by (score desc, id asc), -inf / -1 padded."""
    scores = np.asarray(scores, np.float64)
    Q, N = scores.shape
    os_ = np.full((Q, k), -np.inf)
    oi = np.full((Q, k), -1, np.int64)
    for q in range(Q):
        row = scores[q]
        ok = np.ones(N, bool) if mode == 0 else (row >= thr if mode == 1 else row > thr)
        ids = np.flatnonzero(ok)
        ids = ids[np.lexsort((ids, -row[ids]))][:k]
        os_[q, :len(ids)] = row[ids]
        oi[q, :len(ids)] = ids + id_base
    return os_, oi
