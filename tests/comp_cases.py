"""Cases for the comprehensive frame similarity (hq_comp.hip, rag/similarity.py; rag/search/engine.py:478-727):
the golden of tests/golden/make_comprehensive.py, a NumPy float64 model of hq_comp_scores (any pair) and of the
composite row behind the fused route, and seeded stores at the shapes the GPU tests need.  Pure NumPy: shared by
tests/test_comp_cpu.py (which checks the models against the golden) and tests/test_gpu_comp.py."""
import functools
import os

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "comprehensive.npz")

FAMILIES = ("f9d", "f18d", "f9f", "f34f", "f67f")
F32_FAMILIES = ("f9f", "f34f", "f67f")
EDGES = ("zero", "short", "zeromean")
STANDALONE = ("ws3", "ws3f", "gap", "gapf", "tiny")
WIDTH_ERROR = "Query and candidate indices must have the same shape"


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def tolerance(dtype) -> float:
    """Exact route / float64 model against the reference: float64 frames agree to rounding; for float32 frames the
    reference computes the embedding and spatial parts in float32."""
    return 1e-12 if np.dtype(dtype) == np.float64 else 1e-6


# ------------------------------------------------------------------------------------------- reference pieces
def granularity_weights(m: int) -> np.ndarray:
    """engine.py:1101-1138."""
    if m <= 0:
        return np.array([])
    if m == 1:
        return np.array([1.0])
    w = np.array([8.0 ** (m - i - 1) for i in range(m)])
    w = w / np.sum(w)
    w[0] = w[0] * 2.0
    return w / np.sum(w)


def detect_height(e: np.ndarray) -> int:
    H, W = e.shape
    for r in range(H - 1, -1, -1):
        if 2 * int(np.sum(e[r] == 0)) < W:
            return r + 1
    return H


def describe(e: np.ndarray):
    """(h, L, width, row_mask) as hq_comp_describe writes them."""
    h = detect_height(e)
    L = width = mask = 0
    for r in range(h, e.shape[0]):
        nz = np.nonzero(e[r])[0]
        if len(nz):
            L += 1
            mask |= 1 << (r - h)
            width = max(width, int(nz[-1]) + 1)
    return h, L, width, mask


def windows(h: int, W: int):
    """(ws, stride, ni, nj); ws = 0 when the reference's window_size is below 2."""
    ws = min(4, h // 4, W // 4)
    if ws < 2:
        return 0, 1, 1, 1
    st = ws // 2
    return ws, st, (h - ws) // st + 1, (W - ws) // st + 1


def _cos01(a, b, zero=0.0):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    na, nb = np.sqrt(np.dot(a, a)), np.sqrt(np.dot(b, b))
    if na == 0 or nb == 0:
        return zero
    return (np.dot(a, b) / (na * nb) + 1.0) / 2.0


# ---------------------------------------------------------------------------- model of hq_comp_scores (any pair)
def exact_parts(q, c, weights_of="max", compact=True, zero_window=0.0):
    """(hierarchical, embedding, spatial) of two enhanced frames in float64.  The keyword arguments switch single
    rules off for the discrimination test: weights_of="query" uses w(L_q), compact=False leaves dropped index rows
    in place, zero_window=0.5 scores a zero-norm window 0.5."""
    q, c = np.asarray(q, np.float64), np.asarray(c, np.float64)
    H, W = q.shape
    hq, Lq, wq, mq = describe(q)
    hc, Lc, wc, mc = describe(c)

    def rows(e, h, mask):
        if compact:
            return [e[h + b] for b in range(H - h) if mask >> b & 1]
        return [e[r] for r in range(h, H)] if mask else []

    hier = 0.0
    if Lq and Lc:
        if wq != wc:
            raise ValueError(WIDTH_ERROR)
        rq, rc = rows(q, hq, mq), rows(c, hc, mc)
        M = max(len(rq), len(rc))
        w = granularity_weights(len(rq) if weights_of == "query" else M)
        tot = tw = 0.0
        for l in range(M):
            s = _cos01(rq[l], rc[l]) if l < len(rq) and l < len(rc) else 0.0
            wl = w[l] if l < len(w) else 0.0
            tot += s * wl
            tw += wl
        hier = tot / tw if tw else 0.0
    m = min(hq, hc) * W
    emb = _cos01(q.reshape(-1)[:m], c.reshape(-1)[:m])
    spa = 0.0
    if hq == hc:
        ws, st, ni, nj = windows(hq, W)
        if ws == 0:
            spa = emb
        else:
            a = sliding_window_view(q[:hq], (ws, ws))[::st, ::st].reshape(ni * nj, -1)
            b = sliding_window_view(c[:hq], (ws, ws))[::st, ::st].reshape(ni * nj, -1)
            spa = float(np.mean(np.array([_cos01(x, y, zero_window) for x, y in zip(a, b)])))
    return hier, emb, spa


def exact_score(q, c, **kw):
    hier, emb, spa = exact_parts(q, c, **kw)
    return 0.5 * hier + 0.3 * emb + 0.2 * spa


# ------------------------------------------------------------------------------------- model of the composite row
def composite_k(H: int, W: int, h: int) -> int:
    ws, st, ni, nj = windows(h, W)
    return (H - h) * W + h * W + 1 + ni * nj * ((ws * ws if ws else h * W) + 1) + 1


def composite_rows(frames, h: int, side: int, indicators=True) -> np.ndarray:
    """Float64 composite rows [N, K] of frames [N, H, W] of profile (h, L = H - h): the row hq_comp_prepare writes,
    before its scaling and f16 split.  (rows_q . rows_c + 1) / 2 is the comprehensive score.  indicators=False
    leaves the validity columns out (the discrimination test)."""
    x = np.asarray(frames, np.float64)
    N, H, W = x.shape
    L = H - h
    w = granularity_weights(L)
    tw = 0.0
    for l in range(L):
        tw += w[l]
    coef = np.sqrt(0.5 * w / tw) if L else np.zeros(0)
    ws, st, ni, nj = windows(h, W)
    nw = ni * nj
    sb, sg = np.sqrt(0.3), np.sqrt(0.2 / nw)

    def unit(v):
        with np.errstate(invalid="ignore"):  # a frame holding a NaN keeps NaN entries: the caller leaves it out
            n = np.sqrt(np.sum(v * v, axis=-1, keepdims=True))
            ok = n != 0
            return np.where(ok, v / np.where(ok, n, 1.0), 0.0), ok.astype(np.float64)

    lev, _ = unit(x[:, h:, :])
    org, oi = unit(x[:, :h, :].reshape(N, 1, h * W))
    if ws:
        win = sliding_window_view(x[:, :h, :], (ws, ws), axis=(1, 2))[:, ::st, ::st].reshape(N, nw, ws * ws)
    else:
        win = x[:, :h, :].reshape(N, 1, h * W)
    wn, wi = unit(win)
    if not indicators:
        oi, wi = oi * 0.0, wi * 0.0
    const = np.full((N, 1), (np.sum(coef * coef) - 1.0) if side == 0 else 1.0)
    # section order of hq_comp_layout: windows, original block, levels, constant, block indicator, window indicators
    return np.concatenate([sg * wn.reshape(N, -1), sb * org.reshape(N, -1), (lev * coef[None, :, None]).reshape(N, -1),
                           const, sb * oi.reshape(N, 1), sg * wi.reshape(N, -1)], axis=1)


def composite_scores(queries, frames, h: int, **kw) -> np.ndarray:
    return (composite_rows(queries, h, 0, **kw) @ composite_rows(frames, h, 1, **kw).T + 1.0) / 2.0


def on_profile(e, h: int) -> bool:
    d = describe(e)
    return d[0] == h and d[1] == e.shape[0] - h and h < e.shape[0]


# ---------------------------------------------------------------------------------------------- seeded stores
GRANULARITIES = {8: (2,), 16: (4, 2), 32: (4, 2), 64: (8, 4, 2)}
PROFILE_H = {8: 8, 16: 17, 32: 32, 64: 65}   # detected height of an enhanced n x n frame


def enhance(img: np.ndarray) -> np.ndarray:
    """n x n image -> (n + rows) x n enhanced frame: block means per granularity, finest first, one row each (the
    RAG generator's layout; the order of the blocks inside a row does not matter to the scorer)."""
    n = img.shape[-1]
    rows = []
    for g in GRANULARITIES[n]:
        r = np.zeros(n, img.dtype)
        r[:g * g] = img.reshape(g, n // g, g, n // g).mean(axis=(1, 3)).reshape(-1)
        rows.append(r)
    return np.concatenate([img, np.stack(rows)], axis=0)


def family_images(rng, kind: str, n: int, N: int) -> np.ndarray:
    """gaussian / same-sign / near-duplicate float32 images [N, n, n]."""
    if kind == "gaussian":
        x = rng.standard_normal((N, n, n))
    elif kind == "same_sign":
        x = np.abs(rng.standard_normal((N, n, n))) + 1.0
    elif kind == "near_duplicate":
        x = rng.standard_normal((1, n, n)) + 1e-3 * rng.standard_normal((N, n, n))
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


def store(seed: int, n: int, N: int, Q: int, kind: str = "gaussian"):
    """(queries [Q, H, n], frames [N, H, n]) float32 enhanced frames on one profile."""
    rng = np.random.default_rng(seed)
    x = family_images(rng, kind, n, N + Q)
    e = np.stack([enhance(im) for im in x])
    return e[:Q], e[Q:]


# (n, N, Q): every composite length, a 384-frame tile boundary with pad rows in the last 16-row tile, a 128-query
# tile boundary; one 67 x 64 case
DENSE_CASES = ((8, 400, 3), (16, 400, 3), (32, 400, 3), (8, 400, 130), (64, 40, 2))
TOPK_KS = (1, 10, 64)
TOPK_GAP = 2e-5


def _topk_store(seed: int, n: int, N: int, Q: int, near: int):
    rng = np.random.default_rng(seed)
    qs = rng.standard_normal((Q, n, n))
    fr = rng.standard_normal((N, n, n))
    pos = rng.permutation(N)
    for a in range(Q):  # `near` frames per query at growing distances: well separated scores at the top
        for i in range(near):
            fr[pos[a * near + i]] = qs[a] + (0.05 + 0.02 * i) * rng.standard_normal((n, n))
    return (np.stack([enhance(im) for im in qs.astype(np.float32)]),
            np.stack([enhance(im) for im in fr.astype(np.float32)]))


def topk_gaps(scores: np.ndarray, k: int) -> float:
    """Smallest gap between consecutive places 1 .. k + 1 over all rows of an exact score matrix."""
    s = -np.sort(-scores, axis=1)[:, :k + 1]
    return float(np.min(s[:, :-1] - s[:, 1:]))


@functools.lru_cache(maxsize=None)
def topk_case(n: int, N: int = 400, Q: int = 3, near: int = 80):
    """(queries, frames, exact float64 scores [Q, N]) whose places 1 .. 65 are more than TOPK_GAP apart (the fused
    route's error is far below that, so its ranking must equal the exact one): re-seeded until that holds."""
    for seed in range(1000, 1050):
        qs, fr = _topk_store(seed, n, N, Q, near)
        sc = composite_scores(qs, fr, PROFILE_H[n])
        if topk_gaps(sc, max(TOPK_KS)) > TOPK_GAP:
            return qs, fr, sc
    raise AssertionError("no seed gives the required gaps")


def ranking(scores: np.ndarray, k: int):
    """(score desc, id asc) top-k ids of every row."""
    return np.stack([np.lexsort((np.arange(len(r)), -r))[:k] for r in scores])


def off_profile_queries(n: int, seed: int = 5) -> np.ndarray:
    """Three float32 queries no fused store of n x n images takes: an all-zero frame (h = H), a frame whose last
    data row is cut to the index width (another detected height where the first index row is sparse, n = 8, 32), and
    a frame with its last index row zeroed (L differs)."""
    rng = np.random.default_rng(seed)
    a, b = (enhance(rng.standard_normal((n, n)).astype(np.float32)) for _ in range(2))
    z = np.zeros_like(a)
    short = rng.standard_normal((n, n)).astype(np.float32)
    short[n - 1, GRANULARITIES[n][0] ** 2:] = 0.0
    b[-1] = 0.0
    return np.stack([z, enhance(short), b])
