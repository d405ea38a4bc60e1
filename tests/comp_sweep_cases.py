"""Shape, profile and edge sweep of the comprehensive frame similarity (hq_comp.hip, rag/similarity.py): a
vectorised float64 any-pair model (the rules of comp_cases.exact_parts for whole [Q, ...] x [N, ...] sets), hand-built
frames of given descriptors at the shapes that reach each kernel path, heterogeneous sets of them, and the second
golden (tests/golden/comprehensive_shapes.npz).  Pure NumPy: shared by tests/test_comp_sweep_cpu.py and
tests/test_gpu_comp_sweep.py."""
import functools
import os

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

import comp_cases as C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "comprehensive_shapes.npz")
GOLDEN_SETS = ("wide", "widef", "odd", "oddf", "small", "smallf", "rows31", "rows31f", "nonfinite", "nonfinitef")

# (H, W, h): the smallest frames that reach each path
SHAPES = (
    (6, 4, 4),       # ws < 2 with index rows
    (9, 8, 8),       # ws 2
    (13, 12, 12),    # ws 3, stride 1
    (15, 16, 14),    # ws 3, stride 1
    (18, 16, 17),    # ws 4
    (12, 100, 10),   # W > 64 and not a multiple of 64
    (20, 65, 17),    # odd W
    (35, 128, 32),   # 945 windows: more than the 256 threads and the 64 lanes
    (40, 8, 9),      # 31 index rows: mask bit 30, 31 weight levels
)
LDS_BYTES = 160 * 1024


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


# ------------------------------------------------------------------------------------------ vectorised model
def describe_all(frames) -> np.ndarray:
    """int64 [N, 4] = (h, L, width, mask) of every frame, the rules of comp_cases.describe without a loop per frame
    (NaN and inf are non-zero; -0.0 is zero)."""
    x = np.asarray(frames)
    N, H, W = x.shape
    nz = x != 0
    dense = 2 * (W - nz.sum(axis=2)) < W                       # [N, H]: a data row
    last = H - 1 - np.argmax(dense[:, ::-1], axis=1)
    h = np.where(dense.any(axis=1), last + 1, H)
    below = np.arange(H)[None, :] >= h[:, None]
    live = nz.any(axis=2) & below                                # non-zero index rows
    trimmed = np.where(nz, np.arange(1, W + 1)[None, None, :], 0).max(axis=2)
    width = np.where(live, trimmed, 0).max(axis=1)
    bit = np.clip(np.arange(H)[None, :] - h[:, None], 0, 62)
    mask = np.where(live, np.int64(1) << bit, 0).sum(axis=1)
    return np.stack([h, live.sum(axis=1), width, mask], axis=1).astype(np.int64)


def _windows(h, W, ws3_stride=1):
    ws, st, ni, nj = C.windows(h, W)
    if ws == 3 and ws3_stride != 1:
        st = ws3_stride
        ni, nj = (h - ws) // st + 1, (W - ws) // st + 1
    return ws, st, ni, nj


def _cos01(dot, na, nb, zero=0.0):
    """(cos + 1) / 2 from dot products and square norms (arrays), `zero` where a norm is 0."""
    ok = (na != 0) & (nb != 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        v = (dot / (np.sqrt(np.where(ok, na, 1.0)) * np.sqrt(np.where(ok, nb, 1.0))) + 1.0) / 2.0
    return np.where(ok, v, zero)


def _level_rows(x, d, compact):
    """(rows [N, Lmax, W] zero padded, count [N]): each frame's non-zero index rows moved up (compact) or every row
    below its height left in place."""
    N, H, W = x.shape
    h, L = d[:, 0], d[:, 1]
    below = np.arange(H)[None, :] >= h[:, None]
    if compact:
        keep = below & (x != 0).any(axis=2)
        count = L.copy()
    else:
        keep = below & (L > 0)[:, None]
        count = np.where(L > 0, H - h, 0)
    Lmax = int(count.max(initial=0))
    rows = np.zeros((N, max(Lmax, 1), W))
    slot = np.cumsum(keep, axis=1) - 1
    n_i, r_i = np.nonzero(keep)
    rows[n_i, slot[n_i, r_i]] = x[n_i, r_i]
    return rows, count


def model_parts(queries, frames, weights_of="max", compact=True, zero_window=0.0, columns=None, ws3_stride=1,
                spatial_any_height=False):
    """float64 (parts [Q, N, 3] = hierarchical, embedding, spatial; score [Q, N]) of every pair.  The keyword
    arguments switch single rules off (the discrimination test): the three of comp_cases.exact_parts, columns=64
    ignores the columns from 64 on in every sum (the descriptors stay those of the whole frames), ws3_stride=2
    walks 3 x 3 windows in steps of 2, spatial_any_height=True scores the windows of the query's height whatever the
    frame's height is."""
    q, c = np.asarray(queries, np.float64), np.asarray(frames, np.float64)
    Q, H, W = q.shape
    N = c.shape[0]
    dq, dc = describe_all(queries), describe_all(frames)
    wq, wc = set(dq[dq[:, 1] > 0, 2].tolist()), set(dc[dc[:, 1] > 0, 2].tolist())
    if wq and wc and len(wq | wc) > 1:
        raise ValueError(C.WIDTH_ERROR)
    if columns is not None:
        q, c = q.copy(), c.copy()
        q[:, :, columns:] = 0.0
        c[:, :, columns:] = 0.0
    parts = np.zeros((Q, N, 3))

    # hierarchical: level l of both frames, zero padded to M levels, weights of M levels, summed left to right
    rq, nq = _level_rows(q, dq, compact)
    rc, nc = _level_rows(c, dc, compact)
    Lmax = max(rq.shape[1], rc.shape[1])
    M = np.maximum(nq[:, None], nc[None, :])
    table = np.zeros((max(int(M.max(initial=0)), 1) + 1, Lmax + 1))
    for m in range(1, table.shape[0]):
        table[m, :m] = C.granularity_weights(m)[:Lmax + 1]
    wsel = table[(nq[:, None] if weights_of == "query" else M) + np.zeros_like(M)]     # [Q, N, Lmax + 1]
    tot, tw = np.zeros((Q, N)), np.zeros((Q, N))
    for l in range(Lmax):
        s = np.zeros((Q, N))
        if l < rq.shape[1] and l < rc.shape[1]:
            both = (l < nq)[:, None] & (l < nc)[None, :]
            s = np.where(both, _cos01(rq[:, l] @ rc[:, l].T, np.sum(rq[:, l] ** 2, axis=1)[:, None],
                                      np.sum(rc[:, l] ** 2, axis=1)[None, :]), 0.0)
        wl = np.where(l < M, wsel[:, :, l], 0.0)
        tot += s * wl
        tw += wl
    with np.errstate(invalid="ignore", divide="ignore"):
        hier = np.where(tw != 0, tot / np.where(tw != 0, tw, 1.0), 0.0)
    parts[:, :, 0] = np.where((dq[:, 1] > 0)[:, None] & (dc[:, 1] > 0)[None, :], hier, 0.0)

    # embedding: the blocks flattened, truncated to the common length
    hq, hc = dq[:, 0], dc[:, 0]
    hmin = np.minimum(hq[:, None], hc[None, :])
    qf, cf = q.reshape(Q, -1), c.reshape(N, -1)
    for hh in np.unique(hmin):
        m = int(hh) * W
        a, b = qf[:, :m], cf[:, :m]
        e = _cos01(a @ b.T, np.sum(a * a, axis=1)[:, None], np.sum(b * b, axis=1)[None, :])
        parts[:, :, 1] = np.where(hmin == hh, e, parts[:, :, 1])

    # spatial: pairs of one height
    for hh in np.unique(hq):
        iq = np.flatnonzero(hq == hh)
        ic = np.arange(N) if spatial_any_height else np.flatnonzero(hc == hh)
        if not len(ic):
            continue
        ws, st, ni, nj = _windows(int(hh), W, ws3_stride)
        if ws == 0:
            m = int(hh) * W
            a, b = qf[iq, :m], cf[ic, :m]
            s = _cos01(a @ b.T, np.sum(a * a, axis=1)[:, None], np.sum(b * b, axis=1)[None, :])
        else:
            a = sliding_window_view(q[iq, :hh], (ws, ws), axis=(1, 2))[:, ::st, ::st].reshape(len(iq), ni * nj, -1)
            b = sliding_window_view(c[ic, :hh], (ws, ws), axis=(1, 2))[:, ::st, ::st].reshape(len(ic), ni * nj, -1)
            dot = np.einsum("qwe,nwe->qnw", a, b)
            s = _cos01(dot, np.sum(a * a, axis=2)[:, None, :], np.sum(b * b, axis=2)[None, :, :], zero_window).mean(axis=2)
        parts[np.ix_(iq, ic, [2])] = s[:, :, None]
    return parts, 0.5 * parts[:, :, 0] + 0.3 * parts[:, :, 1] + 0.2 * parts[:, :, 2]


def model_scores(queries, frames, **kw) -> np.ndarray:
    return model_parts(queries, frames, **kw)[1]


# --------------------------------------------------------------------------------------------- hand-built frames
def index_width(W: int) -> int:
    """Non-zero entries of a built index row: at least half of the row stays zero."""
    return max(1, W // 2)


def index_columns(W: int) -> np.ndarray:
    """Where they are: the leading columns and the last one, so that the trimmed width is W and an index row has an
    entry in the last trip of every 64-lane column loop."""
    return np.array(list(range(index_width(W) - 1)) + [W - 1])


def _mask(bits) -> int:
    return int(sum(1 << b for b in bits))


def build_frame(rng, H, W, h, kind="full", base=None):
    """(float64 frame [H, W], (h, L, width, mask) it is built for).  A dense gaussian block of h rows (or `base`,
    a full frame of this profile), then H - h index rows, non-zero at index_columns(W)."""
    L, cols = H - h, index_columns(W)
    off = np.setdiff1d(np.arange(W), cols)
    if base is None:
        x = np.zeros((H, W))
        x[:h] = rng.standard_normal((h, W))
        x[h:, cols] = rng.standard_normal((L, len(cols)))
    else:
        x = np.array(base, np.float64)
    live = list(range(L))
    hh = h
    if kind == "full":
        pass
    elif kind == "zero":
        x[:] = 0.0
        hh, live = H, []
    elif kind in ("drop_first", "drop_middle", "drop_last", "negzero_row"):
        b = {"drop_first": 0, "drop_middle": L // 2, "drop_last": L - 1, "negzero_row": L // 2}[kind]
        x[h + b] = -0.0 if kind == "negzero_row" else 0.0
        live.remove(b)
    elif kind == "short":
        if L + 1 <= 31 and h >= 2:
            x[h - 1, off] = 0.0          # the last data row cut to the index columns: one more index row
            hh, live = h - 1, list(range(L + 1))
        else:
            x[h] = rng.standard_normal(W)  # the first index row made dense: one more data row
            hh, live = h + 1, list(range(L - 1))
    elif kind == "zero_patch":
        r0, c0 = (2, 2) if h > 3 and W > 3 else (0, 0)
        x[r0:max(r0 + 1, min(6, h - 1)), c0:max(c0 + 1, min(8, W))] = 0.0
    elif kind == "negated":
        x = -x
    elif kind == "same_sign":
        x = np.where(x != 0, np.abs(x) + 1.0, 0.0)
    elif kind == "tiny":
        x = x * 1e-20
    elif kind == "huge":
        x = x * 1e18
    elif kind == "const_rows":
        v = rng.standard_normal(H) + np.where(rng.random(H) < 0.5, -2.0, 2.0)
        x[:h] = v[:h, None]
        x[h:, cols] = v[h:, None]
    elif kind == "noisy":
        x = np.where(x != 0, x + 0.3 * rng.standard_normal((H, W)), 0.0)
    else:
        raise ValueError(kind)
    return x, (hh, len(live), W if live else 0, _mask(live))


KINDS = ("full", "zero", "drop_first", "drop_middle", "drop_last", "short", "zero_patch", "negated", "same_sign", "tiny",
         "huge", "const_rows", "negzero_row", "noisy")


@functools.lru_cache(maxsize=None)
def hetero_set(H: int, W: int, h: int, dtype="float64", seed: int = 0):
    """(frames [42, H, W] of `dtype`, descriptors [42, 4] they were built for): every kind of KINDS on three
    independent bases.  Index rows share one width, so no pair raises."""
    rng = np.random.default_rng(1000 * H + 10 * W + h + seed)
    frames, desc = [], []
    for _ in range(3):
        base, _d = build_frame(rng, H, W, h)
        for kind in KINDS:
            x, d = build_frame(rng, H, W, h, kind, base)
            frames.append(x)
            desc.append(d)
    out = np.stack(frames).astype(dtype)
    out.setflags(write=False)
    return out, np.array(desc, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def hetero_model(H: int, W: int, h: int, dtype="float64"):
    """(parts, score) of the whole set against itself, computed once."""
    x, _ = hetero_set(H, W, h, dtype)
    parts, score = model_parts(x, x)
    parts.setflags(write=False)
    score.setflags(write=False)
    return parts, score


# ------------------------------------------------------------------------------------------ fused-route stores
GRANULARITIES = dict(C.GRANULARITIES)
GRANULARITIES[128] = (8, 4, 2)     # the RAG generator at n = 128: sqrt(128) rounded down to a power of two, halved to 2
FUSED_FAMILIES = ("gaussian", "same_sign", "near_duplicate", "negated")
FUSED_PROFILES = tuple(s for s in SHAPES if s[0] > s[2])


def enhance128(img: np.ndarray) -> np.ndarray:
    """comp_cases.enhance at n = 128: 131 x 128, detected height 128 (the 64-entry row of g = 8 is half zeros)."""
    n = img.shape[-1]
    rows = []
    for g in GRANULARITIES[n]:
        r = np.zeros(n, img.dtype)
        r[:g * g] = img.reshape(g, n // g, g, n // g).mean(axis=(1, 3)).reshape(-1)
        rows.append(r)
    return np.concatenate([img, np.stack(rows)], axis=0)


def fused_store(H: int, W: int, h: int, kind: str, Q: int = 4, N: int = 48, seed: int = 21):
    """(queries [Q, H, W], frames [N, H, W]) float32 on the profile (h, H - h): built frames, every index row non-zero at
    index_columns(W).  negated: the queries are negated stored frames plus 5 % noise."""
    rng = np.random.default_rng(seed + 7 * H + W)
    off = np.setdiff1d(np.arange(W), index_columns(W))

    def draw(M, fam):
        if fam == "same_sign":
            return np.abs(rng.standard_normal((M, H, W))) + 1.0
        if fam == "near_duplicate":
            return draw.base + 1e-3 * rng.standard_normal((M, H, W))
        return rng.standard_normal((M, H, W))

    draw.base = rng.standard_normal((1, H, W))
    fr = draw(N, kind if kind != "negated" else "gaussian")
    qs = -fr[:Q] + 0.05 * rng.standard_normal((Q, H, W)) if kind == "negated" else draw(Q, kind)
    for x in (qs, fr):
        x[:, h:, off] = 0.0
    return qs.astype(np.float32), fr.astype(np.float32)


def lds_bytes(H: int, W: int, itemsize: int) -> int:
    """The header's rule for hq_comp_scores: (5 max_windows + H W) values, the window lists in float64."""
    return 5 * 8 * max(max(ni * nj for _, _, ni, nj in (C.windows(h, W) for h in range(1, H + 1))), 1) + H * W * itemsize


def lds_edge(itemsize: int):
    """((H, W) of the largest square-ish frame the rule accepts, (H, W) of the first it refuses) along
    1 x 1, 2 x 1, 2 x 2, 3 x 2, ..."""
    k = 2
    while lds_bytes((k + 2) // 2, (k + 1) // 2, itemsize) <= LDS_BYTES:
        k += 1
    return ((k + 1) // 2, k // 2), ((k + 2) // 2, (k + 1) // 2)
