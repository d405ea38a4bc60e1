"""Cases for the progressive hierarchical search (hq_hier.hip, rag/similarity.py; rag/search/engine.py:51-95, 97-162,
178-287): the golden of tests/golden/make_progressive_rag.py, a float64 NumPy model stated as the lexicographic rule
(independent of the kernels), the margin check that keeps both the reference and the model away from undecidable
comparisons, and generated larger stores.  Pure NumPy: shared by tests/test_hier_cpu.py and tests/test_gpu_hier.py."""
import functools
import os

import numpy as np

import comp_cases as C
import comp_sweep_cases as SW

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "progressive_rag.npz")
HARD_CAP = 1e-5          # the project's bound on a fused score's error: no golden decision lies closer than this
MAX_LEVELS = 8


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def golden_cases():
    """Names of the golden cases, in file order."""
    return [str(n) for n in golden()["names"]]


def golden_case(name: str):
    """(frames [N, H, W], queries [Q, H, W], lists: Q int64 arrays, counts [Q, 8], scores: Q arrays [len, 8] of the
    reference's own level scores of the listed frames)."""
    g = golden()
    qs = g[f"{name}_queries"]
    flat, lens = g[f"{name}_lists"], g[f"{name}_list_lens"]
    off = np.concatenate([[0], np.cumsum(lens)])
    lists = [flat[off[a]:off[a + 1]].astype(np.int64) for a in range(len(qs))]
    sc = g[f"{name}_scores"]
    scores = [sc[off[a]:off[a + 1]] for a in range(len(qs))]
    return g[f"{name}_frames"], qs, lists, g[f"{name}_counts"], scores


# ----------------------------------------------------------------------------------------------- reference pieces
def level_tables(n: int = MAX_LEVELS):
    """(thr [n], ratio [n]) of _apply_progressive_threshold (engine.py:261-277), its own float expressions."""
    thr, ratio = [], []
    for level in range(n):
        t = 0.3 + (0.1 * (3 - min(level, 3)))
        thr.append(min(t, 0.8))
        ratio.append(0.3 if level == 0 else (0.5 if level == 1 else 0.7))
    return np.array(thr), np.array(ratio)


def extract(e, compact=True):
    """The frame's levels (engine.py:97-132): the rows below the detected height, all-zero rows dropped, each cut
    after its last non-zero value -> list of float64 arrays.  compact=False (a mutation) keeps an all-zero row as an
    empty level."""
    e = np.asarray(e)
    if e.ndim != 2:
        return []
    rows = []
    for r in range(C.detect_height(e), e.shape[0]):
        nz = np.nonzero(e[r])[0]
        if len(nz):
            rows.append(e[r, :nz[-1] + 1].astype(np.float64))
        elif not compact:
            rows.append(np.zeros(0))
    return rows


def packed_levels(frames, compact=True):
    """(rows [N, Lmax, W] float64 zero padded, lens [N, Lmax]) of a store."""
    x = np.asarray(frames)
    N, H, W = x.shape
    lv = [extract(e, compact) for e in x]
    Lmax = max([len(v) for v in lv], default=0)
    rows = np.zeros((N, max(Lmax, 1), W))
    lens = np.zeros((N, max(Lmax, 1)), dtype=np.int64)
    have = np.zeros((N, max(Lmax, 1)), dtype=bool)
    for i, v in enumerate(lv):
        for l, r in enumerate(v):
            rows[i, l, :len(r)] = r
            lens[i, l] = len(r)
            have[i, l] = True
    return rows, lens, have


def level_scores(query, frames, truncate=True, compact=True, packed=None):
    """S [L_q, N] float64: s_l(q, c) = 0.0 when c has no level l, else (cos + 1) / 2 over the first min(len_q, len_c)
    values, 0.0 for a zero norm.  Sums run in element order, one candidate per array lane, so that bit-identical rows
    score bit-identically.  truncate=False (a mutation): both rows zero padded to the longer one instead."""
    ql = extract(query, compact)
    rows, lens, have = packed if packed is not None else packed_levels(frames, compact)
    N = rows.shape[0]
    S = np.zeros((len(ql), N))
    for l, q in enumerate(ql):
        if l >= rows.shape[1] or len(q) == 0:
            continue
        lq = len(q)
        m = np.minimum(lens[:, l], lq) if truncate else np.full(N, max(lq, int(lens[:, l].max(initial=0))))
        qpad = np.zeros(rows.shape[2] + 1)
        qpad[:lq] = q
        dot, na, nb = np.zeros(N), np.zeros(N), np.zeros(N)
        for k in range(int(m.max(initial=0))):
            on = k < m
            y = np.where(on, rows[:, l, k], 0.0)
            x = np.where(on, qpad[k], 0.0)
            dot, na, nb = dot + x * y, na + x * x, nb + y * y
        ok = have[:, l] & (lens[:, l] > 0) & (na != 0) & (nb != 0)
        with np.errstate(invalid="ignore", divide="ignore"):
            s = (dot / (np.sqrt(np.where(ok, na, 1.0)) * np.sqrt(np.where(ok, nb, 1.0))) + 1.0) / 2.0
        S[l] = np.where(ok, s, 0.0)   # (a NaN inside the compared prefix makes a norm NaN != 0: the score is NaN)
    return S


def lex_order(S, ids, top, ties="lex"):
    """`ids` ordered by (s_top desc, s_{top-1} desc, ..., s_0 desc, id asc); ties="id" (a mutation): (s_top desc, id
    asc) only."""
    ids = np.asarray(ids, dtype=np.int64)
    levels = [top] if ties == "id" else list(range(top + 1))
    keys = (ids,) + tuple(-S[l, ids] for l in levels)   # np.lexsort: the last key is the primary one
    return ids[np.lexsort(keys)]


def cascade(S, N, cap_from="survivors", strict=False, ties="lex"):
    """The lexicographic rule on level scores S [L_q, N] -> (list int64, counts [8]): after level l the survivors are
    the first cap_l = max(1, int(n_prev ratio_l)) of the order (s_l desc, ..., s_0 desc, id asc) among the survivors
    with s_l >= thr_l.  Mutations: cap_from="N", strict (> for >=), ties="id"."""
    thr, ratio = level_tables()
    alive = np.arange(N, dtype=np.int64)
    counts = np.zeros(MAX_LEVELS, dtype=np.int64)
    if S.shape[0] == 0:
        return np.zeros(0, dtype=np.int64), counts
    for l in range(S.shape[0]):
        if len(alive) == 0:
            break
        with np.errstate(invalid="ignore"):
            keep = S[l, alive] > thr[l] if strict else S[l, alive] >= thr[l]
        cap = max(1, int((N if cap_from == "N" else len(alive)) * ratio[l]))
        alive = lex_order(S, alive[keep], l, ties)[:cap]
        counts[l] = len(alive)
    return alive, counts


def model(query, frames, packed=None, **kw):
    """(list, counts, S) of one query: the float64 model end to end."""
    score_kw = {k: kw.pop(k) for k in ("truncate", "compact") if k in kw}
    if score_kw:
        packed = None
    S = level_scores(query, frames, packed=packed, **score_kw)
    lst, counts = cascade(S, len(frames), **kw)
    return lst, counts, S


# ------------------------------------------------------------------------------------------------------- margins
def _same_rows(rows, lens, i, j, l):
    return lens[i, l] == lens[j, l] and rows[i, l].tobytes() == rows[j, l].tobytes()


def _pair_margin(S, rows, lens, top, i, j):
    """The two keys of frames i, j with top level `top`: the gap of the first score word that differs (inf when every
    word is an exact tie of bit-identical rows, so that the id decides); 0.0 for a tie of rows that are not identical."""
    for l in range(top, -1, -1):
        d = abs(S[l, i] - S[l, j])
        if d != 0:
            return d
        if not _same_rows(rows, lens, i, j, l):
            return 0.0
    return np.inf


def decision_margin(query, frames, packed=None) -> float:
    """The smallest distance of a deciding score from its decision over the model's cascade: every then-alive
    candidate against the level's threshold, the two keys at each cap cut, and every two neighbours of the final
    list.  Exact ties of bit-identical rows (decided by the id in the reference and here alike) do not count."""
    rows, lens, have = packed if packed is not None else packed_levels(frames)
    S = level_scores(query, frames, packed=(rows, lens, have))
    thr, ratio = level_tables()
    N = len(frames)
    alive = np.arange(N, dtype=np.int64)
    best = np.inf
    for l in range(S.shape[0]):
        if len(alive) == 0:
            break
        best = min(best, float(np.min(np.abs(S[l, alive] - thr[l]))))
        cap = max(1, int(len(alive) * ratio[l]))
        order = lex_order(S, alive[S[l, alive] >= thr[l]], l)
        if len(order) > cap:
            best = min(best, _pair_margin(S, rows, lens, l, order[cap - 1], order[cap]))
        alive = order[:cap]
    top = S.shape[0] - 1
    for a, b in zip(alive[:-1], alive[1:]):
        best = min(best, _pair_margin(S, rows, lens, top, a, b))
    return float(best)


# ------------------------------------------------------------------------------------------------ generated stores
def clustered(rng, n_img: int, N: int, clusters: int = 6, noise: float = 0.25, dtype=np.float32):
    """[N, n, n] images around `clusters` centres: level scores spread over the thresholds."""
    centres = rng.standard_normal((clusters, n_img, n_img))
    x = centres[rng.integers(0, clusters, N)] + noise * rng.standard_normal((N, n_img, n_img))
    return x.astype(dtype)


def built_store(seed: int, H: int, W: int, h: int, N: int, Q: int = 3, clusters: int = 5, noise: float = 0.35):
    """(queries [Q, H, W], frames [N, H, W]) float64 hand-built frames (comp_sweep_cases.build_frame's layout: h dense
    rows, H - h index rows non-zero at index_columns(W)) whose index rows cluster, so that every level cuts."""
    rng = np.random.default_rng(seed)
    cols = SW.index_columns(W)
    L = H - h
    centres = rng.standard_normal((clusters, L, len(cols)))

    def draw(M):
        x = np.zeros((M, H, W))
        x[:, :h] = rng.standard_normal((M, h, W))
        x[:, h:, cols] = centres[rng.integers(0, clusters, M)] + noise * rng.standard_normal((M, L, len(cols)))
        return x

    return draw(Q), draw(N)


SIZES = (2, 63, 64, 65, 1023, 1025, 4100)
SIZE_PROFILES = ((9, 8, 8), (12, 8, 8))   # one level; four levels (thr 0.3 / ratio 0.7 at level 3)


@functools.lru_cache(maxsize=None)
def size_case(H: int, W: int, h: int, N: int):
    """(queries, frames, [(list, counts, S) per query]) of a generated store, re-seeded until no decision of the
    model lies within 1e-9 of a tie (the kernel's sums differ from the model's by a few ulp)."""
    for seed in range(200, 260):
        qs, fr = built_store(seed + 1000 * N + H, H, W, h, N)
        packed = packed_levels(fr)
        if min(decision_margin(q, fr, packed) for q in qs) > 1e-9:
            out = [model(q, fr, packed) for q in qs]
            for a in (qs, fr):
                a.setflags(write=False)
            return qs, fr, out
    raise AssertionError("no seed gives the required margins")


@functools.lru_cache(maxsize=None)
def duplicate_store(N: int = 4100):
    """(query, frames): N copies of one 12 x 8 frame, the query a noisy copy of it that passes all four levels: every
    key word ties, the list is the id order cut by the caps."""
    rng = np.random.default_rng(4100)
    base, _ = SW.build_frame(rng, 12, 8, 8)
    q = SW.build_frame(rng, 12, 8, 8, "noisy", base)[0]
    fr = np.repeat(base[None], N, axis=0)
    return q, fr


@functools.lru_cache(maxsize=None)
def orthogonal_case():
    """(query, frames [10, 10, 8]) float64: every frame's level-1 row is supported on columns the query's level-1 row
    leaves zero, so each level-1 dot product is a sum of exact zeros and s_1 = 0.5 = thr_1 in any arithmetic: the one
    situation that tells s >= thr from s > thr.  Level 0 orders the frames (noise grows with the id)."""
    rng = np.random.default_rng(5)
    q = np.zeros((10, 8))
    q[:8] = rng.standard_normal((8, 8))
    q[8, [0, 1, 2, 7]] = rng.standard_normal(4)
    q[9, [0, 1, 7]] = rng.standard_normal(3)
    fr = np.zeros((10, 10, 8))
    for i in range(10):
        fr[i, :8] = rng.standard_normal((8, 8))
        fr[i, 8, [0, 1, 2, 7]] = q[8, [0, 1, 2, 7]] + 0.05 * (i + 1) * rng.standard_normal(4)
        fr[i, 9, [2, 3]] = rng.standard_normal(2)
    return q, fr
