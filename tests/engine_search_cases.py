"""Cases for the engine's search workflow on the device (hq_comp_scores_listed, hq_list_topk, hq_list_windows,
HierarchicalFrameCorpus.search; rag/search/engine.py:754-781 steps 2 - 5, rag/search/frame_cache.py:66-72): NumPy
statements of the window rule and of the list ranking, the golden of tests/golden/make_rag_engine_search.py, the
margin check that keeps its decisions away from rounding, and input builders.  Pure NumPy: shared by
tests/test_engine_search_cpu.py and tests/test_gpu_engine_search.py."""
import functools
import os

import numpy as np

import comp_cases as C
import hier_cases as HC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rag_engine_search.npz")
# (max_results, threshold, window); window 0 = the step-3-free variant (the scored list is the head itself)
SETTINGS = ((2, 0.1, 10), (10, 0.1, 10), (2, 0.55, 10), (10, 0.1, 3), (2, 0.1, 0), (10, 0.1, 0), (2, 0.55, 0))
LIST_MAX = 1024


# ------------------------------------------------------------------------------------------------------- the models
def windows_model(heads, N: int, w: int, clip: bool = True, dedup: bool = True):
    """The scored list of one query: every head f >= 0 widened to start = max(0, f - w // 2) .. min(start + w,
    f + w // 2 + 1) - 1, frames >= N dropped, windows in head order, each ascending, first appearances only.
    clip=False / dedup=False (mutations) leave out the start + w clip / the de-duplication."""
    out = []
    for f in (int(x) for x in heads if x >= 0):
        start = max(0, f - w // 2)
        end = min(start + w, f + w // 2 + 1) if clip else f + w // 2 + 1
        out += [x for x in range(start, end) if x < N and not (dedup and x in out)]
    return np.array(out, dtype=np.int64)


def list_topk_model(scores, ids, k: int, thr: float = 0.0, mode: int = 0, ties: str = "position"):
    """(scores, ids) of the first k eligible entries (id >= 0, score not NaN, mode 0 none / 1 >= / 2 >) of one list
    in (score desc, position asc) order: a stable sort.  ties="id" (a mutation): (score desc, id asc)."""
    s, ids = np.asarray(scores, dtype=np.float64), np.asarray(ids, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        ok = (ids >= 0) & ~np.isnan(s) & (True if mode == 0 else (s >= thr if mode == 1 else s > thr))
    pos = np.flatnonzero(ok)
    if ties == "id":
        pos = pos[np.argsort(ids[pos], kind="stable")]
    pos = pos[np.argsort(-s[pos], kind="stable")][:k]
    return s[pos], ids[pos]


def padded_topk(scores, ids, k: int, thr: float = 0.0, mode: int = 0):
    """list_topk_model of every row, padded as hq_list_topk pads -> (scores [Q, k], ids [Q, k], counts [Q])."""
    Q = len(scores)
    os_, oi, cnt = np.full((Q, k), -np.inf), np.full((Q, k), -1, dtype=np.int64), np.zeros(Q, dtype=np.int32)
    for a in range(Q):
        s, i = list_topk_model(scores[a], ids[a], k, thr, mode)
        os_[a, :len(s)], oi[a, :len(s)], cnt[a] = s, i, len(s)
    return os_, oi, cnt


def model_scores(query, frames, ids):
    """The float64 comprehensive model (comp_cases.exact_score) of the listed frames."""
    return np.array([C.exact_score(query, frames[int(i)]) for i in ids])


# ------------------------------------------------------------------------------------------------------- the golden
@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def golden_cases():
    return [str(n) for n in golden()["names"]]


def _split(flat, lens):
    off = np.concatenate([[0], np.cumsum(lens)])
    return [flat[off[a]:off[a + 1]] for a in range(len(lens))]


def golden_case(name: str):
    """(frames [N, H, W], queries [Q, H, W], records): records[s] for SETTINGS[s] = dict(raised bool [Q]: the
    reference raised its index-width ValueError for that query, scored / scores: Q arrays, the scored frame numbers
    in dictionary order and the reference's scores of them; final_ids / final_scores: Q arrays, the final list)."""
    g = golden()
    assert [tuple(r) for r in g["settings"].tolist()] == [tuple(float(v) for v in s) for s in SETTINGS]
    rec = []
    for s in range(len(SETTINGS)):
        p = f"{name}_s{s}_"
        rec.append(dict(raised=g[p + "raised"],
                        scored=_split(g[p + "scored"], g[p + "scored_lens"]),
                        scores=_split(g[p + "scores"], g[p + "scored_lens"]),
                        final_ids=_split(g[p + "final_ids"], g[p + "final_lens"]),
                        final_scores=_split(g[p + "final_scores"], g[p + "final_lens"])))
    return g[f"{name}_frames"], g[f"{name}_queries"], rec


def margin(frames, scored, scores, thr: float) -> float:
    """How far one query's record is from being decided by rounding: the smallest score gap between two scored
    frames that are not bit-identical, and the smallest distance of a score from the threshold."""
    best = np.inf
    s = np.asarray(scores, dtype=np.float64)
    if len(s):
        best = float(np.min(np.abs(s - thr)))
    order = np.argsort(s, kind="stable")
    # a gap below the bound can only lie between score neighbours; walk each neighbourhood
    for a in range(len(order)):
        for b in range(a + 1, len(order)):
            i, j = order[a], order[b]
            d = float(s[j] - s[i])
            if d >= best:
                break
            if frames[int(scored[i])].tobytes() != frames[int(scored[j])].tobytes():
                best = d
    return best


# --------------------------------------------------------------------------------------------------- input builders
def listed_ids(N: int, C_: int, Q: int = 3):
    """ids [Q, C] for the listed scorer: 0 and N - 1, repeated ids, -1 in the middle and at the end, an id >= N,
    the last row all pads."""
    rng = np.random.default_rng(1000 * N + C_)
    ids = rng.integers(0, N, (Q, C_)).astype(np.int64)
    special = [0, N - 1, 5, 5, -1, N, N + 7, -3]
    for a in range(Q - 1):
        for j, v in enumerate(special):
            ids[a, (j * 7 + a) % C_] = v
        ids[a, C_ - 1] = -1 if a == 0 else N - 1
        ids[a, C_ // 2] = -1
    if C_ == 1:
        ids[0, 0], ids[1, 0] = N - 1, 0
    ids[Q - 1] = np.where(np.arange(C_) % 2 == 0, -1, N)
    return ids


def topk_rows(C_: int):
    """(scores [R, C], ids [R, C], thr): rows for hq_list_topk: gaussian scores with ties, NaN, -inf and +-0.0 entries
    and pads interleaved; all scores equal; +-0.0 only; a score equal to the threshold; an all-ineligible row."""
    rng = np.random.default_rng(C_)
    thr = 0.25
    s = np.round(rng.standard_normal((6, C_)), 1)           # one decimal: many ties
    ids = rng.permutation(6 * C_).reshape(6, C_).astype(np.int64)
    for r in (0, 1):
        s[r, rng.integers(0, C_, max(1, C_ // 8))] = np.nan
        s[r, rng.integers(0, C_, max(1, C_ // 8))] = -np.inf
        s[r, rng.integers(0, C_, max(1, C_ // 8))] = 0.0
        s[r, rng.integers(0, C_, max(1, C_ // 8))] = -0.0
        ids[r, rng.integers(0, C_, max(1, C_ // 4))] = -1
    s[1, ::3] = thr                                          # scores equal to the threshold, spread over the row
    ids[1, 0] = 6 * C_                                       # ... the first of them never a pad
    s[2] = 0.5                                               # all equal: position decides
    s[3] = np.where(rng.integers(0, 2, C_) == 0, 0.0, -0.0)  # +-0.0 compare equal
    s[4, :] = np.nan                                         # all ineligible: NaN ...
    ids[4, ::2] = -1
    ids[5] = -1                                              # ... and all pads
    return s, ids, thr


def window_heads(N: int, w: int):
    """heads [Q, C0]: 0, 1, N - 2, N - 1, adjacent heads whose windows overlap, repeated heads, -1 between heads."""
    c0 = min(16, LIST_MAX // w)
    base = [0, 1, -1, N - 2, N - 1, N // 2, N // 2 + 1, -1, N // 2, 0, N - 1, N // 3, -1, N // 3 + w // 2, 1, N // 2 + 2]
    rng = np.random.default_rng(N * 100 + w)
    rows = [np.array([min(max(v, -1), N - 1) for v in base[:c0]]), rng.integers(-1, N, c0), np.full(c0, -1), np.full(c0, N - 1),
            np.arange(c0) % N]
    return np.stack(rows).astype(np.int64)


@functools.lru_cache(maxsize=None)
def listed_store(kind: str):
    """(queries [3, H, W], frames [N, H, W]) for the listed scorer, N = 70: '9d' / '9f' 9 x 8 (one level), '12d' /
    '12f' 12 x 8 (four levels), '34d' / '34f' 34 x 32 (4 x 4 windows); 'mixed': the golden's mixed-height store as
    recorded, with its own queries."""
    if kind == "mixed":
        fr, qs, _ = golden_case("emix")
        return qs[:3], fr
    H, W, h = {"9": (9, 8, 8), "12": (12, 8, 8), "34": (34, 32, 32)}[kind[:-1]]
    qs, fr = HC.built_store(70 + H, H, W, h, 70)
    dt = np.float64 if kind[-1] == "d" else np.float32
    return qs.astype(dt), fr.astype(dt)
