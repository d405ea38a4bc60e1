"""Golden data of the RAG engine's search workflow, steps 2 - 5 (search_similar_documents_with_caching,
rag/search/engine.py:754-781; the window rule of FrameCacheManager.cache_consecutive_frames, rag/search/
frame_cache.py:66-72) -> tests/golden/rag_engine_search.npz.  Build-container only, like make_progressive_rag.py (same
inert cv2 stub, the engine made with cls.__new__ on the concrete class, _get_all_candidate_embeddings replaced by the
case's list).

    python tests/golden/make_rag_engine_search.py --ref /path/to/reference

names: the cases; settings [S, 3]: (max_results, threshold, cache_size), cache_size 0 = the step-3-free variant
(cached_frames = the head itself).  Per case <c>: <c>_frames [N, H, W], <c>_queries [Q, H, W], and per setting s, with
the Q queries concatenated: <c>_s<s>_scored (the frame numbers handed to the scorer, in dictionary order) and
<c>_s<s>_scores (the reference's scores of them; NaN where it raised) with <c>_s<s>_scored_lens [Q],
<c>_s<s>_final_ids / _final_scores (the list after the threshold and the cut) with <c>_s<s>_final_lens [Q],
<c>_s<s>_raised [Q] (the reference raised its index-width ValueError while scoring that query's list).

Step 2 is the reference's progressive_hierarchical_search.  Step 3 is its own cache_consecutive_frames over the first
2 max_results candidates, with a fresh cache manager per query that is large enough to evict nothing and whose
placeholder loader _load_frames_from_video is replaced by a lookup in the case's store (frame numbers >= N are left
out).  Step 4 is its calculate_embedding_similarity, step 5 the threshold and the cut as the workflow writes them.

Every record is asserted here (and again by tests/test_engine_search_cpu.py from the file) not to be decided by
rounding: any two scored frames of a query differ in score by more than 1e-5 or are bit-identical frames, no score
lies within 1e-5 of its threshold, and the cascade's own decisions keep hier_cases.decision_margin.  Stores are
re-seeded until that holds."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

WIDTH_ERROR = "Query and candidate indices must have the same shape"


def _engine():
    from hilbert_quantization.rag.search import engine as E
    cls = [v for v in vars(E).values() if isinstance(v, type) and "_filter_candidates_at_level" in vars(v)][0]
    return cls.__new__(cls)


def _run(obj, query, store, mr, thr, w):
    """dict(scored, scores, final, raised) of the reference for one query and one setting."""
    from hilbert_quantization.rag.search.frame_cache import FrameCacheManagerImpl
    N = len(store)
    obj._get_all_candidate_embeddings = lambda: store
    cands = obj.progressive_hierarchical_search(query)
    head = cands[:min(len(cands), mr * 2)]
    if w == 0:
        cached = {f: store[f] for f in head}
    else:
        fm = FrameCacheManagerImpl({"max_cache_size": 1 << 20})
        fm._load_frames_from_video = lambda path, numbers: {n: store[n] for n in numbers if n < N}
        obj.frame_cache_manager = fm
        cached = {}
        for f in head:
            cached.update(obj.cache_consecutive_frames(f, "", w))
    scored = np.array(list(cached.keys()), dtype=np.int64)
    try:
        sims = obj.calculate_embedding_similarity(query, cached)
    except ValueError as e:
        assert str(e) == WIDTH_ERROR, e
        return dict(scored=scored, scores=np.full(len(scored), np.nan), final=[], raised=True)
    of = {f: float(s) for f, s in sims}
    final = [(f, float(s)) for f, s in sims if s >= thr][:mr]
    return dict(scored=scored, scores=np.array([of[int(f)] for f in scored], dtype=np.float64), final=final,
                raised=False)


def fixtures():
    import engine_search_cases as EC
    import hier_cases as HC
    from hilbert_quantization.rag.embedding_generation.hierarchical_index_generator import (
        HierarchicalIndexGenerator as RagGen)
    from hilbert_quantization.rag.embedding_generation.hilbert_mapper import HilbertCurveMapperImpl
    obj, rg, mapper = _engine(), RagGen(), HilbertCurveMapperImpl(None)
    out, names = {"settings": np.array(EC.SETTINGS, dtype=np.float64)}, []

    def frame(values, n, dt):
        img = np.asarray(mapper.map_to_2d(np.asarray(values, dtype=dt), (n, n)))
        return np.asarray(rg.generate_multi_level_indices(img)).astype(dt)

    def embeddings(rng, d, N, clusters=4, noise=0.6):
        centres = rng.standard_normal((clusters, d))
        return centres[rng.integers(0, clusters, N)] + noise * rng.standard_normal((N, d))

    def attempt(frames, queries, accept):
        """The records of every setting, or None when a margin fails or `accept` says no."""
        fr, qs = np.stack(frames), np.stack(queries)
        if min(HC.decision_margin(q, fr) for q in qs) <= 2 * HC.HARD_CAP:
            return None
        store = [np.asarray(f) for f in fr]
        rec = []
        for mr, thr, w in EC.SETTINGS:
            got = [_run(obj, q, store, int(mr), thr, int(w)) for q in qs]
            for g in got:
                if not g["raised"] and EC.margin(fr, g["scored"], g["scores"], thr) <= HC.HARD_CAP:
                    return None
            rec.append(got)
        return rec if accept is None or accept(rec) else None

    def seeded(name, build, accept=None, seeds=range(400)):
        for seed in seeds:
            frames, queries = build(np.random.default_rng(seed + sum(map(ord, name))))
            rec = attempt(frames, queries, accept)
            if rec is None:
                continue
            names.append(name)
            out[f"{name}_frames"], out[f"{name}_queries"] = np.stack(frames), np.stack(queries)
            for s, got in enumerate(rec):
                p = f"{name}_s{s}_"
                out[p + "raised"] = np.array([g["raised"] for g in got])
                out[p + "scored"] = np.concatenate([g["scored"] for g in got]).astype(np.int64)
                out[p + "scores"] = np.concatenate([g["scores"] for g in got]).astype(np.float64)
                out[p + "scored_lens"] = np.array([len(g["scored"]) for g in got], dtype=np.int64)
                out[p + "final_ids"] = np.array([f for g in got for f, _ in g["final"]], dtype=np.int64)
                out[p + "final_scores"] = np.array([v for g in got for _, v in g["final"]], dtype=np.float64)
                out[p + "final_lens"] = np.array([len(g["final"]) for g in got], dtype=np.int64)
            print(f"{name}: seed {seed}, N = {len(frames)}, scored "
                  f"{[[len(g['scored']) for g in got] for got in rec]}, final "
                  f"{[[len(g['final']) for g in got] for got in rec]}, raised "
                  f"{[int(sum(g['raised'] for g in got)) for got in rec]}")
            return
        raise AssertionError(f"{name}: no seed gives the required margins")

    # 34 x 32 float32, two levels, N = 60, three queries
    def e34(rng):
        e = embeddings(rng, 1024, 63)
        return [frame(v, 32, np.float32) for v in e[3:]], [frame(v, 32, np.float32) for v in e[:3]]

    seeded("e34", e34, lambda rec: all(len(g["final"]) > 0 for g in rec[1]))

    # hand-built 12 x 8 float64 frames with four levels, N = 60, three queries.  Two bit-identical copies of one frame
    # D sit next to two heads of query 0, the copy with the larger frame number next to the earlier head: D matches the
    # query's original block and its upper levels but not its level-0 row, so it fails the cascade, is scored only as
    # a neighbour, and lands in the final list: the only place where (score, position) and (score, id) differ
    def e12(rng):
        qs, fr = HC.built_store(int(rng.integers(1 << 30)), 12, 8, 8, 60, Q=3, clusters=3, noise=0.5)
        fr = fr.copy()
        head = HC.model(qs[0], fr)[0]
        pairs = [(a, b) for i, a in enumerate(head) for b in head[i + 1:] if a > b + 12 and a + 1 < len(fr)]
        if pairs:
            a, b = pairs[0]
            d = qs[0].copy()
            d[:8] += 0.2 * rng.standard_normal((8, 8))
            nz = d[8] != 0
            r = rng.standard_normal(int(nz.sum()))
            u = d[8, nz] / np.linalg.norm(d[8, nz])
            r -= (r @ u) * u
            d[8, nz] = np.linalg.norm(d[8, nz]) * (0.15 * u + np.sqrt(1 - 0.15 ** 2) * r / np.linalg.norm(r))
            fr[a + 1] = fr[b + 1] = d
        return list(fr), list(qs)

    def tie_by_position(rec):
        f = rec[1][0]["final"]   # (10, 0.1, 10), query 0
        return any(s0 == s1 and i0 > i1 for (i0, s0), (i1, s1) in zip(f[:-1], f[1:]))

    seeded("e12", e12, tie_by_position)

    # a store mixing 1024-value and 768-value embeddings (make_progressive_rag.py's g34_mixed recipe): index widths 16
    # and 12, so a list that mixes both raises the reference's width error
    def emix(rng):
        e = [embeddings(rng, d, n + 2) for d, n in zip((1024, 768), (12, 12))]
        frames = [frame(v, 32, np.float32) for x in e for v in x[2:]]
        order = rng.permutation(len(frames))
        return [frames[i] for i in order], [frame(v, 32, np.float32) for x in e for v in x[:2]]

    seeded("emix", emix)
    out["names"] = np.array(names)
    return out


def main():
    from make_golden import _import_reference
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of the reference checkout")
    a = ap.parse_args()
    _import_reference(a.ref)
    d = fixtures()
    path = os.path.join(HERE, "rag_engine_search.npz")
    np.savez_compressed(path, **d)
    print(f"wrote {path}: {len(d)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
