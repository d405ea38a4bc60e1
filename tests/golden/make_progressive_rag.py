"""Golden data of the RAG engine's progressive hierarchical search (rag/search/engine.py:51-95, 97-162, 178-287)
-> tests/golden/progressive_rag.npz.  Build-container only, like make_comprehensive.py (same inert cv2 stub, the
engine made with cls.__new__ on the concrete class, _get_all_candidate_embeddings replaced by the case's list).

    python tests/golden/make_progressive_rag.py --ref /path/to/reference

names: the cases.  Per case <c>: <c>_frames [N, H, W], <c>_queries [Q, H, W], <c>_lists (the reference's
progressive_hierarchical_search lists of the Q queries, concatenated) with <c>_list_lens [Q], <c>_counts [Q, 8]
(survivors after each level, 0 for a level that did not run), <c>_scores [sum of lens, 8] (the reference's own level
scores of the listed frames, its float32 arithmetic for float32 frames; 0 beyond the query's levels).

Every case is asserted here (and again by tests/test_hier_cpu.py from the file) to keep every deciding score more
than 1e-5 away from its decision, or an exact tie of bit-identical rows (tests/hier_cases.decision_margin): a
candidate against its threshold, the two keys at a cap cut, neighbours in the final list.  Stores are re-seeded until
that holds, so the reference's own float32 rounding never decides anything."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def _engine():
    from hilbert_quantization.rag.search import engine as E
    cls = [v for v in vars(E).values() if isinstance(v, type) and "_filter_candidates_at_level" in vars(v)][0]
    return cls.__new__(cls)


def _run(obj, query, frames):
    """(list, counts [8], scores [len, 8]) of the reference for one query."""
    store = [np.asarray(f) for f in frames]
    obj._get_all_candidate_embeddings = lambda: store
    counts = []
    inner = type(obj)._filter_candidates_at_level

    def recording(q_level, cands, current, level):
        out = inner(obj, q_level, cands, current, level)
        counts.append(len(out))
        return out

    obj._filter_candidates_at_level = recording
    try:
        lst = obj.progressive_hierarchical_search(query)
    finally:
        del obj._filter_candidates_at_level
    c8 = np.zeros(8, dtype=np.int64)
    c8[:len(counts)] = counts
    ql = obj._extract_hierarchical_indices(query)
    sc = np.zeros((len(lst), 8))
    for a, i in enumerate(lst):
        cl = obj._extract_hierarchical_indices(store[i])
        for l, qrow in enumerate(ql):
            if l < len(cl):
                m = min(len(qrow), len(cl[l]))
                sc[a, l] = float(obj._compare_single_level_indices(qrow[:m], cl[l][:m])) if m else 0.0
    return np.array(lst, dtype=np.int64), c8, sc


def fixtures():
    import hier_cases as HC
    import comp_sweep_cases as SW
    from hilbert_quantization.rag.embedding_generation.hierarchical_index_generator import (
        HierarchicalIndexGenerator as RagGen)
    from hilbert_quantization.rag.embedding_generation.hilbert_mapper import HilbertCurveMapperImpl
    obj, rg, mapper = _engine(), RagGen(), HilbertCurveMapperImpl(None)
    out, names = {}, []

    def frame(values, n, dt):
        """An embedding of len(values) numbers -> the enhanced (n + rows) x n frame the RAG pipeline stores."""
        img = np.asarray(mapper.map_to_2d(np.asarray(values, dtype=dt), (n, n)))
        return np.asarray(rg.generate_multi_level_indices(img)).astype(dt)

    def record(name, frames, queries):
        frames, queries = np.stack(frames), np.stack(queries)
        assert frames.dtype == queries.dtype and len(frames) <= 200
        margin = min(HC.decision_margin(q, frames) for q in queries)
        assert margin > HC.HARD_CAP, (name, margin)
        got = [_run(obj, q, frames) for q in queries]
        names.append(name)
        out[f"{name}_frames"], out[f"{name}_queries"] = frames, queries
        out[f"{name}_lists"] = np.concatenate([g[0] for g in got]).astype(np.int64)
        out[f"{name}_list_lens"] = np.array([len(g[0]) for g in got], dtype=np.int64)
        out[f"{name}_counts"] = np.stack([g[1] for g in got])
        out[f"{name}_scores"] = np.concatenate([g[2] for g in got])
        print(f"{name}: N = {len(frames)}, lists {[len(g[0]) for g in got]}, counts "
              f"{[g[1][:4].tolist() for g in got]}, margin {margin:.2e}")

    def seeded(name, build, accept=None, seeds=range(200)):
        """build(rng) -> (frames, queries); the first seed whose margins hold (and whose float64 model lists and counts
        `accept`, where the case is built to show one situation)."""
        for seed in seeds:
            frames, queries = build(np.random.default_rng(seed + sum(map(ord, name))))
            fr, qs = np.stack(frames), np.stack(queries)
            if min(HC.decision_margin(q, fr) for q in qs) <= 2 * HC.HARD_CAP:
                continue
            if accept is None or accept([HC.model(q, fr)[:2] for q in qs]):
                return record(name, frames, queries)
        raise AssertionError(f"{name}: no seed gives the required margins")

    def embeddings(rng, d, N, clusters=4, noise=0.6):
        centres = rng.standard_normal((clusters, d))
        return centres[rng.integers(0, clusters, N)] + noise * rng.standard_normal((N, d))

    # 34 x 32 float32: full 1024-value embeddings, 768-value ones (level 0 trimmed to 12 values), a store mixing both
    def g34(dims, N):
        def build(rng):
            e = [embeddings(rng, d, n + 2) for d, n in zip(dims, N)]
            frames = [frame(v, 32, np.float32) for x in e for v in x[2:]]
            order = rng.permutation(len(frames))
            return [frames[i] for i in order], [frame(v, 32, np.float32) for x in e for v in x[:2]]
        return build

    seeded("g34_full", g34((1024,), (36,)))
    seeded("g34_768", g34((768,), (24,)))
    seeded("g34_mixed", g34((1024, 768), (12, 12)))
    assert [len(r) for r in obj._extract_hierarchical_indices(out["g34_full_frames"][0])] == [16, 4]
    assert [len(r) for r in obj._extract_hierarchical_indices(out["g34_768_frames"][0])][0] == 12

    # 67 x 64 float32: 4096 values (the g = 8 row is fully non-zero and counts as data: h = 65, levels [16, 4]) and one
    # frame of 1536 values (no row under 50 % zeros: no levels), stored and as a query
    def g67(rng):
        e = embeddings(rng, 4096, 12, clusters=2)
        short = frame(rng.standard_normal(1536), 64, np.float32)
        frames = [frame(v, 64, np.float32) for v in e[2:]]
        frames.insert(4, short)
        return frames, [frame(e[0], 64, np.float32), frame(e[1], 64, np.float32), short]

    seeded("g67", g67)
    assert obj._detect_original_embedding_height(out["g67_frames"][0]) == 65
    assert [len(r) for r in obj._extract_hierarchical_indices(out["g67_frames"][0])] == [16, 4]
    assert obj._extract_hierarchical_indices(out["g67_frames"][4]) == [] and out["g67_list_lens"][2] == 0

    # 9 x 8 float64, one level; the last query is an all-zero frame (no levels)
    def g9(rng):
        x = HC.clustered(rng, 8, 122, clusters=5, noise=0.5, dtype=np.float64)
        fr = [np.asarray(rg.generate_multi_level_indices(im)).astype(np.float64) for im in x]
        return fr[2:], fr[:2] + [np.zeros((9, 8))]

    seeded("g9d", g9)

    # hand-built 12 x 8 float64 frames with four levels (thr 0.3 / ratio 0.7 at level 3), some with dropped rows
    def g12(rng):
        qs, fr = HC.built_store(int(rng.integers(1 << 30)), 12, 8, 8, 100, Q=3, clusters=3, noise=0.5)
        fr = fr.copy()
        fr[5, 8] = 0.0      # first index row dropped: the levels shift
        fr[17, 10] = 0.0    # a middle row dropped
        fr[40, 11] = 0.0    # the last row dropped: one level fewer
        return list(fr), list(qs)

    seeded("g12d", g12)
    assert out["g12d_counts"][:, 3].max() > 0

    def near(rng, base, s, h=8):
        """base with gaussian noise of size s on its non-zero index entries."""
        x = base.copy()
        nz = x[h:] != 0
        x[h:][nz] += s * rng.standard_normal(int(nz.sum()))
        return x

    # exact duplicates straddling the cap cut (N = 10, cap 3): two nearer frames, then three copies of one frame
    def dup(rng):
        q, _ = SW.build_frame(rng, 9, 8, 8)
        far = [near(rng, SW.build_frame(rng, 9, 8, 8)[0], 0.0) for _ in range(5)]
        d = near(rng, q, 0.5)
        fr = [far[0], d.copy(), near(rng, q, 0.1), far[1], d.copy(), near(rng, q, 0.25), d.copy(), far[2],
              far[3], far[4]]
        return fr, [q]

    seeded("dup_cut", dup, lambda m: m[0][0].tolist() == [2, 5, 1])
    assert out["dup_cut_lists"].tolist() == [2, 5, 1]

    # three frames share their level-1 row and differ at level 0: the earlier level orders them (N = 20: caps 6, 3)
    def shared(rng):
        q, _ = SW.build_frame(rng, 10, 8, 8)
        fr = [near(rng, q, 0.9 + 0.05 * i) for i in range(20)]
        row = near(rng, q, 0.05)[9]
        for i, s in ((3, 0.2), (11, 0.1), (15, 0.3)):
            fr[i] = near(rng, q, s)
            fr[i][9] = row
        return fr, [q]

    seeded("shared_l1", shared, lambda m: m[0][0].tolist() == [11, 3, 15])
    assert out["shared_l1_lists"].tolist() == [11, 3, 15]

    # a candidate with fewer levels (frame 2: the best level-0 match, no level 1) and one whose first index row is zero
    # (frame 6: its second row is the query's level-0 row, so it passes level 0 only because the rows are compacted)
    def fewer(rng):
        q, _ = SW.build_frame(rng, 10, 8, 8)
        fr = [near(rng, q, 0.3 + 0.1 * i) for i in range(10)]
        fr[2] = near(rng, q, 0.02)
        fr[2][9] = 0.0
        fr[6] = q.copy()
        fr[6][9] = near(rng, q, 0.05)[8]
        fr[6][8] = 0.0
        q1 = q.copy()
        q1[9] = 0.0   # the same query with one level: the two frames stay in its list
        return fr, [q, q1]

    seeded("fewer_shift", fewer, lambda m: m[0][1][0] == 3 and {2, 6} <= set(m[1][0].tolist()))
    assert out["fewer_shift_counts"][0, 0] == 3 and 2 not in out["fewer_shift_lists"][:out["fewer_shift_list_lens"][0]]
    assert set(out["fewer_shift_lists"][out["fewer_shift_list_lens"][0]:].tolist()) >= {2, 6}

    # no candidate passes level 0 (negated frames); every candidate passes and the cap binds
    def none_pass(rng):
        q, _ = SW.build_frame(rng, 12, 8, 8)
        return [-near(rng, q, 0.2) for _ in range(12)], [q]

    def all_pass(rng):
        q, _ = SW.build_frame(rng, 12, 8, 8)
        return [near(rng, q, 0.05 + 0.01 * i) for i in rng.permutation(30)], [q]

    seeded("none_pass", none_pass)
    assert out["none_pass_list_lens"].tolist() == [0] and out["none_pass_counts"].max() == 0
    seeded("all_pass", all_pass, lambda m: m[0][1][:4].tolist() == [9, 4, 2, 1])
    assert out["all_pass_counts"][0, :4].tolist() == [9, 4, 2, 1]

    # N = 1, 3, 4: int(0.3), int(0.9) = 0 and int(1.2) = 1, so cap = 1; then int(0.5) = int(0.7) = 0
    for n in (1, 3, 4):
        def tiny(rng, n=n):
            q, _ = SW.build_frame(rng, 12, 8, 8)
            return [near(rng, q, 0.05 + 0.05 * i) for i in rng.permutation(n)], [q]
        seeded(f"n{n}", tiny, lambda m: m[0][1][:4].tolist() == [1, 1, 1, 1])
        assert out[f"n{n}_counts"][0, :4].tolist() == [1, 1, 1, 1]

    out["names"] = np.array(names)
    return out


def main():
    from make_golden import _import_reference
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of the reference checkout")
    a = ap.parse_args()
    _import_reference(a.ref)
    d = fixtures()
    path = os.path.join(HERE, "progressive_rag.npz")
    np.savez_compressed(path, **d)
    print(f"wrote {path}: {len(d)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
