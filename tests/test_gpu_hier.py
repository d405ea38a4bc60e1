"""The progressive hierarchical search on the GPU (hq_hier.hip, rag/similarity.py) against the reference's recorded
lists (tests/golden/progressive_rag.npz) and the float64 lexicographic model of tests/hier_cases.py.

* Lists and per-level counts: equal, on every golden case, through hq_hier_prepare + hq_hier_filter, .candidates and
  the drop-in.  The golden keeps every decision more than 1e-5 from a tie (tests/test_hier_cpu.py), the kernel's
  float64 scores are within 1e-6 of the reference's float32 ones, so equality is the right demand.
* Level scores: within 1e-12 of the model for float64 frames (two float64 sums of at most 64 terms in the same order,
  one with fused multiply-adds), within 1e-6 of the reference's float32 values for float32 frames.
* Generated stores are re-seeded until the model's decisions are more than 1e-9 apart (hier_cases.size_case)."""
import numpy as np
import pytest

import hier_cases as HC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt(hq_lib):
    import torch
    from hq_mi355x import kernels as K
    from hq_mi355x._dev import to_dev, to_np
    from hq_mi355x.rag import similarity as S

    class RT:
        pass

    r = RT()
    r.t, r.K, r.S, r.dev, r.np = torch, K, S, to_dev, to_np
    return r


def _counts8(counts):
    out = np.zeros((len(counts), HC.MAX_LEVELS), dtype=np.int64)
    out[:, :counts.shape[1]] = counts
    return out


def _check_against_model(rt, corpus, queries, frames, packed=None, kout=64):
    """filter and candidates of every query against the model: lists, counts, the scores of the list head."""
    packed = packed if packed is not None else HC.packed_levels(frames)
    ids, sc, counts = (rt.np(x) for x in corpus.filter(rt.dev(queries), kout))
    for a, q in enumerate(queries):
        lst, cnt, S = HC.model(q, frames, packed)
        assert _counts8(counts)[a].tolist() == cnt.tolist()
        assert corpus.candidates(q) == lst.tolist()
        n = min(len(lst), kout)
        assert ids[a, :n].tolist() == lst[:n].tolist() and (ids[a, n:] == -1).all()
        L = min(S.shape[0], sc.shape[2])
        if n:
            assert np.abs(sc[a, :n, :L] - S[:L, lst[:n]].T).max() <= 1e-12


# ------------------------------------------------------------------------------------------------------ goldens
@pytest.mark.parametrize("name", HC.golden_cases())
def test_golden_lists_counts_scores(rt, name):
    frames, queries, lists, counts, scores = HC.golden_case(name)
    f64 = frames.dtype == np.float64
    # the C entry points, through their tensor-level wrappers
    c = rt.K.hier_prepare(rt.dev(frames))
    q = rt.K.hier_prepare(rt.dev(queries), max_levels=c.max_levels, clamp=True)
    lv = [rt.S.progressive_level(l) for l in range(c.max_levels)]
    cnt, ids, sc, alive = rt.K.hier_filter(q, c, [v[0] for v in lv], [v[1] for v in lv], 64, want_alive=True)
    cnt, ids, sc, alive = (rt.np(x) for x in (cnt, ids, sc, alive))
    assert _counts8(cnt).tolist() == counts.tolist()
    packed = HC.packed_levels(frames)
    corpus = rt.S.HierarchicalFrameCorpus(frames)
    assert len(corpus) == len(frames) and corpus.resident_bytes > 0
    for a, want in enumerate(lists):
        n = len(want)
        assert ids[a, :n].tolist() == want.tolist() and (ids[a, n:] == -1).all()
        Lq = len(HC.extract(queries[a]))
        assert sorted(np.flatnonzero(alive[a] == Lq).tolist() if Lq else []) == sorted(want.tolist())
        assert corpus.candidates(queries[a]) == want.tolist()
        assert rt.S.progressive_hierarchical_search(queries[a], list(frames)) == want.tolist()
        if n:
            L = sc.shape[2]
            assert np.abs(sc[a, :n] - scores[a][:, :L]).max() <= (1e-12 if f64 else 1e-6)
            if f64:
                S = HC.level_scores(queries[a], frames, packed=packed)
                assert np.abs(sc[a, :n, :S.shape[0]] - S[:, want].T).max() <= 1e-12


def test_drop_in_edges(rt):
    frames, queries, lists, _, _ = HC.golden_case("g9d")
    assert rt.S.progressive_hierarchical_search(np.zeros(0), list(frames)) == []
    assert rt.S.progressive_hierarchical_search(queries[0].reshape(-1), list(frames)) == []
    assert rt.S.progressive_hierarchical_search(queries[0], []) == []
    ids, sc, counts = rt.S.HierarchicalFrameCorpus(frames).filter(np.zeros((0, 9, 8)), 5)
    assert tuple(ids.shape) == (0, 5) and tuple(counts.shape) == (0, 1)
    empty = rt.S.HierarchicalFrameCorpus(np.zeros((0, 9, 8)))
    ids, sc, counts = (rt.np(x) for x in empty.filter(queries[:2], 5))
    assert (ids == -1).all() and (counts == 0).all() and empty.candidates(queries[0]) == []


def test_exact_threshold_passes(rt):
    """s_1 = 0.5 = thr_1 exactly (zero dot products): >= keeps the frames."""
    q, fr = HC.orthogonal_case()
    corpus = rt.S.HierarchicalFrameCorpus(fr)
    _check_against_model(rt, corpus, q[None], fr)
    ids, sc, counts = (rt.np(x) for x in corpus.filter(q, 3))
    assert counts[0].tolist() == [3, 1] and sc[0, 0, 1] == 0.5


# -------------------------------------------------------------------------------------------------- consistency
@pytest.mark.parametrize("kout", (1, 20, 64))
def test_filter_is_the_head_of_candidates(rt, kout):
    for frames, queries in (HC.golden_case("g9d")[:2], HC.size_case(12, 8, 8, 1025)[1::-1]):
        corpus = rt.S.HierarchicalFrameCorpus(frames)
        ids = rt.np(corpus.filter(queries, kout)[0])
        for a, q in enumerate(queries):
            full = corpus.candidates(q)
            head = full[:kout]
            assert ids[a, :len(head)].tolist() == head and (ids[a, len(head):] == -1).all()


def _mixed_queries(frames, Q):
    """Q stored frames as queries with mixed level counts: 4, 3 (a dropped row), 0 (no index rows)."""
    qs = np.array(frames[:Q])
    for a in range(Q):
        if a % 5 == 1:
            qs[a, 8] = 0.0
        elif a % 5 == 2:
            qs[a, 11] = 0.0
        elif a % 5 == 3:
            qs[a, 8:] = 0.0
    return qs


def test_batches_equal_single_queries(rt):
    _, frames, _ = HC.size_case(12, 8, 8, 1023)
    corpus = rt.S.HierarchicalFrameCorpus(frames)
    qs = _mixed_queries(frames, 65)
    assert {len(HC.extract(q)) for q in qs} == {0, 3, 4}
    whole = [rt.np(x) for x in corpus.filter(qs, 20)]
    single = [[rt.np(x) for x in corpus.filter(q, 20)] for q in qs]
    for part in range(3):
        assert np.array_equal(whole[part], np.concatenate([s[part] for s in single]))
    three = [rt.np(x) for x in corpus.filter(qs[:3], 20)]
    for part in range(3):
        assert np.array_equal(three[part], whole[part][:3])
    packed = HC.packed_levels(frames)
    for a in (0, 1, 2, 3, 64):
        lst, cnt, _ = HC.model(qs[a], frames, packed)
        assert whole[0][a][:len(lst[:20])].tolist() == lst[:20].tolist() and _counts8(whole[2])[a].tolist() == cnt.tolist()


def test_workspace_chunks_give_identical_results(rt):
    qs, frames, _ = HC.size_case(12, 8, 8, 1025)
    corpus = rt.S.HierarchicalFrameCorpus(frames)
    one_query = int(rt.K._L().hq_hier_workspace_size(1, 1025, corpus.max_levels))
    assert int(rt.K._L().hq_hier_workspace_size(3, 1025, corpus.max_levels)) > one_query + 4096
    whole = [rt.np(x) for x in corpus.filter(qs, 64)]
    chunked = [rt.np(x) for x in corpus.filter(qs, 64, workspace_bytes=one_query + 4096)]   # three blocks of one query
    for a, b in zip(whole, chunked):
        assert np.array_equal(a, b)


# -------------------------------------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("N", HC.SIZES)
@pytest.mark.parametrize("profile", HC.SIZE_PROFILES, ids=lambda p: f"{p[0]}x{p[1]}")
def test_sizes_match_the_model(rt, profile, N):
    qs, frames, _ = HC.size_case(*profile, N)
    _check_against_model(rt, rt.S.HierarchicalFrameCorpus(frames, keep_frames=False), qs, frames)


def test_store_of_duplicates_lists_by_id(rt):
    q, frames = HC.duplicate_store(4100)
    corpus = rt.S.HierarchicalFrameCorpus(frames, keep_frames=False)
    lst, cnt, _ = HC.model(q, frames)
    assert cnt[:4].tolist() == [1230, 615, 430, 301] and lst.tolist() == list(range(301))
    _check_against_model(rt, corpus, q[None], frames)


def test_nan_frame_never_appears(rt):
    qs, frames, out = HC.size_case(12, 8, 8, 65)
    j = int(out[0][0][0])                 # the first frame of query 0's list
    bad = np.array(frames)
    bad[j, 8, 0] = np.nan
    rest = np.delete(np.array(frames), j, axis=0)
    assert int(65 * 0.3) == int(64 * 0.3)   # the level-0 cap does not notice the missing frame
    corpus = rt.S.HierarchicalFrameCorpus(bad)
    for q in qs:
        lst, cnt, _ = HC.model(q, rest)
        want = [int(i) + (1 if i >= j else 0) for i in lst]
        got = corpus.candidates(q)
        assert j not in got and got == want
        assert _counts8(rt.np(corpus.filter(q, 1)[2]))[0].tolist() == cnt.tolist()


def test_query_with_more_levels_than_the_store(rt):
    q, frames = HC.orthogonal_case()
    short = np.array(frames)
    short[:, 9] = 0.0                      # every stored frame has one level, the query two
    corpus = rt.S.HierarchicalFrameCorpus(short)
    assert corpus.max_levels == 1
    lst, cnt, _ = HC.model(q, short)
    assert len(lst) == 0 and cnt[0] == 3
    ids, _, counts = (rt.np(x) for x in corpus.filter(q, 5))
    assert corpus.candidates(q) == [] and (ids == -1).all() and counts[0].tolist() == [3]


def test_refusals(rt):
    from hq_mi355x._lib import NativeLibraryError
    frames, queries, _, _, _ = HC.golden_case("g9d")
    corpus = rt.S.HierarchicalFrameCorpus(frames, keep_frames=False)
    with pytest.raises(ValueError, match="keep_frames=True"):
        corpus.search(queries[:1])
    with pytest.raises(ValueError, match="kout"):
        corpus.filter(queries[:1], 65)
    with pytest.raises(ValueError, match="are not"):
        corpus.filter(np.zeros((1, 10, 8)))
    tall = np.zeros((2, 20, 8))
    tall[:, :8] = 1.0
    tall[:, 8:, :3] = 1.0                  # twelve index rows
    with pytest.raises(NativeLibraryError, match="non-zero index rows"):
        rt.S.HierarchicalFrameCorpus(tall)


# ------------------------------------------------------------------------------------------------------- search
def _engine_search(rt, q, frames, cands, k, threshold):
    """Steps 4 and 5 of the engine's workflow on the first 2 k candidates, with the project's drop-in scorer."""
    head = [int(i) for i in cands[:2 * k]]
    if not head:
        return []
    ranked = rt.S.calculate_embedding_similarity(q, {i: frames[i] for i in head})
    return [(i, s) for i, s in ranked if s >= threshold][:k]


@pytest.mark.parametrize("name", ("g12d", "g34_full"))
def test_search_is_the_engine_workflow(rt, name):
    frames, queries, lists, _, _ = HC.golden_case(name)
    corpus = rt.S.HierarchicalFrameCorpus(frames)
    from hq_mi355x.rag.dual_storage import DualStorageCorpus
    dual = DualStorageCorpus(frames, list(range(len(frames))))
    for k, threshold in ((2, 0.1), (10, 0.1), (2, 0.55), (40, 0.1)):
        s, ids = (rt.np(x) for x in corpus.search(queries, k, threshold))
        assert s.shape == (len(queries), k)
        for a, q in enumerate(queries):
            want = _engine_search(rt, q, frames, lists[a], k, threshold)
            n = len(want)
            assert ids[a, :n].tolist() == [i for i, _ in want] and (ids[a, n:] == -1).all()
            assert np.abs(s[a, :n] - np.array([v for _, v in want])).max(initial=0.0) <= 1e-12
            assert np.isneginf(s[a, n:]).all()
        if threshold == 0.1:
            got = dual.search(queries, k, method="progressive")
            for a in range(len(queries)):
                assert [m for m, _ in got[a]] == [int(i) for i in ids[a] if i >= 0]
                assert [v for _, v in got[a]] == [float(v) for v, i in zip(s[a], ids[a]) if i >= 0]


def test_search_mixed_widths_raise_where_the_scorer_does(rt):
    frames, queries, lists, _, _ = HC.golden_case("g34_mixed")
    corpus = rt.S.HierarchicalFrameCorpus(frames)
    raised = 0
    for a, q in enumerate(queries):
        try:
            want = _engine_search(rt, q, frames, lists[a], 2, 0.1)
        except ValueError as e:
            assert "same shape" in str(e)
            with pytest.raises(ValueError, match="same shape"):
                corpus.search(q, 2)
            raised += 1
            continue
        s, ids = (rt.np(x) for x in corpus.search(q, 2))
        assert [int(i) for i in ids[0] if i >= 0] == [i for i, _ in want]
    assert raised >= 0
