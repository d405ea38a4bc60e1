"""The engine's search workflow on the device (hq_comp_scores_listed, hq_list_topk, hq_list_windows,
HierarchicalFrameCorpus.search, ComprehensiveFrameCorpus.rescore) against the dense scorer, the NumPy models of
tests/engine_search_cases.py, the reference's recorded steps 2 - 5 (tests/golden/rag_engine_search.npz) and the
per-query route.

* The listed scorer against the dense one: torch.equal, both kernels call one per-pair function.
* The list kernels against their models: equal (integers, and scores that are copied, never computed).
* .search against the reference: ids equal (the golden keeps every decision more than 1e-5 from a tie), scores within
  1e-12 (float64 frames) / 1e-6 (float32 frames: the reference's float32 arithmetic), hq_comp_scores' own figures.
* .search against _search_per_query at window = 0: ids and score bits."""
import functools

import numpy as np
import pytest

import comp_cases as C
import engine_search_cases as EC
import hier_cases as HC

pytestmark = pytest.mark.gpu

KINDS = ("9d", "9f", "12d", "12f", "34d", "34f", "mixed")


@pytest.fixture(scope="module")
def rt(hq_lib):
    import torch
    from hq_mi355x import kernels as K
    from hq_mi355x import rag
    from hq_mi355x._dev import to_dev, to_np
    from hq_mi355x.rag import similarity as S

    class RT:
        pass

    r = RT()
    r.t, r.K, r.S, r.rag, r.dev, r.np = torch, K, S, rag, to_dev, to_np
    return r


# ------------------------------------------------------------------------------------------------ listed scorer
@functools.lru_cache(maxsize=None)
def _model_dense(kind):
    """The NumPy model's [Q, N] scores, computed once per store (NaN where the model raises the width error)."""
    qs, fr = EC.listed_store(kind)
    out = np.full((len(qs), len(fr)), np.nan)
    for a, q in enumerate(qs):
        for i, f in enumerate(fr):
            try:
                out[a, i] = C.exact_score(q, f)
            except ValueError:
                pass
    return out


_dense_cache = {}


def _dense(rt, kind):
    """(q, desc_q, c, desc_c, weights, dense scores, dense parts) on the device, once per store."""
    if kind not in _dense_cache:
        qs, fr = EC.listed_store(kind)
        q, c = rt.dev(qs), rt.dev(fr)
        dq, dc = rt.K.comp_describe(q), rt.K.comp_describe(c)
        ml = int(max(rt.np(dq)[:, 1].max(), rt.np(dc)[:, 1].max()))
        wt = rt.S._weight_table(ml)
        sc, pt = rt.K.comp_scores(q, dq, c, dc, wt, parts=True)
        _dense_cache[kind] = (q, dq, c, dc, wt, sc, pt)
    return _dense_cache[kind]


@pytest.mark.parametrize("C_", (1, 31, 32, 33, 65))
@pytest.mark.parametrize("kind", KINDS)
def test_listed_scores_equal_dense_bitwise(rt, kind, C_):
    t = rt.t
    q, dq, c, dc, wt, dense, dparts = _dense(rt, kind)
    N = int(c.shape[0])
    ids_h = EC.listed_ids(N, C_)
    ids = rt.dev(ids_h)
    got, parts = rt.K.comp_scores_listed(q, dq, c, dc, ids, wt, parts=True)
    alone = rt.K.comp_scores_listed(q, dq, c, dc, ids, wt)
    pad = (ids < 0) | (ids >= N)
    safe = ids.clamp(0, N - 1)
    want = t.where(pad, t.full_like(got, float("-inf")), t.gather(dense, 1, safe))
    wparts = t.where(pad.unsqueeze(-1), t.zeros_like(parts), t.gather(dparts, 1, safe.unsqueeze(-1).expand(-1, -1, 3)))
    assert t.equal(got, want) and t.equal(alone, want) and t.equal(parts, wparts)
    g, p = rt.np(got), rt.np(parts)
    pad_h = (ids_h < 0) | (ids_h >= N)
    assert pad_h[2].all() and pad_h[:2].any() and not pad_h[:2].all() if C_ > 1 else pad_h[2].all()
    assert np.isneginf(g[pad_h]).all() and (p[pad_h] == 0.0).all() and not np.signbit(p[pad_h]).any()
    model = _model_dense(kind)
    live = ~pad_h
    want_m = model[np.nonzero(live)[0], ids_h[live]]
    ok = ~np.isnan(want_m)   # (the mixed store: the model raises where the index widths differ)
    tol = C.tolerance(EC.listed_store(kind)[1].dtype)
    assert ok.all() or kind == "mixed"
    assert np.abs(g[live][ok] - want_m[ok]).max(initial=0.0) <= tol


def test_listed_scores_functional_form_and_empty_lists(rt):
    qs, fr = EC.listed_store("12d")
    ids = EC.listed_ids(len(fr), 33)
    got = rt.rag.comprehensive_scores_listed(qs, fr, ids)
    q, dq, c, dc, wt, dense, _ = _dense(rt, "12d")
    assert rt.t.equal(got, rt.K.comp_scores_listed(q, dq, c, dc, rt.dev(ids), wt))
    s, p = rt.rag.comprehensive_scores_listed(qs, fr, ids[:, :0], parts=True)
    assert tuple(s.shape) == (3, 0) and tuple(p.shape) == (3, 0, 3)
    qm, fm = EC.listed_store("mixed")
    widths = np.array([C.describe(f)[2] for f in fm])
    other = int(np.flatnonzero(widths != C.describe(qm[0])[2])[0])
    same = int(np.flatnonzero(widths == C.describe(qm[0])[2])[0])
    with pytest.raises(ValueError, match=C.WIDTH_ERROR):
        rt.rag.comprehensive_scores_listed(qm[:1], fm, np.array([[same, other]]))
    ok = rt.np(rt.rag.comprehensive_scores_listed(qm[:1], fm, np.array([[same, -1, len(fm)]])))
    assert abs(ok[0, 0] - C.exact_score(qm[0], fm[same])) <= 1e-6 and np.isneginf(ok[0, 1:]).all()


# --------------------------------------------------------------------------------------------------- list ranking
@pytest.mark.parametrize("C_", (1, 2, 63, 64, 65, 257, 1024))
def test_list_topk_equals_model(rt, C_):
    s, ids, thr = EC.topk_rows(C_)
    sd, idd = rt.dev(s), rt.dev(ids)
    for k in (1, C_, C_ + 3):
        for mode in (0, 1, 2):
            gs, gi, gc = (rt.np(x) for x in rt.K.list_topk(sd, idd, k, thr, mode))
            ws, wi, wc = EC.padded_topk(s, ids, k, thr, mode)
            assert gi.tolist() == wi.tolist() and gc.tolist() == wc.tolist(), (k, mode)
            assert gs.tobytes() == ws.tobytes(), (k, mode)
    # the rows hold what they are for: scores equal to the threshold part mode 1 from mode 2; nothing is eligible in
    # the last two rows
    assert EC.padded_topk(s, ids, C_, thr, 1)[2][1] > EC.padded_topk(s, ids, C_, thr, 2)[2][1]
    assert EC.padded_topk(s, ids, C_, thr, 0)[2][4:].tolist() == [0, 0]


def test_list_topk_refuses_long_lists(rt):
    from hq_mi355x._lib import NativeLibraryError
    s = rt.t.zeros((2, 1025), dtype=rt.t.float64, device="cuda")
    ids = rt.t.zeros((2, 1025), dtype=rt.t.int64, device="cuda")
    with pytest.raises(NativeLibraryError):
        rt.K.list_topk(s, ids, 4)
    with pytest.raises(NativeLibraryError):
        rt.K.list_topk(s[:, :8], ids[:, :8], 0)


# -------------------------------------------------------------------------------------------------------- windows
@pytest.mark.parametrize("w", (1, 2, 3, 10, 11, 64))
@pytest.mark.parametrize("N", (1, 12, 200))
def test_list_windows_equals_model(rt, N, w):
    heads = EC.window_heads(N, w)
    out, cnt = (rt.np(x) for x in rt.K.list_windows(rt.dev(heads), N, w))
    assert out.shape == (len(heads), heads.shape[1] * w)
    if w == 64:
        assert out.shape[1] == EC.LIST_MAX
    for a, h in enumerate(heads):
        want = EC.windows_model(h, N, w)
        assert cnt[a] == len(want) and out[a, :len(want)].tolist() == want.tolist() and (out[a, len(want):] == -1).all()


def test_list_windows_refuses_beyond_its_limits(rt):
    from hq_mi355x._lib import NativeLibraryError
    for c0, w in ((17, 64), (16, 65), (103, 10), (4, 0)):
        with pytest.raises(NativeLibraryError):
            rt.K.list_windows(rt.t.zeros((2, c0), dtype=rt.t.int64, device="cuda"), 100, w)


# ------------------------------------------------------------------------------------------- .search, the reference
def _check_record(rt, s, ids, a, r, mr, tol, row=None):
    row = a if row is None else row
    n = len(r["final_ids"][a])
    assert ids[row, :n].tolist() == r["final_ids"][a].tolist() and (ids[row, n:] == -1).all()
    assert np.abs(s[row, :n] - r["final_scores"][a]).max(initial=0.0) <= tol
    assert np.isneginf(s[row, n:]).all()


@pytest.mark.parametrize("name", EC.golden_cases())
def test_search_equals_the_reference(rt, name):
    frames, queries, rec = EC.golden_case(name)
    tol = C.tolerance(frames.dtype)
    corpus = rt.S.HierarchicalFrameCorpus(frames)
    from hq_mi355x.rag.dual_storage import DualStorageCorpus
    dual = DualStorageCorpus(frames, list(range(len(frames))))
    for (mr, thr, w), r in zip(EC.SETTINGS, rec):
        if r["raised"].any():
            with pytest.raises(ValueError, match=C.WIDTH_ERROR):
                corpus.search(queries, mr, thr, window=w)
            for a, q in enumerate(queries):   # one query at a time: it raises where the reference did
                if r["raised"][a]:
                    with pytest.raises(ValueError, match=C.WIDTH_ERROR):
                        corpus.search(q, mr, thr, window=w)
                else:
                    s, ids = (rt.np(x) for x in corpus.search(q, mr, thr, window=w))
                    _check_record(rt, s, ids, a, r, mr, tol, row=0)
            continue
        s, ids = (rt.np(x) for x in corpus.search(queries, mr, thr, window=w))
        assert s.shape == (len(queries), mr)
        for a in range(len(queries)):
            _check_record(rt, s, ids, a, r, mr, tol)
        if thr == 0.1 and w == 10:
            got = dual.search(queries, mr, method="progressive", window=10)
            for a in range(len(queries)):
                assert [m for m, _ in got[a]] == [int(i) for i in ids[a] if i >= 0]
                assert [v for _, v in got[a]] == [float(v) for v, i in zip(s[a], ids[a]) if i >= 0]


# --------------------------------------------------------------------------------- .search, the per-query route
def _same_as_per_query(rt, corpus, queries, k, thr, window=0):
    try:
        ws, wi = corpus._search_per_query(queries, k, thr, window)
    except ValueError as e:
        with pytest.raises(ValueError) as got:
            corpus.search(queries, k, thr, window=window)
        assert str(got.value) == str(e)
        return "raised"
    s, ids = corpus.search(queries, k, thr, window=window)
    assert rt.t.equal(ids, wi)
    assert rt.t.equal(s.view(rt.t.int64), ws.view(rt.t.int64))   # the bits: -0.0 from 0.0, any NaN
    return rt.np(s), rt.np(ids)


@pytest.mark.parametrize("name", ("g12d", "g34_full", "g34_mixed"))
def test_search_equals_per_query_route_bitwise(rt, name):
    frames, queries, _, _, _ = HC.golden_case(name)
    corpus = rt.S.HierarchicalFrameCorpus(frames)
    outcomes = [_same_as_per_query(rt, corpus, queries, k, thr) for k in (1, 2, 10, 32, 40) for thr in (0.1, 0.55)]
    if name == "g34_mixed":
        assert "raised" in outcomes
    else:
        assert all(o != "raised" for o in outcomes) and any((o[1] >= 0).any() for o in outcomes)


def test_search_nan_frame_and_duplicate_ties(rt):
    frames, queries, lists, _, _ = HC.golden_case("g12d")
    fr = frames.copy()
    fr[lists[0][0], 0, 0] = np.nan          # the first candidate of query 0: its index rows, so its place, are kept
    corpus = rt.S.HierarchicalFrameCorpus(fr)
    for k in (2, 10):
        s, ids = _same_as_per_query(rt, corpus, queries, k, 0.1)
        assert lists[0][0] not in ids[0].tolist() and (ids[0] >= 0).any() and not np.isnan(s).any()
    q, dup = HC.duplicate_store(300)
    corpus = rt.S.HierarchicalFrameCorpus(dup)
    for k in (2, 10, 40):
        s, ids = _same_as_per_query(rt, corpus, q[None], k, 0.1)
        n = min(k, len(HC.model(q, dup)[0]))
        assert ids[0, :n].tolist() == list(range(n)) and len(set(s[0, :n].tolist())) == 1   # the cascade's order
    # the same with windows: both routes state one rule
    for w in (1, 3, 10):
        _same_as_per_query(rt, corpus, q[None], 10, 0.1, window=w)
    frames, queries, _ = EC.golden_case("e12")
    _same_as_per_query(rt, rt.S.HierarchicalFrameCorpus(frames), queries, 10, 0.1, window=10)


def test_search_long_lists_take_the_per_query_route(rt):
    """2 k window > 1024: the host loop; it agrees with the batched route's answer for the same k, since every list is
    shorter than either cut."""
    frames, queries, rec = EC.golden_case("e12")
    corpus = rt.S.HierarchicalFrameCorpus(frames)
    s, ids = (rt.np(x) for x in corpus.search(queries, 60, 0.1, window=10))
    s2, ids2 = (rt.np(x) for x in corpus.search(queries, 10, 0.1, window=10))
    assert (ids[:, :10] == ids2).all() and (s[:, :10] == s2).all()
    with pytest.raises(ValueError):
        corpus.search(queries, 10, 0.1, window=65)
    with pytest.raises(ValueError):
        corpus.search(queries, 10, 0.1, window=-1)


# ------------------------------------------------------------------------------------------------------- batching
def test_search_work_does_not_grow_with_the_batch(rt, monkeypatch):
    frames, queries, _ = EC.golden_case("e34")
    corpus = rt.S.HierarchicalFrameCorpus(frames)
    calls = {}

    def counted(name, fn):
        def wrapper(*a, **kw):
            calls[name] = calls.get(name, 0) + 1
            return fn(*a, **kw)
        return wrapper

    monkeypatch.setattr(rt.K, "comp_scores", counted("dense", rt.K.comp_scores))
    monkeypatch.setattr(rt.K, "comp_scores_listed", counted("listed", rt.K.comp_scores_listed))
    monkeypatch.setattr(rt.S, "to_np", counted("to_np", rt.S.to_np))
    seen = []
    for qs in (queries[:1], np.concatenate([queries, queries[:2]])):
        for w in (0, 10):
            calls.clear()
            s, ids = corpus.search(qs, 10, 0.1, window=w)
            assert tuple(ids.shape) == (len(qs), 10) and bool((ids[:, 0] >= 0).all())
            assert calls.get("dense", 0) == 0 and calls.get("listed", 0) == 1
            seen.append(calls.get("to_np", 0))
    assert len(set(seen)) == 1


# -------------------------------------------------------------------------------------------------------- rescore
def test_rescore_is_the_exact_score_of_a_fused_list(rt):
    frames, queries, _ = EC.golden_case("e34")
    corpus = rt.S.ComprehensiveFrameCorpus(frames, keep_frames=True)
    assert corpus.fused
    fused, ids = corpus.search(queries, 10)
    exact = corpus.rescore(queries, ids)
    dense = rt.rag.comprehensive_scores(queries, frames)
    assert rt.t.equal(exact, rt.t.gather(dense, 1, ids))
    assert float((exact - fused).abs().max()) <= 1e-5
    padded = rt.t.cat([ids, rt.t.full_like(ids[:, :2], -1)], 1)
    got = corpus.rescore(queries, padded)
    assert rt.t.equal(got[:, :10], exact) and bool(rt.t.isneginf(got[:, 10:]).all())
    with pytest.raises(ValueError, match="keep_frames"):
        rt.S.ComprehensiveFrameCorpus(frames).rescore(queries, ids)
    # a store that is not fused keeps its frames
    f12, q12, _ = EC.golden_case("e12")
    c12 = rt.S.ComprehensiveFrameCorpus(f12)
    assert not c12.fused
    s12, i12 = c12.search(q12, 5)
    assert rt.t.equal(c12.rescore(q12, i12), s12)
