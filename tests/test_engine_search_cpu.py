"""The NumPy models of tests/engine_search_cases.py (window rule, comprehensive score, list ranking) against the
reference's recorded steps 2 - 5 (tests/golden/rag_engine_search.npz), the margins that keep the records decidable,
the rules the cases must be able to tell apart, and the declarations of the new entry points.  No GPU."""
import os
import re

import numpy as np
import pytest

import comp_cases as C
import engine_search_cases as EC
import hier_cases as HC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _records():
    for name in EC.golden_cases():
        frames, queries, rec = EC.golden_case(name)
        for s, (mr, thr, w) in enumerate(EC.SETTINGS):
            for a, q in enumerate(queries):
                yield name, frames, q, a, rec[s], mr, thr, w


def test_golden_covers_the_cases():
    assert EC.golden_cases() == ["e34", "e12", "emix"]
    g = EC.golden()
    assert g["e34_frames"].shape == (60, 34, 32) and g["e34_frames"].dtype == np.float32
    assert len(g["e34_queries"]) == 3 and [len(r) for r in HC.extract(g["e34_frames"][0])] == [16, 4]
    assert g["e12_frames"].shape == (60, 12, 8) and g["e12_frames"].dtype == np.float64
    assert len(g["e12_queries"]) == 3 and len(HC.extract(g["e12_queries"][0])) == 4
    assert {C.describe(f)[2] for f in g["emix_frames"]} == {12, 16}   # 768-value and 1024-value embeddings
    assert os.path.getsize(EC.GOLDEN) <= os.path.getsize(HC.GOLDEN)
    # every setting of the non-mixed stores was scored; the mixed store raises wherever a list mixes index widths
    for name in ("e34", "e12"):
        assert not any(r["raised"].any() for r in EC.golden_case(name)[2])
    raised = [r["raised"] for r in EC.golden_case("emix")[2]]
    assert all(r.all() for r in raised[:4]) and any(r.any() for r in raised[4:]) and not all(r.all() for r in raised[4:])
    # a window that is cut by the store's end, and one cut by frame 0
    N = 60
    assert any(w and len(r["scored"][a]) and r["scored"][a].max() == N - 1 and r["final_ids"][a].max() < N
               for _, _, _, a, r, _, _, w in _records())
    assert any(w and len(r["scored"][a]) and r["scored"][a].min() == 0 for _, _, _, a, r, _, _, w in _records())


def test_windows_model_gives_recorded_order():
    for name, frames, q, a, r, mr, thr, w in _records():
        head = HC.model(q, frames)[0][:2 * mr]
        lst = EC.windows_model(head, len(frames), w) if w else head
        assert lst.tolist() == r["scored"][a].tolist(), (name, a, mr, w)


def test_comprehensive_model_gives_recorded_scores():
    for name, frames, q, a, r, mr, thr, w in _records():
        if r["raised"][a]:
            with pytest.raises(ValueError, match=C.WIDTH_ERROR):
                EC.model_scores(q, frames, r["scored"][a])
            continue
        got = EC.model_scores(q, frames, r["scored"][a])
        assert len(got) == len(r["scores"][a])
        if len(got):
            assert np.abs(got - r["scores"][a]).max() <= C.tolerance(frames.dtype), (name, a, mr, w)


def test_list_topk_model_gives_recorded_lists():
    for name, frames, q, a, r, mr, thr, w in _records():
        if r["raised"][a]:
            assert len(r["final_ids"][a]) == 0
            continue
        s, ids = EC.list_topk_model(r["scores"][a], r["scored"][a], mr, thr, 1)
        assert ids.tolist() == r["final_ids"][a].tolist(), (name, a, mr, thr, w)
        assert s.tobytes() == r["final_scores"][a].tobytes()


def test_golden_margins_hold():
    """No record is decided by rounding: two scored frames of a query differ by more than 1e-5 or are bit-identical
    frames, no score lies within 1e-5 of its threshold, and the cascade keeps its own margin."""
    for name in EC.golden_cases():
        frames, queries, _ = EC.golden_case(name)
        for q in queries:
            assert HC.decision_margin(q, frames) > HC.HARD_CAP
    for name, frames, q, a, r, mr, thr, w in _records():
        if not r["raised"][a]:
            assert EC.margin(frames, r["scored"][a], r["scores"][a], thr) > HC.HARD_CAP, (name, a, mr, thr, w)


@pytest.mark.parametrize("mutation", ({"clip": False}, {"dedup": False}, {"ties": "id"}, {"strict": True}),
                         ids=lambda m: next(iter(m)))
def test_cases_discriminate(mutation):
    """Each rule left out changes at least one recorded list."""
    if "strict" in mutation:
        # the margins keep every recorded score off its threshold.  The e12 store holds two bit-identical frames whose
        # recorded scores are therefore one value: with that value as the threshold, >= keeps both and > drops both
        frames, queries, rec = EC.golden_case("e12")
        r = rec[1]
        f, s = r["final_ids"][0], r["final_scores"][0]
        j = [i for i in range(len(f) - 1) if s[i] == s[i + 1]][0]
        assert frames[f[j]].tobytes() == frames[f[j + 1]].tobytes()
        keep = EC.list_topk_model(r["scores"][0], r["scored"][0], 10, s[j], 1)[1]
        drop = EC.list_topk_model(r["scores"][0], r["scored"][0], 10, s[j], 2)[1]
        assert keep.tolist() == f[:j + 2].tolist() and drop.tolist() == f[:j].tolist()
        return
    changed = []
    for name, frames, q, a, r, mr, thr, w in _records():
        if r["raised"][a]:
            continue
        if "ties" in mutation:
            ids = EC.list_topk_model(r["scores"][a], r["scored"][a], mr, thr, 1, **mutation)[1]
            if ids.tolist() != r["final_ids"][a].tolist():
                changed.append((name, a, mr, w))
        elif w:
            head = HC.model(q, frames)[0][:2 * mr]
            if EC.windows_model(head, len(frames), w, **mutation).tolist() != r["scored"][a].tolist():
                changed.append((name, a, mr, w))
    assert changed, mutation


def test_models_on_small_examples():
    assert EC.windows_model([7], 100, 10).tolist() == list(range(2, 12))        # f - 5 .. f + 4: ten frames
    assert EC.windows_model([7], 100, 3).tolist() == [6, 7, 8]
    assert EC.windows_model([2], 100, 10).tolist() == list(range(0, 8))         # start clipped at 0: 0 .. f + 5
    assert EC.windows_model([98], 100, 10).tolist() == list(range(93, 100))     # frames >= N dropped
    assert EC.windows_model([7, -1, 9, 7], 100, 4).tolist() == [5, 6, 7, 8, 9, 10]
    assert EC.windows_model([3, 3, -1, 0], 100, 1).tolist() == [3, 0]
    s, i = EC.list_topk_model([0.5, np.nan, 0.5, 0.9, -0.0, 0.0], [9, 1, 2, -1, 7, 3], 4)
    assert i.tolist() == [9, 2, 7, 3] and s.tolist() == [0.5, 0.5, -0.0, 0.0]
    assert EC.list_topk_model([0.5, 0.7], [4, 5], 5, 0.5, 1)[1].tolist() == [5, 4]
    assert EC.list_topk_model([0.5, 0.7], [4, 5], 5, 0.5, 2)[1].tolist() == [5]


def test_input_builders_hold_what_the_gpu_tests_need():
    for C_ in (1, 31, 32, 33, 65):
        ids = EC.listed_ids(70, C_)
        assert ids.shape == (3, C_) and ((ids[2] < 0) | (ids[2] >= 70)).all()
        if C_ >= 31:
            flat = ids[:2]
            assert (flat == 0).any() and (flat == 69).any() and (flat >= 70).any() and (flat[:, 1:-1] == -1).any()
            assert ids[0, -1] == -1 and any(len(set(r.tolist())) < C_ for r in flat)
    for w in (1, 2, 3, 10, 11, 64):
        for N in (1, 12, 200):
            h = EC.window_heads(N, w)
            assert h.shape[1] * w <= EC.LIST_MAX and h.max() < N and h.min() >= -1
    assert EC.window_heads(200, 64).shape[1] * 64 == EC.LIST_MAX


def test_symbols_declared_exported_registered():
    with open(os.path.join(ROOT, "include", "hq_mi355x.h")) as f:
        header = f.read()
    nargs = {"hq_comp_scores_listed": 16, "hq_list_topk": 11, "hq_list_windows": 8}
    from hq_mi355x import _lib
    for name, n in nargs.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert len(_lib.SIGNATURES[name][1]) == n
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        for name in nargs:
            assert hasattr(lib, name)
        # argument checks return before any device work
        assert lib.hq_comp_scores_listed(0, None, None, 0, None, None, 5, 9, 8, None, 4, None, 0, None, None, None) == 0
        assert lib.hq_comp_scores_listed(0, None, None, 3, None, None, 5, 9, 8, None, 0, None, 0, None, None, None) == 0
        assert lib.hq_comp_scores_listed(0, None, None, 3, None, None, 5, 9, 8, None, 4, None, 0, None, None,
                                         None) == _lib.HQ_E_INVALID
        assert lib.hq_comp_scores_listed(0, None, None, 3, None, None, 5, 131, 128, None, 4, None, 0, None, None,
                                         None) == _lib.HQ_E_INVALID    # null comes first, as in hq_comp_scores
        assert lib.hq_list_topk(None, None, 2, 1025, 1, 0.0, 0, None, None, None, None) == _lib.HQ_E_UNSUPPORTED
        assert lib.hq_list_topk(None, None, 2, 0, 1, 0.0, 0, None, None, None, None) == _lib.HQ_E_UNSUPPORTED
        assert lib.hq_list_topk(None, None, 2, 8, 0, 0.0, 0, None, None, None, None) == _lib.HQ_E_UNSUPPORTED
        assert lib.hq_list_topk(None, None, 0, 8, 3, 0.0, 0, None, None, None, None) == 0
        assert lib.hq_list_windows(None, 2, 16, 100, 65, None, None, None) == _lib.HQ_E_UNSUPPORTED
        assert lib.hq_list_windows(None, 2, 17, 100, 64, None, None, None) == _lib.HQ_E_UNSUPPORTED
        assert lib.hq_list_windows(None, 2, 16, 100, 0, None, None, None) == _lib.HQ_E_UNSUPPORTED
        assert lib.hq_list_windows(None, 0, 16, 100, 64, None, None, None) == 0
        assert lib.hq_list_windows(None, 2, 16, 100, 64, None, None, None) == _lib.HQ_E_INVALID    # null
    from hq_mi355x import kernels, rag
    for name in ("comp_scores_listed", "list_topk", "list_windows"):
        assert hasattr(kernels, name)
    assert "comprehensive_scores_listed" in rag.__all__ and hasattr(rag, "comprehensive_scores_listed")
    assert hasattr(rag.ComprehensiveFrameCorpus, "rescore")
    assert hasattr(rag.HierarchicalFrameCorpus, "_search_per_query")
    import inspect
    assert "window" in inspect.signature(rag.HierarchicalFrameCorpus.search).parameters
    from hq_mi355x.rag.dual_storage import DualStorageCorpus
    assert "window" in inspect.signature(DualStorageCorpus.search).parameters
    assert "One scoring launch per query" not in inspect.getsource(rag.similarity)
