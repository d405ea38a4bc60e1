"""The float64 model of tests/hier_cases.py (the progressive hierarchical search stated as one lexicographic order)
against the reference's recorded lists (tests/golden/progressive_rag.npz), the margins that keep the golden cases
decidable, the rules the cases must be able to tell apart, and the declarations of the new entry points.  No GPU."""
import os
import re

import numpy as np
import pytest

import hier_cases as HC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", HC.golden_cases())
def test_model_matches_golden(name):
    frames, queries, lists, counts, scores = HC.golden_case(name)
    packed = HC.packed_levels(frames)
    tol = 1e-12 if frames.dtype == np.float64 else 1e-6
    for a, q in enumerate(queries):
        lst, cnt, S = HC.model(q, frames, packed)
        assert lst.tolist() == lists[a].tolist()
        assert cnt.tolist() == counts[a].tolist()
        if len(lst):
            got = np.zeros((len(lst), HC.MAX_LEVELS))
            got[:, :S.shape[0]] = S[:, lst].T
            assert np.abs(got - scores[a]).max() <= tol


@pytest.mark.parametrize("name", HC.golden_cases())
def test_golden_margins_hold(name):
    """No deciding score within 1e-5 of its decision, except exact ties of bit-identical rows."""
    frames, queries, _, _, _ = HC.golden_case(name)
    packed = HC.packed_levels(frames)
    assert len(frames) <= 200
    for q in queries:
        assert HC.decision_margin(q, frames, packed) > HC.HARD_CAP


def test_golden_covers_the_cases():
    g = HC.golden()
    assert g["g34_full_frames"].shape[1:] == (34, 32) and g["g34_full_frames"].dtype == np.float32
    assert [len(r) for r in HC.extract(g["g34_full_frames"][0])] == [16, 4]
    assert [len(r) for r in HC.extract(g["g34_768_frames"][0])][0] == 12
    assert len({len(HC.extract(f)[0]) for f in g["g34_mixed_frames"]}) == 2
    assert g["g67_frames"].shape[1:] == (67, 64) and [len(r) for r in HC.extract(g["g67_frames"][0])] == [16, 4]
    assert HC.extract(g["g67_frames"][4]) == [] and g["g67_list_lens"][2] == 0   # the 1536-value frame
    assert 4 not in g["g67_lists"].tolist()
    assert g["g9d_frames"].dtype == np.float64 and len(HC.extract(g["g9d_frames"][0])) == 1
    assert g["g9d_list_lens"][2] == 0                                             # the all-zero query
    assert len(HC.extract(g["g12d_queries"][0])) == 4 and g["g12d_counts"][:, 3].max() > 0
    assert [len(HC.extract(g["g12d_frames"][i])) for i in (5, 17, 40)] == [3, 3, 3]
    f = g["dup_cut_frames"]
    assert f[1].tobytes() == f[4].tobytes() == f[6].tobytes() and g["dup_cut_lists"].tolist() == [2, 5, 1]
    f = g["shared_l1_frames"]
    assert f[3][9].tobytes() == f[11][9].tobytes() == f[15][9].tobytes() and f[3][8].tobytes() != f[11][8].tobytes()
    assert g["shared_l1_lists"].tolist() == [11, 3, 15]
    assert len(HC.extract(g["fewer_shift_frames"][2])) == 1 and not g["fewer_shift_frames"][6][8].any()
    assert g["none_pass_list_lens"].tolist() == [0] and g["all_pass_counts"][0, :4].tolist() == [9, 4, 2, 1]
    for n in (1, 3, 4):
        assert len(g[f"n{n}_frames"]) == n and g[f"n{n}_counts"][0, :4].tolist() == [1, 1, 1, 1]
    thr, ratio = HC.level_tables()
    assert thr[:5].tolist() == [0.6000000000000001, 0.5, 0.4, 0.3, 0.3] and ratio[:4].tolist() == [0.3, 0.5, 0.7, 0.7]


@pytest.mark.parametrize("mutation", ({"cap_from": "N"}, {"strict": True}, {"ties": "id"}, {"truncate": False},
                                      {"compact": False}), ids=lambda m: next(iter(m)))
def test_cases_discriminate(mutation):
    """Each rule left out changes the list or the counts of at least one golden case."""
    changed = []
    cases = HC.golden_cases()
    if "strict" in mutation:
        # the margins keep every golden score off its threshold; a zero dot product gives exactly 0.5 = thr_1 in any
        # arithmetic (hier_cases.orthogonal_case), which is where >= and > part
        q, fr = HC.orthogonal_case()
        lst, cnt, S = HC.model(q, fr)
        assert (S[1] == 0.5).all() and cnt[:2].tolist() == [3, 1] and len(lst) == 1
        assert HC.model(q, fr, strict=True)[1][:2].tolist() == [3, 0]
        return
    for name in cases:
        frames, queries, lists, counts, _ = HC.golden_case(name)
        for a, q in enumerate(queries):
            lst, cnt, _ = HC.model(q, frames, **mutation)
            if lst.tolist() != lists[a].tolist() or cnt.tolist() != counts[a].tolist():
                changed.append(name)
    assert changed, mutation


def test_generated_cases_are_decidable():
    for H, W, h in HC.SIZE_PROFILES:
        qs, fr, out = HC.size_case(H, W, h, 65)
        assert len(HC.extract(fr[0])) == H - h
        assert any(len(lst) for lst, _, _ in out)
    q, fr = HC.duplicate_store(50)
    lst, cnt, _ = HC.model(q, fr)
    assert cnt[:4].tolist() == [15, 7, 4, 2] and lst.tolist() == [0, 1]


def test_symbols_declared_exported_registered():
    with open(os.path.join(ROOT, "include", "hq_mi355x.h")) as f:
        header = f.read()
    for name in ("hq_hier_prepare", "hq_hier_workspace_size", "hq_hier_filter"):
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, header), name
    from hq_mi355x import _lib
    assert len(_lib.SIGNATURES["hq_hier_prepare"][1]) == 11
    assert len(_lib.SIGNATURES["hq_hier_workspace_size"][1]) == 3
    assert len(_lib.SIGNATURES["hq_hier_filter"][1]) == 18
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        for name in ("hq_hier_prepare", "hq_hier_workspace_size", "hq_hier_filter"):
            assert hasattr(lib, name)
        assert lib.hq_hier_workspace_size(0, 10, 2) == 0
        assert lib.hq_hier_workspace_size(3, 1000, 2) >= 2 * 3 * 1000 * 8 + 3 * 1000
    from hq_mi355x import kernels, rag
    for name in ("hier_prepare", "hier_filter", "HierRows"):
        assert hasattr(kernels, name)
    for name in ("HierarchicalFrameCorpus", "progressive_hierarchical_search"):
        assert name in rag.__all__ and hasattr(rag, name)
    # the tables the Python layer hands to the kernel are progressive_threshold's
    thr, ratio = HC.level_tables()
    for l in range(HC.MAX_LEVELS):
        assert rag.similarity.progressive_level(l) == (thr[l], ratio[l])
        assert rag.progressive_threshold(l, 77) == (thr[l], max(1, int(77 * ratio[l])))
