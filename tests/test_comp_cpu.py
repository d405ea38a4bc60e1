"""The NumPy models of tests/comp_cases.py against the reference's recorded comprehensive scores
(tests/golden/comprehensive.npz): the float64 model of hq_comp_scores on every golden pair, the composite-row dot
product on the families it applies to, the rules each of them must not lose, and the score gaps the GPU ranking
tests rely on.  No GPU."""
import numpy as np
import pytest

import comp_cases as C


def _family_model(tag, **kw):
    e = C.golden()[f"{tag}_enh"]
    return np.array([[C.exact_score(a, b, **kw) for b in e] for a in e])


@pytest.mark.parametrize("tag", C.FAMILIES)
def test_exact_model_matches_golden_families(tag):
    g = C.golden()
    e = g[f"{tag}_enh"]
    tol = C.tolerance(e.dtype)
    assert [list(C.describe(x)[:3]) for x in e] == g[f"{tag}_desc"].tolist()
    parts = np.array([[C.exact_parts(a, b) for b in e] for a in e])
    assert np.abs(parts - g[f"{tag}_parts"]).max() <= tol
    assert np.abs(_family_model(tag) - g[f"{tag}_score"]).max() <= tol


@pytest.mark.parametrize("tag", C.FAMILIES)
@pytest.mark.parametrize("edge", C.EDGES)
def test_exact_model_matches_golden_edges(tag, edge):
    g = C.golden()
    fam, e = g[f"{tag}_enh"], g[f"e_{edge}_{tag}_enh"]
    assert list(C.describe(e)[:3]) == g[f"e_{edge}_{tag}_desc"].tolist()
    cs = list(fam) + [e]
    got = np.array([[C.exact_score(e, c) for c in cs], [C.exact_score(c, e) for c in cs]])
    assert np.abs(got - g[f"e_{edge}_{tag}_score"]).max() <= C.tolerance(e.dtype)


@pytest.mark.parametrize("name", C.STANDALONE)
def test_exact_model_matches_golden_standalone(name):
    g = C.golden()
    e = g[f"s_{name}_enh"]
    assert [list(C.describe(x)[:3]) for x in e] == g[f"s_{name}_desc"].tolist()
    parts = np.array([[C.exact_parts(a, b) for b in e] for a in e])
    assert np.abs(parts - g[f"s_{name}_parts"]).max() <= C.tolerance(e.dtype)


def test_golden_covers_the_edges():
    g = C.golden()
    assert g["e_zero_f34f_desc"].tolist() == [34, 0, 0]
    assert g["e_short_f34f_desc"].tolist()[:2] == [31, 3] and g["e_short_f9d_desc"].tolist()[:2] == [7, 2]
    assert g["e_zeromean_f34f_desc"].tolist()[1] == 1 and g["e_zeromean_f67f_desc"].tolist()[1] == 1
    assert g["s_ws3_desc"][:, 0].tolist() == [14, 14, 14] and C.windows(14, 16)[:2] == (3, 1)
    assert g["s_tiny_desc"][:, :2].tolist() == [[5, 0]] * 3 and C.windows(5, 4)[0] == 0
    assert g["s_gap_desc"][:, 1].tolist() == [3, 2, 2, 3]
    assert int(g["e_width_raised"]) == 1 and g["e_width_desc"][:, 2].tolist() == [4, 3]
    with pytest.raises(ValueError, match="same shape"):
        C.exact_score(*g["e_width_enh"])
    assert g["weights"].tolist() == [0.5, 0.3, 0.2]


@pytest.mark.parametrize("tag", C.FAMILIES)
def test_composite_dot_matches_golden(tag):
    g = C.golden()
    e = g[f"{tag}_enh"]
    h = int(g[f"{tag}_desc"][0, 0])
    assert all(C.on_profile(x, h) for x in e)
    rows = C.composite_rows(e, h, 1)
    assert rows.shape[1] == C.composite_k(e.shape[1], e.shape[2], h)
    assert np.abs(C.composite_scores(e, e, h) - g[f"{tag}_score"]).max() <= C.tolerance(e.dtype)


def test_composite_lengths():
    assert [C.composite_k(H, W, h) for H, W, h in ((67, 64, 65), (34, 32, 32), (18, 16, 17), (9, 8, 8))] == \
        [20627, 4915, 1123, 319]


def _max_move(model, gold):
    return float(np.abs(model - gold).max())


def test_models_discriminate():
    """Each rule left out moves at least one golden case by more than 1e-4."""
    g = C.golden()
    # validity indicators: the zero-patch frame (family member 7) has zero-norm windows
    for tag in ("f9d", "f34f"):
        e, h = g[f"{tag}_enh"], int(g[f"{tag}_desc"][0, 0])
        assert _max_move(C.composite_scores(e, e, h, indicators=False), g[f"{tag}_score"]) > 1e-4
        # a zero window scores 0.0, not 0.5
        assert _max_move(_family_model(tag, zero_window=0.5), g[f"{tag}_score"]) > 1e-4
    # w(max(L_q, L_c)), not w(L_q): the short frame (L = 3) as the candidate of an L = 2 query
    fam, e = g["f34f_enh"], g["e_short_f34f_enh"]
    got = np.array([C.exact_score(c, e, weights_of="query") for c in fam])
    assert _max_move(got, g["e_short_f34f_score"][1, :8]) > 1e-4
    # dropped index rows are compacted: the later rows move up
    s = g["s_gap_enh"]
    got = np.array([[C.exact_score(a, b, compact=False) for b in s] for a in s])
    assert _max_move(got, g["s_gap_score"]) > 1e-4


@pytest.mark.parametrize("n", (8, 32))
def test_topk_cases_have_gaps(n):
    qs, fr, sc = C.topk_case(n)
    assert C.topk_gaps(sc, max(C.TOPK_KS)) > C.TOPK_GAP
    h = C.PROFILE_H[n]
    assert all(C.on_profile(x, h) for x in qs) and all(C.on_profile(x, h) for x in fr)
    # the composite model is the exact score on these stores too (spot check against the pair model)
    for a, b in ((0, 0), (1, 17), (2, 399)):
        assert abs(sc[a, b] - C.exact_score(qs[a], fr[b])) <= 1e-12


def test_seeded_stores_are_on_profile():
    for n, N, Q in C.DENSE_CASES:
        qs, fr = C.store(3, n, min(N, 20), min(Q, 3))
        assert all(C.on_profile(x, C.PROFILE_H[n]) for x in list(qs) + list(fr))
        for kind in ("same_sign", "near_duplicate"):
            qs, fr = C.store(4, n, 6, 2, kind)
            assert all(C.on_profile(x, C.PROFILE_H[n]) for x in list(qs) + list(fr))
    for n in (8, 32):
        assert not any(C.on_profile(x, C.PROFILE_H[n]) for x in C.off_profile_queries(n))
