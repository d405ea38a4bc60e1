"""The comprehensive frame similarity on the GPU (hq_comp.hip, rag/similarity.py) against the reference's recorded
scores (tests/golden/comprehensive.npz) and the NumPy models of tests/comp_cases.py.

* hq_comp_describe: exact.  hq_comp_scores (the exact route): 1e-12 for float64 frames, 1e-6 for float32 frames
  (the reference computes those in float32), components included, on every family, edge frame and stand-alone set.
* The fused route (hq_comp_prepare + the unchanged hq_cos_scores_mfma / hq_cos_topk): within 1e-5, the project's
  score contract, of the golden and of hq_comp_scores on seeded stores; lists bit-identical to hq_select_topk of
  the fused dense scores, ids equal to the exact ranking where the exact scores are more than 2e-5 apart."""
import numpy as np
import pytest

import comp_cases as C

pytestmark = pytest.mark.gpu

FUSED_TOL = 1e-5


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


def _fused_dense(rt, qs, fr, h):
    coef = rt.S._level_coef(fr.shape[1] - h)
    q = rt.K.comp_prepare(rt.dev(qs), h, 0, coef)
    c = rt.K.comp_prepare(rt.dev(fr), h, 1, coef)
    return q, c, rt.K.cosine_scores_mfma(q, c)


# ------------------------------------------------------------------------------------------------ describe
def test_describe_matches_golden(rt):
    g = C.golden()
    sets = [(g[f"{t}_enh"], g[f"{t}_desc"]) for t in C.FAMILIES]
    sets += [(g[f"e_{e}_{t}_enh"][None], g[f"e_{e}_{t}_desc"][None]) for t in C.FAMILIES for e in C.EDGES]
    sets += [(g[f"s_{n}_enh"], g[f"s_{n}_desc"]) for n in C.STANDALONE] + [(g["e_width_enh"], g["e_width_desc"])]
    for enh, want in sets:
        got = rt.np(rt.K.comp_describe(rt.dev(enh)))
        assert got[:, :3].tolist() == want.tolist()
        assert [int(m) for m in got[:, 3]] == [C.describe(e)[3] for e in enh]


def test_describe_rejects_more_than_31_index_rows(rt):
    from hq_mi355x._lib import NativeLibraryError
    x = np.zeros((1, 40, 8), np.float32)
    x[0, :4] = 1.0
    with pytest.raises(NativeLibraryError, match="31 index rows"):
        rt.K.comp_describe(rt.dev(x))


# --------------------------------------------------------------------------------------------- exact route
@pytest.mark.parametrize("tag", C.FAMILIES)
def test_exact_scores_match_golden_families_and_edges(rt, tag):
    g = C.golden()
    fam = g[f"{tag}_enh"]
    tol = C.tolerance(fam.dtype)
    sc, parts = rt.S.comprehensive_scores(fam, fam, parts=True)
    print(tag, "exact max err", np.abs(rt.np(sc) - g[f"{tag}_score"]).max())
    assert np.abs(rt.np(sc) - g[f"{tag}_score"]).max() <= tol
    assert np.abs(rt.np(parts) - g[f"{tag}_parts"]).max() <= tol
    for edge in C.EDGES:
        e = g[f"e_{edge}_{tag}_enh"]
        cs = np.concatenate([fam, e[None]])
        s0, p0 = rt.S.comprehensive_scores(e, cs, parts=True)
        s1, p1 = rt.S.comprehensive_scores(cs, e, parts=True)
        got = np.stack([rt.np(s0)[0], rt.np(s1)[:, 0]])
        gotp = np.stack([rt.np(p0)[0], rt.np(p1)[:, 0]])
        assert np.abs(got - g[f"e_{edge}_{tag}_score"]).max() <= tol, edge
        assert np.abs(gotp - g[f"e_{edge}_{tag}_parts"]).max() <= tol, edge


@pytest.mark.parametrize("name", C.STANDALONE)
def test_exact_scores_match_golden_standalone(rt, name):
    g = C.golden()
    e = g[f"s_{name}_enh"]
    sc, parts = rt.S.comprehensive_scores(e, e, parts=True)
    assert np.abs(rt.np(sc) - g[f"s_{name}_score"]).max() <= C.tolerance(e.dtype)
    assert np.abs(rt.np(parts) - g[f"s_{name}_parts"]).max() <= C.tolerance(e.dtype)


def test_width_mismatch_raises_like_the_reference(rt):
    g = C.golden()
    assert int(g["e_width_raised"]) == 1
    w = g["e_width_enh"]
    with pytest.raises(ValueError, match=C.WIDTH_ERROR):
        rt.S.comprehensive_scores(w[0], w[1])
    with pytest.raises(ValueError, match=C.WIDTH_ERROR):
        rt.S.calculate_comprehensive_similarity(w[0], None, w[1], 3)
    # a frame without index rows pairs with either width
    z = np.zeros_like(w[0])
    assert rt.np(rt.S.comprehensive_scores(z, w)).tolist() == [[0.0, 0.0]]


@pytest.mark.parametrize("tag", C.FAMILIES)
def test_calculate_embedding_similarity_ranking(rt, tag):
    g = C.golden()
    fam, keys = g[f"{tag}_enh"], g[f"{tag}_rank_keys"]
    got = rt.S.calculate_embedding_similarity(fam[1], {int(k): fam[i] for i, k in enumerate(keys)})
    assert [k for k, _ in got] == g[f"{tag}_rank_ids"].tolist()
    assert np.abs(np.array([s for _, s in got]) - g[f"{tag}_rank_scores"]).max() <= C.tolerance(fam.dtype)
    assert all(isinstance(k, int) and isinstance(s, float) for k, s in got)


def test_drop_ins(rt):
    g = C.golden()
    fam = g["f18d_enh"]
    assert abs(rt.S.calculate_comprehensive_similarity(fam[0], [], fam[2], 7) - g["f18d_score"][0, 2]) <= 1e-12
    assert rt.S.calculate_embedding_similarity(np.zeros((0, 8)), {1: fam[0]}) == []
    assert rt.S.calculate_embedding_similarity(fam[0], {}) == []
    assert rt.S.similarity_weights() == {"hierarchical": 0.5, "embedding": 0.3, "spatial": 0.2}


# --------------------------------------------------------------------------------------------- fused route
def test_layout_matches_the_model(rt):
    for H, W, h in ((67, 64, 65), (34, 32, 32), (18, 16, 17), (9, 8, 8), (15, 16, 14), (5, 4, 5)):
        lay = rt.K.comp_layout(H, W, h)
        ws, st, ni, nj = C.windows(h, W)
        assert (lay["K"], lay["L"], lay["ws"], lay["stride"], lay["ni"], lay["nj"]) == \
            (C.composite_k(H, W, h), H - h, ws, st, ni, nj)
        nw, we = ni * nj, (ws * ws if ws else h * W)
        assert [lay[f] for f in ("off_win", "off_orig", "off_levels", "off_const", "off_orig_ind", "off_win_ind")] == \
            [0, nw * we, nw * we + h * W, nw * we + H * W, nw * we + H * W + 1, nw * we + H * W + 2]
        assert lay["off_win_ind"] + nw == lay["K"]


@pytest.mark.parametrize("tag", C.FAMILIES)
def test_fused_scores_match_golden(rt, tag):
    """Every family as float32 frames (the float64 ones narrowed: that moves a score by about 1e-7)."""
    g = C.golden()
    fam = g[f"{tag}_enh"].astype(np.float32)
    h = int(g[f"{tag}_desc"][0, 0])
    q, c, sc = _fused_dense(rt, fam, fam, h)
    assert q.K == c.K == C.composite_k(fam.shape[1], fam.shape[2], h)
    err = np.abs(rt.np(sc) - g[f"{tag}_score"]).max()
    print(tag, "fused max err vs golden", err)
    assert err <= FUSED_TOL


@pytest.mark.parametrize("n,N,Q", C.DENSE_CASES)
def test_fused_scores_match_exact_route(rt, n, N, Q):
    qs, fr = C.store(11, n, N, Q)
    h = C.PROFILE_H[n]
    _, _, sc = _fused_dense(rt, qs, fr, h)
    exact = rt.S.comprehensive_scores(qs, fr)
    err = float((sc - exact).abs().max())
    print(n, N, Q, "fused max err vs comp_scores", err)
    assert err <= FUSED_TOL
    # the exact route itself against the float64 composite model on a corner of the problem
    assert np.abs(rt.np(exact)[:2, :50] - C.composite_scores(qs[:2], fr[:50], h)).max() <= 1e-12


@pytest.mark.parametrize("kind", ("same_sign", "near_duplicate"))
def test_fused_scores_same_sign_and_near_duplicate(rt, kind):
    qs, fr = C.store(12, 32, 48, 3, kind)
    _, _, sc = _fused_dense(rt, qs, fr, 32)
    err = float((sc - rt.S.comprehensive_scores(qs, fr)).abs().max())
    print(kind, "fused max err", err)
    assert err <= FUSED_TOL


def test_prepare_zeroes_pad_rows_and_non_finite_frames(rt):
    qs, fr = C.store(13, 8, 20, 2)
    fr = fr.copy()
    fr[3, 2, 2] = np.nan
    fr[5, 8, 0] = np.inf
    q, c, sc = _fused_dense(rt, qs, fr, 8)
    inv = rt.np(c.inv)
    assert inv[3] == 0.0 and inv[5] == 0.0 and (inv[20:] == 0.0).all() and (inv[[0, 1, 2, 4, 19]] == 1.0).all()
    s = rt.np(sc)
    assert (s[:, [3, 5]] == 0.0).all() and np.isfinite(s).all()
    # the operand itself: fragment (tile, kb, plane) = 64 lanes x 8 halves, lane 16 g + j = row j, k = 32 kb + 8 g + u
    Np, _, Kp = c.X16.shape
    x = rt.np(c.X16.view(-1).double()).reshape(Np // 16, Kp // 32, 2, 4, 16, 8)
    assert (x[1][:, :, :, 4:, :] == 0.0).all() and (x[2:] == 0.0).all()  # rows 20 .. 127 are pad rows
    rows = (x[:, :, 0] + x[:, :, 1]).transpose(0, 3, 1, 2, 4).reshape(Np, Kp)  # hi + lo
    model = C.composite_rows(fr, 8, 1)
    keep = [i for i in range(20) if i not in (3, 5)]
    assert (rows[:20, model.shape[1]:] == 0.0).all()
    assert np.abs(rows[keep, :model.shape[1]] - model[keep]).max() <= 2.0 ** -22
    qrows = rt.np(q.X16.view(-1).double()).reshape(-1, Kp // 32, 2, 4, 16, 8)
    qrows = (qrows[:, :, 0] + qrows[:, :, 1]).transpose(0, 3, 1, 2, 4).reshape(-1, Kp)
    assert np.abs(qrows[:2, :model.shape[1]] - C.composite_rows(qs, 8, 0)).max() <= 2.0 ** -22


# ------------------------------------------------------------------------------------------------- corpus
@pytest.mark.parametrize("n", (8, 32))
def test_corpus_search_ranks_exactly_and_matches_dense_bits(rt, n):
    qs, fr, exact = C.topk_case(n)
    h = C.PROFILE_H[n]
    corpus = rt.S.ComprehensiveFrameCorpus(fr)
    assert corpus.fused and corpus.profile[:2] == (h, fr.shape[1] - h) and len(corpus) == 400
    assert corpus.K == C.composite_k(fr.shape[1], n, h)
    assert corpus.resident_bytes == corpus._rows.X16.numel() * 2 + corpus._rows.inv.numel() * 8
    q, c, dense = _fused_dense(rt, qs, fr, h)
    assert rt.t.equal(corpus.scores(qs), dense)
    for k in C.TOPK_KS:
        s, ids = corpus.search(qs, k)
        assert rt.np(ids).tolist() == C.ranking(exact, k).tolist()
        ws, wi, _, _ = rt.K.select_topk(dense, k)
        assert rt.t.equal(ids, wi) and rt.t.equal(s, ws)
    # threshold form: the frames scoring >= the 5th best, the rest of the list padded
    thr = float(rt.np(dense)[0].max()) - 0.05
    s, ids = corpus.search(qs, 10, threshold=thr)
    ws, wi, _, _ = rt.K.select_topk(dense, 10, thr, 1)
    assert rt.t.equal(ids, wi) and rt.t.equal(s, ws)
    assert bool((s[ids < 0] == float("-inf")).all()) and bool((s[ids >= 0] >= thr).all())
    # k = 100: the dense fused scores and hq_select_topk
    s, ids = corpus.search(qs, 100)
    ws, wi, _, _ = rt.K.select_topk(dense, 100)
    assert rt.t.equal(ids, wi) and rt.t.equal(s, ws)
    # one frame as the query
    s1, i1 = corpus.search(qs[1], 3)
    assert rt.np(i1).tolist() == C.ranking(exact[1:2], 3).tolist()


@pytest.mark.parametrize("n", (8, 32))
def test_corpus_mixed_batch_keeps_each_query_on_its_route(rt, n):
    qs, fr, _ = C.topk_case(n)
    h = C.PROFILE_H[n]
    off = C.off_profile_queries(n)
    batch = np.stack([off[0], qs[0], off[1], qs[1], off[2], qs[2]])
    corpus = rt.S.ComprehensiveFrameCorpus(fr, keep_frames=True)
    assert corpus.fused
    s, ids = corpus.search(batch, 10)
    fs, fi = corpus.search(qs, 10)
    es, ei, _, _ = rt.K.select_topk(rt.S.comprehensive_scores(off, fr), 10)
    assert rt.t.equal(s[1::2], fs) and rt.t.equal(ids[1::2], fi)
    assert rt.t.equal(s[0::2], es) and rt.t.equal(ids[0::2], ei)
    dense = corpus.scores(batch)
    assert rt.t.equal(dense[1::2], corpus.scores(qs)) and rt.t.equal(dense[0::2], rt.S.comprehensive_scores(off, fr))
    # without the raw frames an off-profile query has no route
    with pytest.raises(ValueError, match="keep_frames"):
        rt.S.ComprehensiveFrameCorpus(fr).search(off[:1], 5)


def test_corpus_non_uniform_store_takes_the_exact_route(rt):
    qs, fr, _ = C.topk_case(32)
    mixed = np.concatenate([fr[:60], C.off_profile_queries(32)[2:], fr[60:90]])
    corpus = rt.S.ComprehensiveFrameCorpus(mixed)
    assert corpus.fused is False and corpus.K is None and corpus.profile is None
    want = rt.S.comprehensive_scores(qs, mixed)
    assert rt.t.equal(corpus.scores(qs), want)
    s, ids = corpus.search(qs, 10, threshold=0.4)
    ws, wi, _, _ = rt.K.select_topk(want, 10, 0.4, 1)
    assert rt.t.equal(ids, wi) and rt.t.equal(s, ws)
    # float64 frames are never fused
    g = C.golden()
    c64 = rt.S.ComprehensiveFrameCorpus(g["f18d_enh"])
    assert c64.fused is False
    assert np.abs(rt.np(c64.scores(g["f18d_enh"])) - g["f18d_score"]).max() <= 1e-12


def test_dual_storage_comprehensive_method(rt):
    from hq_mi355x.rag.dual_storage import DocumentChunk, DualStorageCorpus, VideoFrameMetadata
    qs, fr, exact = C.topk_case(8)
    fr, exact = fr[:50], exact[:, :50]
    meta = [VideoFrameMetadata(i, f"c{i}", "h", "d", 0.5, [], "m", 0.0,
                               DocumentChunk("x", "h", "p", 0, 1, i, "t", 1)) for i in range(len(fr))]
    ds = DualStorageCorpus(fr, meta)
    got = ds.search(qs, 5, method="comprehensive")
    assert [[m.frame_index for m, _ in row] for row in got] == C.ranking(exact, 5).tolist()
    want = -np.sort(-exact, axis=1)[:, :5]
    assert np.abs(np.array([[s for _, s in row] for row in got]) - want).max() <= 1e-6
    assert ds.search(qs[:1], 3)[0][0][1] == ds.search(qs[:1], 3, method="spatial")[0][0][1]  # the default is unchanged
    with pytest.raises(ValueError, match="unknown method"):
        ds.scores(qs, "nope")
