"""Fused frame-cosine top-k (hq_cos_topk: k_cos_t's top-k epilogue + k_cos_topk_merge) against the dense
route it replaces, select_topk(cosine_scores_mfma(q, c)): ids, order and score bits must be equal; and against
an exact NumPy float64 cosine within the project's measured bound of the split-f16 contraction, 2e-6
(test_cosine_mfma_vs_f64).  Shapes and plants: costopk_cases.py."""
import numpy as np
import pytest

import costopk_cases as C

pytestmark = pytest.mark.gpu

ID_BASES = (0, 10 ** 9)
ERR = 2e-6  # |MFMA score - exact score|


def _np(x):
    return x.detach().cpu().numpy()


_PREPARED = {}


def _prepared(case):
    """Per case, computed once and shared: prepared rows, the dense MFMA scores, the exact scores."""
    import torch
    from hq_mi355x import kernels as K
    if case not in _PREPARED:
        _PREPARED.clear()  # tests run case by case: keep one case's buffers
        A, B = C.build(case)
        pa, pb = K.cos_prepare(torch.tensor(A, device="cuda")), K.cos_prepare(torch.tensor(B, device="cuda"))
        dense = K.cosine_scores_mfma(pa, pb)
        _PREPARED[case] = (pa, pb, dense, C.exact_scores(A, B))
    return _PREPARED[case]


def _equal(got, want, msg):
    gs, gi = _np(got[0]), _np(got[1])
    ws, wi = _np(want[0]), _np(want[1])
    np.testing.assert_array_equal(gi, wi, err_msg=msg)
    assert gs.tobytes() == ws.tobytes(), msg


@pytest.mark.parametrize("case", C.CASES, ids=[c.name for c in C.CASES])
def test_cosine_topk_equals_dense_select(hq_lib, hq_option, case):
    """kernels.cosine_topk == select_topk(cosine_scores_mfma) in ids, order and score bits, id_base 0 and 1e9,
    hint on and off; every score within 2e-6 of the exact score of its id; every frame whose exact score
    exceeds the exact score of the k-th returned id by more than 4e-6 is in the list (no frame exempt)."""
    from hq_mi355x import kernels as K
    pa, pb, dense, exact = _prepared(case)
    thr = C.threshold_of(case, _np(dense))
    if case.thr_at is not None:
        assert (_np(dense) == thr).any()
    for base in ID_BASES:
        want = K.select_topk(dense, case.k, thr, case.thr_mode, base)[:2]
        hq_option("cos_topk_hint", 1)
        on = K.cosine_topk(pa, pb, case.k, thr, case.thr_mode, base)
        hq_option("cos_topk_hint", 0)
        off = K.cosine_topk(pa, pb, case.k, thr, case.thr_mode, base)
        hq_option("cos_topk_hint", None)
        dflt = K.cosine_topk(pa, pb, case.k, thr, case.thr_mode, base)
        _equal(on, want, f"{case.name} hint on, id_base {base}")
        _equal(off, want, f"{case.name} hint off, id_base {base}")
        _equal(dflt, want, f"{case.name} default, id_base {base}")
    # against the exact float64 cosine (id_base 10^9 results, ids shifted back)
    s, ids = _np(dflt[0]), _np(dflt[1])
    have = ids >= 0
    ids0 = np.where(have, ids - ID_BASES[-1], 0)
    ex = np.take_along_axis(exact, ids0, axis=1)
    assert np.all(np.abs(s - ex)[have] <= ERR), float(np.max(np.abs(s - ex)[have]))
    assert np.all(np.isneginf(s[~have]))
    # completeness.  A frame passes the kernel's threshold test on its MFMA score, which is within ERR of the
    # exact one: exact scores above thr + ERR pass for certain, so those are the frames that must be listed
    # when they beat the k-th returned frame by more than 2 ERR (or when the list is not full).
    passing = np.ones_like(exact, bool) if case.thr_mode == 0 else exact > thr + ERR
    full = have[:, -1]
    kth = np.where(full, ex[:, -1], -np.inf)
    must = passing & (exact > (kth + 2 * ERR)[:, None])
    listed = np.zeros_like(must)
    rows = np.repeat(np.arange(case.Q), have.sum(axis=1))
    listed[rows, ids0[have]] = True
    assert not np.any(must & ~listed), np.argwhere(must & ~listed)[:5]
    # no duplicate ids in a row (the clamped last tile must not re-report real rows)
    srt = np.sort(np.where(have, ids, -np.arange(1, ids.shape[1] + 1)[None, :]), axis=1)
    assert np.all(srt[:, 1:] != srt[:, :-1])


def test_query_block_split_equals_unsplit(hq_lib):
    """workspace_limit small enough to force three query blocks: the same lists, fused and dense fallback."""
    import torch
    from hq_mi355x import _lib, kernels as K
    rng = np.random.default_rng(7)
    Q, N, Kd, k = 300, 769, 64, 10
    A = rng.standard_normal((Q, Kd)).astype(np.float32)
    B = rng.standard_normal((N, Kd)).astype(np.float32)
    pa, pb = K.cos_prepare(torch.from_numpy(A).cuda()), K.cos_prepare(torch.from_numpy(B).cuda())
    one = K.cosine_topk(pa, pb, k, id_base=5)
    size = _lib.load().hq_cos_topk_workspace_size
    limit = int(size(128, N, k))  # one 128-query block fits, two do not: 128 + 128 + 44
    assert int(size(256, N, k)) > limit
    _equal(K.cosine_topk(pa, pb, k, id_base=5, workspace_limit=limit), one, "fused, three blocks")
    want = K.select_topk(K.cosine_scores_mfma(pa, pb), 65, 0.0, 0, 5)[:2]
    _equal(K.cosine_topk(pa, pb, 65, id_base=5, workspace_limit=128 * N * 8), want, "dense fallback, three blocks")


def test_k65_fallback_equals_dense(hq_lib):
    import torch
    from hq_mi355x import kernels as K
    case = next(c for c in C.CASES if c.name == "qk-Q129-K64")
    pa, pb, dense, _ = _prepared(case)
    for k in (65, 200):
        _equal(K.cosine_topk(pa, pb, k, 0.45, 2, 3), K.select_topk(dense, k, 0.45, 2, 3)[:2], f"k = {k}")
    with pytest.raises(ValueError, match="query length"):
        K.cosine_topk(K.cos_prepare(torch.zeros((2, 32), device="cuda")), pb, 5)


def test_frame_corpus_and_batch_equal_cosine_topk(hq_lib):
    """FrameCosineCorpus.search and rag.cosine_topk_batch (large float32 problem) == kernels.cosine_topk; a
    small or float64 problem gives select_topk(cosine_scores_batch) as before."""
    import torch
    from hq_mi355x import kernels as K, rag
    rng = np.random.default_rng(9)
    Q, N, H, W, k = 5, 900, 32, 32, 10
    F = rng.standard_normal((N, H, W)).astype(np.float32)
    X = (F[rng.integers(0, N, Q)] + 0.5 * rng.standard_normal((Q, H, W))).astype(np.float32)
    assert Q * N * H * W >= K.MFMA_COS_MIN_WORK
    pa = K.cos_prepare(torch.from_numpy(X.reshape(Q, -1)).cuda())
    pb = K.cos_prepare(torch.from_numpy(F.reshape(N, -1)).cuda())
    corpus = rag.FrameCosineCorpus(F)
    assert (len(corpus), corpus.N, corpus.K) == (N, N, H * W)
    _equal(corpus.search(X, k), K.cosine_topk(pa, pb, k), "corpus.search")
    _equal(corpus.search(X, k, threshold=0.6), K.cosine_topk(pa, pb, k, 0.6, 1), "corpus.search, threshold")
    _equal(corpus.search(X[0], 3), K.cosine_topk(K.cos_prepare(torch.from_numpy(X[:1].reshape(1, -1)).cuda()), pb, 3),
           "one query frame")
    _equal(rag.cosine_topk_batch(X, F, k), K.cosine_topk(pa, pb, k), "cosine_topk_batch, fused")
    _equal(rag.cosine_topk_batch(X, F, k, 0.6), K.cosine_topk(pa, pb, k, 0.6, 1), "cosine_topk_batch, threshold")
    for a, b in ((X[:1, :2], F[:50, :2]), (X.astype(np.float64), F.astype(np.float64))):
        want = K.select_topk(rag.cosine_scores_batch(a, b), k)[:2]
        _equal(rag.cosine_topk_batch(a, b, k), want, f"cosine_topk_batch, {a.dtype} {a.shape}")


def _store(N, H, W, h, rng):
    """Enhanced frames [N, H, W] float32: rows above h hold the embedding; the rows from h down are index rows,
    two values and zeros (more than half zeros: what the height detection of engine.py:134-162 looks for)."""
    from hq_mi355x.rag.dual_storage import DocumentChunk, VideoFrameMetadata
    F = rng.standard_normal((N, H, W)).astype(np.float32)
    F[:, h:, 2:] = 0.0
    meta = []
    for i in range(N):
        ch = DocumentChunk("c", f"h{i}", "p", 0, 1, i, "t", 1)
        meta.append(VideoFrameMetadata(i, f"chunk{i}", f"h{i}", "doc", 0.5, [], "m", 0.0, ch))
    return F, meta


def test_dual_storage_search_topk(hq_lib):
    """search_topk on a float32 store of one height (32 x 32 embeddings, enough frames to pass
    MFMA_COS_MIN_WORK) lists the same frames as search(..., "embedding"), whose scores come from the float64
    kernel: the scores agree within 2e-6 (the MFMA bound), and the order is the same wherever two neighbours of
    the dense list differ by more than 4e-6.  A store of mixed heights takes the dense route: identical lists."""
    from hq_mi355x import kernels as K
    from hq_mi355x.rag import similarity as S
    from hq_mi355x.rag.dual_storage import DualStorageCorpus
    rng = np.random.default_rng(21)
    Q, N, H, W, k = 6, 800, 34, 32, 10
    h = 32
    F, meta = _store(N, H, W, h, rng)
    X = F[rng.integers(0, N, Q)].copy()
    X[:, :h] += (0.7 * rng.standard_normal((Q, h, W))).astype(np.float32)
    hs = S.detect_original_embedding_heights(F)
    hq = S.detect_original_embedding_heights(X)
    assert np.all(hs == h) and np.all(hq == h)
    assert Q * N * h * W >= K.MFMA_COS_MIN_WORK
    corpus = DualStorageCorpus(F, meta)
    got = corpus.search_topk(X, k)
    assert corpus._cos[0] is not None and corpus._cos[0].N == N and corpus._cos[0].K == h * W  # resident, fused
    rows = corpus._cos[0]
    again = corpus.search_topk(X, k)
    assert corpus._cos[0] is rows and again == got  # prepared once
    want = corpus.search(X, k, "embedding")
    assert len(got) == len(want) == Q
    for g, w in zip(got, want):
        assert len(g) == len(w) == k
        ws = np.array([s for _, s in w])
        for (gm, gs), (wm, wsc) in zip(g, w):
            assert abs(gs - wsc) <= ERR
        clear = np.all(np.abs(np.diff(ws)) > 2 * ERR)
        assert clear, "seeded inputs: the dense list's neighbours are more than 4e-6 apart"
        assert [m.frame_index for m, _ in g] == [m.frame_index for m, _ in w]
    thr = float(np.median([s for _, s in want[0]]))
    assert [m.frame_index for m, _ in corpus.search_topk(X[:1].repeat(Q, 0), k, threshold=thr + 1e-4)[0]] == \
        [m.frame_index for m, s in want[0] if s >= thr + 1e-4]
    # mixed heights: the fallback, identical to search()
    F2 = F.copy()
    F2[1::2, h // 2:] = 0.0
    h2 = S.detect_original_embedding_heights(F2)
    assert len(set(h2.tolist())) > 1
    mixed = DualStorageCorpus(F2, meta)
    assert mixed.search_topk(X, k) == mixed.search(X, k, "embedding")
    assert mixed._cos[0] is None
    # float64 frames: the fallback too
    f64 = DualStorageCorpus(F.astype(np.float64), meta)
    assert f64.search_topk(X, 3) == f64.search(X, 3, "embedding")
