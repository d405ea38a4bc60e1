"""Host-side checks of the fused frame-cosine top-k (hq_cos_topk): exports, argument validation, the
workspace bound, and that the case generator of the GPU test discriminates.  No kernel is launched here."""
import ctypes

import numpy as np
import pytest

import costopk_cases as C


@pytest.fixture(scope="module", autouse=True)
def lib():
    """The library with the entry points these inputs are for (every test here needs them to mean anything)."""
    from hq_mi355x import _lib
    l = _lib.load()
    assert hasattr(l, "hq_cos_topk") and hasattr(l, "hq_cos_topk_workspace_size")
    return l


def test_library_exports_cos_topk(lib):
    from hq_mi355x import _lib
    for name, nargs in (("hq_cos_topk_workspace_size", 3), ("hq_cos_topk", 16)):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
    import hq_mi355x.kernels as K
    import hq_mi355x.rag as rag
    from hq_mi355x.rag.dual_storage import DualStorageCorpus
    assert callable(K.cosine_topk) and callable(rag.cosine_topk_batch)
    assert "FrameCosineCorpus" in rag.__all__ and hasattr(DualStorageCorpus, "search_topk")


def test_cos_topk_argument_validation(lib):
    from hq_mi355x import _lib
    one = ctypes.c_void_p(256)  # a non-null address that is never dereferenced: every call returns before a launch

    def call(Q=3, N=5, K=64, k=10, A=one, ia=one, B=one, ib=one, ws=one, wb=1 << 30, os_=one, oi=one):
        return lib.hq_cos_topk(A, ia, Q, B, ib, N, K, k, 0.0, 0, 0, ws, wb, os_, oi, None)

    # empty problems are no-ops before any pointer check
    assert call(Q=0, A=None, ia=None, B=None, ib=None, ws=None, wb=0, os_=None, oi=None) == _lib.HQ_OK
    assert call(N=0, A=None, ia=None, B=None, ib=None, ws=None, wb=0, os_=None, oi=None) == _lib.HQ_OK
    assert call(Q=0, k=100, A=None) == _lib.HQ_OK
    # negative shapes and k < 1
    for kw in (dict(Q=-1), dict(N=-1), dict(K=0), dict(k=0), dict(k=-3)):
        assert call(**kw) == _lib.HQ_E_INVALID, kw
        assert "bad shape" in _lib.last_error()
    # k > 64: the Python layer falls back on this code
    assert call(k=65) == _lib.HQ_E_UNSUPPORTED
    assert "k=65" in _lib.last_error() and "64" in _lib.last_error()
    assert call(k=64, ws=None) == _lib.HQ_E_INVALID  # k = 64 itself passes the limit (null workspace next)
    # null buffers
    for name in ("A", "ia", "B", "ib", "ws", "os_", "oi"):
        assert call(**{name: None}) == _lib.HQ_E_INVALID, name
        assert _lib.last_error() == "null buffer"
    # workspace smaller than the size function says
    need = lib.hq_cos_topk_workspace_size(3, 5, 10)
    assert need > 0
    assert call(wb=need - 1) == _lib.HQ_E_INVALID
    assert _lib.last_error() == "workspace too small"
    # the row-major layout of the superseded kernels is refused with a message
    for code in (1, 2, 3):
        with _lib.option("cos_kernel", code):
            assert call() == _lib.HQ_E_UNSUPPORTED
            assert f"cos_kernel={code}" in _lib.last_error() and "tiled" in _lib.last_error()
    assert _lib.get_option("cos_topk_hint") is None
    with _lib.option("cos_topk_hint", 0):
        assert _lib.get_option("cos_topk_hint") == 0


def test_cos_topk_workspace_is_monotone_and_small(lib):
    size = lib.hq_cos_topk_workspace_size
    assert size(0, 10, 1) == 0 and size(10, 0, 1) == 0 and size(10, 10, 0) == 0
    prev = 0
    for Q in (1, 2, 127, 128, 129, 1000, 5000):
        assert size(Q, 250_000, 10) >= prev
        prev = size(Q, 250_000, 10)
    prev = 0
    for N in (1, 383, 384, 385, 768, 769, 24_576, 24_577, 250_000, 1_000_000, 10_000_000):
        assert size(1000, N, 10) >= prev
        prev = size(1000, N, 10)
    prev = 0
    for k in range(1, 65):
        assert size(1000, 250_000, k) > prev
        prev = size(1000, 250_000, k)
    # the bench's frames shape: 16 Q k N / 384 (+ the merge buffers), a twentieth of the score matrix
    dense = 1000 * 250_000 * 8
    assert size(1000, 250_000, 10) < dense // 16
    assert size(1000, 250_000, 10) >= 1000 * 652 * 10 * 16  # holds the stage-1 slab: 652 tiles of 384 frames


def test_cases_cover_the_shapes():
    assert {c.N for c in C.CASES} >= set(C.NS) | {C.LATE_N}
    assert {c.Q for c in C.CASES} == set(C.QS)
    assert {c.K for c in C.CASES} == set(C.KS)
    assert {c.k for c in C.CASES} >= set(C.TOPKS)
    assert {(c.Q, c.K) for c in C.CASES} >= {(q, k) for q in C.QS for k in C.KS}
    assert any(c.k > c.N for c in C.CASES)
    assert len({c.name for c in C.CASES}) == len(C.CASES)
    assert {c.thr_mode for c in C.CASES} == {0, 1, 2}
    for c in C.CASES:
        A, B = C.build(c)
        assert A.shape == (c.Q, c.K) and B.shape == (c.N, c.K) and A.dtype == B.dtype == np.float32


def test_planted_duplicates_are_bit_ties():
    for c in (x for x in C.CASES if x.kind == "ties"):
        A, B = C.build(c)
        for t, (i, j) in enumerate(C.TIE_PAIRS):
            assert i // 48 != j // 48 and j < c.N
            assert B[i].tobytes() == B[j].tobytes()
            s = C.exact_columns(A, B, (i, j))
            assert s[:, 0].tobytes() == s[:, 1].tobytes()
            # the pair leads its query's list, so the tie is decided inside the returned top k
            full = C.exact_scores(A[t % c.Q: t % c.Q + 1], B)[0]
            assert set(np.argsort(-full)[:2]) == {i, j}
    assert C.TIE_PAIRS[0] == (47, 48) and C.TIE_PAIRS[1] == (383, 384)
    i, j = C.TIE_PAIRS[2]
    assert i // 384 == 0 and j // 384 == 8  # frame tiles 0 and 8: the same XCD, one wrap apart


def test_zero_rows_tie_at_zero():
    for c in (x for x in C.CASES if x.kind == "zeros"):
        A, B = C.build(c)
        s = C.exact_scores(A, B)
        assert np.all(s[:, C.ZERO_FROM:] == 0.0) and np.all(s[C.ZERO_QUERY] == 0.0)
        live = np.delete(s[:, :C.ZERO_FROM], C.ZERO_QUERY, axis=0)
        assert np.all(live > 0.0)
        _, ids = C.reference_topk(s, c.k, 0.0, 0)
        if c.k > C.ZERO_FROM:  # the list runs into the zero rows: ids ascending across the wave boundary 47 | 48
            assert list(ids[0, C.ZERO_FROM:]) == list(range(C.ZERO_FROM, c.k))
        assert list(ids[C.ZERO_QUERY]) == list(range(c.k))


def test_threshold_cases_separate_the_modes():
    seen = set()
    for c in (x for x in C.CASES if x.kind == "thr"):
        A, B = C.build(c)
        s = C.exact_scores(A, B)
        thr = C.threshold_of(c, s)
        tq, r = c.thr_at
        assert np.any(s == thr)                                   # an actual score of the matrix
        ge, gt = int((s[tq] >= thr).sum()), int((s[tq] > thr).sum())
        assert (ge, gt) == (r + 1, r)                             # >= keeps the frame, > drops it
        s1, i1 = C.reference_topk(s, c.k, thr, 1)
        s2, i2 = C.reference_topk(s, c.k, thr, 2)
        assert not np.array_equal(i1[tq], i2[tq])
        seen.add(c.thr_mode)
    assert seen == {1, 2}


def test_few_passers_case_has_fewer_than_k():
    for c in (x for x in C.CASES if x.kind == "few"):
        A, B = C.build(c)
        s = C.exact_scores(A, B)
        n = (s >= c.thr).sum(axis=1)
        assert n[0] == C.FEW_PASS < c.k and np.all(n[1:] < c.k) and np.any(n == 0)
        # no score lies within the kernel's 2e-6 of the threshold: the same frames pass on the MFMA scores
        assert np.min(np.abs(s - c.thr)) > 1e-5


def test_late_winners_lie_in_the_last_tile():
    for c in (x for x in C.CASES if x.kind == "late"):
        A, B = C.build(c)
        assert c.N == C.LATE_N and C.LATE_TILE0 == 384 * ((c.N - 1) // 384)
        s = C.exact_scores(A, B)
        _, ids = C.reference_topk(s, c.k, 0.0, 0)
        assert np.all(ids >= C.LATE_TILE0)
        # ... while every earlier tile holds k frames of its own, one of them good: the hint rises before
        assert np.all(np.sort(s[:, :C.LATE_TILE0], axis=1)[:, -1] > 0.75)
        assert np.all(s[np.arange(c.Q)[:, None], ids][:, -1] > np.max(s[:, :C.LATE_TILE0], axis=1) + 1e-3)
