"""The appendable device corpus (hq_seg_append, kernels.seg_append, IndexCorpus.append / reserve, the
engine's pool cache and HilbertQuantizer's registry): a corpus grown by appends holds the same bytes as
one built from the same rows, answers every search bit for bit like it, and equals the CPU oracle.

Oracle parity is this suite's standard (tests/test_gpu_search.py): identical ids and order, scores within
TOL = 1e-10 of the reference NumPy path.  Grown-against-fresh comparisons are exact (torch.equal)."""
import ctypes

import numpy as np
import pytest

from oracle import hq_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-10
PAD0 = 48

# (resident rows, appended rows); the last one grows in chunks from a small capacity (two reallocations)
PAIRS = [(1, 1), (3, 1), (4, 4), (15, 1), (15, 2), (16, 1), (17, 33), (63, 130), (0, 5), (5, 200)]


def _np(x):
    from hq_mi355x._dev import to_np
    return to_np(x)


def _t(x):
    from hq_mi355x._dev import to_dev
    return to_dev(x)


def _special_lengths(lib):
    """(an L without a split overall layout, an L whose level-0 segment exceeds 32 values), L <= 1024.
    The first prefers an L that still has the level-0 copies, so both halves of the kernel are told apart."""
    no_ov, big0 = [], []
    v = [ctypes.c_int() for _ in range(4)]
    for L in range(2, 1025, 2):
        if lib.hq_seg_count(L) <= 0:
            continue
        l0 = lib.hq_seg_level0_len(L)
        if l0 > 32:
            big0.append(L)
        elif lib.hq_seg_packov_info(L, *[ctypes.byref(x) for x in v]) != 0:
            no_ov.append(L)
    return (no_ov[0] if no_ov else None), (big0[0] if big0 else None)


def _rows(n, L, seed, f32=False):
    """Seeded index rows with the degenerate shapes the layouts flag: constant rows, zero rows, rows whose
    level-0 segment has zero variance — spread so that resident and appended parts both get some."""
    rng = np.random.default_rng(seed)
    C = rng.standard_normal((n, L)) * 0.5 + 0.1
    a, b = O.segment_bounds(L)[0]
    for i in range(n):
        if i % 7 == 3:
            C[i] = 0.25
        elif i % 11 == 5:
            C[i] = 0.0
        elif i % 5 == 1:
            C[i, a:b] = -0.75
    if f32:
        C = C.astype(np.float32).astype(np.float64)
    return C


def _fresh(x, flags=None):
    from hq_mi355x import kernels as K
    return K.flag_rows(K.packov(K.pack0(K.seg_prepare(_t(x), row_f32=flags))))


def _grown(x, n0, flags=None, chunk=None, reserve=None):
    from hq_mi355x import kernels as K
    p = _fresh(x[:n0], None if flags is None else flags[:n0])
    if reserve:
        p = K.seg_reserve(p, reserve)
    caps = [p.cap]
    step = chunk or (len(x) - n0)
    for s in range(n0, len(x), step):
        e = min(s + step, len(x))
        p = K.seg_append(p, _t(x[s:e]), row_f32=None if flags is None else flags[s:e])
        caps.append(p.cap)
    return p, caps


def _same_layouts(g, f):
    """Every valid extent of the grown Prepared g equals the fresh one f (hq_mi355x.h: hq_seg_append)."""
    N = f.N
    assert g.N == N and g.R.shape[0] == N and g.Z.shape[0] == N and g.S.shape[0] == N
    assert (g.f32, g.all32) == (f.f32, f.all32)
    r16, r4 = (N + 15) // 16 * 16 + PAD0, (N + 3) // 4 * 4 + PAD0
    for name, rows in (("R", N), ("Z", N), ("S", N), ("Z16", r16), ("S32", r4), ("Zov16", r16), ("Sov32", r4 // 4)):
        a, b = getattr(g, name), getattr(f, name)
        assert (a is None) == (b is None), name
        if b is None:
            continue
        assert b.shape[0] == rows and a.shape[0] >= rows, name
        assert _np(a[:rows]).tobytes() == _np(b[:rows]).tobytes(), name
    assert (g.F0 is None) == (f.F0 is None)
    if f.F0 is not None:
        ga, fa = _np(g.F0), _np(f.F0)
        assert ga[0] == fa[0]
        assert sorted(ga[1:1 + ga[0]]) == sorted(fa[1:1 + fa[0]])


def test_special_lengths_exist(hq_lib):
    no_ov, big0 = _special_lengths(hq_lib)
    assert no_ov is not None, "no L <= 1024 without a split overall layout"
    assert big0 is not None, "no L <= 1024 with a level-0 segment of more than 32 values"


@pytest.mark.parametrize("which", ["L64", "L32", "no_packov", "level0_gt32"])
def test_layout_bytes(hq_lib, which):
    from hq_mi355x import kernels as K
    no_ov, big0 = _special_lengths(hq_lib)
    assert no_ov is not None and big0 is not None
    L = {"L64": 64, "L32": 32, "no_packov": no_ov, "level0_gt32": big0}[which]
    if which == "no_packov":
        assert K.packov_info(L) is None
    if which == "level0_gt32":
        assert K.seg_level0_len(L) > 32
    for n0, m in PAIRS:
        x = _rows(n0 + m, L, 100 * n0 + m)
        f = _fresh(x)
        if (n0, m) == (5, 200):
            g, caps = _grown(x, n0, chunk=50, reserve=8)
            assert caps[0] == 8 and len(set(caps)) >= 3, caps     # at least two reallocations
            assert all(b >= 2 * a for a, b in zip(caps, caps[1:]) if b != a), caps  # geometric
        else:
            g, caps = _grown(x, n0)
        assert g.cap >= g.N
        _same_layouts(g, f)
        if which in ("L64", "L32"):
            assert g.Z16 is not None and g.Zov16 is not None and g.F0 is not None
            assert int(_np(g.F0)[0]) > 0 or n0 + m < 4            # the degenerate rows are listed
        # rows() keeps working on prefix views
        sel = _t(np.arange(0, n0 + m, 2, dtype=np.int64))
        assert _np(g.rows(sel).Z).tobytes() == _np(f.rows(sel).Z).tobytes()


@pytest.mark.parametrize("L", [64, 32])
def test_layout_bytes_mixed_float32(hq_lib, L):
    from hq_mi355x.core.search_engine import IndexCorpus
    for n0, m in [(15, 2), (17, 33), (63, 130)]:
        n = n0 + m
        tail32 = np.concatenate([np.zeros(n0, bool), np.ones(m, bool)])
        head32 = ~tail32
        alt = np.arange(n) % 3 == 0
        for flags in (tail32, head32, alt):
            x = _rows(n, L, 7 * n0 + m)
            x[flags] = x[flags].astype(np.float32).astype(np.float64)
            g, _ = _grown(x, n0, flags=flags)
            _same_layouts(g, _fresh(x, flags))
    # an f32 tail whose squares underflow in float32: outside the scans' model -> dense exact path
    x = _rows(40, L, 3)
    flags = np.arange(40) >= 30
    x[flags] = x[flags].astype(np.float32).astype(np.float64)
    corpus = IndexCorpus(x[:30])
    assert not corpus.dense_only
    assert corpus.append(x[30:36], row_f32=flags[30:36]) == 36 and not corpus.dense_only
    x[37] = np.float32(1e-20)
    x[37, 0] = np.float32(2e-20)
    assert corpus.append(x[36:], row_f32=flags[36:]) == 40
    assert corpus.dense_only
    fresh = IndexCorpus(x, row_f32=flags)
    assert fresh.dense_only
    _same_layouts(corpus.prep, fresh.prep)
    q = x[[2, 33, 37]] + 1e-3
    for a, b in zip(corpus.progressive(q, 5, 0.1, 20), fresh.progressive(q, 5, 0.1, 20)):
        assert np.array_equal(_np(a), _np(b), equal_nan=True)


def _equal_searches(grown, fresh, Q):
    import torch
    for M in (20, 100):
        for a, b in zip(grown.progressive(Q, 10, 0.1, M), fresh.progressive(Q, 10, 0.1, M)):
            assert torch.equal(a, b), M
    for a, b in zip(grown.brute_force(Q, 10), fresh.brute_force(Q, 10)):
        assert torch.equal(a, b)
    for a, b in zip(grown.frame_search(Q, 10, 0.1), fresh.frame_search(Q, 10, 0.1)):
        assert torch.equal(a, b)


def _oracle_progressive(corpus, Q, C, M, base=0):
    ids, ov, lv, cnt = (_np(t) for t in corpus.progressive(Q, 10, 0.1, M))
    worst = 0.0
    for a in range(len(Q)):
        rid, rsc, rlv, _ = O.progressive_search(Q[a], C, 10, 0.1, M)
        assert list(ids[a][: cnt[a]]) == [base + i for i in rid], a
        assert all(ids[a][cnt[a]:] == -1)
        worst = max(worst, float(np.max(np.abs(ov[a][: cnt[a]] - rsc), initial=0.0)))
        np.testing.assert_allclose(ov[a][: cnt[a]], rsc, atol=TOL)
        np.testing.assert_allclose(lv[a][: cnt[a]], rlv, atol=TOL)
    print(f"progressive M={M} N={len(C)}: max |overall - oracle| = {worst:.3e}")


@pytest.mark.parametrize("n0", [17, 300])
def test_search_equals_fresh_and_oracle(hq_lib, n0):
    from hq_mi355x.core.search_engine import IndexCorpus
    BASE = 1000
    C = _rows(n0 + 64, 64, n0)
    rng = np.random.default_rng(n0 + 1)
    pick = rng.integers(0, len(C), 8)
    Q = C[pick] + rng.normal(0, 0.01, (8, 64))
    grown = IndexCorpus(C[:n0], id_base=BASE)
    n = n0
    for chunk in (1, 16, 47):
        assert grown.append(C[n:n + chunk]) == n + chunk
        n += chunk
        fresh = IndexCorpus(C[:n], id_base=BASE)
        _equal_searches(grown, fresh, Q)
    assert grown.N == len(C) and grown.id_base == BASE
    for M in (20, 100):
        _oracle_progressive(grown, Q, C, M, BASE)
    bids, bov, _ = (_np(t) for t in grown.brute_force(Q, 10))
    fids, fsc = (_np(t) for t in grown.frame_search(Q, 10, 0.1))
    for a in range(8):
        rid, rsc, _ = O.brute_force_search(Q[a], C, 10)
        assert list(bids[a]) == [BASE + i for i in rid]
        np.testing.assert_allclose(bov[a], rsc, atol=TOL)
        rid, rsc = O.hierarchical_frame_search(Q[a], C, 10, 0.1)
        assert list(fids[a][: len(rid)]) == [BASE + i for i in rid] and all(fids[a][len(rid):] == -1)
        np.testing.assert_allclose(fsc[a][: len(rid)], rsc, atol=TOL)
    # appended rows are found under their global ids
    j = max(i for i in range(len(C)) if i % 7 != 3 and i % 11 != 5 and i % 5 != 1)  # the last ordinary row
    assert j >= n0
    ids = _np(grown.progressive(C[j:j + 1], 1, 0.1, 20)[0])
    assert ids[0, 0] == BASE + j


def test_growth_across_sample_threshold_switch(hq_lib):
    """65,530 -> 65,600 rows: across the 16 x 4096-row switch from the provable to the sampled starting
    threshold of the level-0 scan (hq_mi355x.h)."""
    import torch
    from hq_mi355x.core.search_engine import IndexCorpus
    rng = np.random.default_rng(65)
    C = rng.standard_normal((65600, 64)) * 0.5 + 0.1
    C[65531] = 0.25
    C[65540, :32] = 0.5
    pick = np.concatenate([rng.integers(0, 65530, 48), np.arange(65530, 65546)])
    Q = C[pick] + rng.normal(0, 0.01, (64, 64))
    grown = IndexCorpus(C[:65530])
    grown.progressive(Q, 10, 0.1, 20)                      # a search below the switch first
    assert grown.append(C[65530:65540]) == 65540
    assert grown.append(C[65540:]) == 65600
    fresh = IndexCorpus(C)
    for a, b in zip(grown.progressive(Q, 10, 0.1, 20), fresh.progressive(Q, 10, 0.1, 20)):
        assert torch.equal(a, b)
    _same_layouts(grown.prep, fresh.prep)
    sel = [0, 17, 50, 63]
    _oracle_progressive(grown, Q[sel], C, 20)


def test_append_is_a_writer(hq_lib):
    import torch
    from hq_mi355x.core.search_engine import IndexCorpus
    C = _rows(340, 64, 9)
    Q = C[:4] + 1e-3
    corpus = IndexCorpus(C[:300])
    p = corpus.progressive_submit(Q, 10, 0.1, 20)
    assert p.done is None                                  # queued, not finished
    with pytest.raises(RuntimeError):
        corpus.append(C[300:])
    with pytest.raises(RuntimeError):
        corpus.reserve(1000)
    assert corpus.N == 300
    first = corpus.progressive_finish(p)
    assert corpus.progressive_finish(p) is first           # finishing twice counts once
    assert corpus.reserve(1000) >= 1000
    assert corpus.append(C[300:]) == 340
    assert corpus.prep.cap >= 1000                         # no reallocation inside the reserve
    fresh = IndexCorpus(C)
    for a, b in zip(corpus.progressive(Q, 10, 0.1, 20), fresh.progressive(Q, 10, 0.1, 20)):
        assert torch.equal(a, b)
    with pytest.raises(ValueError):
        corpus.append(np.zeros((2, 32)))


def test_append_on_side_stream_orders_later_searches(hq_lib):
    import torch
    from hq_mi355x.core.search_engine import IndexCorpus
    rng = np.random.default_rng(12)
    C = rng.standard_normal((20300, 64)) * 0.5 + 0.1
    Q = C[[5, 299, 300, 10000, 20299]] + rng.normal(0, 0.01, (5, 64))
    fresh = IndexCorpus(C)
    want = fresh.progressive(Q, 10, 0.1, 20)
    corpus = IndexCorpus(C[:300])
    tail = _t(C[300:])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        assert corpus.append(tail) == 20300
    got = corpus.progressive(Q, 10, 0.1, 20)               # default stream, no host sync in between
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    torch.cuda.synchronize()


def test_registry_search_appends(hq_lib):
    """Every registry search quantizes its query into the registry first, so the pool grows by one row per
    call: the first search builds the resident corpus, each later one appends to it.  One search builds,
    the 5 successive ones that follow append."""
    from hq_mi355x.api import HilbertQuantizer
    rng = np.random.default_rng(40)
    P = rng.standard_normal((40, 1024)).astype(np.float32)
    hq = HilbertQuantizer(use_precomputed_indexing=False)
    for i in range(40):
        hq.quantize(P[i], model_id=f"m{i}")
    K_out, thr = hq.max_results, hq.similarity_threshold

    def check(q):
        res = hq.search(q)
        reg = hq._model_registry
        C = np.stack([m.hierarchical_indices for m in reg])
        rid, rsc, _, _ = O.progressive_search(C[-1], C, K_out, thr, 2 * K_out)
        keep = [j for j in range(len(rid)) if min(1.0, max(0.0, rsc[j])) >= thr]
        pos = {id(m): i for i, m in enumerate(reg)}
        assert [pos[id(r.model)] for r in res] == [int(rid[j]) for j in keep]
        np.testing.assert_allclose([r.similarity_score for r in res], np.clip(rsc[keep], 0.0, 1.0), atol=TOL)
        assert res[0].model is reg[-1]                     # the query itself, now registered, ranks first

    check(P[3] + rng.normal(0, 0.01, 1024).astype(np.float32))
    assert hq.search_engine.pool_stats == {"builds": 1, "appends": 0}
    for i in range(5):
        check(P[5 + i] + rng.normal(0, 0.01, 1024).astype(np.float32))
    assert hq.search_engine.pool_stats == {"builds": 1, "appends": 5}
    assert len(hq._model_registry) == 46 and hq.search_engine._pool_cache[1].N == 46
    assert hq.remove_model_from_registry("m20") is True
    check(P[30] + rng.normal(0, 0.01, 1024).astype(np.float32))
    assert hq.search_engine.pool_stats["builds"] == 2
