"""The mutable device corpus (hq_seg_gather, hq_seg_replace, kernels.seg_gather / seg_replace,
IndexCorpus.remove / replace / select, the engine's shrink_resident switch): a corpus after removals,
replacements or a selection holds the same bytes as one built from the resulting rows, answers every search bit
for bit like it, and equals the CPU oracle.

Oracle parity is this suite's standard (tests/test_gpu_search.py): identical ids and order, scores within
TOL = 1e-10 of the reference NumPy path.  Mutated-against-fresh comparisons are exact (torch.equal, bytes)."""
import numpy as np
import pytest

import mutate_cases as MC
from oracle import hq_oracle as O

pytestmark = pytest.mark.gpu

TOL = MC.TOL
_np, _t = MC.np_, MC.dev

WHICH = ["L64", "L32", "no_packov", "level0_gt32"]


def _length(lib, which):
    from hq_mi355x import kernels as K
    no_ov, big0 = MC.special_lengths(lib)
    assert no_ov is not None and big0 is not None
    if which == "above4096":
        L = next(L for L in range(4098, 8192, 2) if lib.hq_seg_count(L) > 0)
        assert L > 4096
        return L
    L = {"L64": 64, "L32": 32, "no_packov": no_ov, "level0_gt32": big0}[which]
    if which == "no_packov":
        assert K.packov_info(L) is None
    if which == "level0_gt32":
        assert K.seg_level0_len(L) > 32
    return L


def _ids(rows):
    return _t(np.asarray(rows, dtype=np.int64))


# ---- layout bytes: gather -----------------------------------------------------------------------
@pytest.mark.parametrize("which", WHICH + ["above4096"])
def test_gather_layout_bytes(hq_lib, which):
    from hq_mi355x import kernels as K
    L = _length(hq_lib, which)
    for n, gone in MC.REMOVALS:
        if gone is None:
            gone = MC.seeded_rows(n, 37, n)
        x = MC.rows(n, L, 31 * n + len(gone))
        p = MC.fresh(x)
        sel = np.setdiff1d(np.arange(n), gone)
        g = K.seg_gather(p, _ids(sel))
        assert g.cap == max(p.cap, len(sel)) and g.base is not None and g.base[1].shape[0] == g.cap
        MC.same_layouts(g, MC.fresh(x[sel]))
        MC.same_layouts(p, MC.fresh(x))                       # the source is only read
        if which in ("L64", "L32"):
            assert g.Z16 is not None and g.Zov16 is not None and g.F0 is not None
    # every row gone (the kernels level only): the pad rows and the empty list of a corpus of no rows
    x = MC.rows(5, L, 5)
    g = K.seg_gather(MC.fresh(x), _ids([]))
    assert g.N == 0
    MC.same_layouts(g, MC.fresh(x[:0]))


@pytest.mark.parametrize("which", ["L64", "L32"])
def test_gather_permutation_repeats_and_capacity(hq_lib, which):
    from hq_mi355x import kernels as K
    L = _length(hq_lib, which)
    x = MC.rows(70, L, 70)
    rng = np.random.default_rng(7)
    sel = np.concatenate([rng.permutation(70), [3, 3, 69, 0, 3], rng.integers(0, 70, 22)])   # 97 rows > N
    p = MC.fresh(x)
    g = K.seg_gather(p, _ids(sel))
    assert g.N == 97 and g.cap == 97
    MC.same_layouts(g, MC.fresh(x[sel]))
    assert len(MC.flagged(g)) > len(MC.flagged(p))            # repeated degenerate rows are listed once each
    # a source whose buffers hold more rows than it has; the result keeps that capacity, or the one asked for
    big = K.seg_reserve(MC.fresh(x), 300)
    assert big.cap == 300
    keep = np.setdiff1d(np.arange(70), [0, 16, 17, 69])
    g = K.seg_gather(big, _ids(keep))
    assert g.cap == 300
    MC.same_layouts(g, MC.fresh(x[keep]))
    g = K.seg_gather(big, keep, cap=80)                       # host row numbers work too
    assert g.cap == 80
    MC.same_layouts(g, MC.fresh(x[keep]))
    with pytest.raises(IndexError):
        K.seg_gather(big, _ids([0, 70]))
    with pytest.raises(IndexError):
        K.seg_gather(big, [-1])


@pytest.mark.parametrize("which", WHICH)
def test_remove_then_append_round_trip(hq_lib, which):
    """The pad rows and partial tiles / groups the gather leaves are what hq_seg_append builds on."""
    from hq_mi355x import kernels as K
    L = _length(hq_lib, which)
    for n, gone, m in ((17, [0], 5), (17, [16], 1), (65, list(range(64)), 20), (200, MC.seeded_rows(200, 37, 2), 30),
                       (33, list(range(0, 33, 2)), 40)):
        x = MC.rows(n + m, L, n + m)
        sel = np.setdiff1d(np.arange(n), gone)
        g = K.seg_gather(MC.fresh(x[:n]), _ids(sel))
        cap0 = g.cap
        g = K.seg_append(g, _t(x[n:]))
        assert (g.cap == cap0) == (len(sel) + m <= cap0)      # inside the capacity: no reallocation
        final = np.concatenate([x[sel], x[n:]])
        MC.same_layouts(g, MC.fresh(final))


@pytest.mark.parametrize("L", [64, 32])
def test_gather_mixed_float32(hq_lib, L):
    from hq_mi355x import kernels as K
    from hq_mi355x.core.search_engine import IndexCorpus
    for n0, m in [(15, 2), (17, 33)]:
        n = n0 + m
        tail32 = np.concatenate([np.zeros(n0, bool), np.ones(m, bool)])
        alt = np.arange(n) % 3 == 0
        for flags in (tail32, ~tail32, alt):
            x = MC.rows(n, L, 7 * n0 + m)
            x[flags] = x[flags].astype(np.float32).astype(np.float64)
            p = MC.fresh(x, flags)
            assert p.f32 and not p.all32
            some = np.setdiff1d(np.arange(n), [0, n0 - 1, n0, n - 1])
            g = K.seg_gather(p, _ids(some))
            MC.same_layouts(g, MC.fresh(x[some], flags[some]))
            g = K.seg_gather(p, _ids(np.flatnonzero(~flags)))  # every float32 row removed
            assert g.f32 is False and g.all32 is False
            MC.same_layouts(g, MC.fresh(x[~flags], flags[~flags]))
            g = K.seg_gather(p, _ids(np.flatnonzero(flags)))   # every float64 row removed
            assert g.f32 is True and g.all32 is True
            MC.same_layouts(g, MC.fresh(x[flags], flags[flags]))
    # an all-float32 corpus stays so
    x = MC.rows(21, L, 21, f32=True)
    corpus = IndexCorpus(x.astype(np.float32))
    assert corpus.prep.all32 and corpus.remove([4, 20]) == 19 and corpus.prep.f32 and corpus.prep.all32
    MC.same_layouts(corpus.prep, IndexCorpus(np.delete(x, [4, 20], axis=0).astype(np.float32)).prep)
    # dense_only because of one float32 row whose squares underflow in float32: gone with that row
    x = MC.rows(40, L, 3)
    flags = np.arange(40) >= 30
    x[flags] = x[flags].astype(np.float32).astype(np.float64)
    x[37] = np.float32(1e-20)
    x[37, 0] = np.float32(2e-20)
    corpus = IndexCorpus(x, row_f32=flags)
    assert corpus.dense_only
    assert corpus.remove([2, 31]) == 38 and corpus.dense_only  # the row is still there
    assert corpus.remove([35]) == 37 and not corpus.dense_only  # row 37 is row 35 by now
    keep = np.setdiff1d(np.arange(40), [2, 31, 37])
    fresh = IndexCorpus(x[keep], row_f32=flags[keep])
    assert not fresh.dense_only
    MC.same_layouts(corpus.prep, fresh.prep)
    q = x[[3, 33, 36]] + 1e-3
    for a, b in zip(corpus.progressive(q, 5, 0.1, 20), fresh.progressive(q, 5, 0.1, 20)):
        assert np.array_equal(_np(a), _np(b), equal_nan=True)


# ---- layout bytes: replace ----------------------------------------------------------------------
@pytest.mark.parametrize("which", WHICH)
def test_replace_layout_bytes(hq_lib, which):
    from hq_mi355x import kernels as K
    L = _length(hq_lib, which)
    for n, rs in MC.REPLACEMENTS:
        if rs is None:
            rs = MC.seeded_rows(n, 40, n)
        x = MC.rows(n, L, 17 * n)
        new = MC.swapped_rows(rs, L, n)
        src = _t(x)
        p = K.flag_rows(K.packov(K.pack0(K.seg_prepare(src))))
        before = MC.flagged(p) if p.F0 is not None else None
        g = K.seg_replace(p, _ids(rs), _t(new))
        assert _np(src).tobytes() == x.tobytes()              # the caller's tensor keeps its rows
        x2 = x.copy()
        x2[rs] = new
        MC.same_layouts(g, MC.fresh(x2))
        if which in ("L64", "L32") and n == 200:             # (the other lengths may flag every row)
            after = MC.flagged(g)
            assert after - before and before - after          # rows entered the flagged-row list, and left it
        g2 = K.seg_replace(g, rs[::-1], _t(x[rs[::-1]]))      # back again, rows given on the host, other order
        MC.same_layouts(g2, MC.fresh(x))
    with pytest.raises(ValueError):
        K.seg_replace(g2, _ids([1, 1]), _t(x[:2]))
    with pytest.raises(IndexError):
        K.seg_replace(g2, _ids([n]), _t(x[:1]))


@pytest.mark.parametrize("L", [64, 32])
def test_replace_mixed_float32(hq_lib, L):
    from hq_mi355x import kernels as K
    n = 63
    flags = np.arange(n) % 3 == 0
    x = MC.rows(n, L, 63)
    x[flags] = x[flags].astype(np.float32).astype(np.float64)
    rs = [3, 4, 62]                                           # float32 -> float64, float64 -> float32, -> float32
    nf = np.array([False, True, True])
    new = MC.swapped_rows(rs, L, 5)
    new[nf] = new[nf].astype(np.float32).astype(np.float64)
    g = K.seg_replace(MC.fresh(x, flags), _ids(rs), _t(new), row_f32=nf)
    x2, f2 = x.copy(), flags.copy()
    x2[rs], f2[rs] = new, nf
    assert g.f32 and not g.all32
    MC.same_layouts(g, MC.fresh(x2, f2))
    # the only float32 row replaced by a float64 one, and the only float64 row by a float32 one
    one = np.arange(5) == 2
    y = MC.rows(5, L, 55)
    y[2] = y[2].astype(np.float32).astype(np.float64)
    g = K.seg_replace(MC.fresh(y, one), [2], _t(new[:1]), row_f32=[False])
    y2 = y.copy()
    y2[2] = new[0]
    assert not g.f32 and not g.all32
    MC.same_layouts(g, MC.fresh(y2, np.zeros(5, bool)))
    y32 = MC.rows(5, L, 56, f32=True)
    g = K.seg_replace(MC.fresh(y32, ~one), [2], _t(y32[2:3]), row_f32=[True])
    assert g.f32 and g.all32
    MC.same_layouts(g, MC.fresh(y32, np.ones(5, bool)))


def test_corpus_edits_above_4096(hq_lib):
    """Index vectors longer than hq_seg_replace takes: replace rebuilds from the updated raw rows (as append
    does), remove and select gather as at any length."""
    from hq_mi355x.core.search_engine import IndexCorpus
    L = _length(hq_lib, "above4096")
    x = MC.rows(9, L, 9)
    new = MC.swapped_rows([0, 8], L, 1)
    corpus = IndexCorpus(x)
    assert corpus.replace([0, 8], new) == 9
    x2 = x.copy()
    x2[[0, 8]] = new
    MC.same_layouts(corpus.prep, IndexCorpus(x2).prep)
    assert corpus.remove([1, 8]) == 7
    keep = [0, 2, 3, 4, 5, 6, 7]
    MC.same_layouts(corpus.prep, IndexCorpus(x2[keep]).prep)
    MC.same_layouts(corpus.select([6, 0, 0]).prep, IndexCorpus(x2[keep][[6, 0, 0]]).prep)


# ---- searches -----------------------------------------------------------------------------------
def _equal_searches(a, b, Q):
    import torch
    for M in (20, 100):
        for u, v in zip(a.progressive(Q, 10, 0.1, M), b.progressive(Q, 10, 0.1, M)):
            assert torch.equal(u, v), M
    for u, v in zip(a.brute_force(Q, 10), b.brute_force(Q, 10)):
        assert torch.equal(u, v)
    for u, v in zip(a.frame_search(Q, 10, 0.1), b.frame_search(Q, 10, 0.1)):
        assert torch.equal(u, v)


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


def _equals_fresh_and_oracle(corpus, C, Q, base):
    """corpus answers like a fresh corpus of the rows C (bit for bit) and like the oracle over C."""
    from hq_mi355x.core.search_engine import IndexCorpus
    assert corpus.N == len(C) and corpus.id_base == base
    _equal_searches(corpus, IndexCorpus(C, id_base=base), Q)
    for M in (20, 100):
        _oracle_progressive(corpus, Q, C, M, base)
    bids, bov, _ = (_np(t) for t in corpus.brute_force(Q, 10))
    fids, fsc = (_np(t) for t in corpus.frame_search(Q, 10, 0.1))
    for a in range(len(Q)):
        rid, rsc, _ = O.brute_force_search(Q[a], C, 10)
        assert list(bids[a]) == [base + i for i in rid]
        np.testing.assert_allclose(bov[a], rsc, atol=TOL)
        rid, rsc = O.hierarchical_frame_search(Q[a], C, 10, 0.1)
        assert list(fids[a][: len(rid)]) == [base + i for i in rid] and all(fids[a][len(rid):] == -1)
        np.testing.assert_allclose(fsc[a][: len(rid)], rsc, atol=TOL)


BASE, NS = 1000, 317


def _search_case():
    C = MC.rows(NS, 64, NS)
    rng = np.random.default_rng(NS + 1)
    plain = [i for i in range(NS) if MC.kind(i) == "plain"]
    gone = MC.seeded_rows(NS, 17, 17)
    victim = next(i for i in gone if MC.kind(i) == "plain")           # removed: its near-duplicate query stays
    stays = max(i for i in plain if i not in gone)                    # survives under a smaller id
    pick = [victim, stays] + list(rng.choice(plain, 3, replace=False))
    Q = C[pick] + rng.normal(0, 0.01, (len(pick), 64))
    return C, Q, gone, victim, stays


def test_remove_searches_equal_fresh_and_oracle(hq_lib):
    from hq_mi355x.core.search_engine import IndexCorpus
    C, Q, gone, victim, stays = _search_case()
    corpus = IndexCorpus(C, id_base=BASE)
    assert _np(corpus.progressive(Q[:2], 1, 0.1, 20)[0])[:, 0].tolist() == [BASE + victim, BASE + stays]
    assert corpus.remove(np.array(gone + gone[:3])) == NS - 17          # duplicates are tolerated
    orig = np.setdiff1d(np.arange(NS), gone)                          # original row of every survivor
    _equals_fresh_and_oracle(corpus, C[orig], Q, BASE)
    ids = _np(corpus.progressive(Q[:2], 10, 0.1, 20)[0])
    assert victim not in orig[ids[0][ids[0] >= 0] - BASE]             # the removed row is not returned any more
    new_id = BASE + int(np.searchsorted(orig, stays))
    assert new_id < BASE + stays and ids[1, 0] == new_id              # the survivor, under its new id
    # 64 more, as a device tensor of local row numbers of the corpus as it is now
    local = MC.seeded_rows(NS - 17, 64, 64)
    assert corpus.remove(_ids(local)) == NS - 81
    orig = np.delete(orig, local)
    _equals_fresh_and_oracle(corpus, C[orig], Q, BASE)
    MC.same_layouts(corpus.prep, IndexCorpus(C[orig]).prep)
    assert corpus.remove([]) == NS - 81


def test_replace_searches_equal_fresh_and_oracle(hq_lib):
    from hq_mi355x.core.search_engine import IndexCorpus
    C, Q, gone, victim, stays = _search_case()
    corpus = IndexCorpus(C, id_base=BASE)
    rs = sorted(set(gone) | {stays - 1})
    new = MC.swapped_rows(rs, 64, 9)
    assert corpus.replace(rs, new) == NS
    C2 = C.copy()
    C2[rs] = new
    _equals_fresh_and_oracle(corpus, C2, Q, BASE)
    MC.same_layouts(corpus.prep, IndexCorpus(C2).prep)
    ids = _np(corpus.progressive(np.stack([Q[0], new[0] + 1e-4]), 1, 0.1, 20)[0])
    assert ids[0, 0] != BASE + victim and ids[1, 0] == BASE + rs[0]   # the old vector is gone, the new one found
    assert np.array_equal(C, MC.rows(NS, 64, NS))                     # the caller's rows are untouched
    # a device tensor the corpus was built from keeps its rows too
    src = _t(C)
    corpus = IndexCorpus(src)
    corpus.replace(_ids(rs), _t(new))
    assert _np(src).tobytes() == C.tobytes()
    MC.same_layouts(corpus.prep, IndexCorpus(C2).prep)


def test_select_searches_equal_fresh_and_oracle(hq_lib):
    from hq_mi355x.core.search_engine import IndexCorpus
    C, Q, gone, victim, stays = _search_case()
    corpus = IndexCorpus(C, id_base=BASE)
    rng = np.random.default_rng(3)
    sel = np.concatenate([[victim, stays], rng.permutation(NS)[:120], [victim, 5, 5]])   # any order, repeats
    sub = corpus.select(sel, id_base=77)
    assert sub is not corpus and sub.N == len(sel) and corpus.N == NS and corpus.id_base == BASE
    _equals_fresh_and_oracle(sub, C[sel], Q, 77)
    MC.same_layouts(sub.prep, IndexCorpus(C[sel]).prep)
    assert _np(sub.progressive(Q[:2], 1, 0.1, 20)[0])[:, 0].tolist() == [77, 78]   # ties: the first copy
    # independent: writing to either leaves the other as it was
    sub.remove([0, 1])
    corpus.remove(gone)
    MC.same_layouts(sub.prep, IndexCorpus(C[sel[2:]]).prep)
    MC.same_layouts(corpus.prep, IndexCorpus(np.delete(C, gone, axis=0)).prep)
    assert corpus.select(_ids([4]), id_base=3).N == 1


def test_shrink_across_sample_threshold_switch(hq_lib):
    """65,600 -> 65,530 rows: downwards across the 16 x 4096-row switch between the sampled and the provable
    starting threshold of the level-0 scan (hq_mi355x.h)."""
    import torch
    from hq_mi355x.core.search_engine import IndexCorpus
    rng = np.random.default_rng(66)
    C = rng.standard_normal((65600, 64)) * 0.5 + 0.1
    C[65531] = 0.25
    C[65540, :32] = 0.5
    gone = np.concatenate([rng.choice(65500, 60, replace=False), np.arange(65590, 65600)])
    keep = np.setdiff1d(np.arange(65600), gone)
    pick = np.concatenate([rng.choice(keep, 48, replace=False), keep[-16:]])
    Q = C[pick] + rng.normal(0, 0.01, (64, 64))
    corpus = IndexCorpus(C)
    corpus.progressive(Q, 10, 0.1, 20)                       # a search above the switch first
    assert corpus.remove(gone) == 65530
    fresh = IndexCorpus(C[keep])
    for a, b in zip(corpus.progressive(Q, 10, 0.1, 20), fresh.progressive(Q, 10, 0.1, 20)):
        assert torch.equal(a, b)
    MC.same_layouts(corpus.prep, fresh.prep)
    _oracle_progressive(corpus, Q[[0, 17, 50, 63]], C[keep], 20)


# ---- the writer rule, streams, argument errors ----------------------------------------------------
def test_remove_and_replace_are_writers(hq_lib):
    import torch
    from hq_mi355x.core.search_engine import IndexCorpus
    C = MC.rows(340, 64, 9)
    Q = C[:4] + 1e-3
    corpus = IndexCorpus(C)
    p = corpus.progressive_submit(Q, 10, 0.1, 20)
    assert p.done is None                                  # queued, not finished
    with pytest.raises(RuntimeError):
        corpus.remove([5])
    with pytest.raises(RuntimeError):
        corpus.replace([5], C[:1])
    assert corpus.N == 340
    corpus.progressive_finish(p)
    assert corpus.replace([5], C[6:7]) == 340
    assert corpus.remove([7, 339]) == 338
    C2 = C.copy()
    C2[5] = C[6]
    fresh = IndexCorpus(np.delete(C2, [7, 339], axis=0))
    for a, b in zip(corpus.progressive(Q, 10, 0.1, 20), fresh.progressive(Q, 10, 0.1, 20)):
        assert torch.equal(a, b)
    sub = corpus.select([1, 2, 3])                         # select is a reader: allowed while a batch is out
    p = corpus.progressive_submit(Q, 10, 0.1, 20)
    assert corpus.select([1, 2, 3]).N == sub.N == 3
    corpus.progressive_finish(p)


def test_remove_on_side_stream_orders_later_searches(hq_lib):
    import torch
    from hq_mi355x.core.search_engine import IndexCorpus
    rng = np.random.default_rng(13)
    C = rng.standard_normal((20300, 64)) * 0.5 + 0.1
    gone = rng.choice(20300, 300, replace=False)
    keep = np.setdiff1d(np.arange(20300), gone)
    Q = C[keep[[5, 299, 300, 10000, 19999]]] + rng.normal(0, 0.01, (5, 64))
    want = IndexCorpus(C[keep]).progressive(Q, 10, 0.1, 20)
    corpus = IndexCorpus(C)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        assert corpus.remove(gone) == 20000
    got = corpus.progressive(Q, 10, 0.1, 20)               # default stream, no host sync in between
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    torch.cuda.synchronize()


def test_argument_errors_launch_nothing(hq_lib):
    from hq_mi355x.core.search_engine import IndexCorpus
    C = MC.rows(30, 64, 30)
    corpus = IndexCorpus(C, id_base=5)
    prep = corpus.prep
    for bad in ([30], [-1], [0, 31], np.array([29, 30]), _ids([3, 30])):
        with pytest.raises(IndexError):
            corpus.remove(bad)
        with pytest.raises(IndexError):
            corpus.replace(bad, C[:len(bad)])
        with pytest.raises(IndexError):
            corpus.select(bad)
    with pytest.raises(ValueError):
        corpus.remove(np.arange(30))                       # nothing would be left
    with pytest.raises(ValueError):
        corpus.remove(list(range(30)) + [3, 3])
    with pytest.raises(ValueError):
        corpus.replace([4, 4], C[:2])                      # repeated rows
    with pytest.raises(ValueError):
        corpus.replace([4, 5], np.zeros((2, 32)))          # another index length
    with pytest.raises(ValueError):
        corpus.replace([4, 5], C[:3])                      # one vector per row
    with pytest.raises(ValueError):
        corpus.replace([4, 5], C[:2], row_f32=[True])
    assert corpus.prep is prep and corpus.N == 30 and corpus.id_base == 5
    MC.same_layouts(corpus.prep, IndexCorpus(C).prep)


# ---- the registry -------------------------------------------------------------------------------
def test_registry_search_shrinks(hq_lib):
    """tests/test_gpu_append.py::test_registry_search_appends with shrink_resident=True: a removal costs a
    shrink and an append, not a rebuild."""
    from hq_mi355x.api import HilbertQuantizer
    rng = np.random.default_rng(40)
    P = rng.standard_normal((40, 1024)).astype(np.float32)
    hq = HilbertQuantizer(use_precomputed_indexing=False, shrink_resident=True)
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

    eng = hq.search_engine
    check(P[3] + rng.normal(0, 0.01, 1024).astype(np.float32))
    for i in range(5):
        check(P[5 + i] + rng.normal(0, 0.01, 1024).astype(np.float32))
    assert eng.pool_stats == {"builds": 1, "appends": 5} and eng.pool_shrinks == 0
    corpus = eng._pool_cache[1]
    assert hq.remove_model_from_registry("m20") is True
    check(P[30] + rng.normal(0, 0.01, 1024).astype(np.float32))
    assert eng.pool_stats == {"builds": 1, "appends": 6} and eng.pool_shrinks == 1
    assert eng._pool_cache[1] is corpus and corpus.N == len(hq._model_registry) == 46
    check(P[31] + rng.normal(0, 0.01, 1024).astype(np.float32))       # and goes on appending
    assert eng.pool_stats == {"builds": 1, "appends": 7} and eng.pool_shrinks == 1
    assert corpus.N == len(hq._model_registry) == 47
    # the first and the last model in one go
    assert hq.remove_model_from_registry("m0") is True
    del hq._model_registry[-1]
    check(P[32] + rng.normal(0, 0.01, 1024).astype(np.float32))
    assert eng.pool_stats == {"builds": 1, "appends": 8} and eng.pool_shrinks == 2
    assert eng._pool_cache[1] is corpus and corpus.N == len(hq._model_registry) == 46
    assert all(a is m.hierarchical_indices for a, m in zip(eng._pool_cache[0], hq._model_registry))
