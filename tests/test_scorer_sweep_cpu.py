"""The oracle's exact scorers and searches against the real reference over the index-length sweep
(tests/golden/scorer_sweep.npz, written by tests/golden/make_golden.py from tests/scorer_sweep_cases.py).

Every score table is compared by dtype, shape and bytes (an 8-byte digest per length and dtype combination,
full arrays at a few lengths), every search by ids and scores, so the GPU tests of
tests/test_gpu_scorer_sweep.py need only the oracle.  Also here: np_sum_rows against NumPy's own reduction at
every length class, the proof that the tables reach every branch of the scorer in every dtype combination and
summation form, and the library's host-side level structure.  Runs anywhere: no reference, no GPU."""
import ctypes

import numpy as np
import pytest

import scorer_sweep_cases as S
from oracle import hq_oracle as O

SUM_LENGTHS = list(range(1, 301)) + [659, 1024, 1025, 2731, 2733]


@pytest.fixture(scope="module")
def g(golden):
    return golden("scorer_sweep")


def test_case_tables_match_the_golden(g):
    assert list(g["LS"]) == S.LS and list(g["LS_FULL"]) == S.LS_FULL and list(g["LS_SEARCH"]) == S.LS_SEARCH
    assert set(S.LS_FULL) <= set(S.LS) and set(S.LS_SEARCH) <= set(S.LS) and len(set(S.LS)) == len(S.LS)
    bad = [L for i, L in enumerate(S.LS) if S.inputs_digest(S.make_rows(L)).tobytes() != g["inputs_dig"][i].tobytes()]
    assert not bad, f"the seeded rows drifted at L={bad[:10]}"
    bad = [L for i, L in enumerate(S.LS_SEARCH)
           if S.inputs_digest(S.make_pool(L)).tobytes() != g["pool_dig"][i].tobytes()]
    assert not bad, f"the seeded pools drifted at L={bad}"
    rows = S.make_rows(66)
    assert rows["C64"].shape == (S.N_ROWS, 66) and rows["Q32"].shape == (S.N_QUERIES, 66)
    assert rows["C32"].dtype == np.float32 and rows["Q64"].dtype == np.float64


def test_segment_lengths_of_the_sweep():
    """The summation forms the issue names all occur: segment lengths 1, 2, 3, 7, 10, 21, 33, 45, 129, 170, 659
    and 2733, and every length class at the first and at a later level."""
    lens = {e - s for L in S.LS for (s, e) in O.segment_bounds(L)}
    assert {1, 2, 3, 7, 10, 21, 33, 45, 129, 170, 659, 2733} <= lens
    assert set(range(1, 65)) <= lens
    first = {S.seg_class(O.segment_bounds(L)[0][1]) for L in S.LS}
    later = {S.seg_class(e - s) for L in S.LS for (s, e) in O.segment_bounds(L)[1:]}
    assert first == later == {"lt8", "leaf", "split"}


@pytest.mark.parametrize("combo", S.COMBOS)
def test_score_tables(g, combo):
    """level_similarity at every level and past the last one, level_types and overall_similarity reproduce the
    reference's values and result types at every length."""
    bad = []
    for i, L in enumerate(S.LS):
        val, ty = S.oracle_tables(*S.combo_inputs(S.make_rows(L), combo))
        if S.digest(val) != g[f"val_dig_{combo}"][i].tobytes() or S.digest(ty) != g[f"type_dig_{combo}"][i].tobytes():
            bad.append(L)
        if L in S.LS_FULL:
            want, wty = g[f"val_{combo}_L{L}"], g[f"type_{combo}_L{L}"]
            assert val.dtype == want.dtype and val.shape == want.shape, L
            diff = np.argwhere(val.view(np.int64) != want.view(np.int64))
            assert len(diff) == 0, f"L={L} {combo}: (query, row, column) {diff[:5].tolist()}"
            assert np.array_equal(ty, wty), f"L={L} {combo}: types at {np.argwhere(ty != wty)[:5].tolist()}"
            assert S.digest(want) == g[f"val_dig_{combo}"][i].tobytes()
            assert S.digest(wty) == g[f"type_dig_{combo}"][i].tobytes()
    assert not bad, f"{combo}: the oracle differs from the reference at L={bad[:20]}"


def test_level_past_the_structure_is_zero(g):
    for L in S.LS_FULL:
        nseg = len(O.segment_bounds(L))
        for combo in S.COMBOS:
            assert not g[f"val_{combo}_L{L}"][:, :, nseg].any() and not g[f"type_{combo}_L{L}"][:, :, nseg].any()


@pytest.mark.parametrize("L", S.LS_SEARCH)
def test_searches(g, L):
    """progressive_search (M = 20 of 40, so the level filter runs) and brute_force_search: ids and scores."""
    pool = S.make_pool(L)
    flags = S.mix_flags(S.N_POOL)
    for ptag, Q, C in (("p64", pool["Q64"], pool["C64"]), ("p32", pool["Q32"], pool["C32"]),
                       ("pmix", pool["Q32"], None)):
        for a, q in enumerate(Q):
            with np.errstate(all="ignore"):
                if C is None:
                    bf, pg = mixed_search(q, pool["C32"], flags)
                else:
                    r = O.brute_force_search(q, C, S.TOP_K)
                    p = O.progressive_search(q, C, S.TOP_K, 0.1, S.M_GOLDEN)
                    bf, pg = (r[0], r[1]), (p[0], p[1])
            for stag, (ids, sc) in (("bf", bf), ("pg", pg)):
                want = g[f"{stag}_ids_{ptag}_L{L}"][a]
                n = int((want >= 0).sum())
                assert list(ids) == list(want[:n]), (L, ptag, stag, a)
                assert np.asarray(sc, dtype=np.float64).tobytes() == g[f"{stag}_sc_{ptag}_L{L}"][a][:n].tobytes(), \
                    (L, ptag, stag, a)


def mixed_search(q, C32, flags):
    """brute_force_search and progressive_search of a float32 query on a pool mixing float32 rows (flags) and
    rows widened to float64, from the oracle's per-dtype scorers: the reference's loop with per-pair dtypes
    (core/search_engine.py:232-300, :340-388; sort keys compare as Python / NumPy scalars do: a numpy float32
    score against a Python float in float32 only when every score is float32-typed, which a mixed pool is not
    where a float64 row is in play, so float64 keys)."""
    rows = [C32[b] if flags[b] else C32[b].astype(np.float64) for b in range(len(C32))]
    val, ty = S.oracle_tables(q[None], rows)
    nseg = val.shape[2] - 2
    per, ov = val[0, :, :nseg], val[0, :, nseg + 1]
    order = np.argsort(-ov, kind="stable")[:S.TOP_K]
    bf = (order, ov[order])
    cur = np.arange(len(rows))
    for lv in range(nseg):
        if len(cur) <= S.M_GOLDEN:
            break
        s = per[cur, lv]
        is32 = ty[0, cur, lv].astype(bool)
        keep = s >= np.where(is32, np.float64(np.float32(0.1)), 0.1)
        w = [1.0 / (i + 1) for i in range(lv + 1)]
        comb = sum(per[cur, i] * w[i] for i in range(lv + 1)) / sum(w)
        pos = np.nonzero(keep)[0]
        if len(pos):
            cur = cur[pos[np.argsort(-comb[pos], kind="stable")][:S.M_GOLDEN]]
        else:
            cur = cur[[int(np.argmax(s))]]
    perm = np.argsort(-ov[cur], kind="stable")[:S.TOP_K]
    return bf, (cur[perm], np.clip(ov[cur][perm], 0.0, 1.0))


def test_length_one_has_no_level_structure(g):
    """L = 1: the reference finds no level, scores 0.0 and its searches return nothing / every model at 0.0."""
    assert int(g["L1_nlevels"]) == 0 and O.parse_index_structure(1) == []
    one = np.array([0.5])
    assert float(g["L1_level0"]) == 0.0 == O.level_similarity(one, one[None], 0)[0]
    assert float(g["L1_overall"]) == 0.0 == O.overall_similarity(one, one[None])[0][0]
    C = np.array([[0.5], [0.25], [0.5]])
    assert int(g["L1_pg_count"]) == 0 == len(O.progressive_search(one, C, 10)[0])
    ids, sc, _ = O.brute_force_search(one, C, 10)
    assert list(ids) == list(g["L1_bf_ids"]) and list(sc) == list(g["L1_bf_sc"])


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_np_sum_rows_is_numpy_order(dt):
    """O.np_sum_rows equals np.add.reduce bytewise below 8 values, inside one leaf, and across recursive splits
    (659 = 328 + 331, 2733: three levels of splits), on data whose sum depends on the order."""
    rng = np.random.default_rng(5)
    for n in SUM_LENGTHS:
        x = (rng.standard_normal((8, n)) * 10.0 ** rng.integers(-3, 4, (8, n))).astype(dt)
        want = np.stack([np.add.reduce(r) for r in x])
        got = O.np_sum_rows(x)
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), n
    x = (rng.standard_normal(2733) * 1e3).astype(dt)
    assert len({np.add.reduce(x).tobytes(), np.add.reduce(x[::-1].copy()).tobytes(),
                dt(sum(x.tolist())).tobytes()}) > 1, "the data does not tell summation orders apart"


COVER_LS = [7, 16, 66, 214, 258, 1025]


@pytest.mark.parametrize("combo", S.COMBOS)
def test_every_branch_in_every_length_class(combo):
    """The tables reach every branch of compare_indices_at_level that can be reached - both std zero with means
    equal / differing, one std zero, the general branch, the distance term clamped at 0 - with segments below 8
    values, of 8..128 and above 128, in this dtype combination (classified by NumPy's own statistics)."""
    seen = set()
    for L in COVER_LS:
        Q, cand = S.combo_inputs(S.make_rows(L), combo)
        for (s, e) in O.segment_bounds(L):
            cls = S.seg_class(e - s)
            for q in Q:
                for c in cand:
                    seen |= {(cls, b) for b in S.branches(q, c, s, e)}
    # a float64 query's squares never vanish where its float32 partner's values are non-zero: with q64 c32 the
    # `max_possible_mse > 0` test cannot fail outside the constant branches
    need = {(cls, b) for cls in ("lt8", "leaf", "split") for b in S.BRANCHES if b != "maxmse0" or combo != "q64c32"}
    assert need <= seen, f"{combo}: never reached {sorted(need - seen)}"
    assert combo != "q64c32" or not {x for x in seen if x[1] == "maxmse0"}


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_rows_with_vanishing_squares(dt):
    """Rows 22 / 23: in every segment of even length np.std is non-zero while np.mean(x ** 2) is exactly zero
    (each square rounds to 0 or one subnormal unit, their mean u / 2 ties to even), so a pair of them reaches the
    scorer's `max_possible_mse > 0` else-branch (distance similarity 1.0); the oracle's statistics agree."""
    for L in (16, 66, 1025):
        C = S.make_rows(L)["C64" if dt == np.float64 else "C32"]
        for (s, e) in O.segment_bounds(L):
            x = C[22:24, s:e]
            with np.errstate(under="ignore"):
                std, msq = np.stack([np.std(r) for r in x]), np.stack([np.mean(r ** 2) for r in x])
                assert np.array_equal(O.np_std_rows(x), std) and np.array_equal(O.np_mean_rows(x * x), msq)
            if (e - s) % 2 == 0:
                assert (std != 0).all() and (msq == 0).all(), (L, s, e)


def test_library_level_structure(g):
    """hq_parse_structure / hq_seg_count / hq_seg_padded_len / hq_seg_level0_len (host code) against the
    reference's _parse_index_structure and the oracle at every length of the tables and at L = 1."""
    from hq_mi355x import _lib
    lib = _lib.load()
    buf = (ctypes.c_int32 * 64)()
    got = []
    for L in [1] + S.LS:
        n = lib.hq_parse_structure(L, buf, 16)
        lv = [(buf[4 * i], buf[4 * i + 1], buf[4 * i + 2], bool(buf[4 * i + 3])) for i in range(n)]
        assert lv == O.parse_index_structure(L), L
        got += [(L,) + x[:3] + (int(x[3]),) for x in lv]
        assert lib.hq_seg_count(L) == n, L
        assert lib.hq_seg_padded_len(L) == sum((e - s + 3) // 4 * 4 for (_, s, e, _) in lv), L
        # (the padded length of level 0: what the scans contract over)
        assert lib.hq_seg_level0_len(L) == ((lv[0][2] - lv[0][1] + 3) // 4 * 4 if lv else 0), L
    np.testing.assert_array_equal(np.array(got), g["parse_struct"])
