"""The exact scorers and re-rank kernels of hq_search.hip against the CPU oracle over index length
(tests/scorer_sweep_cases.py; the oracle is pinned to the reference over the same tables by
tests/test_scorer_sweep_cpu.py).  Every comparison of a score is BYTEWISE: include/hq_mi355x.h states that
hq_seg_prepare*, hq_level_scores, hq_rescore, the hq_refine_* family and hq_pair_scores_raw* reproduce the
reference bit for bit.

The kernel refine_launch picks for a list of kp entries at index length L (hq_search.hip, as it stands):

    L                     kp = 28            kp = 64            kp = 108                        kp = 520
    16, 66, 76 (even,     k_rank_small<6,32> k_rank_small<6,64> k_rank_pairs<6> +               k_rank_pairs<6> +
      <= 6 pieces / lane)                                       k_rank_sort<128,128>            k_rank_sort<256>
    78, 100, 140 (<= 10)  k_rank_small<10,32> k_rank_small<10,64> k_rank_pairs<10> + <128,128>  k_rank_pairs<10> + <256>
    142 (even, no coop)   k_refine_lds_sm    k_refine_lds_sm    k_refine_big_sm                 k_refine_big_sm_raw
    143, 213 (odd)        k_refine<true>     k_refine<true>     k_refine_big_sm                 k_refine_big_sm_raw
    214, 258 (a segment   k_refine_lds       k_refine<false>    k_refine_big                    k_refine_big_raw
      above 128 values)                      (rows > 96 KiB)
    215, 259 (odd)        k_refine<false>    k_refine<false>    k_refine_big                    k_refine_big_raw
    1024 (7 segments)     k_refine<false>    k_refine<false>    k_refine_big                    k_refine_big_raw

(k_refine has no record output: hq_refine_rescore_topk then runs k_rescore<8, true | false> behind it;
k_rescore<16, ..> needs more than 8 segments, and no length has more than 7: unreachable.  L = 64 and 32 take the
compile-time forms k_rank_pairs<6, 1 | 2>, which test_gpu_scan_contract.py covers; k_rank_sort<512> only with
option rank_sort_nt = 512.  profiles/scorer_sweep_kernels.txt: the launches of one run of this file.)  Dense scores: k_level_scores_lds for a level of at most 128 values,
k_level_scores<true | false> for the overall score, a level past the structure and option level_scores_v1."""
import functools

import numpy as np
import pytest

import scan_contract as SC
import scorer_sweep_cases as S
from oracle import hq_oracle as O

pytestmark = pytest.mark.gpu

INF = np.inf


def _t(x):
    from hq_mi355x._dev import to_dev
    return to_dev(x)


def _np(x):
    from hq_mi355x._dev import to_np
    return to_np(x)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _same(a, b):
    """Bytewise equality of two float64 arrays (tells -0.0 from 0.0, compares NaN payloads)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _side(X, kind):
    """Rows on the device: "f64", "f32" (every row a float32 vector) or "mix" (even rows float32)."""
    from hq_mi355x import kernels as K
    x = _t(np.asarray(X, dtype=np.float64))
    if kind == "mix":
        return K.seg_prepare(x, row_f32=S.mix_flags(len(X)))
    return K.seg_prepare(x, src_f32=(kind == "f32"))


SIDES = {"c64": ("Q64", "f64", "C64", "f64"), "c32": ("Q32", "f32", "C32", "f32"),
         "q64c32": ("Q32", "f64", "C32", "f32"), "mix": ("Q32", "f32", "C32", "mix")}


def _prep(rows, combo):
    qk, qkind, ck, ckind = SIDES[combo]
    return _side(rows[qk], qkind), _side(rows[ck], ckind)


@functools.lru_cache(maxsize=None)
def _tables(L):
    """{combo: values [6, 24, nseg + 2]} from the oracle, computed once per length and never written to."""
    rows = S.make_rows(L)
    out = {}
    for combo in S.COMBOS:
        val = S.oracle_tables(*S.combo_inputs(rows, combo))[0]
        val.setflags(write=False)
        out[combo] = val
    return out


def expected_prepare(X, is32):
    """hq_seg_prepare_rows' outputs as include/hq_mi355x.h states them, from the oracle's NumPy-order statistics:
    X float64 [N, L] (float32 rows widened), is32 bool [N] -> (Z [N, Lp], stats [N, nseg, 4])."""
    X = np.asarray(X, dtype=np.float64)
    N, L = X.shape
    b = O.segment_bounds(L)
    poff = np.cumsum([0] + [(e - s + 3) // 4 * 4 for (s, e) in b])
    Z, St = np.zeros((N, poff[-1])), np.zeros((N, len(b), 4))
    with np.errstate(all="ignore"):
        for i, (s, e) in enumerate(b):
            x = X[:, s:e]
            mean, sd, msq = O.np_mean_rows(x), O.np_std_rows(x), O.np_mean_rows(x * x)
            z = np.where(sd[:, None] == 0, 0.0, (x - mean[:, None]) / sd[:, None])
            aux = np.zeros(N)
            if is32.any():
                x32 = x[is32].astype(np.float32)
                m32, s32 = O.np_mean_rows(x32), O.np_std_rows(x32)
                z32 = np.where(s32[:, None] == 0, np.float32(0), (x32 - m32[:, None]) / s32[:, None])
                mean[is32] = np.where(s32 == 0, m32.astype(np.float64), mean[is32])
                sd[is32], z[is32] = s32, z32
                aux[is32] = 1 + 2 * ~((msq[is32] >= 2.0 ** -100) & (msq[is32] <= 2.0 ** 100))
            Z[:, poff[i]:poff[i] + e - s] = z
            St[:, i] = np.stack([mean, sd, msq, aux], axis=1)
    return Z, St


# ------------------------------------------------------------------------------------------- statistics


def test_statistics_every_length(hq_lib):
    """hq_seg_prepare_rows: mean, std, mean of squares, aux bits and the normalised rows of float64 rows, float32
    rows and a batch mixing both, at every length; where the level-0 segment has at most 32 values,
    hq_seg_prepare_pack0 (both its kernels) writes the same Z and statistics."""
    from hq_mi355x import kernels as K
    bad = []
    for L in S.LS:
        rows = S.make_rows(L)
        for key, kind in (("C64", "f64"), ("C32", "f32"), ("C32", "mix"), ("Q32", "f32")):
            X = rows[key].astype(np.float64)
            is32 = {"f64": np.zeros(len(X), bool), "f32": np.ones(len(X), bool), "mix": S.mix_flags(len(X))}[kind]
            p = _side(rows[key], kind)
            Z, St = expected_prepare(X, is32)
            if not (_same(_np(p.S), St) and _same(_np(p.Z), Z)):
                bad.append((L, key, kind))
            if K.seg_level0_len(L) <= 32:
                kw = {"row_f32": is32} if kind == "mix" else {"src_f32": kind == "f32"}
                p0 = K.seg_prepare_pack0(_t(X), **kw)
                if not (_same(_np(p0.S), St) and _same(_np(p0.Z), Z)) or p0.Z16 is None:
                    bad.append((L, key, kind, "pack0"))
    assert not bad, f"statistics differ from NumPy's at (L, rows, kind) {bad[:12]}"


def test_statistics_serial_and_batch_kernels(hq_lib, hq_option):
    """The other kernels behind the same entries: hq_seg_prepare_pack0 with option prep_coop = 0 (one lane per
    segment), and k_seg_prepare (more than 16384 rows: one thread per (row, segment)) against the staged form."""
    from hq_mi355x import kernels as K
    hq_option("prep_coop", 0)
    for L in (2, 7, 33, 64):
        rows = S.make_rows(L)
        for key, f32 in (("C64", False), ("C32", True)):
            X = rows[key].astype(np.float64)
            Z, St = expected_prepare(X, np.full(len(X), f32))
            p0 = K.seg_prepare_pack0(_t(X), src_f32=f32)
            assert _same(_np(p0.S), St) and _same(_np(p0.Z), Z), (L, key)
    hq_option("prep_coop", None)
    for L in (66, 214):
        X = np.tile(S.make_rows(L)["C32"].astype(np.float64), (684, 1))[:16400]
        is32 = S.mix_flags(len(X))
        p = K.seg_prepare(_t(X), row_f32=is32)
        Z, St = expected_prepare(X[:48], is32[:48])
        Zg, Sg = _np(p.Z), _np(p.S)
        assert _same(Sg[:48], St) and _same(Zg[:48], Z), L
        assert _same(Sg[:16368].reshape(341, 48, -1), np.broadcast_to(St.reshape(1, 48, -1), (341, 48, St[0].size))), L
        assert _same(Zg[16368:], Z[:32]), L


def test_no_level_structure_at_length_one(hq_lib, golden):
    """L = 1: the entries refuse (HQ_E_INVALID, "no level structure"), the engine answers as the reference does:
    nothing from progressive_search, every model at 0.0 in pool order from brute_force_search."""
    from hq_mi355x import _lib, kernels as K
    from hq_mi355x.core.search_engine import ProgressiveSimilaritySearchEngine
    from hq_mi355x.models import ModelMetadata, QuantizedModel
    g = golden("scorer_sweep")
    import torch
    from hq_mi355x._dev import ptr, stream
    assert K.seg_count(1) == 0 and K.parse_structure(1) == []
    x = _t(np.array([[0.5], [0.25]]))
    with pytest.raises(_lib.NativeLibraryError):      # (its Z and statistics are empty tensors: "null buffer")
        K.seg_prepare(x)
    buf = torch.zeros(16, dtype=torch.float64, device=x.device)
    rc = hq_lib.hq_seg_prepare_rows(ptr(x), 2, 1, 0, None, ptr(buf), ptr(buf), stream())
    assert rc == _lib.HQ_E_INVALID and b"no level structure" in hq_lib.hq_last_error()
    assert not _np(buf).any()
    eng = ProgressiveSimilaritySearchEngine(similarity_threshold=0.1, max_candidates_per_level=20)
    pool = [QuantizedModel(b"x", (8, 8), 1, 0.8, np.array([v]), ModelMetadata(f"m{i}", 1, 1, 1.0, "t"))
            for i, v in enumerate((0.5, 0.25, 0.5))]
    one = np.array([0.5])
    assert len(eng.progressive_search(one, pool, 10)) == int(g["L1_pg_count"]) == 0
    res = eng.brute_force_search(one, pool, 10)
    assert [int(r.model.model_id[1:]) for r in res] == list(g["L1_bf_ids"])
    assert [r.similarity_score for r in res] == list(g["L1_bf_sc"])
    assert eng.compare_indices_at_level(one, one, 0) == float(g["L1_level0"])


# ------------------------------------------------------------------------------------------- dense scores


def _dense_bad(L, combos, levels=None):
    from hq_mi355x import kernels as K
    import torch
    rows = S.make_rows(L)
    bad = []
    for combo in combos:
        qp, cp = _prep(rows, combo)
        val = _tables(L)[combo]
        nseg = qp.nseg
        lvs = list(range(nseg + 1)) + [-1] if levels is None else levels
        got = _np(torch.stack([K.level_scores(qp, cp, lv) for lv in lvs]))
        for i, lv in enumerate(lvs):
            want = val[:, :, nseg + 1] if lv < 0 else val[:, :, lv]
            if not _same(got[i], want):
                bad.append((L, combo, lv, int((_bits(got[i]) != _bits(want)).sum())))
    return bad


@pytest.mark.parametrize("part", range(4))
def test_dense_scores_every_length(hq_lib, part):
    """hq_level_scores at every level, at level = nseg (zeros) and overall (level -1), every dtype combination,
    every length (a quarter of the lengths per case)."""
    bad = []
    for L in S.LS[part::4]:
        bad += _dense_bad(L, S.COMBOS)
    assert not bad, f"(L, combination, level, differing scores) {bad[:12]}"


def test_dense_scores_thread_per_pair_kernel(hq_lib, hq_option):
    """Option level_scores_v1: k_level_scores<true | false> at every level too (by default the levels of at most
    128 values take k_level_scores_lds), so both dense kernels meet the oracle and not only each other."""
    hq_option("level_scores_v1", 1)
    bad = []
    for L in (7, 66, 214, 258, 1025):
        bad += _dense_bad(L, S.COMBOS)
    assert not bad, f"(L, combination, level, differing scores) {bad[:12]}"


def test_pair_scores_raw(hq_lib):
    """hq_pair_scores_raw_src on raw segments of 1..300, 659, 1024, 1025, 2731 and 2733 values: all four
    q_f32 / c_f32 settings, a random and two constant queries, against NumPy's own operations pair by pair."""
    from hq_mi355x import kernels as K
    bad = []
    for m in S.RAW_LENGTHS:
        q32, C32 = S.raw_segment_rows(m, np.float32)
        q64, C64 = S.raw_segment_rows(m, np.float64)
        for qf in (False, True):
            for cf in (False, True):
                # a float64 side of the q64 c32 / q32 c64 settings holds the other table's float64 rows
                qs, C = (q32, C32) if qf else (q64, C64), (C32 if cf else C64)
                q0 = qs[0]
                for q in (q0, C[2][: len(q0)].astype(q0.dtype), C[3].astype(q0.dtype)):
                    got = _np(K.pair_scores_raw(_t(q.astype(np.float64)), _t(C.astype(np.float64)), q_f32=qf, c_f32=cf))
                    if not _same(got, S.raw_pair_scores(q, C)):
                        bad.append((m, qf, cf))
    assert not bad, f"(m, q_f32, c_f32) {sorted(set(bad))[:20]}"


def test_rescore_records(hq_lib):
    """hq_rescore: [overall, level 0 ..] records of hand-picked id lists - rows in and out of order, repeats, -1
    and ids outside the corpus (zeros), an id_base - at every edge length and every tenth length of the sweep."""
    from hq_mi355x import kernels as K
    base = 1000
    ids = np.array([[0, 23, 5, -1, 24, 7, 7, 1000000], [22, 23, -5, 17, 16, 15, 1, 2], [3, 2, 1, 0, 23, 22, 21, 20],
                    [22, 9, 18, 19, -1, -1, 24, 0], [2, 3, 6, 13, 14, 8, 12, 2 ** 40], [6, 7, 11, 10, 4, 5, 25, -1]])
    bad = []
    for L in S.LS_EDGE + S.LS_SWEEP[::10]:
        rows = S.make_rows(L)
        for combo in S.COMBOS:
            qp, cp = _prep(rows, combo)
            val = _tables(L)[combo]
            nseg = qp.nseg
            ok = (ids >= 0) & (ids < S.N_ROWS)
            rec = np.concatenate([val[:, :, nseg + 1:], val[:, :, :nseg]], axis=2)   # [overall, level 0 ..]
            want = np.where(ok[:, :, None], np.take_along_axis(rec, np.where(ok, ids, 0)[:, :, None], axis=1), 0.0)
            got = _np(K.rescore(qp, cp, _t(np.where(ok | (ids < 0), ids + base * (ids >= 0), ids)), id_base=base))
            if not _same(got, want):
                bad.append((L, combo))
    assert not bad, f"(L, combination) {bad[:12]}"


# ------------------------------------------------------------------------------------------- re-rank

RANK_LS = [16, 66, 76, 78, 100, 140, 142, 143, 213, 214, 215, 258, 259, 1024]
RANK_KP = [28, 64, 108, 520]
EPS_C = 2.0 ** -16    # as test_gpu_scan_contract.py: a binary fraction, so `last + eps == thr` can be hit exactly
THR_C = 0.75          # exact in float32 (the kernels compare against min(thr, float32(thr)))
TINY = 2.0 ** -40


@functools.lru_cache(maxsize=None)
def _rank_case(L):
    """About 700 rows per length (scan_contract.build_case: adversarial families, duplicates, negations) with the
    oracle's exact scores of both modes and per-level scores, computed once."""
    c = SC.build_case(L, 48, 40 + L, nq=4, n_unsafe=2)
    with np.errstate(all="ignore"):
        ovp = [O.overall_similarity(q, c.C) for q in c.Q]
    per = np.stack([x[1] for x in ovp])
    ov = np.stack([x[0] for x in ovp])
    for a in (per, ov):
        a.setflags(write=False)
    return c, per, ov


def _sorted_list(ids, e, rng, eps):
    cs = e[ids] + rng.uniform(-0.9 * eps, 0.9 * eps, len(ids))
    o = np.lexsort((ids, -cs))
    return cs[o], ids[o]


def _set_last(cs, target):
    cs = cs.copy()
    cs[:-1] = np.maximum(cs[:-1], target)
    cs[-1] = target
    return cs


def rank_lists(c, exact, kp, k, rng):
    """One list per variant, built from the oracle's exact scores nudged by less than eps and sorted as a scan
    emits them: (name, query, cand_score [kp], cand_id [kp]).  The variants of test_gpu_scan_contract._rule_lists
    that do not depend on the corpus of L = 64 / 32, plus equal scores straddling the k-th place."""
    N, eps = c.N, EPS_C
    qs = iter(np.nonzero(~c.flagged_queries())[0])
    order = [np.lexsort((np.arange(N), -exact[q])) for q in range(len(exact))]

    def base(q, ids=None):
        return _sorted_list(order[q][:kp] if ids is None else ids, exact[q], rng, eps)

    out = []
    q = next(qs)
    cs, ids = base(q)
    out.append(("provable", q, _set_last(cs, min(cs[-1], exact[q][order[q][k - 1]] - 1.5 * eps)), ids))
    q = int(np.nonzero(c.q_fam == SC.FAMILIES.index("const"))[0][0])
    out.append(("const_query", q) + base(q))
    q = next(qs)
    cs, ids = base(q)
    out.append(("within_eps", q, _set_last(cs, exact[q][order[q][k - 1]] - 0.5 * eps), ids))
    q = next(qs)
    out.append(("kth_removed", q) + base(q, np.delete(order[q][:kp + 1], k - 1)))
    for name, fill in (("not_full", -INF), ("truncated", INF)):
        q = next(qs)
        cs, ids = base(q, order[q][:kp - 3])
        out.append((name, q, np.concatenate([cs, [fill] * 3]), np.concatenate([ids, [-1] * 3])))
    # few rows pass THR_C on a full list whose bound lies just below / on / just above the threshold
    for name, d in (("few_below", -TINY), ("few_equal", 0.0), ("few_above", TINY)):
        q = next(qs)
        cs, ids = base(q)
        j = int((exact[q][ids] >= THR_C).sum())
        if j < kp:
            cs[j:] = (THR_C - eps + d) + TINY * np.arange(kp - j - 1, -1, -1)
        out.append((name, q, cs, ids))
    q = next(qs)
    cs, ids = base(q)
    ids = ids.copy()
    ids[k // 2:] = N + np.arange(kp - k // 2)
    out.append(("out_of_range", q, cs, ids))
    # the five copies of query 0's row and the row itself: equal exact scores across the k-th place
    dup = np.concatenate([[c.q_rows[0]], np.arange(N - 5, N)])
    q = next(qs)
    rest = order[q][~np.isin(order[q], dup)]
    e_dup = exact[q][dup[0]]
    above = rest[exact[q][rest] > e_dup][-(k - 3):] if (exact[q][rest] > e_dup).sum() >= k - 3 else None
    if above is not None:
        below = rest[exact[q][rest] < e_dup][:kp - len(above) - 6]
        if len(above) + 6 + len(below) == kp:
            out.append(("dups_at_kth", q) + base(q, np.concatenate([above, dup, below])))
    assert all(len(x[2]) == kp and len(x[3]) == kp for x in out)
    return out


@pytest.mark.parametrize("L", RANK_LS)
def test_rerank_every_kernel(hq_lib, L):
    """hq_refine_topk, hq_refine_rescore_topk and the workspace form on lists made from the oracle's exact scores
    (no scan involved), both modes, kp in {28, 64, 108, 520}: ids, counts, resolved flags and the redo counter
    equal scan_contract.resolved_rule's, scores and [overall, level ..] records bytewise the oracle's."""
    import torch
    from hq_mi355x import kernels as K
    c, per, ov = _rank_case(L)
    cp = _side(c.C, "f64")
    nseg = per.shape[2]
    seen = set()
    for mode in (0, 1):
        exact = per[:, :, 0] if mode == 0 else ov
        for kp in RANK_KP:
            k = kp - 8
            lists = rank_lists(c, exact, kp, k, np.random.default_rng(kp + L + mode))
            qsel = np.array([x[1] for x in lists])
            qp = _side(c.Q[qsel], "f64")
            cs, cid = _t(np.stack([x[2] for x in lists])), _t(np.stack([x[3] for x in lists]).astype(np.int64))
            redo = torch.zeros(1, dtype=torch.int32, device=cid.device)
            # a threshold equal to an exact score the first list holds: `>=` keeps that row, `>` drops it
            t_eq = float(exact[lists[0][1]][lists[0][3][2]])
            for thr_mode, thr in ((0, 0.0), (1, THR_C), (2, THR_C), (1, t_eq), (2, t_eq)):
                want = [SC.resolved_rule(x[2], x[3], exact[x[1]], SC.passes(exact[x[1]], thr, thr_mode), k, thr,
                                         thr_mode, EPS_C) for x in lists]
                w_res, w_cnt = np.array([w[0] for w in want]), np.array([w[1] for w in want])
                w_id, w_sc = np.stack([w[2] for w in want]), np.stack([w[3] for w in want])
                seen |= {(x[0], bool(w[0])) for x, w in zip(lists, want)}
                ok = w_id >= 0
                rec = np.concatenate([ov[qsel][:, :, None], per[qsel]], axis=2)       # [list, N, 1 + nseg]
                w_det = np.where(ok[:, :, None], np.take_along_axis(rec, np.where(ok, w_id, 0)[:, :, None], axis=1), 0.0)
                for count_empty in (False, True):
                    for form in ("topk", "rescore", "ws"):
                        what = f"{form} L {L} mode {mode} kp {kp} thr_mode {thr_mode} thr {thr} ce {count_empty}"
                        if form == "topk":
                            r = K.refine_topk(qp, cp, mode, cs, cid, k, thr, thr_mode, EPS_C, redo=redo,
                                              count_empty=count_empty)
                        elif form == "rescore":
                            r = K.refine_rescore_topk(qp, cp, mode, cs, cid, k, thr, thr_mode, EPS_C, redo=redo,
                                                      count_empty=count_empty)
                        else:
                            r = _refine_ws(qp, cp, mode, cs, cid, k, thr, thr_mode, EPS_C, redo, count_empty)
                        g_sc, g_id, g_cnt, g_res = (_np(x) for x in r[:4])
                        names = [x[0] for x in lists]
                        assert np.array_equal(g_res != 0, w_res), f"{what}: resolved {dict(zip(names, zip(g_res, w_res)))}"
                        assert np.array_equal(g_cnt, w_cnt), what
                        assert np.array_equal(g_id, w_id), what
                        assert _same(g_sc, w_sc), what
                        assert int(_np(redo)[0]) == SC.redo_count(w_res, w_cnt, count_empty), what
                        if len(r) > 4:
                            assert _same(_np(r[4]), w_det), what
    for name, res in (("provable", True), ("within_eps", False), ("not_full", True), ("truncated", False),
                      ("few_below", True), ("few_equal", True), ("few_equal", False), ("few_above", False),
                      ("out_of_range", False), ("dups_at_kth", True)):
        assert (name, res) in seen, f"variant {name} never gave resolved = {res}"


def _refine_ws(qp, cp, mode, cs, cid, k, thr, thr_mode, eps, redo, count_empty):
    """hq_refine_topk_ws with its workspace and records, at any list length."""
    import torch
    from hq_mi355x import kernels as K
    Q, kp = cid.shape
    dev = cid.device
    os_ = torch.empty((Q, k), dtype=torch.float64, device=dev)
    oi = torch.empty((Q, k), dtype=torch.int64, device=dev)
    cnt = torch.empty(Q, dtype=torch.int32, device=dev)
    res = torch.empty(Q, dtype=torch.int32, device=dev)
    det = torch.empty((Q, k, 1 + qp.nseg), dtype=torch.float64, device=dev)
    K._refine_ws(qp, cp, mode, cs, cid, kp, k, thr, thr_mode, eps, 0, os_, oi, cnt, res, count_empty, redo, None, det,
                 None)
    return os_, oi, cnt, res, det


def test_rerank_sort_of_512_threads(hq_lib, hq_option):
    """Option rank_sort_nt = 512 (k_rank_sort<512>, lists above 512 entries) at L = 100."""
    import torch
    from hq_mi355x import kernels as K
    hq_option("rank_sort_nt", 512)
    c, per, ov = _rank_case(100)
    cp = _side(c.C, "f64")
    kp, k = 520, 512
    lists = rank_lists(c, ov, kp, k, np.random.default_rng(3))
    qp = _side(c.Q[[x[1] for x in lists]], "f64")
    cs, cid = _t(np.stack([x[2] for x in lists])), _t(np.stack([x[3] for x in lists]).astype(np.int64))
    redo = torch.zeros(1, dtype=torch.int32, device=cid.device)
    want = [SC.resolved_rule(x[2], x[3], ov[x[1]], SC.passes(ov[x[1]], 0.0, 0), k, 0.0, 0, EPS_C) for x in lists]
    r = K.refine_topk(qp, cp, 1, cs, cid, k, 0.0, 0, EPS_C, redo=redo)
    assert np.array_equal(_np(r[3]) != 0, [w[0] for w in want]) and np.array_equal(_np(r[2]), [w[1] for w in want])
    assert np.array_equal(_np(r[1]), np.stack([w[2] for w in want])) and _same(_np(r[0]), np.stack([w[3] for w in want]))


# ------------------------------------------------------------------------------------------- engine

ENGINE_N = 300


@functools.lru_cache(maxsize=None)
def _engine_rows(L, f32):
    """300 rows (the degenerate rows in front; for float32 without those outside the scans' model - the all-zero
    row and rows 15-17, 22, 23 - so that the scan path runs) and 8 queries."""
    dt = np.float32 if f32 else np.float64
    C = S._rows(L, dt, ENGINE_N + 6, S.SEED + 5 * L + f32)
    if f32:
        C = np.delete(C, [1, 15, 16, 17, 22, 23], axis=0)
    C = C[:ENGINE_N - 6]
    rng = np.random.default_rng(S.SEED + 11 * L + f32)
    C = np.concatenate([C, np.tile(C[30], (6, 1))])          # six equal rows: ties by id
    Q = np.stack([C[10] + rng.normal(0, 0.01, L).astype(dt), C[20], np.full(L, 0.5, dt), rng.standard_normal(L).astype(dt),
                  C[2], C[6], C[30], C[40] + rng.normal(0, 0.05, L).astype(dt)])
    return C, Q


def _check_search(got_ids, got_sc, cnt, want, what):
    for a, (rid, rsc) in enumerate(want):
        n = len(rid) if cnt is None else int(cnt[a])
        assert n == len(rid) and list(got_ids[a][:n]) == list(rid), (what, a)
        assert _same(got_sc[a][:n], rsc), (what, a)
        assert (got_ids[a][n:] < 0).all(), (what, a)


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("L", S.LS_SEARCH)
def test_engine_routes(hq_lib, L, f32):
    """IndexCorpus.progressive (M = 20 and 100), brute_force and frame_search at one length per routing class
    against the oracle's searches: ids and counts equal, scores bytewise (every route ends in the exact scorers:
    hq_rescore's records, the re-rank's level-0 scores)."""
    from hq_mi355x.core.search_engine import IndexCorpus
    C, Q = _engine_rows(L, f32)
    corpus = IndexCorpus(C)
    assert not corpus.dense_only
    with np.errstate(all="ignore"):
        for M in (20, 100):
            ids, ovs, _, cnt = corpus.progressive(Q, 10, 0.1, M)
            want = [O.progressive_search(q, C, 10, 0.1, M)[:2] for q in Q]
            _check_search(_np(ids), _np(ovs), _np(cnt), want, ("progressive", L, M))
        ids, ovs, _ = corpus.brute_force(Q, 10)
        want = [O.brute_force_search(q, C, 10)[:2] for q in Q]
        _check_search(_np(ids), _np(ovs), None, want, ("brute_force", L))
        ids, sc = corpus.frame_search(Q, 10, 0.1)
        want = [O.hierarchical_frame_search(q, C, 10, 0.1) for q in Q]
        _check_search(_np(ids), _np(sc), [len(w[0]) for w in want], want, ("frame_search", L))


def test_engine_float32_rows_outside_the_scans(hq_lib):
    """The whole float32 table (zero rows, squares that under- and overflow) makes the corpus dense-only: the
    same answers from the dense exact path."""
    from hq_mi355x.core.search_engine import IndexCorpus
    L = 66
    pool = S.make_pool(L)
    C, Q = pool["C32"], pool["Q32"]
    corpus = IndexCorpus(C)
    assert corpus.dense_only
    with np.errstate(all="ignore"):
        ids, ovs, _, cnt = corpus.progressive(Q, 10, 0.1, 20)
        _check_search(_np(ids), _np(ovs), _np(cnt), [O.progressive_search(q, C, 10, 0.1, 20)[:2] for q in Q], "pg")
        ids, ovs, _ = corpus.brute_force(Q, 10)
        _check_search(_np(ids), _np(ovs), None, [O.brute_force_search(q, C, 10)[:2] for q in Q], "bf")


def test_engine_append_and_replace_by_rebuild(hq_lib):
    """L = 4098 is past hq_seg_append's limit: append rebuilds the corpus, replace writes in place; the searches
    behind them see exactly the rows a fresh corpus would hold."""
    from hq_mi355x.core.search_engine import IndexCorpus
    L = 4098
    C, Q = _engine_rows(L, False)
    corpus = IndexCorpus(C[:200])
    assert corpus.append(C[200:]) == ENGINE_N
    new = C[[5, 20]] * 0.5 + 0.25
    corpus.replace([7, 250], new)
    C2 = C.copy()
    C2[[7, 250]] = new
    with np.errstate(all="ignore"):
        ids, ovs, _, cnt = corpus.progressive(Q, 10, 0.1, 20)
        _check_search(_np(ids), _np(ovs), _np(cnt), [O.progressive_search(q, C2, 10, 0.1, 20)[:2] for q in Q], "pg")
        ids, ovs, _ = corpus.brute_force(Q, 10)
        _check_search(_np(ids), _np(ovs), None, [O.brute_force_search(q, C2, 10)[:2] for q in Q], "bf")


@pytest.mark.parametrize("L", S.LS_SEARCH)
def test_drop_in_engine_golden_pools(hq_lib, golden, L):
    """ProgressiveSimilaritySearchEngine on the golden pools (float64, float32, mixed): the reference's own ids
    and scores."""
    from hq_mi355x.core.search_engine import ProgressiveSimilaritySearchEngine
    from hq_mi355x.models import ModelMetadata, QuantizedModel
    g = golden("scorer_sweep")
    pool = S.make_pool(L)
    eng = ProgressiveSimilaritySearchEngine(similarity_threshold=0.1, max_candidates_per_level=S.M_GOLDEN)
    for ptag, (Q, cand) in (("p64", (pool["Q64"], list(pool["C64"]))), ("p32", (pool["Q32"], list(pool["C32"]))),
                            ("pmix", S.combo_inputs(pool, "mix"))):
        models = [QuantizedModel(b"x", (8, 8), 1, 0.8, r, ModelMetadata(f"m{i}", 1, 1, 1.0, "t"))
                  for i, r in enumerate(cand)]
        for a in range(len(Q)):
            for stag, fn in (("bf", eng.brute_force_search), ("pg", eng.progressive_search)):
                res = fn(Q[a], models, S.TOP_K)
                ref = g[f"{stag}_ids_{ptag}_L{L}"][a]
                assert [int(r.model.model_id[1:]) for r in res] == list(ref[ref >= 0]), (L, ptag, stag, a)
                assert _same([r.similarity_score for r in res], g[f"{stag}_sc_{ptag}_L{L}"][a][: len(res)]), \
                    (L, ptag, stag, a)
