"""The contract every search rests on - approximate scan, exact re-rank, a proof that the list was complete -
checked piece by piece against the oracle (scan_contract.py holds the inputs and the NumPy statements):

a. every score a scan lists lies within the scan's documented bound of the exact score of the same pair;
b. every list is complete: a row that must be listed, given that bound, is listed;
c. hq_refine_topk / hq_refine_rescore_topk return what the rule in their header says, on lists made here;
d. an empty corpus gives (-inf, -1) lists.
"""
import numpy as np
import pytest

import scan_contract as SC
from oracle import hq_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-10  # the suite's tolerance of exact scores (test_gpu_search.py)
INF = np.inf


def _t(x):
    from hq_mi355x._dev import to_dev
    return to_dev(x)


def _np(x):
    from hq_mi355x._dev import to_np
    return to_np(x)


def _corpus(C, **kw):
    from hq_mi355x import kernels as K
    return K.flag_rows(K.packov(K.pack0(K.seg_prepare(_t(np.asarray(C, dtype=np.float64)), **kw))))


def _queries(Q, **kw):
    from hq_mi355x import kernels as K
    return K.seg_prepare_pack0(_t(np.asarray(Q, dtype=np.float64)), **kw)


def _scan(qp, cp, mode, k, thr=0.0, thr_mode=0, need_best=False):
    from hq_mi355x import kernels as K
    sc, ids, best, bid = K.scan_topk(qp, cp, mode, k, thr, thr_mode, need_best=need_best)
    return _np(sc), _np(ids), (None if best is None else _np(best)), (None if bid is None else _np(bid))


def _check_lists(sc, ids, N, empty=(-INF,), what=""):
    """The shape every scan list has: listed entries first, ids unique and in range, ordered by the list's own
    scores descending then id ascending, empty slots (-inf, -1) (or what `empty` allows: a truncated list and
    the list of a flagged query carry +inf)."""
    k = ids.shape[1]
    v = ids >= 0
    assert (ids[v] < N).all() and (ids[~v] == -1).all(), what
    nv = v.sum(axis=1)
    assert np.array_equal(v, np.arange(k)[None, :] < nv[:, None]), f"{what}: an empty slot before a listed entry"
    for q in range(ids.shape[0]):
        assert len(np.unique(ids[q, :nv[q]])) == nv[q], f"{what}: query {q} lists a row twice"
        e = sc[q, nv[q]:]
        assert len(e) == 0 or (e[0] in empty and (e == e[0]).all()), f"{what}: query {q} empty slots {e[:4]}"
    a, b, both = sc[:, :-1], sc[:, 1:], v[:, 1:]
    ordered = (a > b) | ((a == b) & (ids[:, :-1] < ids[:, 1:]))
    assert ordered[both].all(), f"{what}: list not ordered by (score desc, id asc)"
    assert np.isfinite(sc[v]).all(), what
    return nv


def _listed_errors(sc, ids, exact):
    """|listed - exact| [Q, k] (nan in empty slots)."""
    v = ids >= 0
    ex = np.take_along_axis(exact, np.where(v, ids, 0), axis=1)
    return np.where(v, np.abs(sc - ex), np.nan)


def _print_table(scan, L, err, ids, q_fam, row_fam):
    """Measured maxima per (scan, L, family of query, family of row): the lines of profiles/scan_error_bounds.txt."""
    v = ids >= 0
    qf = np.broadcast_to(q_fam[:, None], ids.shape)[v]
    rf = row_fam[ids[v]]
    e = err[v]
    for a in np.unique(qf):
        for b in np.unique(rf[qf == a]):
            x = e[(qf == a) & (rf == b)]
            print(f"BOUND {scan:12s} L={L:<3d} {SC.FAMILIES[a]:12s} {SC.FAMILIES[b]:12s} max {x.max():.3e}  pairs {len(x)}")
    print(f"BOUND {scan:12s} L={L:<3d} {'ALL':12s} {'ALL':12s} max {e.max():.3e}  pairs {len(e)}")


_PREP = {}


def _prepared(c):
    """(queries, corpus) of a Case on the device, prepared once."""
    if id(c) not in _PREP:
        _PREP[id(c)] = (_queries(c.Q), _corpus(c.C), c)
    return _PREP[id(c)][:2]


def _const_branch(c):
    """[nq, N]: pairs the reference answers from a constant branch of the level-0 score (0.1 / 1.0 / 0.0)."""
    m = c.m
    return (O.np_std_rows(c.Q[:, :m]) == 0)[:, None] | (O.np_std_rows(c.C[:, :m]) == 0)[None, :]


# ---------------------------------------------------------------------------------------------- a


@pytest.mark.parametrize("n", [SC.N_SMALL, SC.N_LARGE])
@pytest.mark.parametrize("L", [64, 32])
@pytest.mark.parametrize("mode", [0, 1])
def test_split_scan_error_bound(hq_lib, mode, L, n):
    """Every pair the split-f16 scans list (level 0: hq_scan0_topk_split, overall: hq_scanov_topk_split) scores
    within the documented bound of the oracle, on every family; with N < k every row is listed, flagged rows
    (constant, f32-unsafe level-0 segments) included, and a constant pair's 0.1 is float32(0.1)."""
    from hq_mi355x.core.search_engine import IndexCorpus
    assert IndexCorpus.EPS == SC.EPS
    c = SC.case(L, n)
    qp, cp = _prepared(c)
    k = max(SC.LIST_LENGTHS)
    sc, ids, _, _ = _scan(qp, cp, mode, k)
    scan, B = ("scan0_split", SC.B_SCAN0) if mode == 0 else ("scanov_split", SC.B_SCANOV)
    fq = c.flagged_queries(mode)
    # a flagged query is not answered by the split scans: its list is (+inf, -1) throughout
    assert fq.any() and (ids[fq] == -1).all() and (sc[fq] == INF).all()
    sc, ids, exact = sc[~fq], ids[~fq], c.exact(mode)[~fq]
    nv = _check_lists(sc, ids, c.N, what=scan)
    assert (nv == min(k, c.N)).all(), "with no threshold the list holds min(k, N) rows"
    err = _listed_errors(sc, ids, exact)
    _print_table(scan, L, err, ids, c.q_fam[~fq], c.row_fam)
    assert np.nanmax(err) <= B
    if mode == 0:
        v = ids >= 0
        cb = np.take_along_axis(_const_branch(c)[~fq], np.where(v, ids, 0), axis=1) & v
        ex = np.take_along_axis(exact, np.where(v, ids, 0), axis=1)
        assert (cb.any() or c.N > k) and np.array_equal(sc[cb], ex[cb].astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("L", [64, 128, 256])
@pytest.mark.parametrize("via", ["scan_v1", "need_best"])
def test_f64_scan_error_bound(hq_lib, hq_option, via, L):
    """hq_scan_topk (reached by option scan_v1 and by the arg-max request) lists scores within 1e-12 of the
    oracle for L <= 64 (hq_mi355x.h) and within the suite's 1e-10 for longer vectors, one 60-row corpus per
    family against every family's queries; constant-branch scores are exact, and the arg-max is the list's
    first entry."""
    from hq_mi355x import _lib, kernels as K
    c = SC.case(L, 60, nq=8, n_unsafe=60, n_const=60, derived=False)
    B = SC.B_F64_SHORT if L <= 64 else SC.B_F64_LONG
    qp = _queries(c.Q)
    if via == "scan_v1":
        hq_option("scan_v1", 1)
    for mode in (0, 1):
        if mode == 1 and K.seg_padded_len(L) > 256:
            continue  # IndexCorpus._fused_ok(1): the overall scan does not fuse
        # 64 entries, or the longest list the scan's LDS holds at this L (57: L = 64 overall, 25: L = 128
        # overall, 57: the 128-value level 0 of L = 256); one entry more is refused, not mis-launched
        k = min(64, K.scan_max_list(L, mode))
        assert k >= 25
        if k < 64:
            with pytest.raises(_lib.NativeLibraryError, match="LDS"):
                K.scan_topk(qp, _corpus(c.C[:60]), mode, k + 1, need_best=(via == "need_best"))
        exact = c.exact(mode)
        const = _const_branch(c)
        worst = 0.0
        for fi, f in enumerate(SC.FAMILIES):
            rows = np.nonzero(c.row_fam == fi)[0]
            assert len(rows) == 60
            cp = _corpus(c.C[rows])
            sc, ids, best, bid = _scan(qp, cp, mode, k, need_best=(via == "need_best"))
            what = f"scan_f64 {via} mode {mode} L {L} rows {f}"
            nv = _check_lists(sc, ids, 60, what=what)
            assert (nv == min(k, 60)).all(), what
            ex = exact[:, rows]
            bad = _complete(sc, ids, ex, -np.sort(-ex, axis=1), 0.0, 0, k, B, what)
            assert not bad.any(), what
            err = _listed_errors(sc, ids, ex)
            worst = max(worst, np.nanmax(err))
            _print_table(f"scan_f64_m{mode}", L, err, ids, c.q_fam, np.full(60, fi))
            assert np.nanmax(err) < B if L <= 64 else np.nanmax(err) <= B, what
            if mode == 0:
                v = ids >= 0
                cb = np.take_along_axis(const[:, rows], np.where(v, ids, 0), axis=1) & v
                exl = np.take_along_axis(ex, np.where(v, ids, 0), axis=1)
                assert np.array_equal(sc[cb], exl[cb]), what
            if best is not None:
                assert np.array_equal(best, sc[:, 0]) and np.array_equal(bid, ids[:, 0]), what
        print(f"BOUND scan_f64_m{mode} L={L:<3d} via {via}: max {worst:.3e}")


def test_brute_force_past_the_f64_scan_list_limit(hq_lib):
    """L = 128 has no split overall layout, and its f64 overall scan holds lists of 25 entries: a brute-force
    search asking for more (max_results + SLACK) must take the dense exact path, not a launch that fails."""
    from hq_mi355x import kernels as K
    from hq_mi355x.core.search_engine import IndexCorpus
    rng = np.random.default_rng(128)
    C = rng.standard_normal((300, 128))
    Q = C[:5] + 0.05 * rng.standard_normal((5, 128))
    corpus = IndexCorpus(C)
    assert corpus.prep.Zov16 is None and corpus._max_list(1) == K.scan_max_list(128, 1) == 25
    for max_results in (10, 17, 18, 30, 56):   # 17 + SLACK = 25: the last list the scan takes
        ids, ov, _ = (_np(x) for x in corpus.brute_force(Q, max_results))
        for a in range(len(Q)):
            rid, rsc, _ = O.brute_force_search(Q[a], C, max_results)
            assert list(ids[a]) == list(rid), (max_results, a)
            assert np.abs(ov[a] - rsc).max() <= TOL


@pytest.mark.parametrize("L", [64, 32])
@pytest.mark.parametrize("src", ["all_f32", "mixed_rows"])
def test_f32_source_scan_error_bound(hq_lib, src, L):
    """float32 index vectors (every row: src_f32; some rows of an f64 pool: row_f32): listed scores within
    IndexCorpus.EPS of the oracle computed on float32 arrays (the tighter figures are derived for f64 sources)."""
    base = SC.case(L, SC.N_SMALL)
    C32, Q32 = base.C.astype(np.float32), base.Q.astype(np.float32)
    C, Q = C32.astype(np.float64), Q32.astype(np.float64)
    k = max(SC.LIST_LENGTHS)
    if src == "all_f32":
        qp, cp = _queries(Q, src_f32=True), _corpus(C, src_f32=True)
        is32 = np.ones(base.N, dtype=bool)
        Qo = Q32
    else:
        is32 = np.random.default_rng(5).random(base.N) < 0.5
        qp, cp = _queries(Q), _corpus(C, row_f32=is32)
        Qo = Q
    assert not bool(_np(cp.unsafe_rows()).any())  # (2^-100, 2^100): every family is inside the f32 model
    for mode in (0, 1):
        if mode == 0:
            e32 = np.stack([O.level_similarity(q, C32, 0) for q in Qo])
            e64 = np.stack([O.level_similarity(q, C, 0) for q in Qo]) if src != "all_f32" else e32
        else:
            e32 = np.stack([O.overall_similarity(q, C32)[0] for q in Qo])
            e64 = np.stack([O.overall_similarity(q, C)[0] for q in Qo]) if src != "all_f32" else e32
        exact = np.where(is32[None, :], e32, e64)
        sc, ids, _, _ = _scan(qp, cp, mode, k)
        fq = base.flagged_queries(mode)
        assert (ids[fq] == -1).all() and (sc[fq] == INF).all()
        what = f"{src} mode {mode}"
        nv = _check_lists(sc[~fq], ids[~fq], base.N, what=what)
        assert (nv == base.N).all(), what
        err = _listed_errors(sc[~fq], ids[~fq], exact[~fq])
        _print_table(f"{src}_m{mode}", L, err, ids[~fq], base.q_fam[~fq], base.row_fam)
        assert np.nanmax(err) <= SC.EPS, what


# ---------------------------------------------------------------------------------------------- b


def _complete(sc, ids, exact, desc, thr, thr_mode, k, B, what):
    """List completeness given |approximate - exact| <= B.  desc: exact sorted descending per query.
    Returns the queries whose lists are NOT complete (bool [Q]) - the caller decides what excuses them."""
    Q, N = exact.shape
    listed = np.zeros((Q, N), dtype=bool)
    r, s = np.nonzero(ids >= 0)
    listed[r, ids[r, s]] = True
    if thr_mode == 0:
        thr = -INF
    few = (exact >= thr - B).sum(axis=1) <= k
    must_few = exact > thr + B if thr_mode == 2 else exact >= thr + B
    kth = desc[:, min(k, N) - 1]
    must = np.where(few[:, None], must_few, exact > kth[:, None] + 2 * B)
    # efficiency, not correctness (kept loose on purpose): nothing far below the threshold is listed
    assert not (listed & (exact < thr - SC.EPS)).any(), f"{what}: a listed row lies below thr - EPS"
    return (must & ~listed).any(axis=1)


@pytest.mark.parametrize("n", [SC.N_SMALL, SC.N_LARGE])
@pytest.mark.parametrize("L", [64, 32])
@pytest.mark.parametrize("mode", [0, 1])
def test_list_completeness_sweep(hq_lib, mode, L, n):
    """Both threshold tests x 13 thresholds (three of them around 0.35, where gstar0's R changes sign) x 5 list
    lengths: with B the scan's bound, a list holds every row scoring >= thr + B when at most k rows reach
    thr - B, and otherwise every row more than 2 B above the k-th best exact score.  The level-0 pre-filter
    (gstar0, the dG slack, kMarginF) drops pairs before they are scored: one dropped wrongly fails here."""
    from hq_mi355x import kernels as K
    c = SC.case(L, n)
    qp, cp = _prepared(c)
    B = SC.B_SCAN0 if mode == 0 else SC.B_SCANOV
    fq = c.flagged_queries(mode)
    exact = c.exact(mode)[~fq]
    desc = -np.sort(-exact, axis=1)
    for thr_mode in (1, 2):
        for thr in SC.THRESHOLDS:
            for k in SC.LIST_LENGTHS:
                what = f"mode {mode} L {L} N {c.N} thr_mode {thr_mode} thr {thr} k {k}"
                sc, ids, _, _ = _scan(qp, cp, mode, k, thr, thr_mode)
                assert (ids[fq] == -1).all() and (sc[fq] == INF).all(), what
                _check_lists(sc[~fq], ids[~fq], c.N, what=what)
                bad = _complete(sc[~fq], ids[~fq], exact, desc, thr, thr_mode, k, B, what)
                assert not bad.any(), f"{what}: incomplete lists of queries {np.nonzero(bad)[0][:8]}"
    # a zero-variance or f32-unsafe query: the re-rank reports its (+inf, -1) list as unresolved
    asc, aid, _, _ = K.scan_topk(qp, cp, mode, 28, 0.1 - SC.EPS, 1)
    _, _, cnt, res = K.refine_topk(qp, cp, mode, asc, aid, 20, 0.1, 1, SC.EPS)
    assert fq.any() and not _np(res)[fq].any() and not _np(cnt)[fq].any()


@pytest.mark.parametrize("L", [64, 32])
@pytest.mark.parametrize("mode", [0, 1])
def test_scan_launch_geometry(hq_lib, mode, L):
    """Query counts around the 64-query wave block and corpus sizes around the 16-row step and the 4-row
    statistics group, at k = 8 without a threshold.  (The product answers N <= M densely, so its tests never
    run the scans at these sizes.)"""
    rng = np.random.default_rng(77 + L)
    C = rng.standard_normal((65, L))
    m = O.segment_bounds(L)[0][1]
    C[3, :m] = 0.25                      # a flagged row in the first group
    C[16] = C[0]                         # a tie across the first step boundary
    Qa = np.concatenate([rng.standard_normal((10, L)), C[np.arange(120) % 65] + 0.05 * rng.standard_normal((120, L))])
    B = SC.B_SCAN0 if mode == 0 else SC.B_SCANOV
    if mode == 0:
        exact = np.stack([O.level_similarity(q, C, 0) for q in Qa])
    else:
        exact = np.stack([O.overall_similarity(q, C)[0] for q in Qa])
    k = 8
    n_marked = n_lists = 0
    for nq in (1, 63, 64, 65, 130):
        qp = _queries(Qa[:nq])
        for N in (1, 15, 16, 17, 31, 33, 63, 65):
            what = f"mode {mode} L {L} Q {nq} N {N}"
            sc, ids, _, _ = _scan(qp, _corpus(C[:N]), mode, k)
            # the overall scan collects a wave's passing pairs (32 queries x the chunk's <= 16 rows) in a 256-entry
            # LDS buffer; a query whose pairs did not fit is handed to the dense path: (+inf, -1) throughout.
            # Nothing else may be, and never a level-0 list (its pools hold nchunks x k entries)
            marked = (ids == -1).all(axis=1) & (sc == INF).all(axis=1)
            assert not marked.any() or (mode == 1 and min(32, nq) * min(16, N) > 256), what
            n_marked += int(marked.sum())
            n_lists += nq
            sc, ids, ex = sc[~marked], ids[~marked], exact[:nq, :N][~marked]
            if not len(ids):
                continue
            nv = _check_lists(sc, ids, N, what=what)
            assert (nv == min(k, N)).all(), what
            assert np.nanmax(_listed_errors(sc, ids, ex)) <= B, what
            bad = _complete(sc, ids, ex, -np.sort(-ex, axis=1), 0.0, 0, k, B, what)
            assert not bad.any(), what
    print(f"mode {mode} L {L}: {n_marked} of {n_lists} lists handed to the dense path")
    assert 2 * n_marked <= n_lists


@pytest.mark.parametrize("mode", [0, 1])
def test_sampled_threshold_lists(hq_lib, hq_option, mode):
    """Past 16 x 4096 rows the scans start from a SAMPLED k-th score, which is not a bound: a list it cut short
    must say so (+inf in its empty slots); every other list, and every list under option sample_kth = 0 (the
    provable start), must be complete."""
    L, k = 64, 28
    c = SC.case(L, 8, nq=1, n_unsafe=1, n_const=1, extra_gauss=65_600)
    sel = np.nonzero(~c.flagged_queries())[0][:8]
    assert len(sel) == 8
    B = SC.B_SCAN0 if mode == 0 else SC.B_SCANOV
    qp, cp = _queries(c.Q[sel]), _corpus(c.C)
    exact = c.exact(mode)[sel]
    desc = -np.sort(-exact, axis=1)
    for kth in (None, 0):
        hq_option("sample_kth", kth)
        for thr_mode, thr in ((0, 0.0), (1, 0.36), (1, 0.8), (2, 0.5)):
            what = f"mode {mode} sample_kth {kth} thr_mode {thr_mode} thr {thr}"
            sc, ids, _, _ = _scan(qp, cp, mode, k, thr, thr_mode)
            _check_lists(sc, ids, c.N, empty=(-INF, INF), what=what)
            cut = (ids[:, -1] < 0) & (sc[:, -1] == INF)
            assert kth is None or not cut.any(), f"{what}: a provable start cut a list"
            err = _listed_errors(sc, ids, exact)
            assert np.nanmax(err) <= B, what
            bad = _complete(sc, ids, exact, desc, thr, thr_mode, k, B, what)
            assert not (bad & ~cut).any(), f"{what}: incomplete and unmarked lists {np.nonzero(bad & ~cut)[0]}"


# ---------------------------------------------------------------------------------------------- c

EPS_C = 2.0 ** -16   # the eps of the rule tests: a binary fraction, so that `last + eps == thr` can be hit exactly
THR_C = 0.75         # exact in float32 (the kernels compare against min(thr, float32(thr)))
TINY = 2.0 ** -40


def _sorted_list(ids, e, rng, eps):
    """(cand_score, cand_id) of the rows `ids`: exact + delta with |delta| <= eps, ordered as a scan orders."""
    cs = e[ids] + rng.uniform(-0.9 * eps, 0.9 * eps, len(ids))
    o = np.lexsort((ids, -cs))
    return cs[o], ids[o]


def _set_last(cs, target):
    cs = cs.copy()
    cs[:-1] = np.maximum(cs[:-1], target)
    cs[-1] = target
    return cs


def _rule_lists(c, exact, kp, k, rng):
    """One hand-made list per variant: (name, query, cand_score [kp], cand_id [kp])."""
    N, eps = c.N, EPS_C
    unfl = np.nonzero(~c.flagged_queries())[0]
    order = [np.lexsort((np.arange(N), -exact[q])) for q in range(len(exact))]
    out = []
    take = iter(unfl)

    def base(q, ids=None):
        return _sorted_list(order[q][:kp] if ids is None else ids, exact[q], rng, eps)

    # complete and provable: the last approximate score well below the k-th exact one
    q = next(take)
    cs, ids = base(q)
    out.append(("provable", q, _set_last(cs, min(cs[-1], exact[q][order[q][k - 1]] - 1.5 * eps)), ids))
    # the same for a constant query (the constant branches of the exact score: 0.1 / 1.0 / 0.0 with ties by id)
    q = int(np.nonzero(c.q_fam == SC.FAMILIES.index("const"))[0][0])
    cs, ids = base(q)
    out.append(("provable_const_query", q, cs, ids))
    # last approximate score within eps of the k-th exact score: nothing is proven
    q = next(take)
    cs, ids = base(q)
    out.append(("within_eps", q, _set_last(cs, exact[q][order[q][k - 1]] - 0.5 * eps), ids))
    # the true k-th entry missing from the list
    q = next(take)
    cs, ids = base(q, np.delete(order[q][:kp + 1], k - 1))
    out.append(("kth_removed", q, cs, ids))
    # not full: ends in (-inf, -1); and cut short by the scan: ends in (+inf, -1)
    for name, fill in (("not_full", -INF), ("truncated", INF)):
        q = next(take)
        cs, ids = base(q, order[q][:kp - 3])
        out.append((name, q, np.concatenate([cs, [fill] * 3]), np.concatenate([ids, [-1] * 3])))
    # too few pass THR_C on a full list, the bound just below / equal to / just above the threshold
    few = [q for q in unfl if 0 < (exact[q] >= THR_C).sum() < k // 2]
    assert len(few) >= 3, "the corpus has no query with few rows above THR_C"
    for name, q, d in (("few_below", few[0], -TINY), ("few_equal", few[1], 0.0), ("few_above", few[2], TINY)):
        cs, ids = base(q)
        j = int((exact[q][ids] >= THR_C).sum())
        cs[j:] = (THR_C - eps + d) + TINY * np.arange(kp - j - 1, -1, -1)  # descending, all below THR_C
        out.append((name, q, cs, ids))
    # ids outside the corpus: too few valid entries on a full list (never resolved without a threshold)
    q = next(take)
    cs, ids = base(q)
    ids = ids.copy()
    ids[k // 2:] = N + np.arange(kp - k // 2)
    out.append(("out_of_range", q, cs, ids))
    # six rows with the same exact score (query 0's row and its five copies) straddling the k-th position
    dup = np.concatenate([[c.q_rows[0]], np.arange(N - 5, N)])
    pos = np.array([int(np.nonzero(order[q] == dup[0])[0][0]) for q in unfl])
    fits = (pos >= k - 3) & (pos + 6 + kp - k - 3 <= N)   # k - 3 rows above the six, kp - k - 3 below
    # ... and no other row sharing their score (the clamp at 0.0 ties many rows)
    fits &= np.array([list(order[q][t:t + 6]) == list(dup) and exact[q][dup[0]] not in exact[q][order[q][[t - 1, t + 6]]]
                      if f else False for q, t, f in zip(unfl, pos, fits)])
    assert fits.any(), "no query ranks the duplicates where the list needs them"
    t = int(pos[fits].max())
    q = unfl[int(np.nonzero(fits & (pos == t))[0][0])]
    cs, ids = base(q, np.concatenate([order[q][t - (k - 3):t], dup, order[q][t + 6:t + 6 + kp - k - 3]]))
    out.append(("dups_at_kth", q, cs, ids))
    assert all(len(x[2]) == kp and len(x[3]) == kp for x in out)
    return out


def _option_sets(kp):
    """The re-rank kernels behind the options that survived the last prune (refine_launch in hq_search.hip)."""
    if kp <= 64:   # default k_rank_small; rank_ct: its compile-time level structures; then k_refine_lds, k_refine
        return [{}, {"rank_ct": 0}, {"rank_ct": 2}, {"refine_small": 0}, {"refine_small": 0, "refine_global": 1}]
    sets = [{}, {"rank_win": 0}, {"refine_coop": 0}]   # k_rank_pairs + k_rank_sort; its bitonic sort; refine_big
    if kp <= 128:
        sets.append({"rank_sort_small": 0})
    if kp > 512:
        sets.append({"rank_sort_nt": 512})
    return sets


@pytest.mark.parametrize("kp,k", [(28, 20), (64, 56), (108, 100), (1008, 1000)])
@pytest.mark.parametrize("L", [64, 32])
@pytest.mark.parametrize("mode", [0, 1])
def test_resolved_rule(hq_lib, hq_option, mode, L, kp, k):
    """out_resolved, out_count, out_id, out_score and the redo counter of both re-rank entry points equal
    scan_contract.resolved_rule on hand-made lists (one query per variant), under every kernel the options
    select, with and without count_empty, for no threshold and for both threshold tests."""
    import torch
    from hq_mi355x import kernels as K
    c = SC.case(L, SC.N_LARGE)
    exact = c.exact(mode)
    lists = _rule_lists(c, exact, kp, k, np.random.default_rng(kp + L + mode))
    qsel = np.array([x[1] for x in lists])
    qp, cp = _queries(c.Q[qsel]), _prepared(c)[1]
    cs, cid = _t(np.stack([x[2] for x in lists])), _t(np.stack([x[3] for x in lists]).astype(np.int64))
    redo = torch.zeros(1, dtype=torch.int32, device=cid.device)
    seen = set()
    for thr_mode, thr in ((0, 0.0), (1, 0.25), (2, 0.25), (1, THR_C), (2, THR_C)):
        want = [SC.resolved_rule(x[2], x[3], exact[x[1]], SC.passes(exact[x[1]], thr, thr_mode), k, thr, thr_mode,
                                 EPS_C) for x in lists]
        w_res, w_cnt = np.array([w[0] for w in want]), np.array([w[1] for w in want])
        w_id, w_sc = np.stack([w[2] for w in want]), np.stack([w[3] for w in want])
        seen |= {(x[0], bool(w[0])) for x, w in zip(lists, want)}
        for opts in _option_sets(kp):
            for name in ("refine_small", "refine_global", "refine_coop", "rank_ct", "rank_win", "rank_sort_nt",
                         "rank_sort_small"):
                hq_option(name, opts.get(name))
            for count_empty in (False, True):
                for fn in (K.refine_topk, K.refine_rescore_topk):
                    what = f"{fn.__name__} mode {mode} L {L} kp {kp} thr_mode {thr_mode} thr {thr} {opts} ce {count_empty}"
                    r = fn(qp, cp, mode, cs, cid, k, thr, thr_mode, EPS_C, redo=redo, count_empty=count_empty)
                    g_sc, g_id, g_cnt, g_res = (_np(x) for x in r[:4])
                    names = [x[0] for x in lists]
                    assert np.array_equal(g_res != 0, w_res), f"{what}: resolved {dict(zip(names, zip(g_res, w_res)))}"
                    assert np.array_equal(g_cnt, w_cnt), what
                    assert np.array_equal(g_id, w_id), what
                    assert np.array_equal(np.isfinite(g_sc), np.isfinite(w_sc)), what
                    fin = np.isfinite(w_sc)
                    assert np.array_equal(g_sc[~fin], w_sc[~fin]) and np.abs(g_sc[fin] - w_sc[fin]).max() <= TOL, what
                    assert int(_np(redo)[0]) == SC.redo_count(w_res, w_cnt, count_empty), what
    # the variants did what they were built for (a list that proves nothing would make the test vacuous)
    for name, res in (("provable", True), ("within_eps", False), ("not_full", True), ("truncated", False),
                      ("few_below", True), ("few_equal", True), ("few_equal", False), ("few_above", False),
                      ("out_of_range", False)):
        assert (name, res) in seen, f"variant {name} never gave resolved = {res}"


# ---------------------------------------------------------------------------------------------- d


@pytest.mark.parametrize("entry", ["hq_scan_topk", "hq_scan0_topk_split_fl", "hq_scanov_topk_split"])
def test_empty_corpus_lists(hq_lib, entry):
    """N == 0: every slot (-inf, -1) as the header promises, the arg-max of hq_scan_topk too (the re-rank
    reads cand_score[kp - 1] == +inf as "the scan cut this list": that slot must not be left unwritten)."""
    import torch
    from hq_mi355x import _lib
    from hq_mi355x._dev import device, ptr, stream
    Q, k, L = 5, 28, 64
    sc = torch.full((Q, k), 7.0, dtype=torch.float64, device=device())
    sc[:, -1] = INF                                  # what a stale buffer may well hold
    ids = torch.full((Q, k), 7, dtype=torch.int64, device=device())
    best = torch.full((Q,), 7.0, dtype=torch.float64, device=device())
    bid = torch.full((Q,), 7, dtype=torch.int64, device=device())
    lib = hq_lib
    if entry == "hq_scan_topk":
        rc = lib.hq_scan_topk(None, None, Q, None, None, 0, L, 0, k, 0.0, 0, 0, None, 0, ptr(sc), ptr(ids), ptr(best),
                              ptr(bid), stream())
    elif entry == "hq_scan0_topk_split_fl":
        rc = lib.hq_scan0_topk_split_fl(None, None, None, Q, None, None, None, 0, L, k, 0.0, 0, 0, None, 0, ptr(sc),
                                        ptr(ids), None, stream())
    else:
        rc = lib.hq_scanov_topk_split(None, None, None, None, Q, None, None, None, None, 0, L, k, 0.0, 0, 0, None, 0,
                                      ptr(sc), ptr(ids), stream())
    _lib.check(rc)
    assert (_np(sc) == -INF).all() and (_np(ids) == -1).all()
    if entry == "hq_scan_topk":
        assert (_np(best) == -INF).all() and (_np(bid) == -1).all()
