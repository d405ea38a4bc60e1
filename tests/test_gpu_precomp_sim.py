"""GPU parity of the pre-computed similarity scorer (`k_pre_stats`, `k_pre_pairs`, `k_pearson`) on the cases of
tests/precomp_sim_cases.py: arbitrary level lengths (every odd-length path of NumPy's pairwise sums), identical
and negated pairs whose result type follows the summation order, constant / NaN / inf / overflowing levels,
differing query and candidate offsets, and Q x N beyond one pass of the grid-stride loops.  Values and result
types are exact against the oracle, which tests/test_precomp_sim_cpu.py pins to the real reference
(tests/golden/precomp_sim.npz); the legacy Pearson's correlation branch, whose summation order is documented to
differ from BLAS, is bounded by np.corrcoef's own error against a long-double Pearson."""
import warnings

import numpy as np
import pytest

import precomp_sim_cases as P
from oracle import hq_oracle as O

pytestmark = pytest.mark.gpu

N_ROWS = 97


def _t(x):
    from hq_mi355x._dev import to_dev
    return to_dev(x)


def _np(x):
    from hq_mi355x._dev import to_np
    return to_np(x)


def _tiled(ref, n):
    reps = -(-n // len(ref))
    return np.tile(ref, (reps,) + (1,) * (ref.ndim - 1))[:n]


def _engine(weights=None):
    from hq_mi355x.core.precomputed_hilbert_index import PrecomputedHilbertIndexer, PrecomputedSimilaritySearchEngine
    return PrecomputedSimilaritySearchEngine(PrecomputedHilbertIndexer(), level_weights=weights)


def _level_type(value, overall_type):
    """The type _compare_precomputed_levels derives for a one-level table: float32 only strictly inside (0, 1)."""
    return P.TYPE_F32 if 0.0 < value < 1.0 and overall_type == P.TYPE_F32 else P.TYPE_PY


def _oracle_level(q, c):
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        v = O.precomputed_level_similarity(q, c)
    return float(v), P.type_code(v)


@pytest.fixture(scope="module")
def g(golden):
    return golden("precomp_sim")


@pytest.fixture(scope="module")
def by_length():
    """{m: (unique query rows, unique candidate rows)} of the single-level cases."""
    out = {}
    for (_, q, c) in P.single_level_cases():
        qs, cs = out.setdefault(len(q), ({}, {}))
        qs.setdefault(q.tobytes(), q)
        cs.setdefault(c.tobytes(), c)
    return {m: (np.stack(list(qs.values())), np.stack(list(cs.values()))) for m, (qs, cs) in out.items()}


@pytest.mark.parametrize("m", P.LENGTHS)
def test_single_level_matrix_vs_oracle(hq_lib, by_length, m):
    """Every query x candidate pair of one length in one launch, one-level table [0], [0], [m]."""
    Q, C = by_length[m]
    _, ty, lv = _engine([1.0]).similarity_matrix(Q, C, [0], [0], [m], levels=True)
    ty, lv = _np(ty), _np(lv)
    assert lv.shape == (len(Q), len(C), 1) and lv.dtype == np.float64 and ty.dtype == np.uint8
    for a in range(len(Q)):
        for b in range(len(C)):
            want, kind = _oracle_level(Q[a], C[b])
            assert lv[a, b, 0] == want, (m, a, b, lv[a, b, 0], want)
            assert _level_type(lv[a, b, 0], ty[a, b]) == kind, (m, a, b, lv[a, b, 0], ty[a, b], kind)


def test_single_level_dropin_matches_reference(hq_lib, g):
    """_compare_precomputed_levels returns the reference's recorded value and type for every named case."""
    from hq_mi355x.core.precomputed_hilbert_index import PrecomputedLevel
    eng = _engine()
    cases = P.single_level_cases()
    keep = [i for i, (n, q, _) in enumerate(cases) if len(q) <= 481 or n.endswith(("_same", "_neg", "_const"))]
    for i in keep:
        n, q, c = cases[i]
        v = eng._compare_precomputed_levels(PrecomputedLevel(2, 2, len(q), q, []), PrecomputedLevel(2, 2, len(c), c, []))
        assert float(v) == g["single_value"][i] and P.type_code(v) == g["single_type"][i], \
            (n, v, type(v), g["single_value"][i], g["single_type"][i])
        assert type(v) in (float, np.float32)


def test_stats_kernel(hq_lib):
    """K.precomputed_stats against np.mean / np.std / np.mean(a ** 2) and (a - mean) / std in float32, level
    lengths on every pairwise path, one empty level, constant rows (the normalised row stays zero)."""
    from hq_mi355x import kernels as K
    counts = [5, 0, 13, 129, 321, 1000, 7, 1]
    offsets, o = [], 3                       # the first level does not start at the row's start
    for c in counts:
        offsets.append(o)
        o += c + 2                           # gaps between levels stay untouched
    T = o
    rng = np.random.default_rng(8)
    A = (rng.standard_normal((9, T)) * rng.uniform(0.01, 100, (9, 1)) + rng.uniform(-5, 5, (9, 1))).astype(np.float32)
    A[3] = 0.5                               # constant: std == 0 at every level
    A[4] = np.float32(0.1)                   # inexact constant: np.std decides
    A[5] = 0.0
    A[6] *= np.float32(1e-30)                # squares underflow
    st, nrm = K.precomputed_stats(_t(A), offsets, counts)
    st, nrm = _np(st), _np(nrm)
    assert st.shape == (9, len(counts), 3) and st.dtype == np.float32 and nrm.shape == A.shape
    want_n = np.zeros_like(A)
    with np.errstate(all="ignore"):
        for r in range(9):
            for l, (o, c) in enumerate(zip(offsets, counts)):
                a = A[r, o:o + c]
                if c == 0:
                    want = np.zeros(3, np.float32)
                else:
                    want = np.array([np.mean(a), np.std(a), np.mean(a ** 2)], dtype=np.float32)
                    if want[1] != 0:
                        want_n[r, o:o + c] = (a - np.mean(a)) / np.std(a)
                assert st[r, l].tobytes() == want.tobytes(), (r, l, st[r, l], want)
    assert nrm.tobytes() == want_n.tobytes()
    assert not nrm[3].any() and not nrm[5].any()


@pytest.mark.parametrize("name", ["n32", "n16", "q32_c16"])
def test_multi_level_matrix(hq_lib, g, name):
    """overall, type and level similarities of every Q x N pair; q32_c16 has differing offsets, four common
    levels and counts = min."""
    Q, C = P.multi_level_cases()[name]
    qa = np.stack([P.pack(x)[0] for x in Q])
    ca = np.stack([P.pack(x)[0] for x in C])
    nl = min(len(Q[0]), len(C[0]))
    qo, co = P.pack(Q[0])[1][:nl], P.pack(C[0])[1][:nl]
    counts = [min(len(Q[0][l]), len(C[0][l])) for l in range(nl)]
    assert (qo != co) == (name == "q32_c16")
    ov, ty, lv = _engine().similarity_matrix(qa, ca, qo, co, counts, levels=True)
    ov, ty, lv = _np(ov), _np(ty), _np(lv)
    assert ov.tobytes() == g[f"multi_{name}_overall"].tobytes(), np.argwhere(ov != g[f"multi_{name}_overall"])[:5]
    assert ty.tobytes() == g[f"multi_{name}_type"].tobytes(), np.argwhere(ty != g[f"multi_{name}_type"])[:5]
    assert lv.tobytes() == g[f"multi_{name}_levels"].tobytes(), np.argwhere(lv != g[f"multi_{name}_levels"])[:5]
    with np.errstate(all="ignore"):
        for a, q in enumerate(Q):
            for b, c in enumerate(C):
                want, _ = O.precomputed_similarity(q, c)
                assert ov[a, b] == float(want) and ty[a, b] == P.type_code(want), (name, a, b)


def _indices(levels_list, n, prefix):
    from hq_mi355x.core.precomputed_hilbert_index import PrecomputedIndex, PrecomputedLevel
    return [PrecomputedIndex(f"{prefix}{i}", (n, n), [PrecomputedLevel(2, 2, len(a), a, []) for a in lv], 0.0, 0)
            for i, lv in enumerate(levels_list)]


def test_cross_layout_dropin_and_typed_threshold(hq_lib, g, monkeypatch):
    """A 32 x 32 query index against 16 x 16 candidate indices through _calculate_precomputed_similarity, and
    through search() with the threshold a quarter of a float32 ulp above one candidate's float32 score: the
    reference compares a numpy float32 score with the threshold in float32 (NEP 50), so that candidate passes;
    a Python-float score compares in float64."""
    import hq_mi355x.core.precomputed_hilbert_index as mod
    from hq_mi355x.models import ModelMetadata, QuantizedModel
    Q, C = P.multi_level_cases()["q32_c16"]
    ov, ty = g["multi_q32_c16_overall"], g["multi_q32_c16_type"]
    eng = _engine()
    qis, cis = _indices(Q, 32, "q"), _indices(C, 16, "c")
    for a, qi in enumerate(qis):
        for b, ci in enumerate(cis):
            v = eng._calculate_precomputed_similarity(qi, ci)
            assert float(v) == ov[a, b] and P.type_code(v) == ty[a, b], (a, b, v, type(v), ov[a, b], ty[a, b])
    # search(): the reference's SearchResult rejects level_similarities=, so record what would be returned
    monkeypatch.setattr(mod, "SearchResult", lambda **kw: (kw["model"].metadata.model_name, kw["similarity_score"]))
    models = [QuantizedModel(b"x", (16, 16), 256, 0.8, np.zeros(16), ModelMetadata(ci.model_id, 1, 1, 1.0, "t"))
              for ci in cis]
    for ci in cis:
        eng.indexer._index_cache[ci.model_id] = ci
    params = np.arange(1024, dtype=np.float32)
    eng.indexer._index_cache[f"query_{hash(params.tobytes())}"] = qis[0]
    f32_scores = sorted({float(v) for v, k in zip(ov[0], ty[0]) if k == P.TYPE_F32})
    assert len(f32_scores) >= 4 and (ty[0] == P.TYPE_PY).any()
    s = np.float32(f32_scores[len(f32_scores) // 2])                 # a float32 score with candidates on both sides
    quarter = float(np.nextafter(s, np.float32(2)) - s) / 4
    for thr in (float(s) + quarter, float(s) - quarter, float(s) + 3 * quarter, 0.09, 0.09 + 1e-12, 1.0):
        eng.similarity_threshold = thr
        want = [(f"c{b}", float(ov[0, b])) for b in range(len(cis))
                if (np.float32(ov[0, b]) >= np.float32(thr) if ty[0, b] == P.TYPE_F32 else float(ov[0, b]) >= thr)]
        want.sort(key=lambda x: x[1], reverse=True)
        got = eng.search(params, models, max_results=len(models))
        assert [(n, float(v)) for n, v in got] == want, thr
        assert all(P.type_code(v) == ty[0, int(n[1:])] for n, v in got)
    # the quarter-ulp threshold is above the score in float64, equal to it in float32
    assert float(s) < float(s) + quarter and np.float32(float(s) + quarter) == s
    eng.similarity_threshold = float(s) + quarter
    assert float(s) in [float(v) for _, v in eng.search(params, models, max_results=len(models))]


def _rows97(m, seed):
    rng = np.random.default_rng(seed)
    R = (rng.standard_normal((N_ROWS, m)) * rng.uniform(0.1, 10.0, (N_ROWS, 1))).astype(np.float32)
    R[11] = 0.0
    R[12] = -2.5
    R[13] = R[14]
    R[15] = -R[14]
    return R


def test_grid_stride_pairs(hq_lib):
    """Q x N = 65 x 65,000 pairs > 16384 x 256 threads: the pair kernel's loop runs a second, partial pass."""
    R = _rows97(5, 21)
    Qr = _rows97(5, 22)[:65]
    Qr[14] = R[14]
    N = 65_000
    assert len(Qr) * N > 16384 * 256
    ov, ty, lv = _engine([1.0]).similarity_matrix(Qr, _tiled(R, N), [0], [0], [5], levels=True)
    ov, ty, lv = _np(ov), _np(ty), _np(lv)[:, :, 0]
    want = np.array([[_oracle_level(q, c) for c in R] for q in Qr])
    wv, wt = want[:, :, 0], want[:, :, 1].astype(np.uint8)
    assert lv.tobytes() == _tiled(wv.T, N).T.tobytes()
    got_t = np.where((lv > 0) & (lv < 1) & (ty == P.TYPE_F32), P.TYPE_F32, P.TYPE_PY).astype(np.uint8)
    assert got_t.tobytes() == _tiled(wt.T, N).T.tobytes()
    assert ov.tobytes() == lv.tobytes()                              # one level of weight 1.0: the same clamp


def test_grid_stride_stats(hq_lib):
    """N x nlev = 530,000 x 8 > 16384 x 256 threads of the stats kernel."""
    from hq_mi355x import kernels as K
    counts = [5, 3, 1, 2, 7, 0, 9, 4]
    offsets = list(np.cumsum([0] + counts[:-1]))
    R = _rows97(sum(counts), 23)
    N = 530_000
    assert N * len(counts) > 16384 * 256
    st, nrm = K.precomputed_stats(_t(_tiled(R, N)), [int(o) for o in offsets], counts)
    s1, n1 = K.precomputed_stats(_t(R), [int(o) for o in offsets], counts)
    s1, n1 = _np(s1), _np(n1)
    with np.errstate(all="ignore"):
        for r in range(N_ROWS):
            for l, (o, c) in enumerate(zip(offsets, counts)):
                a = R[r, o:o + c]
                want = np.array([np.mean(a), np.std(a), np.mean(a ** 2)], np.float32) if c else np.zeros(3, np.float32)
                assert s1[r, l].tobytes() == want.tobytes(), (r, l)
    assert _np(st).tobytes() == _tiled(s1, N).tobytes()
    assert _np(nrm).tobytes() == _tiled(n1, N).tobytes()


@pytest.mark.parametrize("Qn,N", [(1, 1), (1, 257), (3, 1), (2, 256)])
def test_small_shapes(hq_lib, Qn, N):
    R, Qr = _rows97(13, 31), _rows97(13, 32)[:Qn]
    C = _tiled(R, N)
    _, ty, lv = _engine([1.0]).similarity_matrix(Qr, C, [0], [0], [13], levels=True)
    ty, lv = _np(ty), _np(lv)
    for a in range(Qn):
        for b in range(N):
            want, kind = _oracle_level(Qr[a], C[b])
            assert lv[a, b, 0] == want and _level_type(lv[a, b, 0], ty[a, b]) == kind, (a, b)


# ------------------------------------------------------------------------------------------ legacy Pearson


def _legacy_expected(q, c):
    """(exact value or None, long-double value) of the reference's compare_indices_at_level."""
    with np.errstate(all="ignore"):
        qs, cs = np.std(q), np.std(c)
        if qs == 0 and cs == 0:
            return (1.0 if np.allclose(q, c) else 0.0), None
        if qs == 0 or cs == 0:
            return 0.1, None
        if np.isnan(q).any() or np.isnan(c).any():
            return 0.0, None
        a, b = q.astype(np.longdouble), c.astype(np.longdouble)
        a, b = a - a.sum() / len(a), b - b.sum() / len(b)
        r = (a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum())
        return None, (r + 1) / 2


def test_legacy_pearson(hq_lib, g):
    """Branch cases exact; the correlation branch within 4 x np.corrcoef's own error against the long-double
    Pearson of the same vectors, plus 1e-15 (the kernel's summation order differs from BLAS, its accuracy should
    not).  Prints the measured ratios; the worst is recorded in profiles/pearson_error_bounds.txt."""
    from hq_mi355x import kernels as K
    worst = (0.0, "")
    for i, (name, q, c) in enumerate(P.legacy_cases()):
        got = float(_np(K.pearson_f64(_t(q), _t(c[None])))[0])
        ref = g["legacy_value"][i]                                   # the reference (np.corrcoef) on this case
        exact, ld = _legacy_expected(q, c)
        if exact is not None:
            assert ref == exact, (name, ref, exact)
            assert got == exact, (name, got, exact)
            continue
        err_np = abs(float(np.longdouble(ref) - ld))
        err = abs(float(np.longdouble(got) - ld))
        bound = 4 * err_np + 1e-15
        print(f"pearson {name}: kernel error {err:.3e}, corrcoef error {err_np:.3e}, bound {bound:.3e}, "
              f"ratio {err / bound:.3f}")
        if err / bound > worst[0]:
            worst = (err / bound, name)
        assert err <= bound, (name, got, ref, float(ld), err, bound)
    print(f"pearson worst ratio {worst[0]:.3f} at {worst[1]}")


def test_legacy_pearson_dropin_and_long_batch(hq_lib, g):
    """compare_indices_at_level of the drop-in on the branch cases, and N = 2,100,000 > 8192 x 256 candidates at
    m = 3 (97 distinct rows tiled): every output equals the output of its distinct row."""
    from hq_mi355x import kernels as K
    eng = _engine()
    for i, (name, q, c) in enumerate(P.legacy_cases()):
        exact, _ = _legacy_expected(q, c)
        if exact is not None:
            v = eng.compare_indices_at_level(q, c, 0)
            assert type(v) is float and v == exact == g["legacy_value"][i], (name, v, exact)
    R = _rows97(3, 41).astype(np.float64)
    q = R[20] + 0.25
    N = 2_100_000
    assert N > 8192 * 256
    one = _np(K.pearson_f64(_t(q), _t(R)))
    for r in range(N_ROWS):
        exact, ld = _legacy_expected(q, R[r])
        if exact is not None:
            assert one[r] == exact, r
        else:
            with np.errstate(all="ignore"):
                err_np = abs(float(np.longdouble((np.corrcoef(q, R[r])[0, 1] + 1) / 2) - ld))
            assert abs(float(np.longdouble(one[r]) - ld)) <= 4 * err_np + 1e-15, r
    many = _np(K.pearson_f64(_t(q), _t(_tiled(R, N))))
    assert many.tobytes() == _tiled(one, N).tobytes()
