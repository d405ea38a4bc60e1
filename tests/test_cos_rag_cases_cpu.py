"""The cases of cos_rag_cases.py discriminate (no GPU): the exact references agree with each other and with the
oracle, the oracle's cosine propagates NaN as the reference does, a NumPy model of the MFMA route's arithmetic
exceeds a family's asserted bound under every mutation tried, the scale expression the prepare kernels used
before fails the subnormal family, and the spatial shapes reach every branch they claim to."""
import importlib
import importlib.util

import numpy as np

import cos_rag_cases as C
from oracle import hq_oracle as O

FINITE = [f for f in C.FAMILIES if f not in C.NAN_ROWS]
MQ, MN = 6, 24  # the model's batch: fewer pairs than the GPU test's 17 x 130 can only make a mutation harder to see


def test_exact_references_agree():
    """exact_scores (long double) == fsum_scores (math.fsum of the exact float64 products) within 1e-15 on
    every finite family, and both agree with oracle.rag_cosine (float64 BLAS dot) within (K + 4) 2^-53 =
    1.2e-13 at K = 1000; the measured-bound table covers every (family, K) of the GPU test."""
    for fam in FINITE:
        A, B = C.build(fam, 3, 5, 1000, seed=1)
        ex = C.exact_scores(A, B)
        fs = C.fsum_scores(A, B)
        for (q, n), v in fs.items():
            assert abs(ex[q, n] - v) <= 1e-15, (fam, q, n)
        for q in range(3):
            assert np.max(np.abs(O.rag_cosine(A[q], B) - ex[q])) <= 1.2e-13, fam
    A, B = C.build("near_const", 2, 3, 16384, seed=1)  # the longest sum of same-sign products
    ex = C.exact_scores(A, B)
    for (q, n), v in C.fsum_scores(A, B, [(0, 0), (1, 2)]).items():
        assert abs(ex[q, n] - v) <= 1e-15
    A, B = C.build("orthogonal", 3, 5, 1000)
    assert np.all(C.exact_scores(A, B) == 0.5)
    A, B = C.build("antiparallel", 3, 6, 1000)
    assert np.all(np.abs(C.exact_scores(A, B)[np.arange(6) % 3, np.arange(6)]) < 1e-7)  # c_n a rounds to float32
    # float64 rows: the long double product is within 2^-64
    r = np.random.default_rng(5)
    a, b = 1.0 + 1e-7 * r.standard_normal((2, 63)), 1.0 + 1e-7 * r.standard_normal((3, 63))
    for q in range(2):
        assert np.max(np.abs(O.rag_cosine(a[q], b) - C.exact_scores(a, b)[q])) <= 1e-15
    table = C.measured()
    assert set(table) == {(f, K) for f in C.FAMILIES for K in C.MFMA_KS}
    assert all(0 <= C.bound(f, K, table) <= C.HARD_CAP for f, K in table)
    assert (C.ceil_1sig(2e-7), C.ceil_1sig(2.01e-7), C.ceil_1sig(9.5e-7), C.ceil_1sig(0.0)) == (2e-7, 3e-7, 1e-6, 0.0)


def test_families_are_what_they_say():
    for K in (1000, 4096):
        A, B = C.build("subnormal", K=K)
        assert max(np.abs(A).max(), np.abs(B).max()) < 2.0 ** -128 and np.count_nonzero(A) > 0.99 * A.size
        A, B = C.build("huge", K=K)
        for X in (A, B):
            m = np.abs(X).max(axis=1)
            assert np.all(m >= 2.0 ** 127) and np.all(np.isfinite(X))
        A, B = C.build("tiny_normal", K=K)
        assert 1e-32 < np.abs(A).mean() < 1e-29 and np.abs(A).max() > 2.0 ** -126
        A, B = C.build("u8_frames", K=K)
        assert np.all(A == np.round(A)) and A.min() == 0 and A.max() == 255
        A, B = C.build("near_const", K=K)
        assert 0.7 <= A.min() and A.max() <= 0.7011 and 0.9 <= B.min() and B.max() <= 0.9011
        A, B = C.build("spike", K=K)
        assert np.argmax(np.abs(A[0])) != np.argmax(np.abs(B[0])) and np.abs(A).max() >= 2.0 ** 20
        for fam, (qa, nb) in C.NAN_ROWS.items():
            A, B = C.build(fam, K=K)
            assert sorted(np.nonzero(~np.isfinite(A).all(axis=1))[0]) == sorted(qa)
            assert sorted(np.nonzero(~np.isfinite(B).all(axis=1))[0]) == sorted(nb)
            assert C.affected(fam, *C.exact_scores(A, B).shape).sum() == len(qa) * C.MFMA_N + len(nb) * C.MFMA_Q - len(qa) * len(nb)
    Q, N, K = C.ROUTE_SHAPE
    assert Q * N * K == 1 << 22 and Q * (N - 1) * K < 1 << 22


def test_oracle_cosine_propagates_nan():
    """rag/search/engine.py:654-660 returns 0.0 only when a norm is 0 (`if norm1 == 0 or norm2 == 0`) and the
    NaN of dot / (norm1 norm2) otherwise; oracle.rag_cosine must do the same (it mapped every NaN to 0.0, which
    would hide a kernel that swallowed NaN).  Compared with the reference function itself when the reference
    package is importable."""
    a = np.array([1.0, 2.0, 3.0, 4.0])
    B = np.array([[1.0, 2.0, 3.0, 4.0], [np.nan, 1.0, 1.0, 1.0], [0.0, 0.0, 0.0, 0.0], [np.inf, 1.0, 1.0, 1.0],
                  [-1.0, -2.0, -3.0, -4.0]])
    got = O.rag_cosine(a, B)
    assert got[0] == 1.0 and np.isnan(got[1]) and got[2] == 0.0 and np.isnan(got[3]) and got[4] == 0.0
    assert np.all(np.isnan(O.rag_cosine(B[1], B[[0, 1, 3]])))
    assert np.all(O.rag_cosine(B[2], B) == 0.0)                 # a zero norm wins over the partner's NaN
    assert np.all(O.rag_cosine(np.full(4, 1e-170), B[:1]) == 0.0)  # squares underflow: the float64 norm is 0
    for dt in (np.float32, np.float64):
        ex = C.exact_scores(a[None].astype(dt), B.astype(dt))[0]
        np.testing.assert_array_equal(np.isnan(ex), np.isnan(got))
        np.testing.assert_allclose(ex[~np.isnan(ex)], got[~np.isnan(got)], atol=1e-15)
    eng = None
    if importlib.util.find_spec("hilbert_quantization") is not None:
        try:
            eng = importlib.import_module("hilbert_quantization.rag.search.engine")
        except Exception:
            eng = None
    fn = None
    for obj in vars(eng).values() if eng is not None else ():
        if isinstance(obj, type) and hasattr(obj, "_calculate_embedding_cosine_similarity"):
            fn = obj._calculate_embedding_cosine_similarity
    if fn is not None:
        with np.errstate(all="ignore"):
            ref = np.array([fn(None, a, b) for b in B])
        np.testing.assert_array_equal(np.isnan(ref), np.isnan(got))
        np.testing.assert_allclose(ref[~np.isnan(ref)], got[~np.isnan(got)], atol=1e-15)


MUTATIONS = {"drop lo.hi": dict(drop=("lh",)), "drop hi.lo": dict(drop=("hl",)), "zero lo": dict(zero_lo=True),
             "truncating accumulator": dict(trunc=True)}
_MODEL = {}


def _model_errors():
    """{(family, K, mutation or None): max |model - exact|}, computed once."""
    if not _MODEL:
        for fam in FINITE:
            for K in C.MFMA_KS:
                A, B = C.build(fam, MQ, MN, K)
                ex = C.exact_scores(A, B)
                _MODEL[(fam, K, None)] = float(np.max(np.abs(C.model_scores(A, B) - ex)))
                for name, kw in MUTATIONS.items():
                    _MODEL[(fam, K, name)] = float(np.max(np.abs(C.model_scores(A, B, **kw) - ex)))
    return _MODEL


def test_model_as_designed_is_within_every_bound():
    """The unmutated model stays within the asserted bound of every (family, K): the bounds do not sit below
    what the arithmetic as designed can deliver."""
    err, table = _model_errors(), C.measured()
    for fam in FINITE:
        for K in C.MFMA_KS:
            assert err[(fam, K, None)] <= C.bound(fam, K, table), (fam, K, err[(fam, K, None)])
    # exact by construction, with and without mutations
    assert all(err[("orthogonal", K, m)] == 0.0 for K in C.MFMA_KS for m in (None, *MUTATIONS))


def test_families_discriminate_model_mutations():
    """Every mutation of the model pushes at least one family past its asserted bound at every K; u8_frames
    (integers 0 .. 255: hi holds them exactly, lo is 0) cannot see a mutation of the lo planes, and the same-sign
    families at K = 16384 see the truncating accumulator at 1.7e-5, above the 1e-5 contract.
    What the standard-normal family alone would have noticed: under the one bound asserted before this file
    (2e-6, on normal rows) the truncating accumulator passes at every K (2.5e-7 .. 4.3e-7) and so does a dropped
    lo.hi term at K = 16384 (1.7e-6); under its own measured bound (7e-8 .. 1e-7) it notices all four."""
    err, table = _model_errors(), C.measured()
    caught = {m: {(f, K) for f in FINITE for K in C.MFMA_KS if err[(f, K, m)] > C.bound(f, K, table)} for m in MUTATIONS}
    for m in MUTATIONS:
        for K in C.MFMA_KS:
            assert any(k == K for _, k in caught[m]), (m, K)
    for m in ("drop lo.hi", "drop hi.lo", "zero lo"):
        assert not any(f == "u8_frames" for f, _ in caught[m])
        assert all(err[("u8_frames", K, m)] == err[("u8_frames", K, None)] for K in C.MFMA_KS)
    for fam in ("pos_uniform", "near_const"):
        assert err[(fam, 16384, "truncating accumulator")] > C.HARD_CAP
        assert (fam, 16384) in caught["truncating accumulator"]
    old = 2e-6
    unnoticed_old = {(m, K) for m in MUTATIONS for K in C.MFMA_KS if err[("normal", K, m)] <= old}
    assert unnoticed_old == {("truncating accumulator", 1000), ("truncating accumulator", 4096),
                             ("truncating accumulator", 16384), ("drop lo.hi", 16384)}, unnoticed_old
    assert all(("normal", K) in caught[m] for m in MUTATIONS for K in C.MFMA_KS)


def test_scale_expression_on_subnormal_and_huge_rows():
    """x * ldexpf(1, -e) (the prepare kernels before the fix): for amax < 2^-128 the scale 2^-e overflows float32,
    hi is inf, lo is inf - inf = NaN and inv = 1 / (inf sqrt(ss)) = 0, so every accumulator of the row is NaN and
    the epilogue's zero-norm test turns it into 0.0: no score of the row is right (the exact ones are near 0.5,
    the f64 kernels return them).  ldexpf(x, -e) with inv =
    ldexp(1 / sqrt(ss), e) keeps them finite and within the family's bound, and on every other finite family
    (huge included: its scale 2^-128 is a float32 subnormal) the two forms give the same hi, lo and inv bits."""
    A, B = C.build("subnormal", MQ, MN, 1000)
    hi, lo, inv = C.model_prepare(A, "mul")
    assert np.all(np.isinf(hi[A != 0])) and np.all(np.isnan(lo[A != 0])) and np.all(inv == 0.0)
    old = C.model_scores(A, B, scale="mul")
    assert np.all(np.isnan(old) | (old == 0.0)) and np.all(C.exact_scores(A, B) > 0.4)
    hi, lo, inv = C.model_prepare(A, "ldexp")
    assert np.isfinite(hi).all() and np.isfinite(lo).all() and np.all(np.isfinite(inv) & (inv > 0))
    assert 0.5 <= np.abs(hi).max(axis=1).min() and np.abs(hi).max() <= 1.0
    got = C.model_scores(A, B, scale="ldexp")
    assert np.max(np.abs(got - C.exact_scores(A, B))) <= C.bound("subnormal", 1000)
    for fam in FINITE:
        if fam == "subnormal":
            continue
        X = np.concatenate(C.build(fam, MQ, MN, 1000))
        for u, v in zip(C.model_prepare(X, "mul"), C.model_prepare(X, "ldexp")):
            assert u.tobytes() == v.tobytes(), fam
    X = np.zeros((2, 64), np.float32)
    X[1, 3] = -0.0
    assert all(np.all(p == 0) for p in C.model_prepare(X, "ldexp"))


def test_spatial_shapes_reach_every_branch():
    """Window side, stride and window count of every listed (h, W), against the reference's own loops; the sides
    1 -> 2 -> 3 -> 4 change at 8, 12 and 16 on either axis; window counts on both sides of NumPy's 128-element
    pairwise block (126, 128, 130) and past 1024.  No (h, W) gives fewer than 49 windows (ws >= 2 needs h, W >= 8),
    so the pairwise sum's short path (fewer than 8 terms) cannot be reached, nor can 127 or 129."""
    for h, W, ws, st, nw in C.SPATIAL_SHAPES:
        assert C.window_plan(h, W) == (ws, st, nw), (h, W)
        assert ws == min(4, h // 4, W // 4)
        if ws >= 2:
            assert st == ws // 2
            assert nw == len([(i, j) for i in range(0, h - ws + 1, st) for j in range(0, W - ws + 1, st)])
    sides = {(h, W): ws for h, W, ws, _, _ in C.SPATIAL_SHAPES}
    assert (sides[(7, 16)], sides[(8, 8)], sides[(8, 7)]) == (1, 2, 1)
    assert (sides[(11, 12)], sides[(12, 12)], sides[(12, 11)]) == (2, 3, 2)
    assert (sides[(15, 16)], sides[(16, 16)], sides[(16, 15)]) == (3, 4, 3)
    counts = {nw for *_, nw in C.SPATIAL_SHAPES}
    assert {49, 126, 128, 130} <= counts and max(counts) > 1024 and C.window_plan(18, 34) == (4, 2, 128)
    hs = {h for h, *_ in C.SPATIAL_SHAPES} | {W for _, W, *_ in C.SPATIAL_SHAPES}
    assert {1, 3, 4, 7, 8, 11, 12, 15, 16, 17, 19} <= hs
    reachable = {C.window_plan(h, W)[2] for h in range(1, 400) for W in range(1, 400) if h * W <= 8192}
    assert min(reachable - {0}) == 49 and not reachable & {127, 129} and 128 in reachable
    for h, W, *_ in C.SPATIAL_SHAPES:
        assert (h + 2) * W <= 8192


def test_rag_references_agree_with_the_oracle():
    """detect_height_exact / spatial_exact / select_expected (integer rule, exact window cosines and mean, NumPy
    statement of the select) against oracle.rag_detect_height, rag_spatial_locality_enhanced (float64 BLAS; within
    (K + 4) 2^-53 = 1.5e-13 at the largest block, 9 x 150) and rag_progressive_threshold."""
    for H in C.DETECT_H:
        for W in C.DETECT_W:
            for dt in (np.float32, np.float64):
                seen = set()
                for name, img in C.detect_images(H, W, dt):
                    h = C.detect_height_exact(img)
                    assert h == O.rag_detect_height(img), (H, W, name)
                    seen.add(h)
                    if name == "only row 0":
                        assert h == 1
                    if name in ("all zero", "all -0.0"):
                        assert h == H
                    if name.startswith(("boundary row", "subnormal row", "nan row")):
                        assert h == int(name.split()[2].rstrip(",")) + 1, (H, W, name)
                assert {1, H} <= seen
    for h, W, ws, _, _ in C.SPATIAL_SHAPES:
        for dt in (np.float32, np.float64):
            q, c, hq, hc = C.spatial_images(h, W, dt)
            assert [O.rag_detect_height(x) for x in q] == hq and [O.rag_detect_height(x) for x in c] == hc
            for a in q:
                for j, b in enumerate(c):
                    want = O.rag_spatial_locality_enhanced(a, b)
                    assert abs(C.spatial_exact(a, b) - want) <= 1.5e-13, (h, W, j)
                    if hc[j] != h:
                        assert want == 0.0
            if ws >= 2:  # the zero window scores 0.0 inside the mean
                assert O.rag_cosine(q[0][:ws, :ws].ravel(), c[2][:ws, :ws].ravel()[None])[0] == 0.0
    dq, dc, (iq1, iq2), ic, hq, hc = C.many_pair_images(np.float32)
    assert [O.rag_detect_height(x) for x in dq] == list(hq) and [O.rag_detect_height(x) for x in dc] == list(hc)
    assert len(iq1) * len(ic) > 65536 and len(iq1) == len(iq2) == 257
    assert iq1[0] != iq1[256] and hq[iq1[0]] == hq[iq1[256]] == 8 and (hq[iq2[0]], hq[iq2[256]]) == (8, 4)
    assert {hc[i] for i in ic} == {8, 7, 4}
    for N in C.SELECT_N:
        for level in range(4):
            thr = min(0.3 + (0.1 * (3 - min(level, 3))), 0.8)
            cap = max(1, int(N * (0.3 if level == 0 else (0.5 if level == 1 else 0.7))))
            for name, sc in C.select_rows(N):
                sc = np.where(sc == C.SELECT_THR, thr, sc)
                out, cnt = C.select_expected(sc[None], None, thr, cap)
                want = O.rag_progressive_threshold(list(enumerate(sc.tolist())), level)
                assert list(out[0][: cnt[0]]) == want and np.all(out[0][cnt[0]:] == -1), (N, level, name)
