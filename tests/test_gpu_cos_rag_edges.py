"""The frame-cosine and RAG scoring stage (S7) at its numeric and shape edges, against exact references
(cases, references and the derivation of every bound: cos_rag_cases.py; proof that the cases discriminate:
test_cos_rag_cases_cpu.py).

* MFMA cosine (hq_cos_prepare + hq_cos_scores_mfma / _f32): twelve row families x K = 1000 / 4096 / 16384 at
  Q = 17, N = 130 against the exact cosine: never above the contract's 1e-5, and per (family, K) within twice the
  maximum measured on an MI355X (profiles/cos_error_bounds.txt) rounded up to one digit.  pytest -s prints the
  lines that file is made of.
* hq_cosine_scores / hq_cosine_scores_dt, hq_spatial_locality: within 1e-12.  Derived, not measured: a K-term
  fma chain in float64 errs by at most about (K + 4) 2^-53 on the score, below 1e-12 for K <= 8192.
* hq_detect_heights, hq_threshold_select: exact."""
import numpy as np
import pytest

import cos_rag_cases as C
from oracle import hq_oracle as O

pytestmark = pytest.mark.gpu

F64_TOL = 1e-12


def _np(x):
    return x.detach().cpu().numpy()


def _dev(a):
    from hq_mi355x._dev import to_dev
    return to_dev(a)


# ------------------------------------------------------------------------------------------ MFMA cosine

_MFMA = {}


def _mfma(fam, K):
    """(A, B, exact, f64 scores, f32 scores) of one (family, K), computed once."""
    from hq_mi355x import kernels as K_
    if (fam, K) not in _MFMA:
        _MFMA.clear()  # tests run case by case: keep one case's arrays
        A, B = C.build(fam, K=K)
        pa, pb = K_.cos_prepare(_dev(A)), K_.cos_prepare(_dev(B))
        _MFMA[(fam, K)] = (A, B, C.exact_scores(A, B), _np(K_.cosine_scores_mfma(pa, pb)),
                           _np(K_.cosine_scores_mfma(pa, pb, f32=True)))
    return _MFMA[(fam, K)]


def _check_family(fam, K, got, exact):
    """Unaffected pairs finite and within the family's bound; pairs of a row holding a NaN / inf score exactly
    0.0 on this route (its inverse norm is 0: include/hq_mi355x.h)."""
    bad = C.affected(fam, *exact.shape)
    assert np.isfinite(got[~bad]).all(), f"{fam} K={K}: {np.count_nonzero(~np.isfinite(got[~bad]))} non-finite scores"
    err = float(np.max(np.abs(got - exact)[~bad]))
    print(f"  {fam:<14s} K={K:<6d} {err:.3e}")
    assert err <= C.HARD_CAP, (fam, K, err)
    assert err <= C.bound(fam, K), (fam, K, err, C.bound(fam, K))
    assert np.all(got[bad] == 0.0)
    return err


@pytest.mark.parametrize("K", C.MFMA_KS)
@pytest.mark.parametrize("fam", list(C.FAMILIES))
def test_mfma_cosine_family(hq_lib, fam, K):
    """|score - exact| <= min(1e-5, 2 x measured, one digit up) on every pair of finite rows, finite rows give
    finite scores, a NaN / inf row touches only its own outputs (tile padding and neighbouring rows stay
    isolated), and the float32 entry is the float64 score rounded once."""
    A, B, exact, s64, s32 = _mfma(fam, K)
    assert s64.shape == (C.MFMA_Q, C.MFMA_N) and s64.dtype == np.float64 and s32.dtype == np.float32
    _check_family(fam, K, s64, exact)
    np.testing.assert_array_equal(s32, s64.astype(np.float32))
    if fam == "orthogonal":
        assert np.all(s64 == 0.5)


@pytest.mark.parametrize("fam", C.ROUTE_FAMILIES)
def test_cosine_route_consistency(hq_lib, fam):
    """kernels.cosine_scores just below MFMA_COS_MIN_WORK (8 x 127 x 4096: the f64 kernel) and at it (8 x 128 x
    4096 = 2^22: the MFMA route) on the same rows: both finite, the common 8 x 127 block within the family's
    bound, each within its own bound of the exact score."""
    from hq_mi355x import kernels as K_
    Q, N, K = C.ROUTE_SHAPE
    assert K_.MFMA_COS_MIN_WORK == Q * N * K
    A, B = C.build(fam, Q, N, K, seed=3)
    exact = C.exact_scores(A, B)
    below = _np(K_.cosine_scores(_dev(A), _dev(B[: N - 1])))
    at = _np(K_.cosine_scores(_dev(A), _dev(B)))
    assert np.isfinite(below).all() and np.isfinite(at).all(), fam
    print(f"  {fam:<14s} f64 {np.max(np.abs(below - exact[:, : N - 1])):.3e}  mfma {np.max(np.abs(at - exact)):.3e}")
    assert np.max(np.abs(below - exact[:, : N - 1])) <= F64_TOL
    assert np.max(np.abs(at - exact)) <= C.bound(fam, K)
    assert np.max(np.abs(at[:, : N - 1] - below)) <= C.bound(fam, K)


@pytest.mark.parametrize("K", (1000, 4096))
@pytest.mark.parametrize("fam", ("subnormal", "huge"))
def test_mfma_cosine_rowmajor_prepare(hq_lib, hq_option, fam, K):
    """cos_kernel 1 (row-major k_cos_prepare + the register-staged kernel) on the rows whose scale leaves the
    float32 range: the same bound, and the same bits as the default tiled route."""
    from hq_mi355x import kernels as K_
    A, B, exact, s64, _ = _mfma(fam, K)
    hq_option("cos_kernel", 1)
    got = _np(K_.cosine_scores_mfma(K_.cos_prepare(_dev(A)), K_.cos_prepare(_dev(B))))
    hq_option("cos_kernel", None)
    _check_family(fam, K, got, exact)
    assert got.tobytes() == s64.tobytes()


# ------------------------------------------------------- hq_cosine_scores / hq_cosine_scores_dt (f64 kernels)


def _cos_f32(a, b):
    """hq_cosine_scores (float32 rows), straight through the C ABI."""
    import torch
    from hq_mi355x import _lib
    from hq_mi355x._dev import ptr, stream
    ta, tb = _dev(np.ascontiguousarray(a, np.float32)), _dev(np.ascontiguousarray(b, np.float32))
    out = torch.full((a.shape[0], b.shape[0]), -7.0, dtype=torch.float64, device="cuda")
    _lib.check(_lib.lib().hq_cosine_scores(ptr(ta), a.shape[0], ptr(tb), b.shape[0], a.shape[1], ptr(out), stream()))
    return out


def _cos_dt(a, b):
    """hq_cosine_scores_dt in the arrays' dtype (float32 or float64), straight through the C ABI."""
    import torch
    from hq_mi355x import _lib
    from hq_mi355x._dev import dtype_code, ptr, stream
    assert a.dtype == b.dtype
    ta, tb = _dev(np.ascontiguousarray(a)), _dev(np.ascontiguousarray(b))
    out = torch.full((a.shape[0], b.shape[0]), -7.0, dtype=torch.float64, device="cuda")
    _lib.check(_lib.lib().hq_cosine_scores_dt(dtype_code(ta.dtype), ptr(ta), a.shape[0], ptr(tb), b.shape[0],
                                              a.shape[1], ptr(out), stream()))
    return out


ENTRIES = [("hq_cosine_scores", np.float32), ("hq_cosine_scores_dt", np.float32), ("hq_cosine_scores_dt", np.float64)]


def _entry(name, dt):
    return (lambda a, b: _cos_f32(a, b)) if name == "hq_cosine_scores" else (lambda a, b: _cos_dt(a.astype(dt), b.astype(dt)))


@pytest.mark.parametrize("K", (0, 1, 2, 63, 4096))
@pytest.mark.parametrize("name,dt", ENTRIES, ids=[f"{n}-{np.dtype(d).name}" for n, d in ENTRIES])
def test_f64_cosine_edges(hq_lib, name, dt, K):
    """Within 1e-12 of the exact score for K = 0 (every score 0.0: no element, both norms 0), 1, 2, 63, 4096;
    zero rows and rows of -0.0 give 0.0; identical rows within an ulp of 1; antiparallel rows within 1e-15 of 0;
    a NaN row makes exactly its own outputs NaN, except against a zero row (0.0: the norm test comes first)."""
    r = np.random.default_rng(K + 11)
    A = r.standard_normal((5, K)).astype(dt)
    B = r.standard_normal((8, K)).astype(dt)
    if K:
        A[1] = 0.0
        B[2] = -0.0
        B[3] = A[0]
        B[4] = -2.0 * A[0]
        B[5] = 0.5 * A[0]
        A[3, K // 2] = np.nan
        B[6, 0] = np.nan
    got = _np(_entry(name, dt)(A, B))
    exact = C.exact_scores(A, B)
    if K == 0:
        assert np.all(got == 0.0)
        return
    nan = np.isnan(exact)
    want_nan = np.zeros_like(nan)
    want_nan[3, :] = True
    want_nan[:, 6] = True
    want_nan[1, :] = False  # the zero query row
    want_nan[:, 2] = False  # the -0.0 frame row
    np.testing.assert_array_equal(nan, want_nan)
    np.testing.assert_array_equal(np.isnan(got), want_nan)
    assert np.max(np.abs(got - exact)[~nan]) <= F64_TOL
    assert np.all(got[1] == 0.0) and np.all(got[:, 2] == 0.0)
    assert abs(got[0, 3] - 1.0) <= 2.3e-16 and abs(got[0, 5] - 1.0) <= 2.3e-16
    assert abs(got[0, 4]) <= 1e-15


def test_f64_cosine_float64_rows(hq_lib):
    """float64 rows stay float64: 1 + 1e-7 N(0, 1) at 3 x 5 pairs within 1e-12 of the exact score; standard-normal
    float64 rows too, where the same rows narrowed to float32 are more than 1e-11 (ten times the tolerance) away
    from the exact score, so narrowing would show; rows whose squares underflow (1e-170) have a float64 norm of 0 and score 0.0, as
    NumPy and the oracle do."""
    r = np.random.default_rng(3)
    A = 1.0 + 1e-7 * r.standard_normal((3, 4096))
    B = 1.0 + 1e-7 * r.standard_normal((5, 4096))
    got = _np(_cos_dt(A, B))
    assert np.max(np.abs(got - C.exact_scores(A, B))) <= F64_TOL
    assert np.max(np.abs(O.rag_cosine(A[0], B) - got[0])) <= F64_TOL
    A, B = r.standard_normal((3, 4096)), r.standard_normal((5, 4096))
    exact = C.exact_scores(A, B)
    assert np.min(np.abs(C.exact_scores(A.astype(np.float32), B.astype(np.float32)) - exact)) > 10 * F64_TOL
    assert np.max(np.abs(_np(_cos_dt(A, B)) - exact)) <= F64_TOL
    tiny = np.full((2, 8), 1e-170)
    assert np.all(O.rag_cosine(tiny[0], tiny) == 0.0)
    assert np.all(_np(_cos_dt(tiny, tiny)) == 0.0)
    assert np.all(_np(_cos_dt(tiny, np.ones((1, 8)))) == 0.0)


def _torch_scores(a, b):
    """(cos + 1) / 2 on the device in torch float64, the kernels' formula (element-wise: K is 2 or 3)."""
    import torch
    a, b = a.double(), b.double()
    dot = sum(a[:, k:k + 1] * b[:, k][None, :] for k in range(a.shape[1]))
    na, nb = (a * a).sum(1), (b * b).sum(1)
    s = (dot / (na.sqrt()[:, None] * nb.sqrt()[None, :]) + 1.0) / 2.0
    return torch.where((na == 0)[:, None] | (nb == 0)[None, :], torch.zeros_like(s), s)


@pytest.mark.parametrize("name,dt,Q,N,K", [("hq_cosine_scores", np.float32, 2049, 2048, 3),
                                           ("hq_cosine_scores_dt", np.float64, 4097, 4096, 2)],
                         ids=["hq_cosine_scores", "hq_cosine_scores_dt"])
def test_f64_cosine_grid_stride(hq_lib, name, dt, Q, N, K):
    """More outputs than one pass of the grid covers (16384 x 256 for hq_cosine_scores, 65536 x 256 for
    hq_cosine_scores_dt), compared on the device."""
    r = np.random.default_rng(Q)
    A, B = r.standard_normal((Q, K)).astype(dt), r.standard_normal((N, K)).astype(dt)
    A[Q - 1] = 0.0
    B[7] = 0.0
    got = _entry(name, dt)(A, B)
    want = _torch_scores(_dev(A), _dev(B))
    assert float((got - want).abs().max()) <= F64_TOL
    assert bool((got[Q - 1] == 0).all()) and bool((got[:, 7] == 0).all())
    assert float(got[: Q - 1, 8:].min()) >= 0.0  # every output written (prefilled with -7)


# --------------------------------------------------------------------------------------- hq_detect_heights


@pytest.mark.parametrize("dt", (np.float32, np.float64), ids=("f32", "f64"))
def test_detect_heights_edges(hq_lib, dt):
    """Exactly oracle.rag_detect_height for H in {1, 2, 63, 64, 65, 200} x W in {1, 2, 3, 7, 8, 64, 129}: rows with
    exactly W / 2 zeros (even W) or (W + 1) / 2 (odd W) do not end the embedding, one zero fewer does; -0.0 counts
    as zero, subnormals and NaN do not; no qualifying row gives H, only row 0 gives 1."""
    from hq_mi355x.rag import similarity as S
    for H in C.DETECT_H:
        for W in C.DETECT_W:
            cases = C.detect_images(H, W, dt)
            got = S.detect_original_embedding_heights(np.stack([img for _, img in cases]))
            want = [O.rag_detect_height(img) for _, img in cases]
            assert list(got) == want, (H, W, [n for (n, _), g, w in zip(cases, got, want) if g != w])


def test_detect_heights_grid_stride(hq_lib):
    """65537 images of 2 x 2: one more than the grid."""
    from hq_mi355x.rag import similarity as S
    r = np.random.default_rng(1)
    imgs = r.choice(np.array([0.0, -0.0, 1.0, np.nan, 5e-324]), size=(65537, 2, 2))
    ok = 2 * (imgs == 0).sum(axis=2) < 2
    want = np.where(ok[:, 1], 2, np.where(ok[:, 0], 1, 2))
    for i in (0, 1, 65535, 65536):
        assert want[i] == O.rag_detect_height(imgs[i])
    assert len(set(want.tolist())) == 2
    np.testing.assert_array_equal(S.detect_original_embedding_heights(imgs), want)


# -------------------------------------------------------------------------------------- hq_spatial_locality


@pytest.mark.parametrize("dt", (np.float32, np.float64), ids=("f32", "f64"))
def test_spatial_locality_shapes(hq_lib, dt):
    """Within 1e-12 of oracle.rag_spatial_locality_enhanced (which widens float32 images to float64, as the kernel
    does) for every (h, W) of SPATIAL_SHAPES with two index rows appended (h < H): both window-side transitions on
    either axis, window counts 49 .. 1192, a zero-norm window inside the mean, -0.0, and a stored image of another
    detected height (exactly 0.0)."""
    from hq_mi355x.rag import similarity as S
    for h, W, ws, _, _ in C.SPATIAL_SHAPES:
        q, c, hq, hc = C.spatial_images(h, W, dt)
        assert list(S.detect_original_embedding_heights(c)) == hc
        got = _np(S.spatial_locality_scores(q, c))
        want = np.array([[O.rag_spatial_locality_enhanced(a, b) for b in c] for a in q])
        assert np.max(np.abs(got - want)) <= F64_TOL, (h, W, float(np.max(np.abs(got - want))))
        if hc[3] != h:
            assert np.all(got[:, 3] == 0.0), (h, W)
        if ws >= 2:
            assert np.all(got[:, :3] > 0.0), (h, W)


@pytest.mark.parametrize("dt", (np.float32, np.float64), ids=("f32", "f64"))
def test_spatial_locality_many_pairs(hq_lib, dt):
    """One launch of 257 x 256 pairs of 8 x 8 images (more pairs than workgroups): workgroups 0 .. 255 score two
    pairs in a row, first with two different queries of height 8 (49 windows each: a window list kept from the
    first pair shows), then with queries of height 8 and 4 (windows, then the whole-block branch: a stale LDS slot
    shows).  The oracle runs on the 6 x 5 distinct pairs and is expanded by index."""
    from hq_mi355x.rag import similarity as S
    dq, dc, iqs, ic, hq, hc = C.many_pair_images(dt)
    want = np.array([[O.rag_spatial_locality_enhanced(a, b) for b in dc] for a in dq])
    assert len({round(v, 9) for v in want.ravel()}) >= 10  # distinct pairs score differently
    for iq in iqs:
        got = _np(S.spatial_locality_scores(dq[iq], dc[ic]))
        assert got.shape == (257, 256)
        assert np.max(np.abs(got - want[iq][:, ic])) <= F64_TOL
        differ = np.array(hq)[iq][:, None] != np.array(hc)[ic][None, :]
        assert np.all(got[differ] == 0.0) and np.all(got[~differ] > 0.0)


def test_spatial_locality_size_limit(hq_lib):
    """H W = 8192 (128 x 64: 64 KiB of window scores in LDS) works in both dtypes; 64 x 129 is refused with the
    library's "unsupported" error, and the next call still works."""
    from hq_mi355x import _lib
    from hq_mi355x.rag import similarity as S
    r = np.random.default_rng(2)
    for dt in (np.float32, np.float64):
        q = r.standard_normal((1, 128, 64)).astype(dt)
        c = np.stack([q[0] + 0.3 * r.standard_normal((128, 64)), r.standard_normal((128, 64))]).astype(dt)
        want = np.array([[O.rag_spatial_locality_enhanced(q[0], b) for b in c]])
        assert np.max(np.abs(_np(S.spatial_locality_scores(q, c)) - want)) <= F64_TOL
    big = np.ones((1, 64, 129), np.float32)
    with pytest.raises(_lib.NativeLibraryError, match=r"error -5: image 64x129"):
        S.spatial_locality_scores(big, big)
    q, c, _, _ = C.spatial_images(8, 8, np.float32)
    want = np.array([[O.rag_spatial_locality_enhanced(a, b) for b in c] for a in q])
    assert np.max(np.abs(_np(S.spatial_locality_scores(q, c)) - want)) <= F64_TOL


# ------------------------------------------------------------------------------------- hq_threshold_select


def _select(scores, ids, thr, cap, out_ids=True):
    """hq_threshold_select through the C ABI; outputs prefilled with -7."""
    import torch
    from hq_mi355x import _lib
    from hq_mi355x._dev import ptr, stream
    sc = _dev(np.ascontiguousarray(scores, np.float64))
    Q, N = scores.shape
    idt = None if ids is None else _dev(np.ascontiguousarray(ids, np.int64))
    out = torch.full((Q, max(cap, 1)), -7, dtype=torch.int64, device="cuda") if out_ids else None
    cnt = torch.full((Q,), -7, dtype=torch.int64, device="cuda")
    _lib.check(_lib.lib().hq_threshold_select(ptr(sc), ptr(idt), Q, N, float(thr), cap, ptr(out), ptr(cnt), stream()))
    return (None if out is None else _np(out)), _np(cnt)


@pytest.mark.parametrize("N", C.SELECT_N)
def test_threshold_select_edges(hq_lib, N):
    """The first `cap` candidates with score >= threshold, in order, -1 padded, exactly: rows where all / none /
    half pass, scores equal to the threshold (pass) and one ulp below (fail), NaN (never passes) and +-inf; caps
    of 1, inside a 64-lane ballot word, on its last lane, N and past N; with and without ids."""
    from hq_mi355x.rag import similarity as S
    rows = C.select_rows(N)
    sc = np.stack([s for _, s in rows])
    ids = np.random.default_rng(N).permutation(len(rows) * N).reshape(len(rows), N).astype(np.int64) + 10 ** 12
    for cap in C.select_caps(N):
        for use in (None, ids):
            out, cnt = _select(sc, use, C.SELECT_THR, cap)
            want, wcnt = C.select_expected(sc, use, C.SELECT_THR, cap)
            np.testing.assert_array_equal(cnt, wcnt, err_msg=f"N={N} cap={cap}")
            np.testing.assert_array_equal(out, want, err_msg=f"N={N} cap={cap} ids={'yes' if use is not None else 'no'}")
    names = [n for n, _ in rows]
    out, cnt = _select(sc, None, C.SELECT_THR, N)
    assert cnt[names.index("all pass")] == N and cnt[names.index("none pass")] == 0 and cnt[names.index("all nan")] == 0
    # the drop-in against the oracle's _apply_progressive_threshold, thresholds 0.6 .. 0.3 placed on the scores
    for level in range(4):
        thr, cap = S.progressive_threshold(level, N)
        lv = np.where(sc == C.SELECT_THR, thr, sc)
        out, cnt = (_np(x) for x in S.progressive_threshold_batch(lv, level))
        assert out.shape == (len(rows), cap)
        for q in range(len(rows)):
            want = O.rag_progressive_threshold(list(enumerate(lv[q].tolist())), level)
            assert list(out[q][: cnt[q]]) == want and np.all(out[q][cnt[q]:] == -1), (N, level, names[q])


def test_threshold_select_row_loop_and_cap_zero(hq_lib):
    """8193 rows of 70 on 8192 workgroups; cap = 0 (include/hq_mi355x.h): every count is written as 0 and out_ids,
    which has no columns, is neither read nor written (NULL allowed)."""
    r = np.random.default_rng(4)
    sc = r.random((8193, 70))
    out, cnt = _select(sc, None, 0.5, 20)
    want, wcnt = C.select_expected(sc, None, 0.5, 20)
    np.testing.assert_array_equal(cnt, wcnt)
    np.testing.assert_array_equal(out, want)
    out, cnt = _select(sc[:5], None, 0.5, 0)
    assert np.all(cnt == 0) and np.all(out == -7)
    out, cnt = _select(sc[:5], None, 0.5, 0, out_ids=False)
    assert out is None and np.all(cnt == 0)
