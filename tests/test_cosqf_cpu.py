"""Host-side checks of the float32-query route of the compressed-domain frame search (hq_cosqf_*): the contract's
integer formula against the long-double definition on every query and frame family, mutations of it that the
families must catch, the rounding bound against the query's own values, the padding functions, argument
validation through the loaded library, and the no-device behaviour of the Python layer.  No kernel is launched."""
import ctypes

import numpy as np
import pytest

import cosq_cases as C
import cosqf_cases as F

KS = (1, 64, 199, 4096)


@pytest.fixture(scope="module")
def lib():
    from hq_mi355x import _lib
    return _lib.load()


@pytest.mark.parametrize("K", KS)
def test_model_agrees_with_exact_reference(K):
    """The digit-plane formula is within 1e-13 of the long-double cosine of (v, dequantised frame), every query
    family against every frame family; dead rows score exactly 0.0."""
    q, names = F.all_families(K)
    U, MM, fnames = C.all_families(K)
    v, ok, _ = F.fix24(q)
    exact = F.exact_scores(v, U, MM, ok)
    model = F.model_scores(q, U, MM)
    err = np.abs(model - exact)
    print(f"cosqf-err model K{K} {err.max():.3e}")
    assert np.all(np.isfinite(model))
    assert err.max() <= F.TOL, (float(err.max()), names[int(np.argmax(err.max(axis=1)))])
    dead = F.dead_rows(names)
    assert not ok[dead].any() and ok.sum() == len(names) - len(dead)
    assert np.all(model[dead] == 0.0) and np.all(exact[dead] == 0.0)
    deadc = C.rows_of(fnames, {"const_zero", "nonfinite"})
    assert np.all(model[:, deadc] == 0.0)


def test_fix24_definition():
    """v at the edges of the definition: the clamp acts on +2^23 only, -2^23 is kept, ties go to even, subnormal
    rows and rows at FLT_MAX scale exactly, grid rows are exact multiples of q."""
    one_m = F.ONE_M
    v, ok, e = F.fix24(np.array([[one_m, -one_m, 0.5, 0.0]], np.float32))
    assert list(v[0]) == [2 ** 23 - 1, -2 ** 23, 2 ** 22, 0] and ok[0] and e[0] == 0
    assert F.fix24(np.array([[one_m]], np.float32), clamp=False)[0][0, 0] == 2 ** 23
    # ties to even at half a unit: amax = 1 - 2^-23 -> e = 0, unit 2^-23; 2.5 and 3.5 units
    v, _, _ = F.fix24(np.array([[1 - 2.0 ** -23, 2.5 * 2.0 ** -23, 3.5 * 2.0 ** -23, -2.5 * 2.0 ** -23]], np.float32))
    assert list(v[0]) == [2 ** 23 - 1, 2, 4, -2]
    v, ok, e = F.fix24(np.array([[1.4e-45, -4.2e-45], [C.FLT_MAX, -C.FLT_MAX / 2]], np.float32))
    assert ok.all() and list(e) == [-147, 128]
    assert list(v[0]) == [2 ** 21, -3 * 2 ** 21] and list(v[1]) == [2 ** 23 - 1, -2 ** 22]
    q, U, _ = F.grid_rows(5, 199, 3)
    v, _, _ = F.fix24(q)
    assert np.array_equal(v, U.astype(np.int64) << 15)   # 255 = 0.996 * 2^8: the scale is 2^15
    for bad in (np.nan, np.inf, -np.inf):
        assert not F.fix24(np.array([[1.0, bad]], np.float32))[1][0]
    assert not F.fix24(np.zeros((1, 3), np.float32))[1][0]


def test_digit_identity():
    """v = 65536 p2 + 256 p1 + p0 + 32896 with every digit an int8, over the whole 24-bit range's edges."""
    v = np.array([-2 ** 23, -2 ** 23 + 1, -65537, -65536, -257, -256, -129, -128, -1, 0, 1, 127, 128, 255, 256,
                  32767, 32768, 65535, 65536, 2 ** 23 - 2, 2 ** 23 - 1], np.int64)
    v = np.concatenate([v, np.random.default_rng(5).integers(-2 ** 23, 2 ** 23, 4096)])
    p0, p1, p2 = F.digits(v)
    for p in (p0, p1, p2):
        assert p.min() >= -128 and p.max() <= 127
    assert np.array_equal(65536 * p2 + 256 * p1 + p0 + 32896, v)


@pytest.mark.parametrize("mutation", [m for m in F.MUTATIONS if m != "float_t"])
def test_mutations_are_caught(mutation):
    """A dropped digit plane, a wrong digit offset, the unclamped +2^23 and the padded K in place of the true K
    each differ from the exact reference by more than 1e-9 on some family: four orders above the tolerance."""
    worst = 0.0
    for K in KS:
        q, _ = F.all_families(K)
        U, MM, _ = C.all_families(K)
        v, ok, _ = F.fix24(q)
        exact = F.exact_scores(v, U, MM, ok)
        with np.errstate(all="ignore"):
            bad = F.model_scores(q, U, MM, mutate=mutation)
        worst = max(worst, float(np.nanmax(np.abs(bad - exact))))
    print(f"cosqf-err mutation {mutation} {worst:.3e}")
    assert worst > 1e-9, (mutation, worst)


def test_float64_t_is_not_the_integer_t():
    """t = K D - Sv S_c from plain float64 products on the one-255 frames (and on frames of one small byte among
    zeros) with same-sign queries at K = 65536: both terms reach 2^62 and round before they cancel, so the float64
    t differs from the exact int64 t, which is what the contract asks for.  Measured here: the float64 t is off by up
    to 8 on the one-255 frames, which moves a score by 9e-16, and by 2.4e-13 on the one-small-byte frames: scores
    alone tell the two apart only there, and only just above 1e-13, so the integer t itself is compared.  The model
    with the integer t stays within 1e-13 of exact on both."""
    K = C.MAX_K
    q = np.concatenate([F.family("constant", K), F.family("relu", K), F.family("grid", K)])
    v, ok, _ = F.fix24(q)
    U1 = np.zeros((4, K), np.uint8)
    U1[np.arange(4), [5, 77, 1000, K - 1]] = [1, 1, 2, 3]
    M1 = np.array([(0, 1), (0, 255), (-1, 1), (0, 1e-20)], np.float32)
    for name, (U, MM) in (("one255", C.family("one255", K)), ("one-small-byte", (U1, M1))):
        s, ti, tf = F.model_scores(q, U, MM, with_t=True)
        exact = F.exact_scores(v, U, MM, ok)
        bad = F.model_scores(q, U, MM, mutate="float_t")
        dt = np.abs(tf - ti.astype(np.float64)).max()
        print(f"cosqf-err float-t {name} K{K}: |t_f64 - t_int| {dt:.0f}, score {np.abs(bad - exact).max():.3e}, "
              f"integer model {np.abs(s - exact).max():.3e}")
        assert np.abs(ti).max() < 2 ** 62
        assert dt >= 1.0, name                       # the float64 route is not exact
        assert np.abs(s - exact).max() <= F.TOL      # the integer route is, to a few roundings
    # the constant queries cancel exactly on every frame: K D == Sv S_c as integers
    assert np.all(ti[:4] == 0)


@pytest.mark.parametrize("K", KS + (C.MAX_K,))
def test_rounding_bound_against_the_float32_values(K):
    """|score of v - score of q| <= 2^(e - 24) sqrt(K) / |q| for every family, and below 1e-5 for the gaussian,
    post-ReLU and pipeline families."""
    q, names = F.all_families(K)
    U, MM, _ = (C.all_families(K) if K < C.MAX_K else C.random_rows(8, K, 5) + (None,))
    v, ok, _ = F.fix24(q)
    d = np.abs(F.true_scores(q, U, MM) - F.exact_scores(v, U, MM, ok))
    b = F.bound(q, K)
    for fam in F.FAMILIES:
        r = C.rows_of(names, {fam})
        print(f"cosqf-err rounding {fam} K{K} {d[r].max():.3e} (bound {b[r].max():.3e})")
    assert np.all(d <= b[:, None] + 1e-18)
    smooth = C.rows_of(names, set(F.SMOOTH))
    assert d[smooth].max() < 1e-5 and b[smooth].max() < 1e-5


def test_operand_map_inputs_are_asymmetric():
    """The operand-map queries: v = q, the three digit planes differ from one another, and swapping two planes,
    rows and columns, or the k order inside a step moves the scores by far more than the tolerance."""
    q, v = F.operand_map_queries(19, 199)
    assert np.array_equal(F.fix24(q)[0], v)
    p0, p1, p2 = F.digits(v)
    assert not np.array_equal(p0, p1) and not np.array_equal(p1, p2) and not np.array_equal(p0, p2)
    Uc, Mc = C.operand_map_rows(389, 199, 1)
    exact = F.exact_scores(v, Uc, Mc)
    assert np.abs(exact[:, :19] - exact[:, :19].T).max() > 1e-3
    for a, b, c in ((p1, p0, p2), (p0, p2, p1), (p2, p1, p0)):
        swapped = 65536 * c + 256 * b + a + 32896
        assert np.abs(F.exact_scores(swapped, Uc, Mc) - exact).max() > 1e-3
    Kp = C.padded_k(199)
    pad = np.zeros((19, Kp), np.int64)
    pad[:, :199] = v
    for group in (16, 64):
        rev = pad.reshape(19, Kp // group, group)[:, :, ::-1].reshape(19, Kp)[:, :199]
        assert np.abs(F.exact_scores(rev, Uc, Mc) - exact).max() > 1e-3


def test_accumulator_rows_reach_the_int32_extremes():
    q = F.accumulator_queries()
    U, _ = F.accumulator_frames()
    v, ok, _ = F.fix24(q)
    assert ok.all() and np.all(v[0] == -2 ** 23) and np.all(v[1] == 2 ** 23 - 1)
    w = U.astype(np.int64) - 128
    p0, p1, p2 = F.digits(v)
    P2 = p2 @ w[:4].T
    assert P2.max() == 2 ** 30 and P2.min() == -127 * 128 * C.MAX_K
    for p in (p0, p1):
        assert np.abs(p @ w[:4].T).max() <= 2 ** 30
    K = C.MAX_K
    D = v @ w[:4].T
    assert np.abs(K * D[:2, :2]).max() > 2 ** 61 and np.all(K * D[:2, :2] == np.outer(v.sum(axis=1), w.sum(axis=1))[:2, :2])


def test_padded_sizes(lib):
    for Q, want in ((-5, 0), (0, 0), (1, 64), (63, 64), (64, 64), (65, 128), (1000, 1024), (3 << 31, 3 << 31)):
        assert lib.hq_cosqf_padded_rows(Q) == want
    size, ref = lib.hq_cosqf_topk_workspace_size, lib.hq_cos_topk_workspace_size
    assert size(0, 10, 1) == 0 and size(10, 0, 1) == 0 and size(10, 10, 0) == 0
    for Q, N, k in ((1, 1, 1), (129, 769, 10), (1000, 250_000, 64)):
        assert size(Q, N, k) == ref(Q, N, k) > 0


def test_argument_validation(lib):
    from hq_mi355x import _lib
    one = ctypes.c_void_p(256)  # a non-null address that is never dereferenced: every call returns before a launch
    E, U, OK = _lib.HQ_E_INVALID, _lib.HQ_E_UNSUPPORTED, _lib.HQ_OK

    def prepare(Q=5, ld=64, K=64, X=one, Q8=one, st=one):
        return lib.hq_cosqf_prepare(X, Q, ld, K, Q8, st, None)

    def scores(Q=3, N=5, K=64, A=one, sa=one, B=one, sb=one, out=one):
        return lib.hq_cosqf_scores(A, sa, Q, B, sb, N, K, out, None)

    def topk(Q=3, N=5, K=64, k=10, A=one, sa=one, B=one, sb=one, ws=one, wb=1 << 30, os_=one, oi=one):
        return lib.hq_cosqf_topk(A, sa, Q, B, sb, N, K, k, 0.0, 0, 0, ws, wb, os_, oi, None)

    # empty problems are no-ops before any pointer check
    assert prepare(Q=0, X=None, Q8=None, st=None) == OK
    for f in (scores, topk):
        assert f(Q=0, A=None, sa=None, B=None, sb=None) == OK
        assert f(N=0, A=None, sa=None, B=None, sb=None) == OK
    assert topk(Q=0, k=100, ws=None, os_=None, oi=None) == OK
    # negative sizes, K < 1, ld < K
    for kw in (dict(Q=-1), dict(K=0), dict(K=-4), dict(ld=63), dict(ld=0)):
        assert prepare(**kw) == E, kw
        assert "bad shape" in _lib.last_error()
    for f in (scores, topk):
        for kw in (dict(Q=-1), dict(N=-1), dict(K=0)):
            assert f(**kw) == E, kw
            assert "bad shape" in _lib.last_error()
    for kw in (dict(k=0), dict(k=-3)):
        assert topk(**kw) == E, kw
    # the limits
    assert topk(k=65) == U and "k=65" in _lib.last_error()
    assert topk(k=64, ws=None) == E  # k = 64 itself passes the limit (null workspace next)
    for f in (prepare, scores, topk):
        assert f(K=C.MAX_K + 1, **({"ld": C.MAX_K + 1} if f is prepare else {})) == U
        assert "65536" in _lib.last_error()
    assert scores(K=C.MAX_K, A=None) == E and topk(K=C.MAX_K, A=None) == E  # 65536 itself passes the limit
    assert prepare(K=C.MAX_K, ld=C.MAX_K, X=None) == E
    # null buffers
    for name in ("X", "Q8", "st"):
        assert prepare(**{name: None}) == E, name
        assert _lib.last_error() == "null buffer"
    for name in ("A", "sa", "B", "sb", "out"):
        assert scores(**{name: None}) == E, name
        assert _lib.last_error() == "null buffer"
    for name in ("A", "sa", "B", "sb", "ws", "os_", "oi"):
        assert topk(**{name: None}) == E, name
        assert _lib.last_error() == "null buffer"
    need = lib.hq_cosqf_topk_workspace_size(3, 5, 10)
    assert topk(wb=need - 1) == E and _lib.last_error() == "workspace too small"


def test_exports_and_python_layer(lib):
    import inspect
    from hq_mi355x import _lib
    import hq_mi355x.kernels as K
    import hq_mi355x.rag as rag
    for name, nargs in (("hq_cosqf_padded_rows", 1), ("hq_cosqf_prepare", 7), ("hq_cosqf_scores", 9),
                        ("hq_cosqf_topk_workspace_size", 3), ("hq_cosqf_topk", 16)):
        assert hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs
    for name in ("CosQFRows", "cosqf_prepare", "cosqf_scores", "cosqf_topk"):
        assert hasattr(K, name), name
    assert hasattr(rag.QuantizedFrameCorpus, "search_float")
    assert "search_float" in rag.QuantizedFrameCorpus.__doc__
    p = inspect.signature(rag.QuantizedFrameCorpus.search_parameters).parameters
    assert p["quantize_query"].default is True


def test_python_entries_raise_without_a_device():
    import torch
    if torch.cuda.is_available():
        return  # with a device the same entries run (tests/test_gpu_cosqf.py)
    from hq_mi355x import kernels as K
    from hq_mi355x._lib import NativeLibraryError
    x = torch.from_numpy(F.random_queries(5, 64, 3).copy())
    with pytest.raises(NativeLibraryError):
        K.cosqf_prepare(x)
    with pytest.raises(TypeError):
        K.cosqf_prepare(x.to(torch.float64))
    with pytest.raises(ValueError):
        K.cosqf_prepare(x, rows=2)
    q = K.CosQFRows(torch.zeros((64, 192), dtype=torch.int8), torch.zeros((64, 4), dtype=torch.float64), 5, 64)
    c = K.CosQRows(torch.zeros((128, 64), dtype=torch.int8), torch.zeros((128, 4), dtype=torch.float64), 5, 64)
    with pytest.raises(NativeLibraryError):
        K.cosqf_scores(q, c)
    with pytest.raises(NativeLibraryError):
        K.cosqf_topk(q, c, 3)
    with pytest.raises(ValueError, match="query length"):
        K.cosqf_scores(K.CosQFRows(q.Q8, q.stats, 5, 32), c)
