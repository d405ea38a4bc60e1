"""Host-side checks of the compressed-domain frame search (hq_cosq_*): the contract's integer formula against
the long-double definition on every row family, mutations of it that the families must catch, the padding
functions, argument validation through the loaded library, and the no-device behaviour of the Python layer.
No kernel is launched here."""
import ctypes

import numpy as np
import pytest

import cosq_cases as C

KS = (64, 199, 4096)


@pytest.fixture(scope="module")
def lib():
    from hq_mi355x import _lib
    return _lib.load()


def test_long_double_is_wider_than_double():
    assert np.finfo(np.longdouble).eps < 1e-18  # the exact reference needs the 80-bit format


@pytest.mark.parametrize("K", KS)
def test_model_agrees_with_exact_reference(K):
    """The integer formula is within 1e-13 of the long-double cosine, family against family."""
    U, MM, names = C.all_families(K)
    exact = C.exact_scores(U, MM, U, MM)
    model = C.model_scores(U, MM, U, MM)
    err = np.abs(model - exact)
    assert np.all(np.isfinite(model))
    assert err.max() <= C.TOL, (float(err.max()), names[int(np.argmax(err.max(axis=1)))])
    # the special rows: zero rows and non-finite (mn, mx) score exactly 0.0 and nothing else does
    dead = C.rows_of(names, {"const_zero", "nonfinite"})
    live = np.setdiff1d(np.arange(len(names)), dead)
    assert np.all(model[dead] == 0.0) and np.all(model[:, dead] == 0.0)
    assert np.all(exact[dead] == 0.0) and np.all(exact[:, dead] == 0.0)
    # constant frames against each other: 1 or 0 by sign
    pos, neg = C.rows_of(names, {"const_pos"}), C.rows_of(names, {"const_neg"})
    for a, b, want in ((pos, pos, 1.0), (neg, neg, 1.0), (pos, neg, 0.0), (neg, pos, 0.0)):
        assert np.all(np.abs(model[np.ix_(a, b)] - want) <= C.TOL)
    assert np.all(np.abs(np.diag(model)[live] - 1.0) <= C.TOL)


@pytest.mark.parametrize("mutation", C.MUTATIONS)
def test_mutations_are_caught(mutation):
    """Each wrong form of the formula differs from the exact reference by more than 1e-9 on some family."""
    worst = 0.0
    for K in KS:
        U, MM, _ = C.all_families(K)
        exact = C.exact_scores(U, MM, U, MM)
        with np.errstate(all="ignore"):
            bad = C.model_scores(U, MM, U, MM, mutate=mutation)
        worst = max(worst, float(np.nanmax(np.abs(bad - exact))))
    assert worst > 1e-9, (mutation, worst)


def test_operand_map_inputs_are_asymmetric():
    """Swapping rows and columns, or reversing k inside a 16-byte group or a 64-byte step of one operand, moves
    the operand-map case's scores by far more than the tolerance."""
    Uq, Mq = C.operand_map_rows(19, 199, 0)
    Uc, Mc = C.operand_map_rows(389, 199, 1)
    exact = C.exact_scores(Uq, Mq, Uc, Mc)
    assert np.abs(exact[:, :19] - exact[:, :19].T).max() > 1e-3
    for group in (16, 64):
        Kp = C.padded_k(199)
        pad = np.zeros((389, Kp), np.uint8)
        pad[:, :199] = Uc
        rev = pad.reshape(389, Kp // group, group)[:, :, ::-1].reshape(389, Kp)[:, :199]
        assert np.abs(C.exact_scores(Uq, Mq, rev, Mc) - exact).max() > 1e-3


def test_accumulator_rows_reach_the_int32_extremes():
    U, _ = C.accumulator_rows()
    w = U.astype(np.int64) - 128
    P = w[:4] @ w[:4].T
    assert P.max() == 2 ** 30 and P.min() == -128 * 127 * C.MAX_K and P.min() > -2 ** 31
    assert abs(w.sum(axis=1)).max() == 128 * C.MAX_K and (w * w).sum(axis=1).max() == 2 ** 30


def test_padded_sizes(lib):
    for K, want in ((-1, 0), (0, 0), (1, 64), (63, 64), (64, 64), (65, 128), (199, 256), (4096, 4096), (65536, 65536)):
        assert lib.hq_cosq_padded_k(K) == want == (C.padded_k(K) if K > 0 else 0)
    for N, want in ((-5, 0), (0, 0), (1, 128), (128, 128), (129, 256), (250_000, 250_112), (3 << 31, 3 << 31)):
        assert lib.hq_cosq_padded_rows(N) == want
    size, ref = lib.hq_cosq_topk_workspace_size, lib.hq_cos_topk_workspace_size
    assert size(0, 10, 1) == 0 and size(10, 0, 1) == 0 and size(10, 10, 0) == 0
    for Q, N, k in ((1, 1, 1), (129, 769, 10), (1000, 250_000, 64)):
        assert size(Q, N, k) == ref(Q, N, k) > 0


def test_argument_validation(lib):
    from hq_mi355x import _lib
    one = ctypes.c_void_p(256)  # a non-null address that is never dereferenced: every call returns before a launch
    E, U, OK = _lib.HQ_E_INVALID, _lib.HQ_E_UNSUPPORTED, _lib.HQ_OK

    def prepare(N=5, ld=64, K=64, X=one, mm=one, X8=one, st=one):
        return lib.hq_cosq_prepare(X, N, ld, K, mm, X8, st, None)

    def scores(Q=3, N=5, K=64, A=one, sa=one, B=one, sb=one, out=one):
        return lib.hq_cosq_scores(A, sa, Q, B, sb, N, K, out, None)

    def topk(Q=3, N=5, K=64, k=10, A=one, sa=one, B=one, sb=one, ws=one, wb=1 << 30, os_=one, oi=one):
        return lib.hq_cosq_topk(A, sa, Q, B, sb, N, K, k, 0.0, 0, 0, ws, wb, os_, oi, None)

    # empty problems are no-ops before any pointer check
    assert prepare(N=0, X=None, mm=None, X8=None, st=None) == OK
    for f in (scores, topk):
        assert f(Q=0, A=None, sa=None, B=None, sb=None) == OK
        assert f(N=0, A=None, sa=None, B=None, sb=None) == OK
    assert topk(Q=0, k=100, ws=None, os_=None, oi=None) == OK
    # negative sizes, K < 1, ld < K
    for kw in (dict(N=-1), dict(K=0), dict(K=-4), dict(ld=63), dict(ld=0)):
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
    for name in ("X", "mm", "X8", "st"):
        assert prepare(**{name: None}) == E, name
        assert _lib.last_error() == "null buffer"
    for name in ("A", "sa", "B", "sb", "out"):
        assert scores(**{name: None}) == E, name
        assert _lib.last_error() == "null buffer"
    for name in ("A", "sa", "B", "sb", "ws", "os_", "oi"):
        assert topk(**{name: None}) == E, name
        assert _lib.last_error() == "null buffer"
    need = lib.hq_cosq_topk_workspace_size(3, 5, 10)
    assert topk(wb=need - 1) == E and _lib.last_error() == "workspace too small"


def test_exports_and_python_layer(lib):
    from hq_mi355x import _lib
    import hq_mi355x.kernels as K
    import hq_mi355x.rag as rag
    for name, nargs in (("hq_cosq_padded_k", 1), ("hq_cosq_padded_rows", 1), ("hq_cosq_prepare", 8),
                        ("hq_cosq_scores", 9), ("hq_cosq_topk_workspace_size", 3), ("hq_cosq_topk", 16)):
        assert hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs
    assert "QuantizedFrameCorpus" in rag.__all__
    for name in ("CosQRows", "cosq_prepare", "cosq_scores", "cosq_topk"):
        assert hasattr(K, name), name
    assert "out of scope" in rag.QuantizedFrameCorpus.__doc__  # float32 queries against a u8 corpus


def test_python_entries_raise_without_a_device():
    import torch
    if torch.cuda.is_available():
        return  # with a device the same entries run (tests/test_gpu_cosq.py)
    from hq_mi355x import kernels as K, rag
    from hq_mi355x._lib import NativeLibraryError
    U, MM = C.random_rows(5, 64, 3)
    u, mm = torch.from_numpy(U.copy()), torch.from_numpy(MM.copy())
    with pytest.raises(NativeLibraryError):
        K.cosq_prepare(u, mm)
    rows = K.CosQRows(torch.zeros((128, 64), dtype=torch.int8), torch.zeros((128, 4), dtype=torch.float64), 5, 64)
    with pytest.raises(NativeLibraryError):
        K.cosq_scores(rows, rows)
    with pytest.raises(NativeLibraryError):
        K.cosq_topk(rows, rows, 3)
    with pytest.raises(NativeLibraryError):
        rag.QuantizedFrameCorpus(U.reshape(5, 8, 8), MM)
    with pytest.raises(NativeLibraryError):
        rag.QuantizedFrameCorpus.from_parameters(np.zeros((4, 60), np.float32), 8)
