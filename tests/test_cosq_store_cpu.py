"""Host-side checks of the mutable u8 frame store (hq_cosq_append / hq_cosq_replace / hq_cosq_gather): the NumPy
model of the operand layout (cosq_store_cases) gives the same bytes for a fresh build and for every append, replace
and gather of the case lists, wrong forms of the three operations are caught by those cases, the C-ABI is
declared, exported, registered and validates its arguments before any launch, and QuantizedFrameCorpus raises its
host-side errors before any library call.  No kernel is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest

import cosq_store_cases as S

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hq_mi355x.h")


@pytest.fixture(scope="module")
def lib():
    from hq_mi355x import _lib
    return _lib.load()


def _appended(K, N0, M, mutate=None):
    """(operand after the model's append, fresh operand of all rows, rows to compare, capacity rows)."""
    U0, M0 = S.frames(K, 0, N0)
    U1, M1 = S.frames(K, N0, M)
    cap = S.padded_rows(N0 + M) + 128
    X8, st = S.fresh(U0, M0, K, cap)
    S.append(X8, st, N0, U1, M1, K, mutate)
    return (X8, st), S.fresh(np.concatenate([U0, U1]), np.concatenate([M0, M1]), K, cap), S.padded_rows(N0 + M)


@pytest.mark.parametrize("store", S.STORES, ids=S.STORE_IDS)
def test_model_append_equals_fresh(store):
    _, K, _, _ = store
    for N0 in S.N0S:
        for M in S.MS:
            got, want, rows = _appended(K, N0, M)
            assert S.same(got, want, rows, K), (N0, M)
            assert S.untouched(got, rows, K), (N0, M)


def test_appended_frames_meet_the_special_families():
    """Short appends of the case lists include constant (mn == mx) and non-finite (min, max) frames."""
    seen_const = seen_bad = False
    for N0 in S.N0S:
        for M in S.MS:
            _, MM = S.frames(64, N0, M)
            seen_const |= bool(np.any(MM[:, 0] == MM[:, 1]))
            seen_bad |= bool(np.any(~np.isfinite(MM)))
    assert seen_const and seen_bad


@pytest.mark.parametrize("store", S.STORES, ids=S.STORE_IDS)
def test_model_replace_equals_fresh(store):
    _, K, _, _ = store
    for N, rows in S.REPLACES:
        U, MM = (a.copy() for a in S.frames(K, 0, N))
        Un, Mn = S.frames(K, 1000, len(rows))
        cap = S.padded_rows(N) + 128
        got = S.fresh(U, MM, K, cap)
        S.replace(got[0], got[1], N, rows, Un, Mn, K)
        U[list(rows)], MM[list(rows)] = Un, Mn
        assert S.same(got, S.fresh(U, MM, K, cap), S.padded_rows(N), K), (N, rows)
        assert S.untouched(got, S.padded_rows(N), K)
    # ids outside [0, N) are skipped
    U, MM = S.frames(K, 0, 17)
    got = S.fresh(U, MM, K, 256)
    S.replace(got[0], got[1], 17, (-1, 17, 10 ** 12), *S.frames(K, 1000, 3), K)
    assert S.same(got, S.fresh(U, MM, K, 256), 256, K)


@pytest.mark.parametrize("store", S.STORES, ids=S.STORE_IDS)
def test_model_gather_equals_fresh(store):
    _, K, _, _ = store
    N = S.GATHER_N
    U, MM = S.frames(K, 0, N)
    src = S.fresh(U, MM, K)
    keep = (src[0].copy(), src[1].copy())
    for name, sel in S.gather_patterns(N):
        cap = S.padded_rows(len(sel)) + 128
        got = S.gather(src, K, sel, cap)
        assert S.same(got, S.fresh(U[sel], MM[sel], K, cap), S.padded_rows(len(sel)), K), name
        assert S.untouched(got, S.padded_rows(len(sel)), K), name
    assert S.same(src, keep, S.padded_rows(N), K)
    none = S.gather(src, K, np.zeros(0, np.int64), 256)
    assert np.all(none[0][:128 * S.padded_k(K)] == 0) and np.all(none[1][:128] == 0.0) and S.untouched(none, 128, K)


def _caught(mutation):
    """Cases of the lists on which the mutated model differs from a fresh build in a compared byte."""
    hits = []
    for _, K, _, _ in S.STORES:
        if mutation != "gather_no_stats":
            for N0 in S.N0S:
                for M in S.MS:
                    got, want, rows = _appended(K, N0, M, mutation)
                    if not S.same(got, want, rows, K):
                        hits.append(("append", K, N0, M))
        if mutation in ("swap_gj", "gather_no_stats", "no_pad"):
            N = S.GATHER_N
            U, MM = S.frames(K, 0, N)
            src = S.fresh(U, MM, K)
            for name, sel in S.gather_patterns(N):
                cap = S.padded_rows(len(sel)) + 128
                if not S.same(S.gather(src, K, sel, cap, mutation), S.fresh(U[sel], MM[sel], K, cap),
                              S.padded_rows(len(sel)), K):
                    hits.append(("gather", K, name))
        if mutation in ("swap_gj", "resident_rows"):
            for N, rows in S.REPLACES:
                U, MM = (a.copy() for a in S.frames(K, 0, N))
                Un, Mn = S.frames(K, 1000, len(rows))
                got = S.fresh(U, MM, K)
                S.replace(got[0], got[1], N, rows, Un, Mn, K, mutation)
                U[list(rows)], MM[list(rows)] = Un, Mn
                if not S.same(got, S.fresh(U, MM, K), S.padded_rows(N), K):
                    hits.append(("replace", K, N))
    return hits


@pytest.mark.parametrize("mutation", S.MUTATIONS)
def test_mutations_are_caught(mutation):
    """Writing the resident rows of N0's tile, summing S and T over the whole tile, leaving the pad rows
    unwritten, swapping g and j in the piece address, forgetting the stats in gather: each changes a compared
    byte, for every K of the store list and in each operation it applies to."""
    hits = _caught(mutation)
    assert hits, mutation
    assert {h[1] for h in hits} == {s[1] for s in S.STORES}, mutation
    ops = {"resident_rows": {"append", "replace"}, "tile_sums": {"append"}, "no_pad": {"append", "gather"},
           "swap_gj": {"append", "replace", "gather"}, "gather_no_stats": {"gather"}}[mutation]
    assert {h[0] for h in hits} == ops, mutation
    if mutation == "resident_rows":  # only a shared tile can show it
        assert all(h[2] % 16 for h in hits if h[0] == "append")


def test_declared_exported_and_registered(lib):
    from hq_mi355x import _lib
    import hq_mi355x.kernels as K
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, nargs in (("hq_cosq_append", 10), ("hq_cosq_replace", 10), ("hq_cosq_gather", 10)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, text)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs
    for name in ("cosq_reserve", "cosq_append", "cosq_replace", "cosq_gather"):
        assert hasattr(K, name), name
    rows = K.CosQRows(np.zeros((256, 64), np.int8), np.zeros((256, 4)), 5, 64)  # the positional constructor
    assert (rows.N, rows.K, rows.cap) == (5, 64, 256)
    assert K.CosQRows(np.zeros((1, 64), np.int8), np.zeros((1, 4)), 0, 64).cap == 0
    assert K.CosQRows(rows.X8, rows.stats, 5, 64, 128).cap == 128


def test_argument_validation(lib):
    from hq_mi355x import _lib
    one = ctypes.c_void_p(256)  # a non-null address that is never dereferenced: every call returns before a launch
    E, U, OK = _lib.HQ_E_INVALID, _lib.HQ_E_UNSUPPORTED, _lib.HQ_OK

    def append(M=3, ld=64, K=64, N0=5, cap=128, X=one, mm=one, X8=one, st=one):
        return lib.hq_cosq_append(X, M, ld, K, mm, N0, cap, X8, st, None)

    def replace(M=3, ld=64, K=64, N=5, X=one, mm=one, rows=one, X8=one, st=one):
        return lib.hq_cosq_replace(X, M, ld, K, mm, rows, N, X8, st, None)

    def gather(M=3, Ns=5, K=64, cap=128, sel=one, Xs=one, ss=one, X8=one, st=one):
        return lib.hq_cosq_gather(sel, M, Ns, K, Xs, ss, cap, X8, st, None)

    # M = 0 is a no-op before any pointer check
    assert append(M=0, X=None, mm=None, X8=None, st=None) == OK
    assert replace(M=0, X=None, mm=None, rows=None, X8=None, st=None) == OK
    assert gather(M=0, Ns=0, cap=0, sel=None, Xs=None, ss=None, X8=None, st=None) == OK
    # negative sizes, K < 1, ld < K
    for f, bad in ((append, (dict(M=-1), dict(N0=-1), dict(K=0), dict(K=-4), dict(ld=63), dict(ld=0), dict(cap=-128))),
                   (replace, (dict(M=-1), dict(N=-1), dict(K=0), dict(ld=63))),
                   (gather, (dict(M=-1), dict(Ns=-1), dict(K=0), dict(cap=-128), dict(Ns=0)))):
        for kw in bad:
            assert f(**kw) == E, (f.__name__, kw)
            assert "bad shape" in _lib.last_error()
    # the capacity: a multiple of 128, at least the padded rows of the result
    for kw in (dict(cap=100), dict(cap=129), dict(cap=0), dict(N0=126, cap=128), dict(N0=128, M=1, cap=128),
               dict(M=2 ** 62, N0=2 ** 62, cap=1 << 40)):
        assert append(**kw) == E, kw
        assert "bad shape" in _lib.last_error()
    assert append(N0=125, cap=128, X=None) == E and _lib.last_error() == "null buffer"  # 128 rows fit exactly
    for kw in (dict(cap=100), dict(cap=0), dict(M=129, Ns=200, cap=128)):
        assert gather(**kw) == E, kw
        assert "bad shape" in _lib.last_error()
    assert gather(M=128, Ns=200, cap=128, sel=None) == E and _lib.last_error() == "null buffer"
    # the limit
    for f in (append, replace, gather):
        assert f(K=65537, **({} if f is gather else {"ld": 65537})) == U
        assert "65536" in _lib.last_error()
    assert append(K=65536, ld=65536, X=None) == E and replace(K=65536, ld=65536, X=None) == E
    assert gather(K=65536, sel=None) == E  # 65536 itself passes the limit (null buffer next)
    # null buffers
    for f, names in ((append, ("X", "mm", "X8", "st")), (replace, ("X", "mm", "rows", "X8", "st")),
                     (gather, ("sel", "Xs", "ss", "X8", "st"))):
        for name in names:
            assert f(**{name: None}) == E, (f.__name__, name)
            assert _lib.last_error() == "null buffer"
    assert gather(M=0, X8=None) == E and _lib.last_error() == "null buffer"  # M = 0 with room: the pad rows are written


# ---- QuantizedFrameCorpus: host-side errors before any library call ---------------------------------------------


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the host-side checks")


@pytest.fixture
def shell(monkeypatch):
    """A corpus of 5 frames of 9 x 8 around host buffers (never read), with keys, and with every path into the
    native library or onto a device closed."""
    import torch
    from hq_mi355x import _dev, kernels as K, rag
    from hq_mi355x.rag import similarity

    def closed(*a, **k):
        raise AssertionError("device or library use before the host-side checks")

    monkeypatch.setattr(K, "_L", lambda: _NoLibrary())
    for mod in (similarity, K):
        monkeypatch.setattr(mod, "to_dev", closed, raising=False)
        monkeypatch.setattr(mod, "stream", closed, raising=False)
    rows = K.CosQRows(torch.zeros((128, 64), dtype=torch.int8), torch.zeros((128, 4), dtype=torch.float64), 5, 64)

    def make(keys=True):
        return rag.QuantizedFrameCorpus._of_rows(rows, (9, 8), 8, torch.arange(100, 105) if keys else None)

    return make


def test_corpus_errors_come_before_any_launch(shell):
    c, plain = shell(), shell(keys=False)
    f = np.zeros((2, 9, 8), np.uint8)
    mm = np.zeros((2, 2), np.float32)
    k2 = np.array([7, 8])
    assert (c.N, len(c), c.K, c.capacity) == (5, 5, 64, 128)
    # frame shape, count and dtype
    for call in (lambda x, m: c.append(x, m, keys=k2), lambda x, m: c.insert(0, x, m, keys=k2),
                 lambda x, m: c.replace([0, 1], x, m)):
        with pytest.raises(ValueError):
            call(np.zeros((2, 8, 8), np.uint8), mm)
        with pytest.raises(ValueError):
            call(np.zeros((2, 9, 9), np.uint8), mm)
        with pytest.raises(ValueError):
            call(np.zeros((2, 9 * 8), np.uint8), mm)
        with pytest.raises(ValueError):
            call(f, np.zeros((3, 2), np.float32))
        with pytest.raises(TypeError):
            call(f.astype(np.float32), mm)
        with pytest.raises(TypeError):
            call(f.astype(np.int8), mm)
        with pytest.raises(TypeError):
            call(f, np.zeros((2, 2), np.int32))
    # keys: required with keys, refused without, one per frame, integers
    for call in (c.append, lambda *a, **k: c.insert(1, *a, **k)):
        with pytest.raises(ValueError, match="keys"):
            call(f, mm)
        with pytest.raises(ValueError, match="keys"):
            call(f, mm, keys=[1, 2, 3])
        with pytest.raises(TypeError):
            call(f, mm, keys=[1.5, 2.5])
    with pytest.raises(ValueError, match="keys"):
        plain.append(f, mm, keys=k2)
    with pytest.raises(ValueError, match="keys"):
        plain.insert(0, f, mm, keys=k2)
    with pytest.raises(ValueError, match="keys"):
        c.append_parameters(np.zeros((2, 60), np.float32))
    with pytest.raises(ValueError, match="keys"):
        plain.append_parameters(np.zeros((2, 60), np.float32), keys=k2)
    # rows
    for call in (c.remove, c.select, lambda r: c.replace(r, f[:1], mm[:1])):
        with pytest.raises(IndexError):
            call([5])
        with pytest.raises(IndexError):
            call([-1])
        with pytest.raises(TypeError):
            call([0.5])
    with pytest.raises(ValueError, match="repeated"):
        c.replace([1, 1], f, mm)
    with pytest.raises(ValueError):
        c.replace([1, 2, 3], f, mm)
    with pytest.raises(ValueError, match="no frame"):
        c.remove([0, 1, 2, 3, 4])
    with pytest.raises(ValueError, match="no frame"):
        c.remove([4, 3, 2, 1, 0, 0])
    for pos in (-1, 6):
        with pytest.raises(IndexError):
            c.insert(pos, f, mm, keys=k2)
    assert c.remove([]) == 5  # nothing to do: no launch
    assert "out of scope" in type(c).__doc__


def test_writers_raise_without_a_device():
    import torch
    if torch.cuda.is_available():
        return  # with a device the same entries run (tests/test_gpu_cosq_store.py)
    from hq_mi355x import kernels as K
    from hq_mi355x._lib import NativeLibraryError
    rows = K.CosQRows(torch.zeros((128, 64), dtype=torch.int8), torch.zeros((128, 4), dtype=torch.float64), 5, 64)
    u, mm = torch.zeros((2, 64), dtype=torch.uint8), torch.zeros((2, 2))
    with pytest.raises(NativeLibraryError):
        K.cosq_append(rows, u, mm)
    with pytest.raises(NativeLibraryError):
        K.cosq_replace(rows, [0, 1], u, mm)
    with pytest.raises(NativeLibraryError):
        K.cosq_gather(rows, [0, 1])
    with pytest.raises(TypeError):
        K.cosq_append(rows, u.float(), mm)
    with pytest.raises(ValueError, match="frame length"):
        K.cosq_append(rows, torch.zeros((2, 32), dtype=torch.uint8), mm)
    with pytest.raises(IndexError):
        K.cosq_gather(rows, [5])
    with pytest.raises(ValueError, match="repeated"):
        K.cosq_replace(rows, [1, 1], u, mm)
