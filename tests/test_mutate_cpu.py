"""CPU-side checks of the mutable corpus: hq_seg_gather and hq_seg_replace are exported and validate their
arguments before any device work, the engine's pool matcher (_pool_diff) recognises a pool that lost entries, and
the shrink switch is off by default.  No kernel is launched here."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    from hq_mi355x import _lib
    return _lib.load()


_BUFFERS = [(ctypes.c_double * 64)(), (ctypes.c_double * 64)()]   # never dereferenced: every call fails first


@pytest.fixture(scope="module")
def p():
    return ctypes.cast(_BUFFERS[0], ctypes.c_void_p)


@pytest.fixture(scope="module")
def p2():
    return ctypes.cast(_BUFFERS[1], ctypes.c_void_p)


def _lengths(lib):
    import mutate_cases as MC
    no_ov, big0 = MC.special_lengths(lib)
    assert no_ov is not None and big0 is not None
    return no_ov, big0


def test_symbols_exported(lib):
    from hq_mi355x._lib import SIGNATURES
    for name in ("hq_seg_gather", "hq_seg_replace"):
        assert hasattr(lib, name), name
        assert name in SIGNATURES, name


def _gather(lib, src_row, M, N_src, L, R_src, Z_src, S_src, R, Z, stats, Z16=None, S32=None, Zov16=None, Sov32=None,
            flags=None):
    return lib.hq_seg_gather(src_row, M, N_src, L, R_src, Z_src, S_src, R, Z, stats, Z16, S32, Zov16, Sov32, flags,
                             None)


def test_gather_argument_validation(lib, p, p2):
    from hq_mi355x import _lib
    INV, UNS = _lib.HQ_E_INVALID, _lib.HQ_E_UNSUPPORTED
    no_ov, big0 = _lengths(lib)
    # bad shapes
    for M, N, L in ((-1, 4, 64), (0, -1, 64), (0, 4, 0), (1, 0, 64)):
        assert _gather(lib, p, M, N, L, None, p, p, None, p2, p2) == INV, (M, N, L)
        assert _lib.last_error().startswith("bad shape"), (M, N, L)
    # int32 row ids
    assert _gather(lib, p, 2 ** 31 - 1, 2 ** 31, 64, None, p, p, None, p2, p2) == UNS
    assert "int32 row ids" in _lib.last_error()
    # a NULL mandatory buffer
    for args in ((None, 1, 4, 64, None, p, p, None, p2, p2), (p, 1, 4, 64, None, None, p, None, p2, p2),
                 (p, 1, 4, 64, None, p, None, None, p2, p2), (p, 1, 4, 64, None, p, p, None, None, p2),
                 (p, 1, 4, 64, None, p, p, None, p2, None)):
        assert _gather(lib, *args) == INV
        assert _lib.last_error() == "null buffer"
    # half of a pair: the raw rows, a split copy (M = 0 too: nothing has been launched by then)
    assert _gather(lib, p, 1, 4, 64, p, p, p, None, p2, p2) == INV
    assert _lib.last_error() == "the raw rows need both of their buffers"
    assert _gather(lib, p, 1, 4, 64, None, p, p, p2, p2, p2) == INV
    for M in (0, 1):
        assert _gather(lib, p, M, 4, 64, None, p, p, None, p2, p2, Z16=p2) == INV
        assert _lib.last_error() == "a split copy needs both of its buffers"
        assert _gather(lib, p, M, 4, 64, None, p, p, None, p2, p2, S32=p2) == INV
        assert _gather(lib, p, M, 4, 64, None, p, p, None, p2, p2, Zov16=p2) == INV
        assert _gather(lib, p, M, 4, 64, None, p, p, None, p2, p2, Sov32=p2) == INV
        assert _lib.last_error() == "a split copy needs both of its buffers"
        # the flagged-row list needs the level-0 statistics
        assert _gather(lib, p, M, 4, 64, None, p, p, None, p2, p2, flags=p2) == INV
        assert _lib.last_error() == "the flagged-row list needs the level-0 copies"
        # level-0 copies for a level-0 segment longer than 32 values; overall copies without a layout
        assert _gather(lib, p, M, 4, big0, None, p, p, None, p2, p2, Z16=p2, S32=p2) == INV
        assert _lib.last_error().startswith("level-0 copies with a level-0 segment of")
        assert _gather(lib, p, M, 4, no_ov, None, p, p, None, p2, p2, Zov16=p2, Sov32=p2) == INV
        assert _lib.last_error().startswith("overall copies without a split overall layout")
        # a destination that is its source
        assert _gather(lib, p, M, 4, 64, None, p, p2, None, p, p) == INV
        assert _lib.last_error() == "a destination buffer is its source"
        assert _gather(lib, p, M, 4, 64, None, p2, p, None, p, p) == INV
        assert _gather(lib, p, M, 4, 64, p, p2, p2, p, p, p) == INV
        assert _lib.last_error() == "a destination buffer is its source"
    # M = 0 without split copies: valid, and nothing to write
    assert _gather(lib, None, 0, 0, 64, None, None, None, None, None, None) == _lib.HQ_OK
    assert _gather(lib, None, 0, 5, 64, p, p, p, p2, p2, p2) == _lib.HQ_OK


def _replace(lib, idx, M, rows, L, N, Z, stats, Z16=None, S32=None, Zov16=None, Sov32=None, flags=None):
    return lib.hq_seg_replace(idx, M, rows, L, 0, None, N, Z, stats, Z16, S32, Zov16, Sov32, flags, None)


def test_replace_argument_validation(lib, p):
    from hq_mi355x import _lib
    INV, UNS = _lib.HQ_E_INVALID, _lib.HQ_E_UNSUPPORTED
    no_ov, big0 = _lengths(lib)
    assert _replace(lib, None, 0, None, 64, 0, None, None) == _lib.HQ_OK        # M == 0: nothing to write
    assert _replace(lib, None, 0, None, 64, 17, None, None) == _lib.HQ_OK
    for M, L, N in ((-1, 64, 4), (1, 0, 4), (1, 64, -1), (5, 64, 4)):          # more distinct rows than rows
        assert _replace(lib, p, M, p, L, N, p, p) == INV, (M, L, N)
        assert _lib.last_error().startswith("bad shape"), (M, L, N)
    assert _replace(lib, p, 1, p, 4097, 4, p, p) == UNS                         # as hq_seg_append
    assert _replace(lib, p, 1, p, 8192, 4, None, None) == UNS
    for args in ((None, 1, p, 64, 4, p, p), (p, 1, None, 64, 4, p, p), (p, 1, p, 64, 4, None, p),
                 (p, 1, p, 64, 4, p, None)):
        assert _replace(lib, *args) == INV
        assert _lib.last_error() == "null buffer"
    assert _replace(lib, p, 1, p, 64, 4, p, p, Z16=p) == INV
    assert _lib.last_error() == "a split copy needs both of its buffers"
    assert _replace(lib, p, 1, p, 64, 4, p, p, S32=p) == INV
    assert _replace(lib, p, 1, p, 64, 4, p, p, Zov16=p) == INV
    assert _replace(lib, p, 1, p, 64, 4, p, p, Sov32=p) == INV
    assert _replace(lib, p, 1, p, 64, 4, p, p, flags=p) == INV
    assert _lib.last_error() == "the flagged-row list needs the level-0 copies"
    assert _replace(lib, p, 1, p, big0, 4, p, p, Z16=p, S32=p) == INV
    assert _lib.last_error().startswith("level-0 copies with a level-0 segment of")
    assert _replace(lib, p, 1, p, no_ov, 4, p, p, Zov16=p, Sov32=p) == INV
    assert _lib.last_error().startswith("overall copies without a split overall layout")
    assert _replace(lib, p, 1, p, 64, 2 ** 31 - 1, p, p) == UNS
    assert "int32 row ids" in _lib.last_error()


def test_pool_diff():
    from hq_mi355x.core.search_engine import _pool_diff
    a, b, c, d, e, x, y = (np.arange(4) + i for i in range(7))
    assert _pool_diff([a, b, c], [a, b, c]) == ([0, 1, 2], 3)                   # identical
    assert _pool_diff([a, b, c], [a, b, c, x, y]) == ([0, 1, 2], 3)             # grown
    assert _pool_diff([a, b, c], [b, c]) == ([1, 2], 2)                         # first removed
    assert _pool_diff([a, b, c], [a, c]) == ([0, 2], 2)                         # a middle one
    assert _pool_diff([a, b, c], [a, b]) == ([0, 1], 2)                         # the last one
    assert _pool_diff([a, b, c], [a, c, x]) == ([0, 2], 2)                      # removed, and a grown tail
    assert _pool_diff([a, b, c, d, e], [b, d, x, y]) == ([1, 3], 2)             # several removed, plus a tail
    assert _pool_diff([a, b, c], [a, x, y]) == ([0], 1)
    assert _pool_diff([a, b, a], [a, b, a]) == ([0, 1, 2], 3)                   # the same array object twice
    assert _pool_diff([a, a, b], [a, b]) == ([0, 2], 2)
    assert _pool_diff([a, b, a], [a, b]) == ([0, 1], 2)
    assert _pool_diff([a, b], [a, b, a]) == ([0, 1], 2)                         # ... and in the new tail
    assert _pool_diff([a, b, c], [b, a, c]) is None                             # reordered
    assert _pool_diff([a, b, c], [a, c, b]) is None
    assert _pool_diff([a, b, c], [a, x, c]) is None                             # a foreign array in the middle
    assert _pool_diff([a, b, c], [x, a, b, c]) is None
    assert _pool_diff([a, b, c], [x, y]) is None                                # nothing surviving
    assert _pool_diff([a, b, c], []) is None
    assert _pool_diff([], [a, b]) is None                                       # empty cached
    assert _pool_diff([], []) is None
    # equal values are not identity
    assert _pool_diff([a, b], [a.copy(), b]) is None
    assert _pool_diff([a, b], [a, b.copy()]) == ([0], 1)
    big = [np.zeros(1) for _ in range(20000)]
    kept, tail = _pool_diff(big, big[:7] + big[8:] + [x])
    assert len(kept) == 19999 and 7 not in kept and tail == 19999


def test_shrink_is_off_by_default():
    from hq_mi355x.api import HilbertQuantizer
    from hq_mi355x.core.search_engine import ProgressiveSimilaritySearchEngine
    assert ProgressiveSimilaritySearchEngine.shrink_resident is False
    eng = ProgressiveSimilaritySearchEngine()
    assert eng.shrink_resident is False and eng.pool_shrinks == 0
    assert eng.pool_stats == {"builds": 0, "appends": 0}
    hq = HilbertQuantizer()
    assert hq.shrink_resident is False and hq.search_engine.shrink_resident is False
    on = HilbertQuantizer(shrink_resident=True)
    assert on.search_engine.shrink_resident is True
    assert ProgressiveSimilaritySearchEngine.shrink_resident is False           # per instance, not the class
    with pytest.raises(TypeError):
        HilbertQuantizer(None, True, True)                                      # keyword-only
