"""The mutable u8 frame store on the GPU (hq_cosq_append / hq_cosq_replace / hq_cosq_gather, kernels.cosq_*,
rag.QuantizedFrameCorpus.append / replace / remove / insert / select).  The contract: after any sequence of them
the first padded_rows(N) rows of X8 and stats equal, bit for bit, what cosq_prepare writes for the resulting
frames, and nothing past them is written; search results then cannot depend on how a corpus was built.  The case
lists and the layout model are cosq_store_cases'; buffers under test are pre-filled with 0x5A."""
import numpy as np
import pytest

import cosq_cases as C
import cosq_store_cases as S

pytestmark = pytest.mark.gpu


def _np(x):
    return x.detach().cpu().numpy()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dev_rows(U, K, ld, off):
    """The first K bytes of U's rows on the device as a view with row stride ld starting `off` bytes into its buffer."""
    import torch
    R = U.shape[0]
    buf = torch.from_numpy(C.strided(np.ascontiguousarray(U[:, :K]), ld, off)).cuda()
    return buf.as_strided((R, K), (ld, 1), off)


def _filled(cap, K):
    """A CosQRows of cap rows and no frames whose buffers hold 0x5A."""
    import torch
    from hq_mi355x import kernels as Kn
    X8 = torch.full((cap, S.padded_k(K)), S.FILL, dtype=torch.int8, device="cuda")
    stats = torch.full((cap * 32,), S.FILL, dtype=torch.uint8, device="cuda").view(torch.float64).view(cap, 4)
    return Kn.CosQRows(X8, stats, 0, K, cap)


def _bits(x):
    import torch
    return x.view(torch.int64) if x.dtype == torch.float64 else x


def _same(got, want, rows, msg):
    """The first `rows` rows of two CosQRows agree bit for bit (torch.equal on the bytes and on the stats' bits)."""
    import torch
    assert torch.equal(got.X8[:rows], want.X8[:rows]), f"{msg}: X8"
    assert torch.equal(_bits(got.stats[:rows]), _bits(want.stats[:rows])), f"{msg}: stats"


def _untouched(got, rows, msg):
    import torch
    assert bool((got.X8[rows:] == S.FILL).all()), f"{msg}: X8 past row {rows}"
    assert bool((got.stats[rows:].contiguous().view(torch.uint8) == S.FILL).all()), f"{msg}: stats past row {rows}"


def _resident(U, MM, K, ld, off, cap):
    """cosq_prepare of the frames, moved into 0x5A buffers of cap rows."""
    from hq_mi355x import kernels as Kn
    c = _filled(cap, K)
    N = U.shape[0]
    if N:
        p = Kn.cosq_prepare(_dev_rows(U, K, ld, off), _dev(MM))
        Np = S.padded_rows(N)
        c.X8[:Np].copy_(p.X8[:Np])
        c.stats[:Np].copy_(p.stats[:Np])
    return Kn.CosQRows(c.X8, c.stats, N, K, cap)


@pytest.mark.parametrize("store", S.STORES, ids=S.STORE_IDS)
def test_append_is_byte_identical(hq_lib, store):
    """Every N0 x M of the lists: rows [N0, N0 + M) and the pad rows behind them as a fresh build writes them,
    the rows below N0 and everything past padded_rows(N0 + M) as they were."""
    from hq_mi355x import kernels as Kn
    _, K, ld, off = store
    for N0 in S.N0S:
        U0, M0 = S.frames(K, 0, N0)
        for M in S.MS:
            U1, M1 = S.frames(K, N0, M)
            rows = S.padded_rows(N0 + M)
            c = _resident(U0, M0, K, ld, off, rows + 128)
            before = c.X8
            g = Kn.cosq_append(c, _dev_rows(U1, K, ld, off), _dev(M1))
            assert (g.N, g.K, g.cap) == (N0 + M, K, rows + 128) and g.X8 is before  # no reallocation
            want = Kn.cosq_prepare(_dev_rows(np.concatenate([U0, U1]), K, ld, off), _dev(np.concatenate([M0, M1])))
            _same(g, want, rows, f"N0={N0} M={M}")
            _untouched(g, rows, f"N0={N0} M={M}")


def test_append_matches_the_layout_model(hq_lib):
    """The bytes against the NumPy model of the fragment layout (the stats are compared with cosq_prepare's)."""
    from hq_mi355x import kernels as Kn
    for K, N0, M in ((65, 17, 130), (1088, 129, 17)):
        U0, M0 = S.frames(K, 0, N0)
        U1, M1 = S.frames(K, N0, M)
        c = _resident(U0, M0, K, K, 0, S.padded_rows(N0 + M) + 128)
        g = Kn.cosq_append(c, _dev(U1), _dev(M1))
        want, _ = S.fresh(np.concatenate([U0, U1]), np.concatenate([M0, M1]), K, g.cap)
        assert np.array_equal(_np(g.X8).view(np.uint8).reshape(-1), want)


@pytest.mark.parametrize("store", S.STORES, ids=S.STORE_IDS)
def test_replace_is_byte_identical(hq_lib, store):
    import torch
    from hq_mi355x import kernels as Kn
    _, K, ld, off = store
    for N, rows in S.REPLACES:
        U, MM = (a.copy() for a in S.frames(K, 0, N))
        Un, Mn = S.frames(K, 1000, len(rows))
        Np = S.padded_rows(N)
        c = _resident(U, MM, K, ld, off, Np + 128)
        g = Kn.cosq_replace(c, list(rows), _dev_rows(Un, K, ld, off), _dev(Mn))
        assert g.N == N and g.X8 is c.X8
        U[list(rows)], MM[list(rows)] = Un, Mn
        _same(g, Kn.cosq_prepare(_dev_rows(U, K, ld, off), _dev(MM)), Np, f"N={N} rows={rows}")
        _untouched(g, Np, f"N={N} rows={rows}")
    # the C-ABI skips a row id outside [0, N): nothing is written for it
    U, MM = S.frames(K, 0, 17)
    c = _resident(U, MM, K, ld, off, 256)
    keep = (c.X8.clone(), c.stats.clone())
    Un, Mn = S.frames(K, 1000, 3)
    Kn.cosq_replace(c, torch.tensor([-1, 17, 10 ** 12]), _dev_rows(Un, K, ld, off), _dev(Mn), checked=True)
    assert torch.equal(c.X8, keep[0]) and torch.equal(_bits(c.stats), _bits(keep[1]))
    with pytest.raises(IndexError):
        Kn.cosq_replace(c, [17], _dev_rows(Un[:1], K, ld, off), _dev(Mn[:1]))
    with pytest.raises(ValueError, match="repeated"):
        Kn.cosq_replace(c, [3, 3], _dev_rows(Un[:2], K, ld, off), _dev(Mn[:2]))


@pytest.mark.parametrize("store", S.STORES, ids=S.STORE_IDS)
def test_gather_patterns_are_byte_identical(hq_lib, store, monkeypatch):
    """Identity, reverse, repeats, drop first / last / every 16th row / a whole tile, results of 127, 128 and 129
    rows: a fresh build of the selected frames; the source is unchanged; nothing past the result's padded rows."""
    import torch
    from hq_mi355x import kernels as Kn
    _, K, ld, off = store
    N = S.GATHER_N
    U, MM = S.frames(K, 0, N)
    src = Kn.cosq_prepare(_dev_rows(U, K, ld, off), _dev(MM))
    keep = (src.X8.clone(), src.stats.clone())
    # the destination buffers hold 0x5A before the launch
    monkeypatch.setattr(Kn, "_cosq_buffers", lambda cap, c: (lambda f: (f.X8, f.stats))(_filled(cap, c.K)))
    for name, sel in S.gather_patterns(N):
        rows = S.padded_rows(len(sel))
        g = Kn.cosq_gather(src, sel, cap=rows + 128)
        assert (g.N, g.K, g.cap) == (len(sel), K, rows + 128)
        _same(g, Kn.cosq_prepare(_dev_rows(U[sel], K, ld, off), _dev(MM[sel])), rows, name)
        _untouched(g, rows, name)
    assert torch.equal(src.X8, keep[0]) and torch.equal(_bits(src.stats), _bits(keep[1]))
    with pytest.raises(IndexError):
        Kn.cosq_gather(src, [0, N])
    # an id outside [0, N) is clamped for the load (checked=True: the host test is skipped): the other rows are right
    g = Kn.cosq_gather(src, torch.tensor([3, -7, N + 10 ** 9, 4]), cap=128, checked=True)
    want = Kn.cosq_prepare(_dev_rows(U[[3, 3, 3, 4]], K, ld, off), _dev(MM[[3, 3, 3, 4]]))
    pick = torch.tensor([0, 3] + list(range(4, 128)), device="cuda")
    assert torch.equal(_bits(g.stats[pick]), _bits(want.stats[pick]))


def _frames3(N, n, seed):
    """Pipeline-shaped frames: u8 [N, n + 1, n] with (min, max) pairs of mixed ranges."""
    U, MM = C.random_rows(N, (n + 1) * n, seed)
    return U.reshape(N, n + 1, n).copy(), MM.copy()


def _fresh_corpus(F, MM, keys=None):
    from hq_mi355x import rag
    return rag.QuantizedFrameCorpus(F, MM, keys=keys)


def _same_corpus(c, F, MM, msg):
    """c's resident operand is a fresh corpus's, bit for bit."""
    want = _fresh_corpus(F, MM)
    assert (c.N, len(c), c.K) == (F.shape[0], F.shape[0], want.K), msg
    assert c.capacity % 128 == 0 and c.capacity >= S.padded_rows(c.N), msg
    _same(c._rows, want._rows, S.padded_rows(c.N), msg)
    return want


def test_sequence_across_a_reallocation(hq_lib):
    """append, remove, replace, insert, append on a corpus of 17 x 16 frames (searched on their 16 leading rows):
    after every step the operand is a fresh build's; both appends outgrow the buffers."""
    n = 16
    F, MM = _frames3(700, n, 5)
    c = _fresh_corpus(F[:100], MM[:100])
    assert c.capacity == 128 and c.resident_bytes == 128 * (n * n + 32)  # built to size
    cur_F, cur_M = F[:100], MM[:100]
    assert c.append(F[100:230], MM[100:230]) == 230  # 128 -> 256: reallocation
    cur_F, cur_M = F[:230], MM[:230]
    assert c.capacity == 256
    _same_corpus(c, cur_F, cur_M, "append")
    drop = [0, 17, 18, 19, 128, 229, 17]
    assert c.remove(drop) == 224
    keep = np.setdiff1d(np.arange(230), drop)
    cur_F, cur_M = cur_F[keep], cur_M[keep]
    assert c.capacity == 256
    _same_corpus(c, cur_F, cur_M, "remove")
    rows = [223, 0, 16, 31, 100]
    assert c.replace(rows, F[300:305], MM[300:305]) == 224
    cur_F, cur_M = cur_F.copy(), cur_M.copy()
    cur_F[rows], cur_M[rows] = F[300:305], MM[300:305]
    _same_corpus(c, cur_F, cur_M, "replace")
    assert c.insert(17, F[400:403], MM[400:403]) == 227
    cur_F = np.concatenate([cur_F[:17], F[400:403], cur_F[17:]])
    cur_M = np.concatenate([cur_M[:17], MM[400:403], cur_M[17:]])
    _same_corpus(c, cur_F, cur_M, "insert")
    assert c.insert(0, F[403], MM[403]) == 228 and c.insert(228, F[404], MM[404:405]) == 229  # both ends, one frame
    cur_F = np.concatenate([F[403:404], cur_F, F[404:405]])
    cur_M = np.concatenate([MM[403:404], cur_M, MM[404:405]])
    _same_corpus(c, cur_F, cur_M, "insert at the ends")
    assert c.append(F[405:700], MM[405:700]) == 524  # 256 -> 640 (the need beats the factor 2)
    cur_F, cur_M = np.concatenate([cur_F, F[405:700]]), np.concatenate([cur_M, MM[405:700]])
    assert c.capacity == 640
    _same_corpus(c, cur_F, cur_M, "second append")
    assert c.reserve(100) == 640 and c.reserve(1000) == 1024
    _same_corpus(c, cur_F, cur_M, "reserve")
    sub = c.select([523, 0, 0, 77])
    _same_corpus(sub, cur_F[[523, 0, 0, 77]], cur_M[[523, 0, 0, 77]], "select")
    assert sub.capacity == 128 and c.N == 524


def test_forty_single_appends_from_empty(hq_lib):
    from hq_mi355x import kernels as Kn
    K = 65
    U, MM = S.frames(K, 0, 40)
    c = Kn.cosq_prepare(_dev(U[:0]), _dev(MM[:0]))
    assert (c.N, c.cap) == (0, 0)
    for i in range(40):
        c = Kn.cosq_append(c, _dev(U[i:i + 1]), _dev(MM[i:i + 1]))
    assert (c.N, c.cap) == (40, 128)
    _same(c, Kn.cosq_prepare(_dev(U), _dev(MM)), 128, "40 x 1")


def _equal_lists(got, want, msg):
    np.testing.assert_array_equal(_np(got[1]), _np(want[1]), err_msg=msg)
    assert _np(got[0]).tobytes() == _np(want[0]).tobytes(), msg


def test_search_on_a_mutated_corpus(hq_lib):
    """search, search_float and search_parameters (both quantize_query settings) on a corpus that was appended
    to, removed from, replaced in and inserted into list the ids, order and score bits of a fresh corpus of the
    same frames: k = 10 (fused) and k = 70 (the dense route).  The scores are within 1e-13 of the long-double
    reference (cosq_cases.exact_scores, cosq_cases.TOL: the bound the route documents and tests)."""
    import torch
    from hq_mi355x import kernels as Kn, rag
    n, d, N = 16, 200, 300
    rng = np.random.default_rng(7)
    X = rng.standard_normal((N + 60, d)).astype(np.float32)
    frames, _, mm = Kn.map_index_quantize(_dev(X), n)
    F, MM = _np(frames), _np(mm)
    c = rag.QuantizedFrameCorpus(F[:150], MM[:150])
    c.append(F[150:300], MM[150:300])
    c.remove(list(range(5, 300, 16)) + list(range(32, 48)))
    keep = np.setdiff1d(np.arange(300), list(range(5, 300, 16)) + list(range(32, 48)))
    cur_F, cur_M = F[keep].copy(), MM[keep].copy()
    c.replace([1, 200], F[300:302], MM[300:302])
    cur_F[[1, 200]], cur_M[[1, 200]] = F[300:302], MM[300:302]
    c.insert(130, F[302:310], MM[302:310])
    cur_F = np.concatenate([cur_F[:130], F[302:310], cur_F[130:]])
    cur_M = np.concatenate([cur_M[:130], MM[302:310], cur_M[130:]])
    c.append_parameters(X[310:330])
    cur_F, cur_M = np.concatenate([cur_F, F[310:330]]), np.concatenate([cur_M, MM[310:330]])
    want = _same_corpus(c, cur_F, cur_M, "mutated")
    Q = 33
    qf, qm = F[330:330 + Q - 3], MM[330:330 + Q - 3]
    qf, qm = np.concatenate([qf, cur_F[[0, 130, c.N - 1]]]), np.concatenate([qm, cur_M[[0, 130, c.N - 1]]])
    qx = np.concatenate([X[330:330 + Q - 3], X[310:313]])
    qfloat = rng.standard_normal((Q, n, n)).astype(np.float32)
    for k in (10, 70):
        _equal_lists(c.search(qf, qm, k), want.search(qf, qm, k), f"search k={k}")
        _equal_lists(c.search(qf, qm, k, threshold=0.5), want.search(qf, qm, k, threshold=0.5), f"threshold k={k}")
        _equal_lists(c.search_float(qfloat, k), want.search_float(qfloat, k), f"search_float k={k}")
        for quant in (True, False):
            _equal_lists(c.search_parameters(qx, k, quantize_query=quant),
                         want.search_parameters(qx, k, quantize_query=quant), f"search_parameters {quant} k={k}")
    s, ids = (_np(v) for v in c.search(qf, qm, 10))
    assert list(ids[-3:, 0]) == [0, 130, c.N - 1]  # the corpus's own frames find themselves
    exact = C.exact_scores(qf[:, :n].reshape(Q, -1), qm, cur_F[:, :n].reshape(c.N, -1), cur_M)
    ws, wi = C.reference_topk(exact, 10, 0.0, 0)
    err = float(np.max(np.abs(s - np.take_along_axis(exact, ids, axis=1))))
    print(f"cosq-store-err mutated corpus Q{Q} N{c.N} K{n * n} {err:.3e}")
    assert err <= C.TOL
    assert np.max(np.abs(s - ws)) <= C.TOL  # the k best scores are the reference's
    dense = _np(Kn.cosq_scores(Kn.cosq_prepare(_dev(qf), _dev(qm), n), c._rows))
    assert dense.shape == (Q, c.N) and float(np.max(np.abs(dense - exact))) <= C.TOL


def test_nonfinite_frame_scores_zero_and_moves_nothing(hq_lib):
    from hq_mi355x import kernels as Kn
    K = 4096
    U, MM = C.random_rows(200, K, 61)
    Uq, Mq = C.random_rows(20, K, 62)
    bad_U, bad_M = S.nonfinite_frame(K)
    q = Kn.cosq_prepare(_dev(Uq), _dev(Mq))
    c = Kn.cosq_prepare(_dev(U), _dev(MM))
    before = _np(Kn.cosq_scores(q, c))
    g = Kn.cosq_append(c, _dev(bad_U), _dev(bad_M))
    after = _np(Kn.cosq_scores(q, g))
    assert after.shape == (20, 201) and np.all(after[:, 200] == 0.0)
    assert after[:, :200].tobytes() == np.ascontiguousarray(before).tobytes()
    s, ids = Kn.cosq_topk(q, g, 201)
    assert np.all(_np(ids)[:, -1] == 200) and np.all(_np(s)[:, -1] == 0.0)


def test_keys_follow_every_mutation(hq_lib):
    n = 8
    F, MM = _frames3(60, n, 9)
    keys = np.arange(1000, 1040)
    c = _fresh_corpus(F[:40], MM[:40], keys=keys)
    plain = _fresh_corpus(F[:40], MM[:40])
    assert c.resident_bytes == plain.resident_bytes  # the keys are not counted
    c.remove([0, 7, 39])
    c.insert(2, F[40:42], MM[40:42], keys=[77, 78])
    c.append(F[42], MM[42], keys=[79])
    c.replace([5], F[43:44], MM[43:44])
    want_keys = np.concatenate([[1001, 1002, 77, 78], np.arange(1003, 1007), np.arange(1008, 1039), [79]])
    assert c.N == 40 and np.array_equal(_np(c._keys), want_keys)
    qf, qm = F[[41, 42, 1]], MM[[41, 42, 1]]
    s, ids = c.search(qf, qm, 3)
    sk, k = c.search(qf, qm, 3, return_keys=True)
    assert list(_np(ids)[:, 0]) == [3, 39, 0] and list(_np(k)[:, 0]) == [78, 79, 1001]
    assert np.array_equal(_np(k), want_keys[_np(ids)]) and _np(sk).tobytes() == _np(s).tobytes()
    # fewer than k frames pass: the empty slots stay -1
    sk, k = c.search(qf, qm, 5, threshold=0.999999, return_keys=True)
    assert np.all(_np(k)[:, 0] >= 0) and np.all(_np(k)[:, 1:] == -1)
    # search_float and both search_parameters settings map ids the same way
    qx = np.random.default_rng(3).standard_normal((4, 50)).astype(np.float32)
    for call in (lambda **kw: c.search_float(F[:3, :n].astype(np.float32), 4, **kw),
                 lambda **kw: c.search_parameters(qx, 4, **kw),
                 lambda **kw: c.search_parameters(qx, 4, quantize_query=False, **kw)):
        assert np.array_equal(_np(call(return_keys=True)[1]), want_keys[_np(call()[1])])
    sub = c.select([39, 0, 0])
    assert list(_np(sub._keys)) == [79, 1001, 1001]
    assert list(_np(sub.search(qf[1:], qm[1:], 2, return_keys=True)[1])[:, 0]) == [79, 1001]
    # without keys ids are positions, and return_keys has nothing to map through
    assert list(_np(plain.search(F[[3]], MM[[3]], 1)[1])[0]) == [3]
    with pytest.raises(ValueError, match="keys"):
        plain.search(F[[3]], MM[[3]], 1, return_keys=True)
    with pytest.raises(ValueError, match="keys"):
        c.append(F[44], MM[44])
    with pytest.raises(ValueError, match="keys"):
        plain.append(F[44], MM[44], keys=[5])


def test_return_codes(hq_lib):
    """Invalid and unsupported arguments with NULL buffers (the checks come before any launch); M = 0 leaves a 0x5A
    buffer intact; hq_cosq_gather with M = 0 writes the pad rows of an empty corpus."""
    import torch
    from hq_mi355x import _lib
    from hq_mi355x._dev import ptr, stream
    L = hq_lib
    E, U, OK = _lib.HQ_E_INVALID, _lib.HQ_E_UNSUPPORTED, _lib.HQ_OK
    assert L.hq_cosq_append(None, -1, 64, 64, None, 0, 128, None, None, None) == E
    assert L.hq_cosq_append(None, 1, 63, 64, None, 0, 128, None, None, None) == E
    assert L.hq_cosq_append(None, 1, 64, 0, None, 0, 128, None, None, None) == E
    assert L.hq_cosq_append(None, 1, 64, 64, None, 128, 128, None, None, None) == E  # 129 rows need 256
    assert L.hq_cosq_append(None, 1, 64, 64, None, 0, 64, None, None, None) == E    # not a multiple of 128
    assert L.hq_cosq_append(None, 1, 65537, 65537, None, 0, 128, None, None, None) == U
    assert L.hq_cosq_append(None, 1, 64, 64, None, 0, 128, None, None, None) == E and _lib.last_error() == "null buffer"
    assert L.hq_cosq_replace(None, 1, 64, 64, None, None, -1, None, None, None) == E
    assert L.hq_cosq_replace(None, 1, 65537, 65537, None, None, 5, None, None, None) == U
    assert L.hq_cosq_replace(None, 1, 64, 64, None, None, 5, None, None, None) == E and _lib.last_error() == "null buffer"
    assert L.hq_cosq_gather(None, 129, 200, 64, None, None, 128, None, None, None) == E
    assert L.hq_cosq_gather(None, 1, 0, 64, None, None, 128, None, None, None) == E
    assert L.hq_cosq_gather(None, 1, 5, 65537, None, None, 128, None, None, None) == U
    assert L.hq_cosq_gather(None, 1, 5, 64, None, None, 128, None, None, None) == E and _lib.last_error() == "null buffer"
    c = _filled(256, 64)
    assert L.hq_cosq_append(None, 0, 64, 64, None, 3, 256, ptr(c.X8), ptr(c.stats), stream()) == OK
    assert L.hq_cosq_replace(None, 0, 64, 64, None, None, 3, ptr(c.X8), ptr(c.stats), stream()) == OK
    torch.cuda.synchronize()
    _untouched(c, 0, "M = 0")
    assert L.hq_cosq_gather(None, 0, 0, 64, None, None, 256, ptr(c.X8), ptr(c.stats), stream()) == OK
    torch.cuda.synchronize()
    assert bool((c.X8[:128] == 0).all()) and bool((c.stats[:128] == 0).all())
    _untouched(c, 128, "gather M = 0")


def test_search_on_a_second_stream_sees_the_mutation(hq_lib):
    """A mutation on the current stream, then a search issued from another stream: it waits for the writer's event
    on the device and lists the new frames."""
    import torch
    n = 16
    F, MM = _frames3(300, n, 13)
    c = _fresh_corpus(F[:100], MM[:100])
    c.reserve(512)
    side = torch.cuda.Stream()
    qf, qm = _dev(F[[299, 150]]), _dev(MM[[299, 150]])
    torch.cuda.synchronize()
    c.append(F[100:300], MM[100:300])
    with torch.cuda.stream(side):
        s, ids = c.search(qf, qm, 3)
    side.synchronize()
    assert list(_np(ids)[:, 0]) == [299, 150] and np.all(np.abs(_np(s)[:, 0] - 1.0) <= C.TOL)
    torch.cuda.synchronize()
    c.remove(list(range(0, 100)))
    with torch.cuda.stream(side):
        s, ids = c.search(qf, qm, 3)
    side.synchronize()
    assert list(_np(ids)[:, 0]) == [199, 50]
    torch.cuda.synchronize()
    _same_corpus(c, F[100:300], MM[100:300], "after both")
