"""Compressed-domain frame search on the GPU (hq_cosq_prepare / hq_cosq_scores / hq_cosq_topk,
rag.QuantizedFrameCorpus): dense scores against the long-double cosine of the dequantised rows within 1e-13
(cosq_cases.TOL), the fused top-k against select_topk of the dense scores in ids, order and score bits, the
reference's float32 arithmetic within the project's 1e-5, and the public layer.  Every comparison prints its
largest difference (`cosq-err ...`) before it asserts; profiles/cosq_error_bounds.txt records them."""
import numpy as np
import pytest

import cosq_cases as C

pytestmark = pytest.mark.gpu

ID_BASES = (0, 10 ** 9)


def _np(x):
    return x.detach().cpu().numpy()


def _dev_rows(U, ld=None, off=0):
    """U [R, K] on the device as a view with row stride ld starting `off` bytes into its buffer."""
    import torch
    R, K = U.shape
    if ld is None and off == 0:
        return torch.from_numpy(np.ascontiguousarray(U)).cuda()
    ld = K if ld is None else ld
    buf = torch.from_numpy(C.strided(U, ld, off)).cuda()
    return buf.as_strided((R, K), (ld, 1), off)


def _prepare(U, MM, ld=None, off=0):
    import torch
    from hq_mi355x import kernels as K
    return K.cosq_prepare(_dev_rows(U, ld, off), torch.from_numpy(np.ascontiguousarray(MM)).cuda())


def _report(name, got, exact):
    err = float(np.max(np.abs(got - exact))) if got.size else 0.0
    print(f"cosq-err {name} {err:.3e}")
    return err


def _equal(got, want, msg):
    gs, gi = _np(got[0]), _np(got[1])
    ws, wi = _np(want[0]), _np(want[1])
    np.testing.assert_array_equal(gi, wi, err_msg=msg)
    assert gs.tobytes() == ws.tobytes(), msg


def test_operand_map(hq_lib):
    """Asymmetric integer bytes with (mn, mx) = (0, 255): a swapped row / column or a wrong k order inside a step
    is off by many orders of magnitude (test_cosq_cpu.py::test_operand_map_inputs_are_asymmetric)."""
    from hq_mi355x import kernels as K
    Uq, Mq = C.operand_map_rows(19, 199, 0)
    Uc, Mc = C.operand_map_rows(389, 199, 1)
    got = _np(K.cosq_scores(_prepare(Uq, Mq), _prepare(Uc, Mc)))
    assert got.shape == (19, 389)
    assert _report("operand-map Q19 N389 K199", got, C.exact_scores(Uq, Mq, Uc, Mc)) <= C.TOL


_SHAPE = {}


def _shape(shape):
    """Per shape, computed once and shared: prepared rows, dense scores, exact scores."""
    from hq_mi355x import kernels as K
    name, Q, N, Kd, ld, off = shape
    if name not in _SHAPE:
        _SHAPE.clear()  # tests run shape by shape: keep one shape's buffers
        Uq, Mq = C.random_rows(Q, Kd, 11)
        Uc, Mc = C.random_rows(N, Kd, 12)
        pq, pc = _prepare(Uq, Mq, ld, off), _prepare(Uc, Mc, ld, off)
        _SHAPE[name] = (pq, pc, K.cosq_scores(pq, pc), C.exact_scores(Uq, Mq, Uc, Mc), (Uq, Mq, Uc, Mc))
    return _SHAPE[name]


@pytest.mark.parametrize("shape", C.SHAPES, ids=[s[0] for s in C.SHAPES])
def test_shape_edges_dense(hq_lib, shape):
    """K, ld, base, N and Q edges: dense scores within 1e-13 of exact; the strided / offset layouts give the
    bits of the contiguous one (the bytes between rows are never read into the sums)."""
    from hq_mi355x import kernels as K
    name, Q, N, Kd, ld, off = shape
    pq, pc, dense, exact, (Uq, Mq, Uc, Mc) = _shape(shape)
    assert (pq.N, pq.K, pc.N, pc.K) == (Q, Kd, N, Kd)
    assert pc.X8.shape == (C.padded_rows(N), C.padded_k(Kd)) and pc.stats.shape == (C.padded_rows(N), 4)
    got = _np(dense)
    assert got.shape == (Q, N)
    assert _report(f"shape {name} Q{Q} N{N} K{Kd} ld{ld} off{off}", got, exact) <= C.TOL
    if ld != Kd or off:
        plain = K.cosq_scores(_prepare(Uq, Mq), _prepare(Uc, Mc))
        assert _np(plain).tobytes() == got.tobytes()


@pytest.mark.parametrize("shape", C.SHAPES, ids=[s[0] for s in C.SHAPES])
def test_fused_equals_dense_select(hq_lib, hq_option, shape):
    """hq_cosq_topk == select_topk(hq_cosq_scores) in ids, order and score bits: k 1 / 10 / 64 (k > N through the
    dense route), thr_mode 0 / 1 / 2 at a threshold that is a score of the matrix and cuts the lists short,
    id_base 0 and 1e9, hint on / off / default."""
    from hq_mi355x import kernels as K
    name, Q, N, Kd, ld, off = shape
    pq, pc, dense, _, _ = _shape(shape)
    row = np.sort(_np(dense)[Q // 2])[::-1]
    thr = float(row[min(3, N - 1)])
    for k in (1, 10, 64):
        for mode in (0, 1, 2):
            for base in ID_BASES:
                want = K.select_topk(dense, k, thr, mode, base)[:2]
                if mode and N > 4:
                    assert int((_np(want[1])[Q // 2] >= 0).sum()) == min(k, 4 if mode == 1 else 3)
                for hint in (1, 0, None):
                    hq_option("cos_topk_hint", hint)
                    _equal(K.cosq_topk(pq, pc, k, thr, mode, base), want, f"{name} k={k} mode={mode} base={base} hint={hint}")


def test_triplicated_corpus_ties_by_id(hq_lib):
    """Every frame stored three times: equal score bits, listed in ascending id order."""
    from hq_mi355x import kernels as K
    Q, N, Kd = 129, 385, 64
    Uq, Mq = C.random_rows(Q, Kd, 21)
    Uc, Mc = C.random_rows(N, Kd, 22)
    U3, M3 = np.concatenate([Uc] * 3), np.concatenate([Mc] * 3)
    pq, pc = _prepare(Uq, Mq), _prepare(U3, M3)
    dense = K.cosq_scores(pq, pc)
    d = _np(dense)
    assert d[:, :N].tobytes() == d[:, N:2 * N].tobytes() == d[:, 2 * N:].tobytes()
    for k in (3, 10, 64):
        got = K.cosq_topk(pq, pc, k)
        _equal(got, K.select_topk(dense, k)[:2], f"k={k}")
        s, ids = _np(got[0]), _np(got[1])
        ws, wi = C.reference_topk(d, k, 0.0, 0)
        np.testing.assert_array_equal(ids, wi)
        assert s.tobytes() == ws.tobytes()
        assert np.all(ids[:, 1] == ids[:, 0] + N) and np.all(ids[:, 2] == ids[:, 0] + 2 * N)
        assert np.all(s[:, 0] == s[:, 1]) and np.all(s[:, 1] == s[:, 2])


def test_dense_route_and_query_blocks(hq_lib):
    """k = 65 and k > N go through cosq_topk's dense route; a workspace_limit that forces three query blocks
    gives identical lists, fused and dense route."""
    import torch
    from hq_mi355x import _lib, kernels as K
    Q, N, Kd, k = 300, 769, 64, 10
    Uq, Mq = C.random_rows(Q, Kd, 31)
    Uc, Mc = C.random_rows(N, Kd, 32)
    pq, pc = _prepare(Uq, Mq), _prepare(Uc, Mc)
    dense = K.cosq_scores(pq, pc)
    one = K.cosq_topk(pq, pc, k, id_base=5)
    _equal(one, K.select_topk(dense, k, 0.0, 0, 5)[:2], "unsplit")
    size = _lib.load().hq_cosq_topk_workspace_size
    limit = int(size(128, N, k))  # one 128-query block fits, two do not: 128 + 128 + 44
    assert int(size(256, N, k)) > limit
    _equal(K.cosq_topk(pq, pc, k, id_base=5, workspace_limit=limit), one, "fused, three blocks")
    for kk in (65, 200, 1000):
        want = K.select_topk(dense, kk, 0.45, 2, 3)[:2]
        _equal(K.cosq_topk(pq, pc, kk, 0.45, 2, 3), want, f"k = {kk}")
        _equal(K.cosq_topk(pq, pc, kk, 0.45, 2, 3, workspace_limit=128 * N * 8), want, f"k = {kk}, three blocks")
    with pytest.raises(ValueError, match="query length"):
        K.cosq_topk(_prepare(*C.random_rows(2, 32, 1)), pc, 5)
    with pytest.raises(TypeError):
        K.cosq_prepare(torch.zeros((2, 32), device="cuda"), torch.zeros((2, 2), device="cuda"))


def test_row_families(hq_lib):
    """K = 4096, every family as queries and as frames: within 1e-13 of exact; constant frames score 1 or 0 by
    sign; zero frames and non-finite (mn, mx) rows score 0.0 exactly and change no other score."""
    from hq_mi355x import kernels as K
    U, MM, names = C.all_families(4096)
    exact = C.exact_scores(U, MM, U, MM)
    p = _prepare(U, MM)
    got = _np(K.cosq_scores(p, p))
    assert np.all(np.isfinite(got))
    for fam in C.FAMILIES:
        r = C.rows_of(names, {fam})
        err = max(_report(f"family {fam} as queries K4096", got[r], exact[r]),
                  _report(f"family {fam} as frames K4096", got[:, r], exact[:, r]))
        assert err <= C.TOL, fam
    dead = C.rows_of(names, {"const_zero", "nonfinite"})
    assert np.all(got[dead] == 0.0) and np.all(got[:, dead] == 0.0)
    pos, neg = C.rows_of(names, {"const_pos"}), C.rows_of(names, {"const_neg"})
    for a, b, want in ((pos, pos, 1.0), (neg, neg, 1.0), (pos, neg, 0.0), (neg, pos, 0.0)):
        assert np.all(np.abs(got[np.ix_(a, b)] - want) <= C.TOL)
    live = np.setdiff1d(np.arange(len(names)), C.rows_of(names, {"nonfinite"}))
    pl = _prepare(U[live], MM[live])
    assert _np(K.cosq_scores(pl, pl)).tobytes() == np.ascontiguousarray(got[np.ix_(live, live)]).tobytes()
    # the fused route on the same rows (zeros tie at 0.0 by id)
    _equal(K.cosq_topk(p, p, 10), K.select_topk(K.cosq_scores(p, p), 10)[:2], "families, k = 10")


def test_accumulator_range(hq_lib):
    """K = 65536: P = 2^30 and the most negative sum, within 1e-13 of exact; K = 65537 is refused."""
    import torch
    from hq_mi355x import _lib, kernels as K
    U, MM = C.accumulator_rows()
    p = _prepare(U, MM)
    got = _np(K.cosq_scores(p, p))
    assert _report("accumulator Q16 N16 K65536", got, C.exact_scores(U, MM, U, MM)) <= C.TOL
    _equal(K.cosq_topk(p, p, 10), K.select_topk(K.cosq_scores(p, p), 10)[:2], "K = 65536, fused")
    big = torch.zeros((2, C.MAX_K + 1), dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.NativeLibraryError, match="65536"):
        K.cosq_prepare(big, torch.zeros((2, 2), device="cuda"))
    rows = K.CosQRows(p.X8, p.stats, 2, C.MAX_K + 1)
    with pytest.raises(_lib.NativeLibraryError, match="65536"):
        K.cosq_scores(rows, rows)
    with pytest.raises(_lib.NativeLibraryError, match="65536"):
        K.cosq_topk(rows, rows, 1)


def _parameters(N, d, seed):
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((8, d)).astype(np.float32)
    x = base[rng.integers(0, 8, N)] + np.float32(0.6) * rng.standard_normal((N, d)).astype(np.float32)
    return (x * rng.uniform(0.02, 2.0, (N, 1)).astype(np.float32)).astype(np.float32)


def test_against_reference_arithmetic(hq_lib):
    """Frames from map_index_quantize (d = 1536, n = 64): the scores are within the project's 1e-5 of the
    reference's own float32 decode + cosine (oracle denormalize_u8 + rag_cosine), and within 1e-13 of exact."""
    import torch
    from hq_mi355x import kernels as K
    from oracle import hq_oracle as O
    n, d, N, Q = 64, 1536, 500, 40
    X = _parameters(N, d, 41)
    Xq = (X[:Q] + np.float32(0.05) * np.random.default_rng(42).standard_normal((Q, d)).astype(np.float32)).astype(np.float32)
    fr, _, mm = K.map_index_quantize(torch.from_numpy(X).cuda(), n)
    fq, _, mq = K.map_index_quantize(torch.from_numpy(Xq).cuda(), n)
    assert fr.shape == (N, n + 1, n)
    got = _np(K.cosq_scores(K.cosq_prepare(fq, mq, n), K.cosq_prepare(fr, mm, n)))
    fr, mm, fq, mq = _np(fr), _np(mm), _np(fq), _np(mq)
    dec = np.stack([O.denormalize_u8(fr[i, :n], mm[i, 0], mm[i, 1]) for i in range(N)]).reshape(N, -1)
    decq = np.stack([O.denormalize_u8(fq[i, :n], mq[i, 0], mq[i, 1]) for i in range(Q)]).reshape(Q, -1)
    ref = np.stack([O.rag_cosine(decq[i], dec) for i in range(Q)])
    assert _report("reference-f32 Q40 N500 K4096", got, ref) < 1e-5
    exact = C.exact_scores(fq[:, :n].reshape(Q, -1), mq, fr[:, :n].reshape(N, -1), mm)
    assert _report("pipeline-frames Q40 N500 K4096", got, exact) <= C.TOL


def test_public_layer(hq_lib):
    """QuantizedFrameCorpus: from_parameters / search_parameters find every row itself first with score 1;
    search == kernels.cosq_topk on the same operands; rows= honours a store without an index row."""
    import torch
    from hq_mi355x import kernels as K, rag
    n, d, N = 64, 1536, 300
    X = _parameters(N, d, 51)
    corpus = rag.QuantizedFrameCorpus.from_parameters(X, n)
    assert (len(corpus), corpus.N, corpus.K, corpus.rows, corpus.shape) == (N, N, n * n, n, (n + 1, n))
    assert corpus.resident_bytes == C.padded_rows(N) * (n * n + 32)
    pick = np.array([0, 7, 150, 299])
    s, ids = corpus.search_parameters(X[pick], k=5)
    s, ids = _np(s), _np(ids)
    assert s.shape == ids.shape == (4, 5)
    assert list(ids[:, 0]) == list(pick)
    print(f"cosq-err self-score {float(np.max(np.abs(s[:, 0] - 1.0))):.3e}")
    assert np.all(np.abs(s[:, 0] - 1.0) <= C.TOL)
    assert np.all(np.diff(s, axis=1) <= 0)
    fr, _, mm = K.map_index_quantize(torch.from_numpy(X).cuda(), n)
    pc = K.cosq_prepare(fr, mm, n)
    fq, mq = fr[pick.tolist()], mm[pick.tolist()]
    _equal(corpus.search(fq, mq, 5), K.cosq_topk(K.cosq_prepare(fq, mq, n), pc, 5), "search")
    _equal(corpus.search(fq, mq, 5, threshold=0.8), K.cosq_topk(K.cosq_prepare(fq, mq, n), pc, 5, 0.8, 1), "threshold")
    _equal(corpus.search(fq[0], mq[0], 3), K.cosq_topk(K.cosq_prepare(fq[:1], mq[:1], n), pc, 3), "one query frame")
    # a store without an index row: [N, n, n] compares all n rows by default, rows= fewer
    plain = fr[:, :n].contiguous()
    c2 = rag.QuantizedFrameCorpus(plain, mm)
    assert (c2.rows, c2.K) == (n, n * n)
    _equal(c2.search(plain[pick.tolist()], mq, 5), corpus.search(fq, mq, 5), "no index row")
    c3 = rag.QuantizedFrameCorpus(fr, mm, rows=n + 1)  # the index row compared too
    assert c3.K == (n + 1) * n
    _equal(c3.search(fq, mq, 5), K.cosq_topk(K.cosq_prepare(fq, mq), K.cosq_prepare(fr, mm), 5), "rows = n + 1")
    c4 = rag.QuantizedFrameCorpus(fr, mm, rows=16)
    _equal(c4.search(fq, mq, 5), K.cosq_topk(K.cosq_prepare(fq, mq, 16), K.cosq_prepare(fr, mm, 16), 5), "rows = 16")
    with pytest.raises(ValueError):
        corpus.search(fq[:, :, :32], mq)
