"""Float32 queries against the u8 frame store on the GPU (hq_cosqf_prepare / hq_cosqf_scores / hq_cosqf_topk,
rag.QuantizedFrameCorpus.search_float): dense scores against the long-double cosine of (the query's 24-bit
fixed-point row, the dequantised frame) within 1e-13 (cosq_cases.TOL), the fused top-k against select_topk of the
dense scores in ids, order and score bits, the rounding bound against the query's own float32 values, the pinned
u8 route on rows both can represent, and the public layer.  Every comparison prints its largest difference
(`cosqf-err ...`) before it asserts; profiles/cosqf_error_bounds.txt records them."""
import numpy as np
import pytest

import cosq_cases as C
import cosqf_cases as F

pytestmark = pytest.mark.gpu

ID_BASES = (0, 10 ** 9)


def _np(x):
    return x.detach().cpu().numpy()


def _dev_queries(q, ld=None, off=0):
    """q [R, K] float32 on the device as a view with row stride ld starting `off` floats into its buffer."""
    import torch
    R, K = q.shape
    if ld is None and off == 0:
        return torch.from_numpy(np.ascontiguousarray(q)).cuda()
    ld = K if ld is None else ld
    return torch.from_numpy(F.strided(q, ld, off)).cuda().as_strided((R, K), (ld, 1), off)


def _prep_q(q, ld=None, off=0):
    from hq_mi355x import kernels as K
    return K.cosqf_prepare(_dev_queries(q, ld, off))


def _prep_c(U, MM):
    import torch
    from hq_mi355x import kernels as K
    return K.cosq_prepare(torch.from_numpy(np.ascontiguousarray(U)).cuda(),
                          torch.from_numpy(np.ascontiguousarray(MM)).cuda())


def _report(name, got, exact):
    err = float(np.max(np.abs(got - exact))) if got.size else 0.0
    print(f"cosqf-err {name} {err:.3e}")
    return err


def _equal(got, want, msg):
    gs, gi = _np(got[0]), _np(got[1])
    ws, wi = _np(want[0]), _np(want[1])
    np.testing.assert_array_equal(gi, wi, err_msg=msg)
    assert gs.tobytes() == ws.tobytes(), msg


def test_operand_map(hq_lib):
    """Queries whose three digit planes all differ against asymmetric bytes with (mn, mx) = (0, 255): a swapped
    plane, row or column, or a wrong k order inside a step, is off by many orders of magnitude
    (test_cosqf_cpu.py::test_operand_map_inputs_are_asymmetric)."""
    from hq_mi355x import kernels as K
    q, v = F.operand_map_queries(19, 199)
    Uc, Mc = C.operand_map_rows(389, 199, 1)
    got = _np(K.cosqf_scores(_prep_q(q), _prep_c(Uc, Mc)))
    assert got.shape == (19, 389)
    assert _report("operand-map Q19 N389 K199", got, F.exact_scores(v, Uc, Mc)) <= F.TOL


_SHAPE = {}


def _shape(shape):
    """Per shape, computed once and shared: prepared rows, dense scores, exact scores, inputs."""
    import torch
    from hq_mi355x import kernels as K
    name, Q, N, Kd, ld, off, frames = shape
    if name not in _SHAPE:
        _SHAPE.clear()  # tests run shape by shape: keep one shape's buffers
        q = F.random_queries(Q, Kd, 11)
        Uc, Mc = C.random_rows(N, Kd, 12)
        if frames:  # [Q, r, c] frames compared on their K / c leading rows; the rest holds what must not be read
            r, c = frames
            x = np.full((Q, r * c), 3e38, np.float32)
            x[:, :Kd] = q
            pq = K.cosqf_prepare(torch.from_numpy(x.reshape(Q, r, c)).cuda(), Kd // c)
        else:
            pq = _prep_q(q, ld, off)
        pc = _prep_c(Uc, Mc)
        v, ok, _ = F.fix24(q)
        _SHAPE[name] = (pq, pc, K.cosqf_scores(pq, pc), F.exact_scores(v, Uc, Mc, ok), (q, Uc, Mc))
    return _SHAPE[name]


@pytest.mark.parametrize("shape", F.SHAPES, ids=[s[0] for s in F.SHAPES])
def test_shape_edges_dense(hq_lib, shape):
    """K, ld, base, N and Q edges (Q at 63 / 64 / 65 of the 64-query workgroup tile): dense scores within 1e-13 of
    exact; strided, offset and frame layouts give the bits of the contiguous one (nothing between rows is read)."""
    from hq_mi355x import kernels as K
    name, Q, N, Kd, ld, off, frames = shape
    pq, pc, dense, exact, (q, Uc, Mc) = _shape(shape)
    assert (pq.N, pq.K, pc.N, pc.K) == (Q, Kd, N, Kd)
    Qp = (Q + 63) // 64 * 64
    assert pq.Q8.shape == (Qp, 3 * C.padded_k(Kd)) and pq.stats.shape == (Qp, 4)
    got = _np(dense)
    assert got.shape == (Q, N)
    assert _report(f"shape {name} Q{Q} N{N} K{Kd} ld{ld} off{off}", got, exact) <= F.TOL
    if ld != Kd or off:
        assert _np(K.cosqf_scores(_prep_q(q), pc)).tobytes() == got.tobytes()


FUSED = tuple(s for s in F.SHAPES if s[0] in ("K63", "K64-ld72"))


@pytest.mark.parametrize("shape", FUSED, ids=[s[0] for s in FUSED])
def test_fused_equals_dense_select(hq_lib, hq_option, shape):
    """hq_cosqf_topk == select_topk(hq_cosqf_scores) in ids, order and score bits: k 1 / 10 / 64 (k > N through the
    dense route), thr_mode 0 / 1 / 2 at a threshold that is a score of the matrix and cuts the lists short,
    id_base 0 and 1e9, hint on / off / default."""
    from hq_mi355x import kernels as K
    name, Q, N = shape[:3]
    pq, pc, dense, _, _ = _shape(shape)
    row = np.sort(_np(dense)[Q // 2])[::-1]
    thr = float(row[3])
    for k in (1, 10, 64):
        for mode in (0, 1, 2):
            for base in ID_BASES:
                want = K.select_topk(dense, k, thr, mode, base)[:2]
                if mode:
                    assert int((_np(want[1])[Q // 2] >= 0).sum()) == min(k, 4 if mode == 1 else 3)
                for hint in (1, 0, None):
                    hq_option("cos_topk_hint", hint)
                    _equal(K.cosqf_topk(pq, pc, k, thr, mode, base), want,
                           f"{name} k={k} mode={mode} base={base} hint={hint}")
    for k in (65, N + 15):
        _equal(K.cosqf_topk(pq, pc, k, thr, 2, 7), K.select_topk(dense, k, thr, 2, 7)[:2], f"{name} dense route k={k}")
    small = K.CosQRows(pc.X8, pc.stats, 5, pc.K)  # the first five frames: k = 10 > N
    _equal(K.cosqf_topk(pq, small, 10), K.select_topk(K.cosqf_scores(pq, small), 10)[:2], f"{name} k > N")


def test_triplicated_corpus_and_query_blocks(hq_lib):
    """Every frame stored three times: equal score bits, listed in ascending id order; a workspace_limit that
    forces three query blocks gives identical lists."""
    from hq_mi355x import _lib, kernels as K
    Q, N, Kd = 300, 385, 64
    q = F.random_queries(Q, Kd, 21)
    Uc, Mc = C.random_rows(N, Kd, 22)
    pq, pc = _prep_q(q), _prep_c(np.concatenate([Uc] * 3), np.concatenate([Mc] * 3))
    dense = K.cosqf_scores(pq, pc)
    d = _np(dense)
    assert d[:, :N].tobytes() == d[:, N:2 * N].tobytes() == d[:, 2 * N:].tobytes()
    for k in (3, 10, 64):
        got = K.cosqf_topk(pq, pc, k)
        _equal(got, K.select_topk(dense, k)[:2], f"k={k}")
        s, ids = _np(got[0]), _np(got[1])
        ws, wi = C.reference_topk(d, k, 0.0, 0)
        np.testing.assert_array_equal(ids, wi)
        assert s.tobytes() == ws.tobytes()
        assert np.all(ids[:, 1] == ids[:, 0] + N) and np.all(ids[:, 2] == ids[:, 0] + 2 * N)
        assert np.all(s[:, 0] == s[:, 1]) and np.all(s[:, 1] == s[:, 2])
    size = _lib.load().hq_cosqf_topk_workspace_size
    limit = int(size(128, 3 * N, 10))  # one 128-query block fits, two do not: 128 + 128 + 44
    assert int(size(256, 3 * N, 10)) > limit
    one = K.cosqf_topk(pq, pc, 10, id_base=5)
    _equal(K.cosqf_topk(pq, pc, 10, id_base=5, workspace_limit=limit), one, "fused, three blocks")
    _equal(K.cosqf_topk(pq, pc, 70, 0.45, 2, 3, workspace_limit=128 * 3 * N * 8),
           K.select_topk(dense, 70, 0.45, 2, 3)[:2], "dense route, three blocks")


def test_accumulator_extremes(hq_lib):
    """K = 65536: v = -2^23 everywhere, 2^23 - 1 everywhere (the clamp) and half / half against u = 0, u = 255 and
    half / half frames: P2 = +-2^30 and K D, Sv S_c near 2^62 (they cancel to exactly 0 for the constant pairs:
    test_cosqf_cpu.py::test_accumulator_rows_reach_the_int32_extremes); within 1e-13 of exact.  K = 65537 is refused."""
    import torch
    from hq_mi355x import _lib, kernels as K
    q = F.accumulator_queries()
    U, MM = F.accumulator_frames()
    v, ok, _ = F.fix24(q)
    pq, pc = _prep_q(q), _prep_c(U, MM)
    dense = K.cosqf_scores(pq, pc)
    got = _np(dense)
    exact = F.exact_scores(v, U, MM, ok)
    assert _report("accumulator Q3 N16 K65536", got, exact) <= F.TOL
    assert _report("accumulator constant pairs", got[:2, :2], exact[:2, :2]) <= F.TOL
    assert _report("accumulator vs integer model", got, F.model_scores(q, U, MM)) <= 4 * np.finfo(np.float64).eps
    _equal(K.cosqf_topk(pq, pc, 10), K.select_topk(dense, 10)[:2], "K = 65536, fused")
    with pytest.raises(_lib.NativeLibraryError, match="65536"):
        K.cosqf_prepare(torch.zeros((2, C.MAX_K + 1), device="cuda"))
    rows = K.CosQFRows(pq.Q8, pq.stats, 2, C.MAX_K + 1)
    crow = K.CosQRows(pc.X8, pc.stats, 2, C.MAX_K + 1)
    with pytest.raises(_lib.NativeLibraryError, match="65536"):
        K.cosqf_scores(rows, crow)
    with pytest.raises(_lib.NativeLibraryError, match="65536"):
        K.cosqf_topk(rows, crow, 1)


_FAM = {}


def _families():
    """K = 4096, every query family against every frame family: computed once for the two tests below."""
    from hq_mi355x import kernels as K
    if not _FAM:
        q, names = F.all_families(4096)
        U, MM, fnames = C.all_families(4096)
        pc = _prep_c(U, MM)
        _FAM["x"] = (q, names, U, MM, fnames, pc, _np(K.cosqf_scores(_prep_q(q), pc)))
    return _FAM["x"]


def test_domain(hq_lib):
    """A zero row, a NaN row and an inf row score 0.0 everywhere and the other rows keep their bits; a frame with a
    non-finite (mn, mx) scores 0.0; subnormal and 1e30 queries (every family) are within 1e-13 of exact; the fused
    route agrees on the same rows (zeros tie at 0.0 by id)."""
    from hq_mi355x import kernels as K
    q, names, U, MM, fnames, pc, got = _families()
    v, ok, _ = F.fix24(q)
    exact = F.exact_scores(v, U, MM, ok)
    assert np.all(np.isfinite(got))
    for fam in F.FAMILIES:
        r = C.rows_of(names, {fam})
        assert _report(f"family {fam} K4096", got[r], exact[r]) <= F.TOL, fam
    dead = F.dead_rows(names)
    assert np.all(got[dead] == 0.0)
    assert np.all(got[:, C.rows_of(fnames, {"const_zero", "nonfinite"})] == 0.0)
    live = np.setdiff1d(np.arange(len(names)), dead)
    assert np.any(got[live] != 0.0, axis=1).all()
    alone = _np(K.cosqf_scores(_prep_q(q[live]), pc))
    assert alone.tobytes() == np.ascontiguousarray(got[live]).tobytes()
    pq = _prep_q(q)
    _equal(K.cosqf_topk(pq, pc, 10), K.select_topk(K.cosqf_scores(pq, pc), 10)[:2], "families, k = 10")


def test_against_the_querys_own_values(hq_lib):
    """|score - score of the float32 values| <= 2^(e - 24) sqrt(K) / |q| + 1e-13 for every family, and below 1e-5
    for the gaussian, post-ReLU and pipeline families."""
    q, names, U, MM, _, _, got = _families()
    d = np.abs(got - F.true_scores(q, U, MM))
    b = F.bound(q, 4096)
    for fam in F.FAMILIES:
        r = C.rows_of(names, {fam})
        print(f"cosqf-err own-values {fam} K4096 {d[r].max():.3e} (bound {b[r].max():.3e})")
    assert np.all(d <= b[:, None] + F.TOL)
    assert d[C.rows_of(names, set(F.SMOOTH))].max() < 1e-5


def test_grid_queries_agree_with_the_u8_route(hq_lib):
    """Rows of integers 0 .. 255 are exact in both routes (v = 2^15 q; u = q with (mn, mx) = (0, 255)): hq_cosqf_scores
    and hq_cosq_scores agree within 1e-13."""
    from hq_mi355x import kernels as K
    q, Uq, Mq = F.grid_rows(70, 199, 61)
    Uc, Mc = C.random_rows(389, 199, 62)
    pc = _prep_c(Uc, Mc)
    a, b = _np(K.cosqf_scores(_prep_q(q), pc)), _np(K.cosq_scores(_prep_c(Uq, Mq), pc))
    assert _report("grid vs u8 route Q70 N389 K199", a, b) <= F.TOL
    assert _report("grid vs exact", a, C.exact_scores(Uq, Mq, Uc, Mc)) <= F.TOL


def _parameters(N, d, seed):
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((8, d)).astype(np.float32)
    x = base[rng.integers(0, 8, N)] + np.float32(0.6) * rng.standard_normal((N, d)).astype(np.float32)
    return (x * rng.uniform(0.02, 2.0, (N, 1)).astype(np.float32)).astype(np.float32)


def test_public_layer(hq_lib):
    """QuantizedFrameCorpus: search_parameters(quantize_query=False) == search_float of the Hilbert-mapped
    parameters in bits, within 1e-5 of the NumPy float64 cosine of the mapped query and the dequantised frames;
    search_parameters keeps its bits; rows [Q, K] and one frame are accepted; shape and dtype errors."""
    import torch
    from hq_mi355x import kernels as K, rag
    from oracle import hq_oracle as O
    n, d, N, Q = 64, 1536, 385, 9
    X = _parameters(N, d, 51)
    noise = np.random.default_rng(52).standard_normal((Q, d)).astype(np.float32)
    xq = (X[:Q] + np.float32(0.2) * X[:Q].std(axis=1, keepdims=True) * noise).astype(np.float32)
    corpus = rag.QuantizedFrameCorpus.from_parameters(X, n)
    img = K.map_to_2d(torch.from_numpy(xq).cuda(), n)
    got = corpus.search_parameters(xq, 10, quantize_query=False)
    _equal(got, corpus.search_float(img, 10), "quantize_query=False")
    _equal(got, corpus.search_float(img.reshape(Q, n * n), 10), "rows [Q, K]")
    _equal(corpus.search_float(img[0], 3), corpus.search_float(img[:1], 3), "one frame")
    _equal(corpus.search_float(img, 5, threshold=0.8),
           K.cosqf_topk(K.cosqf_prepare(img), corpus._rows, 5, 0.8, 1), "threshold")
    # NumPy float64: the mapped query against the dequantised frames' n leading rows
    fr, _, mm = K.map_index_quantize(torch.from_numpy(X).cuda(), n)
    u, m = _np(fr)[:, :n].reshape(N, -1).astype(np.float64), _np(mm).astype(np.float64)
    dec = m[:, :1] + (m[:, 1:] - m[:, :1]) * u / 255.0
    qm = O.map_to_2d(O.pad_parameters(xq, n), n).reshape(Q, -1).astype(np.float64)
    assert np.array_equal(qm.astype(np.float32), _np(img).reshape(Q, -1))
    ref = ((qm @ dec.T) / np.outer(np.linalg.norm(qm, axis=1), np.linalg.norm(dec, axis=1)) + 1.0) / 2.0
    s, ids = _np(got[0]), _np(got[1])
    assert _report("public layer vs float64 cosine Q9 N385 K4096", s, np.take_along_axis(ref, ids, axis=1)) < 1e-5
    ws, wi = C.reference_topk(ref, 10, 0.0, 0)
    assert list(ids[:, 0]) == list(range(Q)) == list(wi[:, 0])
    # the quantised-query route keeps its bits
    fq, _, mq = K.map_index_quantize(torch.from_numpy(xq).cuda(), n)
    want = K.cosq_topk(K.cosq_prepare(fq, mq, n), corpus._rows, 10)
    _equal(corpus.search_parameters(xq, 10), want, "search_parameters")
    _equal(corpus.search_parameters(xq, 10, quantize_query=True), want, "quantize_query=True")
    with pytest.raises(TypeError):
        corpus.search_float(fq)
    with pytest.raises(TypeError):
        corpus.search_float(img.to(torch.float64))
    with pytest.raises(ValueError):
        corpus.search_float(img[:, :, :32])
    with pytest.raises(ValueError):
        corpus.search_float(img[:, :32])
    with pytest.raises(TypeError):
        corpus.search_parameters(xq.astype(np.float64), 10, quantize_query=False)
