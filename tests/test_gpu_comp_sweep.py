"""Shape, profile and edge sweep of the comprehensive frame similarity on the GPU (hq_comp.hip, kernels.comp_*,
rag/similarity.py) against the float64 models and built frames of tests/comp_sweep_cases.py and the reference's
recorded scores (tests/golden/comprehensive_shapes.npz).

* hq_comp_describe: exact, at widths on both sides of the 64-lane column loop, heights on both sides of the H > 32
  flag path, 0 / 1 / 31 index rows, -0.0 and NaN rows, and past its 65536-block grid.
* hq_comp_scores: 1e-12 of the model for float64 and float32 frames alike (the kernel accumulates the float32 values
  in float64) on heterogeneous sets of every shape of comp_sweep_cases.SHAPES, at the ends of the 4-wave x 32-frame
  walk, past the 65535 cap of grid.y, and on both sides of the header's LDS rule.
* The fused route: within 1e-5, the project's score contract, of the exact route and of the float64 composite model at
  every window geometry hq_comp_prepare takes; the operand itself; frames read in place through `ld`.
* ComprehensiveFrameCorpus: tiny and ragged N, k >= N, mixed batches, empty batches and an empty store."""
import numpy as np
import pytest

import comp_cases as C
import comp_sweep_cases as SW

pytestmark = pytest.mark.gpu

FUSED_TOL = 1e-5
EXACT_TOL = 1e-12


@pytest.fixture(scope="module")
def rt(hq_lib):
    import torch
    from hq_mi355x import kernels as K
    from hq_mi355x._dev import to_dev, to_np
    from hq_mi355x._lib import HQ_E_UNSUPPORTED, NativeLibraryError
    from hq_mi355x.rag import similarity as S

    class RT:
        pass

    r = RT()
    r.t, r.K, r.S, r.dev, r.np = torch, K, S, to_dev, to_np
    r.Error, r.unsupported = NativeLibraryError, f"error {HQ_E_UNSUPPORTED}: "
    return r


def _describe(rt, x):
    return rt.np(rt.K.comp_describe(rt.dev(x))).astype(np.int64) & np.array([-1, -1, -1, 0xFFFFFFFF])


# ------------------------------------------------------------------------------------------------ describe
DESCRIBE_W = (1, 3, 63, 64, 65, 129, 200)
DESCRIBE_H = (1, 2, 32, 33, 40)


def _describe_frames(H, W, dtype):
    """Frames whose descriptors sit at the kernel's edges (expected values: SW.describe_all and C.describe)."""
    rng = np.random.default_rng(100 * H + W)
    cols = [c for c in (0, 63, 64, W - 1) if c < W] if W > 1 else []   # a lone entry in a 1-wide row makes it dense
    out = [rng.standard_normal((H, W)), np.zeros((H, W))]               # 0 rows below h; h = H without a dense row
    for below in (1, 31):
        if H > below:
            for shift in range(max(len(cols), 1)):
                x = np.zeros((H, W))
                x[:H - below] = rng.standard_normal((H - below, W))
                for r in range(below):  # one entry per index row: the last non-zero column at 0, 63, 64, W - 1
                    if cols:
                        x[H - below + r, cols[(r + shift) % len(cols)]] = rng.standard_normal()
                out.append(x)
    if H >= 3:
        x = rng.standard_normal((H, W))
        x[H - 2] = -0.0                                                 # counts as a zero row
        x[H - 1] = 0.0
        if W > 1:
            x[H - 1, min(W - 1, 64)] = np.nan                           # a NaN is not zero: a live index row
        else:
            x[H - 1, 0] = np.nan                                        # dense: h = H
        out.append(x)
        y = rng.standard_normal((H, W))
        y[H - 1] = np.nan                                               # a dense row of NaN
        out.append(y)
    for p in (0.2, 0.5, 0.8):                                           # ragged rows, at most H / 2 rows below h
        x = rng.standard_normal((H, W)) * (rng.random((H, W)) < p)
        x[(H - 1) // 2] = rng.standard_normal(W)
        out.append(x)
    return np.stack(out).astype(dtype)


@pytest.mark.parametrize("dtype", ("float32", "float64"))
def test_describe_sweep(rt, dtype):
    seen = set()
    for H in DESCRIBE_H:
        for W in DESCRIBE_W:
            x = _describe_frames(H, W, dtype)
            want = SW.describe_all(x)
            assert want.tolist() == [list(C.describe(e)) for e in x]
            assert _describe(rt, x).tolist() == want.tolist(), (H, W)
            assert _describe(rt, x[2:3]).tolist() == want[2:3].tolist(), (H, W)         # N = 1
            seen |= {(int(d[1]), int(d[2])) for d in want}
    assert {L for L, _ in seen} >= {0, 1, 31} and {w for _, w in seen} >= {0, 1, 64, 65, 129, 200}


@pytest.mark.parametrize("dtype", ("float32", "float64"))
def test_describe_past_the_grid(rt, dtype):
    """N = 65536 + 5 frames of 3 x 4: the last five blocks take a second frame."""
    d = np.random.default_rng(3).standard_normal((3, 4))
    z = np.zeros(4)
    base = np.array([[z, z, z], [d[0], d[1], d[2]], [d[0], d[1], z], [d[0], d[1], [0, 0, 0, 1.0]],
                     [d[0], [1.0, 0, 0, 0], [0, 2.0, 0, 0]], [d[0], -z, [3.0, 0, 0, 0]], [d[0], z, z],
                     [[1.0, 0, 0, 0], z, z]])
    want = SW.describe_all(base.astype(dtype))
    assert want.tolist() == [[3, 0, 0, 0], [3, 0, 0, 0], [2, 0, 0, 0], [2, 1, 4, 1], [1, 2, 2, 3], [1, 1, 1, 2],
                             [1, 0, 0, 0], [3, 0, 0, 0]]
    idx = np.arange(65536 + 5) % 8
    got = _describe(rt, base.astype(dtype)[idx])
    assert (got == want[idx]).all()


# --------------------------------------------------------------------------------------------- exact route
@pytest.mark.parametrize("H,W,h", SW.SHAPES)
@pytest.mark.parametrize("dtype", ("float64", "float32"))
def test_exact_route_on_heterogeneous_sets(rt, H, W, h, dtype):
    x, desc = SW.hetero_set(H, W, h, dtype)
    parts, score = SW.hetero_model(H, W, h, dtype)
    assert _describe(rt, x).tolist() == desc.tolist()
    sc, pt = rt.S.comprehensive_scores(x, x, parts=True)
    print(H, W, h, dtype, "score err", np.abs(rt.np(sc) - score).max(), "parts err", np.abs(rt.np(pt) - parts).max())
    assert np.abs(rt.np(pt) - parts).max() <= EXACT_TOL
    assert np.abs(rt.np(sc) - score).max() <= EXACT_TOL
    assert rt.t.equal(rt.S.comprehensive_scores(x, x), sc)                               # parts = NULL: the same bits


@pytest.mark.parametrize("name", SW.GOLDEN_SETS)
def test_exact_route_matches_second_golden(rt, name):
    g = SW.golden()
    e = g[f"g_{name}_enh"]
    tol = C.tolerance(e.dtype)
    assert _describe(rt, e)[:, :3].tolist() == g[f"g_{name}_desc"].tolist()
    sc, pt = rt.S.comprehensive_scores(e, e, parts=True)
    for got, want in ((rt.np(sc), g[f"g_{name}_score"]), (rt.np(pt), g[f"g_{name}_parts"])):
        assert (np.isnan(got) == np.isnan(want)).all()     # a NaN or inf in a frame: NaN, as the reference
        print(name, "err", np.nanmax(np.abs(got - want)))
        assert np.nanmax(np.abs(got - want)) <= tol


@pytest.mark.parametrize("Q", (1, 2))
def test_exact_route_at_the_ends_of_the_frame_walk(rt, Q):
    """N around the 4 waves and the 32 frames of a workgroup."""
    x, _ = SW.hetero_set(9, 8, 8, "float32")
    _, score = SW.hetero_model(9, 8, 8, "float32")
    qi = np.array([5, 20])[:Q]
    for N in (1, 3, 4, 5, 31, 32, 33, 65):
        ci = (7 * np.arange(N) + 3) % len(x)
        got = rt.np(rt.S.comprehensive_scores(x[qi], x[ci]))
        assert got.shape == (Q, N)
        assert np.abs(got - score[np.ix_(qi, ci)]).max() <= EXACT_TOL, N


def test_exact_route_past_the_query_grid(rt):
    """Q = 65535 + 3: queries 65535 .. 65537 are the second trip of workgroups y = 0 .. 2."""
    x, _ = SW.hetero_set(5, 4, 4, "float32")
    pick = [SW.KINDS.index(k) for k in ("full", "drop_first", "short", "negated", "same_sign", "noisy")]
    six, fr = x[pick], x[[14, 14 + SW.KINDS.index("zero_patch"), 28]]
    _, model = SW.model_parts(six, fr)
    # the six rows differ: a mis-indexed query shows
    assert min(np.abs(model[a] - model[b]).max() for a in range(6) for b in range(a)) > 1e-3
    idx = np.arange(65535 + 3) % 6
    small = rt.S.comprehensive_scores(six, fr)
    big = rt.S.comprehensive_scores(six[idx], fr)
    assert tuple(big.shape) == (65538, 3)
    assert np.abs(rt.np(big) - model[idx]).max() <= EXACT_TOL
    assert rt.t.equal(big, small[rt.dev(idx)])


def test_exact_route_inputs_through_the_wrappers(rt):
    x64, _ = SW.hetero_set(9, 8, 8, "float64")
    x32, _ = SW.hetero_set(9, 8, 8, "float32")
    keep = [SW.KINDS.index(k) for k in ("full", "drop_first", "short", "zero_patch", "negated", "same_sign",
                                        "const_rows", "noisy")]
    # float32 queries against float64 frames: both promoted to float64
    got = rt.np(rt.S.comprehensive_scores(x32[:6], x64))
    assert np.abs(got - SW.model_scores(x32[:6], x64)).max() <= EXACT_TOL
    # integers and float16 are widened to float64
    ints = (np.sign(x64[keep]) * np.ceil(np.abs(4 * x64[keep]))).astype(np.int32)
    assert np.abs(rt.np(rt.S.comprehensive_scores(ints, ints)) - SW.model_scores(ints, ints)).max() <= EXACT_TOL
    half = x64[keep].astype(np.float16)
    got = rt.S.comprehensive_scores(rt.dev(half), rt.dev(half))
    assert got.dtype == rt.t.float64
    assert np.abs(rt.np(got) - SW.model_scores(half, half)).max() <= EXACT_TOL
    # a non-contiguous view
    view = rt.dev(x32)[::2]
    assert not view.is_contiguous()
    assert np.abs(rt.np(rt.S.comprehensive_scores(view, view)) - SW.hetero_model(9, 8, 8, "float32")[1][::2, ::2]).max() \
        <= EXACT_TOL


@pytest.mark.parametrize("dtype", ("float32", "float64"))
def test_exact_route_lds_rule(rt, dtype):
    """include/hq_mi355x.h: (5 max_windows + H W) values must fit 160 KiB.  The largest square-ish frame the rule
    accepts is scored, the first it refuses returns HQ_E_UNSUPPORTED, from hq_comp_scores and through the corpus."""
    (H0, W0), (H1, W1) = SW.lds_edge(np.dtype(dtype).itemsize)
    print(dtype, "accepted", (H0, W0), SW.lds_bytes(H0, W0, np.dtype(dtype).itemsize), "refused", (H1, W1))
    rng = np.random.default_rng(9)
    x = np.stack([SW.build_frame(rng, H0, W0, H0 - 2)[0] for _ in range(4)] +
                 [SW.build_frame(rng, H0, W0, H0 - 2, "short")[0]]).astype(dtype)
    sc, pt = rt.S.comprehensive_scores(x[:2], x[2:], parts=True)
    parts, score = SW.model_parts(x[:2], x[2:])
    assert np.abs(rt.np(sc) - score).max() <= EXACT_TOL and np.abs(rt.np(pt) - parts).max() <= EXACT_TOL
    y = np.stack([SW.build_frame(rng, H1, W1, H1 - 2)[0] for _ in range(3)]).astype(dtype)
    text = rt.unsupported + f"frame {H1}x{W1}: query and window lists exceed 160 KiB of LDS"
    with pytest.raises(rt.Error, match=text):
        rt.S.comprehensive_scores(y[:1], y)
    corpus = rt.S.ComprehensiveFrameCorpus(y)    # float64: never fused; float32: more windows than prepare stages
    assert corpus.fused is False and not rt.K.comp_prepare_fits(H1, W1, H1 - 2)
    with pytest.raises(rt.Error, match=text):
        corpus.scores(y[:1])
    with pytest.raises(rt.Error, match=text):
        corpus.search(y[:1], 2)


# --------------------------------------------------------------------------------------------- fused route
def _fused_dense(rt, qs, fr, h):
    coef = rt.S._level_coef(fr.shape[1] - h)
    q = rt.K.comp_prepare(rt.dev(qs), h, 0, coef)
    c = rt.K.comp_prepare(rt.dev(fr), h, 1, coef)
    return q, c, rt.K.cosine_scores_mfma(q, c)


@pytest.mark.parametrize("H,W,h", SW.FUSED_PROFILES)
def test_fused_scores_at_every_window_geometry(rt, H, W, h):
    """4 queries x 48 frames per family against the exact route and the float64 composite model; the limit is the
    contract.  Measured on an MI355X: at most 6.8e-7 up to K = 4991, 2.0e-6 at 12 x 100, and 7.1e-6 (negated
    queries), 3.7e-6 (near-duplicate) at 35 x 128, K = 20547; profiles/comp_error_bounds.txt has the 16 x 256
    figures of tools/ab_comp.py --what errors (7.4e-6 there)."""
    assert rt.K.comp_prepare_fits(H, W, h)
    for kind in SW.FUSED_FAMILIES:
        qs, fr = SW.fused_store(H, W, h, kind)
        q, c, sc = _fused_dense(rt, qs, fr, h)
        assert q.K == c.K == C.composite_k(H, W, h)
        exact = rt.S.comprehensive_scores(qs, fr)
        model = C.composite_scores(qs, fr, h)
        e1, e2 = float((sc - exact).abs().max()), float(np.abs(rt.np(sc) - model).max())
        print(H, W, h, kind, "K", q.K, "fused max err vs exact", e1, "vs model", e2)
        assert np.abs(rt.np(exact) - model).max() <= EXACT_TOL
        assert e1 <= FUSED_TOL and e2 <= FUSED_TOL


def test_generator_frames_128_wide_are_refused_not_fused(rt):
    """The RAG generator's 128 x 128 images (131 x 128 frames, h = 128, K = 84243) have 3969 windows: hq_comp_prepare
    stages 16 x (L + 1 + windows) float64 coefficients in LDS (508 KB > 160 KiB) and returns HQ_E_UNSUPPORTED, so
    the profile's fused error cannot be measured and the 1e-5 contract does not cover it.  The corpus does not fuse
    the store; hq_comp_scores cannot stage a 131 x 128 frame either (228 KB), so scoring refuses with its message."""
    rng = np.random.default_rng(4)
    fr = np.stack([SW.enhance128(im) for im in rng.standard_normal((6, 128, 128)).astype(np.float32)])
    assert _describe(rt, fr).tolist() == [[128, 3, 64, 7]] * 6
    assert rt.K.comp_layout(131, 128, 128)["K"] == 84243 and not rt.K.comp_prepare_fits(131, 128, 128)
    with pytest.raises(rt.Error, match=rt.unsupported + "frame 131x128: section coefficients exceed 160 KiB of LDS"):
        rt.K.comp_prepare(rt.dev(fr), 128, 1, rt.S._level_coef(3))
    corpus = rt.S.ComprehensiveFrameCorpus(fr)
    assert corpus.fused is False and corpus.K is None
    with pytest.raises(rt.Error, match=rt.unsupported + "frame 131x128: query and window lists exceed 160 KiB of LDS"):
        corpus.search(fr[:2], 3)


def test_prepare_takes_profiles_up_to_its_lds_rule(rt):
    """16 x (L + 1 + windows) float64 coefficients in 160 KiB: 1280 sections pass, 1281 do not (W = 8: 7 windows
    across, ws = 2 at stride 1)."""
    ok, over = (188, 8, 183), (189, 8, 183)           # 7 * 182 = 1274 windows + 1 + L = 1280 / 1281
    assert rt.K.comp_prepare_fits(*ok) and not rt.K.comp_prepare_fits(*over)
    qs, fr = SW.fused_store(*ok, "negated", Q=2, N=5)
    _, _, sc = _fused_dense(rt, qs, fr, ok[2])
    assert np.abs(rt.np(sc) - C.composite_scores(qs, fr, ok[2])).max() <= FUSED_TOL
    qs, fr = SW.fused_store(*over, "gaussian", Q=1, N=2)
    with pytest.raises(rt.Error, match=rt.unsupported + "frame 189x8: section coefficients exceed 160 KiB of LDS"):
        rt.K.comp_prepare(rt.dev(fr), over[2], 1, rt.S._level_coef(6))


def _operand_rows(rt, rows):
    """hi + lo of a prepared operand as float64 [Np, Kp], and its planes [tile, kb, plane, g, j, u]: fragment (tile,
    kb, plane) = 64 lanes x 8 halves, lane 16 g + j = row j, k = 32 kb + 8 g + u."""
    Np, _, Kp = rows.X16.shape
    x = rt.np(rows.X16.view(-1).double()).reshape(Np // 16, Kp // 32, 2, 4, 16, 8)
    return (x[:, :, 0] + x[:, :, 1]).transpose(0, 3, 1, 2, 4).reshape(Np, Kp), x


@pytest.mark.parametrize("H,W,h", ((20, 65, 17), (6, 4, 4)))
def test_prepare_operand_at_odd_and_tiny_profiles(rt, H, W, h):
    qs, fr = SW.fused_store(H, W, h, "gaussian", Q=2, N=20)
    fr = fr.copy()
    fr[3, 2, W - 1] = np.nan
    fr[5, H - 1, 0] = np.inf
    q, c, sc = _fused_dense(rt, qs, fr, h)
    inv = rt.np(c.inv)
    assert inv[3] == 0.0 and inv[5] == 0.0 and (inv[20:] == 0.0).all() and (inv[[0, 1, 2, 4, 19]] == 1.0).all()
    s = rt.np(sc)
    assert (s[:, [3, 5]] == 0.0).all() and np.isfinite(s).all()
    rows, planes = _operand_rows(rt, c)
    assert (planes[1][:, :, :, 4:, :] == 0.0).all() and (planes[2:] == 0.0).all()       # rows 20 .. are pad rows
    model = C.composite_rows(fr, h, 1)
    K = model.shape[1]
    assert K == C.composite_k(H, W, h) and rows.shape[1] >= K
    keep = [i for i in range(20) if i not in (3, 5)]
    assert (rows[:20, K:] == 0.0).all()
    assert np.abs(rows[keep, :K] - model[keep]).max() <= 2.0 ** -22
    qrows, _ = _operand_rows(rt, q)
    assert np.abs(qrows[:2, :K] - C.composite_rows(qs, h, 0)).max() <= 2.0 ** -22 and (qrows[:2, K:] == 0.0).all()
    keep_s = np.abs(s[:, keep] - C.composite_scores(qs, fr[keep], h)).max()
    assert keep_s <= FUSED_TOL


@pytest.mark.parametrize("H,W,h", ((20, 65, 17), (9, 8, 8)))
@pytest.mark.parametrize("pad", (1, 4))
def test_prepare_reads_frames_in_place_through_ld(rt, H, W, h, pad):
    """Frames cut out of a wider buffer (frame stride H W + pad; + 1 leaves every frame but the first off a 16-byte
    boundary): the operand is the contiguous call's, bit for bit."""
    qs, fr = SW.fused_store(H, W, h, "gaussian", Q=3, N=21)
    coef = rt.S._level_coef(H - h)
    for side, x in ((0, qs), (1, fr)):
        N = len(x)
        buf = rt.t.full((N, H * W + pad), float("nan"), dtype=rt.t.float32, device="cuda")
        buf[:, :H * W] = rt.dev(x).reshape(N, -1)
        view = rt.t.as_strided(buf, (N, H, W), (H * W + pad, W, 1))
        assert not view.is_contiguous() and rt.t.equal(view, rt.dev(x))
        got, want = rt.K.comp_prepare(view, h, side, coef), rt.K.comp_prepare(rt.dev(x), h, side, coef)
        assert (got.N, got.K) == (want.N, want.K)
        assert rt.t.equal(got.X16.view(rt.t.int16), want.X16.view(rt.t.int16))
        assert rt.t.equal(got.inv, want.inv) and bool((got.inv[:N] == 1.0).all())


# ------------------------------------------------------------------------------------------------- corpus
@pytest.mark.parametrize("N", (1, 17, 385))
def test_corpus_small_and_ragged_sizes(rt, N):
    H, W, h = 9, 8, 8
    qs, fr = SW.fused_store(H, W, h, "gaussian", Q=3, N=N)
    model = C.composite_scores(qs, fr, h)
    corpus = rt.S.ComprehensiveFrameCorpus(fr)
    assert corpus.fused and len(corpus) == N
    dense = corpus.scores(qs)
    assert tuple(dense.shape) == (3, N)
    assert np.abs(rt.np(dense) - model).max() <= FUSED_TOL
    for k in sorted({1, min(N, 64), N, N + 3, 100}):
        s, ids = corpus.search(qs, k)
        ws, wi, _, _ = rt.K.select_topk(dense, k)
        assert tuple(s.shape) == tuple(ids.shape) == (3, k)
        assert rt.t.equal(ids, wi) and rt.t.equal(s, ws), k
        got = rt.np(ids)
        assert (np.sort(got[:, :min(k, N)], axis=1) >= 0).all() and (got[:, N:] == -1).all()
        assert bool((s[:, N:] == float("-inf")).all())
        if k >= N:
            assert (np.sort(got[:, :N], axis=1) == np.arange(N)).all()
    # the exact route (a float64 store) at the same sizes
    c64 = rt.S.ComprehensiveFrameCorpus(fr.astype(np.float64))
    assert c64.fused is False
    assert np.abs(rt.np(c64.scores(qs)) - model).max() <= EXACT_TOL
    s, ids = c64.search(qs, N + 3)
    ws, wi, _, _ = rt.K.select_topk(c64.scores(qs), N + 3)
    assert rt.t.equal(ids, wi) and rt.t.equal(s, ws)


def test_corpus_mixed_batch_on_wide_frames(rt):
    H, W, h = 12, 100, 10
    qs, fr = SW.fused_store(H, W, h, "gaussian", Q=3, N=48)
    rng = np.random.default_rng(6)
    off = np.stack([SW.build_frame(rng, H, W, h, kind)[0] for kind in ("zero", "short", "drop_last")]).astype(np.float32)
    assert [tuple(d[:2]) for d in SW.describe_all(off).tolist()] == [(12, 0), (9, 3), (10, 1)]
    batch = np.stack([off[0], qs[0], off[1], qs[1], off[2], qs[2]])
    corpus = rt.S.ComprehensiveFrameCorpus(fr, keep_frames=True)
    assert corpus.fused and corpus.profile == (h, H - h, W)
    dense = corpus.scores(batch)
    model = SW.model_scores(batch, fr)
    print("fused rows err", np.abs(rt.np(dense)[1::2] - model[1::2]).max(), "exact rows err",
          np.abs(rt.np(dense)[0::2] - model[0::2]).max())
    assert np.abs(rt.np(dense)[1::2] - model[1::2]).max() <= FUSED_TOL
    assert np.abs(rt.np(dense)[0::2] - model[0::2]).max() <= EXACT_TOL
    for k in (10, 48, 100):
        s, ids = corpus.search(batch, k)
        ws, wi, _, _ = rt.K.select_topk(dense, k)
        assert rt.t.equal(ids, wi) and rt.t.equal(s, ws), k


@pytest.mark.parametrize("keep_frames", (False, True))
def test_corpus_empty_query_batch(rt, keep_frames):
    qs, fr = SW.fused_store(9, 8, 8, "gaussian", Q=1, N=17)
    corpus = rt.S.ComprehensiveFrameCorpus(fr, keep_frames=keep_frames)
    assert corpus.fused
    none = np.zeros((0, 9, 8), np.float32)
    dense = corpus.scores(none)
    assert tuple(dense.shape) == (0, 17) and dense.dtype == rt.t.float64
    for k in (5, 17, 100):
        s, ids = corpus.search(none, k)
        assert tuple(s.shape) == tuple(ids.shape) == (0, k)
        assert s.dtype == rt.t.float64 and ids.dtype == rt.t.int64
    # a store that is not fused
    c64 = rt.S.ComprehensiveFrameCorpus(fr.astype(np.float64))
    assert tuple(c64.scores(none).shape) == (0, 17) and tuple(c64.search(none, 5)[1].shape) == (0, 5)


def test_corpus_empty_store(rt):
    qs, _ = SW.fused_store(9, 8, 8, "gaussian", Q=2, N=1)
    for dtype in (np.float32, np.float64):
        corpus = rt.S.ComprehensiveFrameCorpus(np.zeros((0, 9, 8), dtype))
        assert len(corpus) == 0 and corpus.fused is False
        assert tuple(corpus.scores(qs).shape) == (2, 0)
        s, ids = corpus.search(qs, 4)
        assert rt.np(ids).tolist() == [[-1] * 4] * 2 and bool((s == float("-inf")).all())
