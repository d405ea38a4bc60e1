"""The vectorised model and the built frames of tests/comp_sweep_cases.py: the model against comp_cases.exact_parts
pair by pair on every set of the first golden and against the second golden (tests/golden/comprehensive_shapes.npz,
the reference's recorded scores), every built frame against the descriptor it was built for, and the rules the new
cases must be able to tell apart.  No GPU."""
import numpy as np
import pytest

import comp_cases as C
import comp_sweep_cases as SW


def _first_golden_sets():
    g = C.golden()
    for tag in C.FAMILIES:
        edges = [g[f"e_{e}_{tag}_enh"] for e in C.EDGES]
        yield tag, np.concatenate([g[f"{tag}_enh"], np.stack(edges)])
    for name in C.STANDALONE:
        yield name, g[f"s_{name}_enh"]


@pytest.mark.parametrize("name,frames", list(_first_golden_sets()), ids=lambda v: v if isinstance(v, str) else "")
def test_vectorised_model_equals_pair_model(name, frames):
    """Families with their edge frames (other heights, other L, dropped rows) and the stand-alone sets: both models
    are float64 models of the same rules, so they agree to rounding whatever the frames' dtype."""
    parts, score = SW.model_parts(frames, frames)
    want = np.array([[C.exact_parts(a, b) for b in frames] for a in frames])
    assert np.abs(parts - want).max() <= 1e-12
    assert np.abs(score - (0.5 * want[..., 0] + 0.3 * want[..., 1] + 0.2 * want[..., 2])).max() <= 1e-12
    assert SW.describe_all(frames).tolist() == [list(C.describe(e)) for e in frames]


def test_vectorised_model_raises_for_two_widths():
    with pytest.raises(ValueError, match="same shape"):
        SW.model_parts(C.golden()["e_width_enh"][:1], C.golden()["e_width_enh"][1:])


@pytest.mark.parametrize("name", SW.GOLDEN_SETS)
def test_vectorised_model_equals_second_golden(name):
    g = SW.golden()
    e = g[f"g_{name}_enh"]
    tol = C.tolerance(e.dtype)
    assert SW.describe_all(e)[:, :3].tolist() == g[f"g_{name}_desc"].tolist()
    parts, score = SW.model_parts(e, e)
    for got, want in ((score, g[f"g_{name}_score"]), (parts, g[f"g_{name}_parts"])):
        assert (np.isnan(got) == np.isnan(want)).all()
        assert np.nanmax(np.abs(got - want)) <= tol


def test_second_golden_covers_its_classes():
    g = SW.golden()
    assert g["g_wide_enh"].shape[1:] == (12, 100) and g["g_wide_desc"][:, 2].tolist() == [100] * 5
    assert g["g_oddf_enh"].shape[1:] == (20, 65) and g["g_oddf_enh"].dtype == np.float32
    assert g["g_small_desc"][:, :2].tolist() == [[4, 2]] * 3 + [[4, 1], [4, 2]] and C.windows(4, 4)[0] == 0
    assert g["g_rows31_desc"][:, 1].tolist() == [31, 31, 31, 30, 31]
    # what the reference does with a NaN or an inf: it raises for no pair and every pair with such a frame scores NaN
    for t in ("nonfinite", "nonfinitef"):
        assert not g[f"g_{t}_raised"].any()
        bad = ~np.isfinite(g[f"g_{t}_enh"]).all(axis=(1, 2))
        assert bad.tolist() == [False, True, True, True, False]
        assert (np.isnan(g[f"g_{t}_score"]) == (bad[:, None] | bad[None, :])).all()
    assert all(not g[f"g_{t}_raised"].any() for t in SW.GOLDEN_SETS)


@pytest.mark.parametrize("H,W,h", SW.SHAPES)
@pytest.mark.parametrize("dtype", ("float64", "float32"))
def test_built_frames_have_their_descriptors(H, W, h, dtype):
    x, want = SW.hetero_set(H, W, h, dtype)
    assert len(x) >= 40 and x.dtype == np.dtype(dtype)
    assert SW.describe_all(x).tolist() == want.tolist()
    assert [list(C.describe(e)) for e in x] == want.tolist()
    L = H - h
    kinds = {k: want[i] for i, k in enumerate(SW.KINDS)}
    assert kinds["full"].tolist() == [h, L, W if L else 0, (1 << L) - 1]
    assert (x[0, h:] != 0).sum(axis=1).tolist() == [SW.index_width(W)] * L and 2 * SW.index_width(W) <= max(W, 2)
    assert kinds["zero"].tolist() == [H, 0, 0, 0]
    assert kinds["short"][0] != h and kinds["short"][1] != L
    if L >= 3:
        assert [int(kinds[k][3]) for k in ("drop_first", "drop_middle", "drop_last")] == \
            [(1 << L) - 2, (1 << L) - 1 - (1 << L // 2), (1 << (L - 1)) - 1]
    assert kinds["negzero_row"].tolist() == kinds["drop_middle"].tolist()
    assert np.signbit(x[SW.KINDS.index("negzero_row"), h + L // 2]).all()
    # one index width in the set: no pair raises
    assert set(want[want[:, 1] > 0, 2].tolist()) == {W}
    ws = {(6, 4, 4): 0, (9, 8, 8): 2, (13, 12, 12): 3, (15, 16, 14): 3, (18, 16, 17): 4, (40, 8, 9): 2}
    if (H, W, h) in ws:
        assert C.windows(h, W)[0] == ws[(H, W, h)]
    if (H, W, h) == (35, 128, 32):
        assert C.windows(h, W)[2] * C.windows(h, W)[3] == 945
    if (H, W, h) == (40, 8, 9):
        assert int(kinds["full"][3]) >> 30 == 1 and L == 31


def test_hetero_model_equals_pair_model_on_a_sample():
    """The vectorised model on the new sets against the pair model, a seeded sample of pairs of every shape."""
    rng = np.random.default_rng(5)
    for H, W, h in SW.SHAPES:
        x, _ = SW.hetero_set(H, W, h)
        parts, _ = SW.hetero_model(H, W, h)
        for a, b in rng.integers(0, len(x), (25, 2)):
            assert np.abs(parts[a, b] - np.array(C.exact_parts(x[a], x[b]))).max() <= 1e-12, (H, W, h, a, b)


def _moved(shape, **kw):
    x, _ = SW.hetero_set(*shape)
    return float(np.abs(SW.model_scores(x, x, **kw) - SW.hetero_model(*shape)[1]).max())


def test_new_cases_discriminate():
    """Each rule switched off in the model moves at least one new case by more than 1e-4: a kernel that lost the rule
    cannot pass the GPU sweep, which holds hq_comp_scores to 1e-12 of the model on these sets."""
    # columns >= 64 ignored in index rows, block and windows
    for shape in ((12, 100, 10), (20, 65, 17), (35, 128, 32)):
        assert _moved(shape, columns=64) > 1e-4
        x, _ = SW.hetero_set(*shape)
        p0, p1 = SW.hetero_model(*shape)[0], SW.model_parts(x, x, columns=64)[0]
        moved = np.abs(p1 - p0).max(axis=(0, 1))  # per part: index rows, block, windows
        assert moved[0] > 1e-4 and moved[1] > 1e-4
        assert moved[2] > 1e-4 or shape == (20, 65, 17)   # no 4 x 4 window at stride 2 reaches column 64 of 65
    # ws = 3 walks with stride 1
    for shape in ((13, 12, 12), (15, 16, 14)):
        assert _moved(shape, ws3_stride=2) > 1e-4
    # weights of max(L_q, L_c) levels, dropped rows move up
    # (at 31 levels the weights of 30 and of 31 levels differ by 8^-30: only short level lists tell them apart)
    for shape in ((12, 100, 10), (20, 65, 17), (9, 8, 8)):
        assert _moved(shape, weights_of="query") > 1e-4
    for shape in ((40, 8, 9), (12, 100, 10), (20, 65, 17)):
        assert _moved(shape, compact=False) > 1e-4
    # zero-norm windows score 0.0
    for shape in ((9, 8, 8), (18, 16, 17), (35, 128, 32), (40, 8, 9)):
        assert _moved(shape, zero_window=0.5) > 1e-4
    # spatial is 0.0 for different heights
    for shape in SW.SHAPES:
        assert _moved(shape, spatial_any_height=True) > 1e-4


def test_fused_stores_are_on_profile():
    for H, W, h in SW.FUSED_PROFILES:
        for kind in SW.FUSED_FAMILIES:
            qs, fr = SW.fused_store(H, W, h, kind)
            assert qs.shape == (4, H, W) and fr.shape == (48, H, W) and qs.dtype == np.float32
            assert all(C.on_profile(e, h) for e in list(qs) + list(fr))
    qs, fr = SW.fused_store(9, 8, 8, "negated")
    assert np.diag(C.composite_scores(qs, fr[:4], 8)).max() < 0.01
    e = SW.enhance128(np.random.default_rng(0).standard_normal((128, 128)).astype(np.float32))
    assert e.shape == (131, 128) and C.describe(e) == (128, 3, 64, 7) and C.composite_k(131, 128, 128) == 84243


def test_composite_model_equals_vectorised_model_on_fused_stores():
    for H, W, h in SW.FUSED_PROFILES:
        qs, fr = SW.fused_store(H, W, h, "gaussian")
        assert np.abs(C.composite_scores(qs, fr, h) - SW.model_scores(qs, fr)).max() <= 1e-12


def test_lds_rule_edges():
    for itemsize in (4, 8):
        (H0, W0), (H1, W1) = SW.lds_edge(itemsize)
        assert SW.lds_bytes(H0, W0, itemsize) <= SW.LDS_BYTES < SW.lds_bytes(H1, W1, itemsize)
        assert 0 <= H0 - W0 <= 1 and (H1, W1) in ((H0 + 1, W0), (H0, W0 + 1))
    # the 128-wide generator frame: neither the exact route's rule nor 16 section-coefficient lists fit
    assert SW.lds_bytes(131, 128, 4) > SW.LDS_BYTES
