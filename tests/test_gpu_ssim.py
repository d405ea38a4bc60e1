"""Gaussian-window SSIM and template correlation on the GPU (hq_ssim.hip, core/cv_features.py, rag.FrameSSIMCorpus)
against the float64 model of tests/ssim_cases.py.

* out_ssim within 1e-5 of the model, the project's bound for similarity scores, on every shape and family;
  out_ncc within 1e-12 of the float64 Pearson from integer sums, 0.0 for constant frames.
* Listed entries equal the dense matrix's bits, pads are -inf.
* calculate_ssim and FrameSSIMCorpus.search return the model's order.
Q = 3 queries against N = 5 frames: the query tile is partial and the corpus count is no multiple of anything.
The largest observed errors are in profiles/ssim_error_bounds.txt (tools/ab_ssim.py writes it)."""
import numpy as np
import pytest

import ssim_cases as S

pytestmark = pytest.mark.gpu

SSIM_TOL = 1e-5
NCC_TOL = 1e-12
# (4, 4): every pixel is border; (7, 9): odd, less than one wave of pixels; (33, 32), (65, 64): ingest shapes
SHAPES = [(4, 4), (7, 9), (33, 32), (65, 64)]
CASES = [(h, w, f) for (h, w) in SHAPES for f in S.FAMILIES] + [(131, 128, "random")]  # the limit: four strips


@pytest.fixture(scope="module")
def rt(hq_lib):
    from hq_mi355x import kernels as K
    from hq_mi355x._dev import to_dev, to_np

    class RT:
        pass

    r = RT()
    r.K, r.dev, r.np = K, to_dev, to_np
    return r


@pytest.mark.parametrize("H,W,family", CASES)
def test_dense_and_listed_match_model(rt, H, W, family):
    q, c = S.make(family, H, W)
    Q, N = len(q), len(c)
    want = np.array([[S.ssim_model(a, b) for b in c] for a in q])
    want_ncc = np.array([[S.ncc_model(a, b) for b in c] for a in q])
    prep = rt.K.ssim_prepare(rt.dev(q))
    got, got_ncc = (rt.np(t) for t in rt.K.ssim_scores(prep, rt.dev(c), ncc=True))
    print(f"{H}x{W} {family}: ssim err {np.abs(got - want).max():.3e} ncc err {np.abs(got_ncc - want_ncc).max():.3e}")
    assert np.abs(got - want).max() <= SSIM_TOL
    assert np.abs(got_ncc - want_ncc).max() <= NCC_TOL
    if family == "const_const":
        assert np.abs(got - 0.9).max() <= 1e-15  # C1 C2 / (C1 C2 + 1e-8) = 9e-8 / 1e-7
    if family.startswith("const"):
        assert np.all(got_ncc == 0.0)
    assert rt.np(rt.K.ssim_scores(prep, rt.dev(c))).tobytes() == got.tobytes()  # without the second output
    # listed: a repeated id, a -1 pad and an N pad; entries carry the dense bits
    ids = np.array([[4, 4, -1, N], [0, N, 2, 2], [-1, 3, 1, 3]], np.int64)
    ls, ln = (rt.np(t) for t in rt.K.ssim_scores_listed(prep, rt.dev(c), rt.dev(ids), ncc=True))
    pad = (ids < 0) | (ids >= N)
    safe = np.where(pad, 0, ids)
    assert np.where(pad, -np.inf, np.take_along_axis(got, safe, 1)).tobytes() == ls.tobytes()
    assert np.where(pad, -np.inf, np.take_along_axis(got_ncc, safe, 1)).tobytes() == ln.tobytes()


def test_prepared_stats_and_maps(rt):
    q, _ = S.make("ranges", 33, 32)
    prep = rt.K.ssim_prepare(rt.dev(q))
    x = q.astype(np.int64)
    want = np.stack([x.min((1, 2)), x.max((1, 2)), x.sum((1, 2)), (x * x).sum((1, 2))], 1)
    assert rt.np(prep.stats).tolist() == want.tolist()
    xn = (x[0] - x[0].min()) / (x[0].max() - x[0].min() + 1e-8)
    mu = S._F(xn)
    maps = rt.np(prep.maps)[0]
    assert np.abs(maps[0] - mu).max() <= 1e-12 and np.abs(maps[1] - (S._F(xn * xn) - mu * mu)).max() <= 1e-12


def test_public_interface_orders_as_model(rt):
    from hq_mi355x.core import calculate_ssim, template_correlation
    from hq_mi355x.rag import FrameSSIMCorpus
    q, c = S.make("random", 33, 32, Q=2, N=6, seed=3)
    c[2] = q[0]                               # the best match of query 0
    c[5] = np.clip(q[0].astype(int) + 9, 0, 255)  # a close second
    c[1] = 255 - q[1]                         # the worst match of query 1
    want = np.array([[S.ssim_model(a, b) for b in c] for a in q])
    corpus = FrameSSIMCorpus(c)
    s, ids = (rt.np(t) for t in corpus.search(q, k=6))
    assert ids.tolist() == np.argsort(-want, axis=1, kind="stable").tolist()
    assert np.abs(s - np.take_along_axis(want, ids, 1)).max() <= SSIM_TOL
    assert rt.np(corpus.rescore(q, ids[:, :3])).tobytes() == s[:, :3].tobytes()
    single = [calculate_ssim(q[0], b) for b in c]
    assert np.argsort(-np.array(single), kind="stable").tolist() == ids[0].tolist()
    assert abs(template_correlation(q[0], c[5]) - S.ncc_model(q[0], c[5])) <= NCC_TOL
    with pytest.raises(ValueError, match="win_size"):
        calculate_ssim(q[0], c[0], win_size=11)
    with pytest.raises(TypeError):
        calculate_ssim(q[0].astype(np.float64), c[0])
