"""Video features and their scorer on the GPU (hq_vfeat.hip, core.VideoFeatureIndex) against the float64 NumPy model of
tests/vfeat_cases.py.

* Features: histogram, min, max and the 8 magnitude counts equal the model; every other slot is within
  4 H W 2.2e-16 max(1, |want|), the worst-case summation bound the model and the kernel share.
* Scores: within 1e-10 of the model (twice the feature bound plus K eps, rounded up) and within 1e-5, the project's
  bound for similarity scores, of the model with the reference's float32 histogram; zeros against zeros is w_h + w_t.
* Listed entries carry the dense bits, pads are -inf, `combined` is the hybrid rule on those bits.
N = 5 frames (a partial workgroup of four) and Q = 3 queries (a partial query tile)."""
import functools

import numpy as np
import pytest

import vfeat_cases as V

pytestmark = pytest.mark.gpu

SHAPES = [(4, 4), (7, 9), (33, 32), (65, 64)]
CASES = [(h, w, f) for (h, w) in SHAPES for f in V.FAMILIES] + [(131, 128, "random")]  # the range limit
Q, N = 3, 5


@pytest.fixture(scope="module")
def rt(hq_lib):
    from hq_mi355x import kernels as K
    from hq_mi355x._dev import to_dev, to_np

    class RT:
        pass

    r = RT()
    r.K, r.dev, r.np = K, to_dev, to_np
    return r


@functools.lru_cache(maxsize=None)
def case(H, W, family):
    fr = V.make(family, H, W)
    q, c = fr[:Q], fr[Q:]
    fq, fc = (np.stack([V.features(g) for g in x]) for x in (q, c))
    return q, c, fq, fc


@pytest.mark.parametrize("H,W,family", CASES)
def test_features(rt, H, W, family):
    _, c, _, want = case(H, W, family)
    rows = rt.np(rt.K.vfeat_extract(rt.dev(c)).rows)
    got = rows[:, :55]
    err = np.abs(got - want) / np.maximum(1, np.abs(want))
    print(f"{H}x{W} {family}: largest feature error {err.max():.3e}")
    assert got[:, V.EXACT].tolist() == want[:, V.EXACT].tolist()
    assert err.max() <= 4 * H * W * 2.2e-16
    norms = np.stack([np.linalg.norm(want[:, p], axis=1) for p in V.PARTS], 1)
    assert np.abs(rows[:, 56:59] - norms).max() <= 4 * H * W * 2.2e-16 * max(1, norms.max())
    assert not rows[:, 55].any() and not rows[:, 59:].any()


@pytest.mark.parametrize("H,W,family", CASES)
def test_scores_dense_and_listed(rt, H, W, family):
    q, c, fq, fc = case(H, W, family)
    pq, pc = rt.K.vfeat_extract(rt.dev(q)), rt.K.vfeat_extract(rt.dev(c))
    got = rt.np(rt.K.vfeat_scores(pq, pc))
    want = np.array([[V.score(a, b) for b in fc] for a in fq])
    want32 = np.array([[V.score(a, b, hist32=True) for b in fc] for a in fq])
    print(f"{H}x{W} {family}: score error {np.abs(got - want).max():.3e}, to float32 typing {np.abs(got - want32).max():.3e}")
    assert np.abs(got - want).max() <= 1e-10
    assert np.abs(got - want32).max() <= 1e-5
    if family == "zeros":
        assert (got == 0.3 + 0.2).all()
    # listed: a repeated id, a -1 pad and an N pad; weights that put the video score on either side of 0.5
    ids = np.array([[4, 4, -1, N], [0, N, 2, 2], [-1, 3, 1, 3]], np.int64)
    pad = (ids < 0) | (ids >= N)
    hier = np.random.default_rng(H).random(ids.shape)
    sides = []
    for w in (None, (0.9, 0.6, 0.3), (0.1, 0.1, 0.1)):
        dense = rt.np(rt.K.vfeat_scores(pq, pc, weights=w))
        bits = np.where(pad, -np.inf, np.take_along_axis(dense, np.where(pad, 0, ids), 1))
        video, comb = (rt.np(t) for t in rt.K.vfeat_scores_listed(pq, pc, rt.dev(ids), rt.dev(hier), weights=w))
        assert video.tobytes() == bits.tobytes()
        assert rt.np(rt.K.vfeat_scores_listed(pq, pc, rt.dev(ids), weights=w)).tobytes() == bits.tobytes()
        assert comb.tobytes() == np.where(pad, -np.inf, V.combine(hier, bits)).tobytes()
        sides.append(bits[~pad] > 0.5)
    assert sides[1].any() and not sides[2].any()


def test_public_interface(rt):
    from hq_mi355x.core import VideoFeatureIndex, extract_video_features
    fr = V.make("random", 33, 32, n=9, seed=3)
    q, c = fr[:2], fr[2:].copy()
    c[3] = q[0]          # an exact duplicate of query 0
    c[5] = 255 - q[0]    # and its inverse
    c[1] = q[0] // 4     # a dark frame: another histogram
    fq, fc = (np.stack([V.features(g) for g in x]) for x in (q, c))
    want = np.array([[V.score(a, b) for b in fc] for a in fq])
    ftol = 4 * 33 * 32 * 2.2e-16
    index = VideoFeatureIndex(c, similarity_threshold=0.5)
    assert (np.abs(rt.np(index.features()) - fc) / np.maximum(1, np.abs(fc))).max() <= ftol
    ids, s = (rt.np(t) for t in index.search(q, 7))
    for a in range(2):
        order = [j for j in np.argsort(-want[a], kind="stable") if want[a, j] > 0.5]
        assert 0 < len(order) < 7 and ids[a, :len(order)].tolist() == order and (ids[a, len(order):] == -1).all()
        assert np.abs(s[a, :len(order)] - want[a, order]).max() <= 1e-10
    assert ids[0, 0] == 3
    # hybrid: the candidate lists of a hierarchical stage, one pad each
    cand = np.array([[5, 3, 0, -1, 6], [1, 2, -1, 4, 0]], np.int64)
    hier = np.array([[0.9, 0.2, 0.5, 0.0, 0.7], [0.3, 0.8, 0.0, 0.6, 0.1]])
    video = np.take_along_axis(rt.np(index.scores(q)), np.where(cand < 0, 0, cand), 1)
    comb = np.where(cand < 0, -np.inf, V.combine(hier, video))
    hi, hc, hv, hh = (rt.np(t) for t in index.hybrid(q, cand, hier, 4))
    order = np.argsort(-comb, axis=1, kind="stable")[:, :4]
    assert hi.tolist() == np.take_along_axis(cand, order, 1).tolist()
    assert hc.tobytes() == np.take_along_axis(comb, order, 1).tobytes()
    assert hv.tobytes() == np.take_along_axis(video, order, 1).tobytes()
    assert hh.tobytes() == np.take_along_axis(hier, order, 1).tobytes()
    one = extract_video_features(q[1])
    assert sorted(one) == ["histogram", "stats", "texture"]
    got1 = np.concatenate([one["histogram"], one["texture"], one["stats"]])
    assert (np.abs(got1 - fq[1]) / np.maximum(1, np.abs(fq[1]))).max() <= ftol
    with pytest.raises(TypeError):
        extract_video_features(q[1].astype(np.float64))
    with pytest.raises(ValueError):
        index.hybrid(q, cand, hier[:, :3], 4)
    with pytest.raises(ValueError, match="16768 pixels"):
        VideoFeatureIndex(np.zeros((1, 132, 128), np.uint8))
