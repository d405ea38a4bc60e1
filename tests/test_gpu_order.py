"""Frame ordering on the device (csrc/hq_order.hip through hq_mi355x.core.frame_order) against the long-double model
of tests/order_cases.py and the reference's own outputs (tests/golden/frame_ordering.npz).

Similarities and scores: 1e-12.  A float64 dot of two unit rows errs by at most L 2^-53 (3e-14 at L = 256) and the
centring keeps |mean| <= 10 std, so the bound leaves about 30x margin; entries with a constant row are exact.
Orders and positions must be equal: every store keeps the model's smallest step gap >= 1e-9 (asserted)."""
import numpy as np
import pytest

import order_cases as OC
from hq_mi355x._dev import to_np as _np
from order_cases import CASES

pytestmark = pytest.mark.gpu
TOL = 1e-12
# a constant pair that np.allclose accepts one way only: |a - b| <= 1e-8 + 1e-5 |b| but > 1e-8 + 1e-5 |a|
ASYM_A, ASYM_B = 1024.0, 1024.0 + 10995170 * 2.0 ** -30


@pytest.fixture(scope="module")
def FO(hq_lib):
    from hq_mi355x.core.frame_order import FrameOrdering
    return FrameOrdering


@pytest.mark.parametrize("L", (2, 5, 32, 64, 100, 256))
@pytest.mark.parametrize("M,N", ((1, 1), (1, 17), (16, 16), (17, 33), (65, 130)))
def test_similarities(FO, M, N, L):
    rng = np.random.default_rng(1000 * M + N + L)
    q, c = OC.gaussian(rng, M, L), OC.gaussian(rng, N, L)
    if N >= 16:
        c[[1, 4, 7, 9, 15]] = np.array([0.0, 0.5, 2.0, ASYM_A, ASYM_B])[:, None]
    if M >= 16:
        q[[0, 5, 6]] = np.array([0.5, ASYM_A, ASYM_B])[:, None]
    assert np.allclose(np.full(L, ASYM_A), np.full(L, ASYM_B)) and not np.allclose(np.full(L, ASYM_B), np.full(L, ASYM_A))
    got, want = _np(FO(c).similarities(q)), OC.sims(q, c)
    assert got.shape == (M, N)
    print(f"M={M} N={N} L={L}: max |got - model| = {float(np.abs(got - want).max()):.2e}")
    assert float(np.abs(got - want).max()) <= TOL
    exact = (q.std(1) == 0)[:, None] | (c.std(1) == 0)[None, :]
    assert np.array_equal(got[exact], want[exact].astype(np.float64))
    if M >= 16 and N >= 16:
        assert got[5, 15] == 1.0 and got[6, 9] == 0.0  # allclose(a, b) holds, allclose(b, a) does not


@pytest.mark.parametrize("L", (3, 7, 100, 129, 249, 250, 253, 255, 256))
def test_constant_rows_decided_as_numpy(FO, L):
    """Constant rows of non-dyadic values: np.std is 0 or a few ulps depending on how the sum rounds, so the flag
    must follow NumPy's pairwise order (every split level: L = 249 .. 255 split the second half again)."""
    rng = np.random.default_rng(L)
    rows = np.repeat(np.concatenate([[0.1], rng.uniform(0.01, 10, 255)])[:, None], L, axis=1)
    want = rows.std(1) == 0
    assert want.any() and not want.all()
    assert np.array_equal((_np(FO(rows).rows.flags[:len(rows)]) & 1).astype(bool), want)


STORES = {f"n{N}": (lambda rng, N=N, L=(32, 64)[k % 2]: OC.gaussian(rng, N, L))
          for k, N in enumerate((1, 2, 16, 17, 64, 1024, 1025, 2049))}
STORES.update(dups64=lambda rng: OC.with_duplicates(rng, 64, 32), anti17=lambda rng: OC.anticorrelated(rng, 17, 32),
              const33=lambda rng: OC.with_constants(rng, 33, 5))


@pytest.mark.parametrize("name", tuple(STORES) + CASES)
def test_greedy_order(FO, golden, name):
    if name in STORES:
        rows = STORES[name](np.random.default_rng(sum(map(ord, name))))
    else:
        rows = golden("frame_ordering")[f"{name}_rows"]
    order, got_steps = (_np(x) for x in FO(rows).greedy_order())
    assert sorted(order.tolist()) == list(range(len(rows)))
    # two rows are equidistant from their midpoint (the reference's start there is rounding noise of np.mean):
    # either start is right; every other store keeps the two nearest rows a relative 1e-9 apart
    tied_start = len(rows) == 2
    assert tied_start or OC.start_gap(rows) >= 1e-9
    want, steps, gap = OC.greedy(rows, int(order[0]) if tied_start else None)
    print(f"{name}: smallest model gap {gap:.2e}, start gap {OC.start_gap(rows):.2e}")
    assert gap >= 1e-9
    assert order.tolist() == want.tolist()
    if name in CASES:
        assert order.tolist() == golden("frame_ordering")[f"{name}_order"].tolist()
    assert got_steps.shape == steps.shape and (len(steps) == 0 or float(np.abs(got_steps - steps).max()) <= TOL)
    if name == "dups64":  # bit-identical rows leave the chain lowest index first
        where = {int(r): p for p, r in enumerate(order)}
        for i in range(len(rows)):
            for j in range(i + 1, len(rows)):
                assert not np.array_equal(rows[i], rows[j]) or where[i] < where[j]


@pytest.mark.parametrize("Q", (1, 17))
@pytest.mark.parametrize("N", (1, 2, 33))
def test_metrics_and_insertion(FO, Q, N):
    rng = np.random.default_rng(10 * N + Q)
    rows = OC.gaussian(rng, N, 32)
    if N == 33:
        rows[11] = rows[12] = rows[10]  # a query equal to them ties positions 11 and 12: the first wins
    fo = FO(rows)
    for order in (None, rng.permutation(N)):
        m = fo.metrics(order)
        assert np.abs(np.array([m[k] for k in OC.KEYS]) - OC.metrics(rows, order)).max() <= TOL
    # head (a copy of the first row), tail, interior (near a middle row), tie (the repeated row), then gaussian rows
    kinds = np.stack([rows[0], rows[-1], rows[N // 2] + 0.05 * rng.standard_normal(32), rows[min(10, N - 1)]])
    batches = [kinds[i:i + 1] for i in range(4)] if Q == 1 else [np.concatenate([kinds, OC.gaussian(rng, Q - 4, 32)])]
    for q in batches:
        pos, score = (_np(x) for x in fo.insertion_positions(q))
        for a, s in enumerate(OC.sims(q, rows)):
            sc = np.unique(np.concatenate([s[:1], (s[:-1] + s[1:]) / 2, s[-1:]]))
            assert len(sc) == 1 or sc[-1] - sc[-2] >= 1e-9
            wp, ws = OC.insertion(s)
            assert int(pos[a]) == wp and abs(float(score[a]) - ws) <= TOL
    if N == 33 and Q == 17:
        assert pos[:4].tolist() == [0, 33, pos[2], 11] and 0 < pos[2] < 33


def test_dropins_and_store(hq_lib):
    from hq_mi355x.core import (find_optimal_insertion_position, frame_ordering_metrics,
                                sort_frames_by_hierarchical_indices)
    from hq_mi355x.core.frame_store import FrameStoreCorpus, VideoFrameMetadata
    rng = np.random.default_rng(7)
    videos = {}
    for v, runs in (("a.mp4", 6), ("b.mp4", 4)):  # shuffled runs of five near-duplicates
        x = np.repeat(OC.gaussian(rng, runs, 64), 5, axis=0) + 0.01 * rng.standard_normal((5 * runs, 64))
        videos[v] = [VideoFrameMetadata(i, f"{v}{i}", 0, 1.0, r, None, 0.0) for i, r in enumerate(rng.permutation(x))]
    store = FrameStoreCorpus([(v, f) for v, fl in videos.items() for f in fl])
    res = store.optimize_frame_ordering()
    for v, fl in videos.items():
        rows = np.stack([f.hierarchical_indices for f in fl])
        want, _, gap = OC.greedy(rows)
        assert gap >= 1e-9 and res[v]["order"].tolist() == want.tolist()
        assert res[v]["optimized_metrics"]["temporal_coherence"] >= res[v]["original_metrics"]["temporal_coherence"]
        assert abs(res[v]["temporal_coherence_improvement"] - (OC.metrics(rows, want)[2] - OC.metrics(rows)[2])) <= 2 * TOL
        assert abs(frame_ordering_metrics(fl)["ordering_efficiency"] - OC.metrics(rows)[3]) <= TOL
        q = rows[3] + 0.001
        assert store.insertion_position(q, v) == find_optimal_insertion_position(q, fl) == OC.insertion(OC.sims(q, rows)[0])[0]
        out = sort_frames_by_hierarchical_indices(fl)
        assert [f.model_id for f in out] == [f"{v}{i}" for i in want] and [f.frame_index for f in out] == list(range(len(fl)))
