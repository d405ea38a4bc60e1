"""The oracle's pre-computed similarity scorer against the real reference (tests/golden/precomp_sim.npz, written
by tests/golden/make_golden.py from tests/precomp_sim_cases.py): value and result type of every single-level and
multi-level case, and the properties that make the cases worth running (every branch taken, and a result type
that flips with the summation order).  Runs anywhere: no reference, no GPU."""
import warnings

import numpy as np
import pytest

import precomp_sim_cases as P
from oracle import hq_oracle as O


@pytest.fixture(scope="module")
def g(golden):
    return golden("precomp_sim")


@pytest.fixture(scope="module")
def single():
    """[(name, q, c, oracle result)]"""
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return [(n, q, c, O.precomputed_level_similarity(q, c)) for (n, q, c) in P.single_level_cases()]


def test_inputs_are_the_recorded_ones(g):
    cases = P.single_level_cases()
    assert [n for (n, _, _) in cases] == list(g["single_names"])
    for i, (n, q, c) in enumerate(cases):
        assert q.dtype == np.float32 and c.dtype == np.float32 and q.shape == c.shape
        assert P.digest(q) + P.digest(c) == g["single_digest"][i].tobytes(), f"seeded input {n} changed"
    cases = P.legacy_cases()
    assert [n for (n, _, _) in cases] == list(g["legacy_names"])
    for i, (n, q, c) in enumerate(cases):
        assert P.digest(q) + P.digest(c) == g["legacy_digest"][i].tobytes(), f"seeded input {n} changed"
    for name, (Q, C) in P.multi_level_cases().items():
        got = np.stack([np.frombuffer(P.digest(P.pack(x)[0]), np.uint8) for x in Q + C])
        assert got.tobytes() == g[f"multi_{name}_digest"].tobytes(), name
    assert P.layout_counts(32) == [c for (_, _, c, _) in O.precomputed_index(np.zeros((1, 32, 32), np.float32))[1]]
    assert P.layout_counts(16) == [c for (_, _, c, _) in O.precomputed_index(np.zeros((1, 16, 16), np.float32))[1]]
    assert P.layout_counts(32) == [481, 113, 25, 5, 1] and P.layout_counts(16) == [113, 25, 5, 1]


def test_single_level_value_and_type(g, single):
    bad = [(n, float(v), P.type_code(v), g["single_value"][i], int(g["single_type"][i]))
           for i, (n, _, _, v) in enumerate(single)
           if float(v) != g["single_value"][i] or P.type_code(v) != g["single_type"][i]]
    assert not bad, bad[:5]


def test_multi_level_value_and_type(g):
    with np.errstate(all="ignore"):
        for name, (Q, C) in P.multi_level_cases().items():
            for a, q in enumerate(Q):
                for b, c in enumerate(C):
                    ov, sims = O.precomputed_similarity(q, c)
                    assert float(ov) == g[f"multi_{name}_overall"][a, b], (name, a, b)
                    assert P.type_code(ov) == g[f"multi_{name}_type"][a, b], (name, a, b)
                    assert [float(s) for s in sims] == list(g[f"multi_{name}_levels"][a, b]), (name, a, b)
                    assert [P.type_code(s) for s in sims] == list(g[f"multi_{name}_ltype"][a, b]), (name, a, b)


def test_every_scorer_branch_is_reached(g, single):
    res = {n: v for (n, _, _, v) in single}
    f32_open = [n for n, v in res.items() if isinstance(v, np.float32) and 0.0 < float(v) < 1.0]
    assert len(f32_open) > 50                                                     # float32 in (0, 1)
    clamp1 = [n for n, v in res.items() if n.endswith("_same") and type(v) is float and v == 1.0]
    clamp0 = [n for n, v in res.items() if n.endswith("_neg") and type(v) is float and v == 0.0]
    assert clamp1 and clamp0                                                       # min(1.0, .) / max(0.0, .)
    assert type(res["m7_const_0.5_0.5"]) is float and res["m7_const_0.5_0.5"] == 1.0   # both constant, equal
    assert type(res["m7_const_1.0_1.000002"]) is float and res["m7_const_1.0_1.000002"] == 0.0
    assert res["m7_const_1.0_1.0000005"] == 1.0 and res["m7_const_0.0_1e-06"] == 0.0   # the float32 `< 1e-6`
    assert type(res["m129_const"]) is float and res["m129_const"] == 0.1               # one side constant
    assert type(res["m7_nan_q"]) is float and res["m7_nan_q"] == 1.0                   # NaN: min(1.0, nan) is 1.0
    assert res["m129_nan_both"] == 1.0 and res["m129_inf_c"] == 1.0
    assert isinstance(res["m129_1e30"], np.float32)                                    # overflowing squares
    ty = np.concatenate([g[f"multi_{k}_type"].ravel() for k in ("n32", "n16", "q32_c16")])
    assert (ty == P.TYPE_F32).any() and (ty == P.TYPE_PY).any()                        # an overall of each type
    cross = g["multi_q32_c16_overall"]
    assert len(np.unique(cross[0])) >= 8                                               # spread-out scores to cut


def test_result_type_follows_the_summation_order(single):
    """x against x scores float32 0.99999994 or the clamped Python 1.0, and x against -x float32 ~6e-8 or the
    Python 0.0, depending on how the length splits NumPy's pairwise sums: one wrong association in a kernel's
    sum changes value and type.  If a NumPy change makes every length agree, this sweep has lost that edge."""
    for suffix, limit in (("_same", 1.0), ("_neg", 0.0)):
        kinds = {n: P.type_code(v) for (n, _, _, v) in single if n.endswith(suffix) and n[1:-len(suffix)].isdigit()}
        assert len(kinds) == len(P.LENGTHS)
        f32 = [n for n, k in kinds.items() if k == P.TYPE_F32]
        py = [n for n, k in kinds.items() if k == P.TYPE_PY]
        assert f32 and py, (f"every {suffix[1:]} pair now has one result type (float32: {len(f32)}, Python float: "
                            f"{len(py)}): the cases no longer tell summation orders apart; pick other lengths or seeds")
        for (n, _, _, v) in single:
            if n in f32:
                assert abs(float(v) - limit) < 1e-6 and float(v) != limit, n


def test_legacy_cases_cover_the_branches(g):
    names, vals = list(g["legacy_names"]), g["legacy_value"]
    by = dict(zip(names, vals))
    assert by["m7_const_equal"] == 1.0 and by["m7_const_close"] == 1.0 and by["m7_const_far"] == 0.0
    assert by["m7_one_const"] == 0.1 and by["m7_nan"] == 0.0
    assert by["m1_neg"] == 0.0 and by["m1_same"] == 1.0            # one value: both "constant", np.allclose decides
    assert by["m2_neg"] == 0.0 and by["m2_same"] == 1.0
    assert 0.0 < by["m129_near_const_pair"] < 1.0 and 0.5 < by["m129_near_const_noisy"] < 1.0
