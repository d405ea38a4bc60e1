"""The scan contract's CPU half: the level-0 split model against the oracle, the share of inputs the
completeness test has to exclude, and resolved_rule on lists worked out by hand.  No GPU."""
import numpy as np
import pytest

import scan_contract as SC


@pytest.mark.parametrize("L", [64, 32])
def test_split_model_within_documented_bound(L):
    """z = hi + lo in f16, three f32 contractions, f32 epilogue: the arithmetic as designed stays within the
    documented 5.5e-6 of the oracle on every pair of unflagged family rows (seen: 4.2e-7 at m = 32, 1.7e-7 at
    m = 16: 13x headroom).  With f16 subnormals flushed the same model leaves the bound (1.3e-5 / 1.7e-5;
    printed, not asserted: it is the figure a GPU bound failure is compared with - the MI355X measures
    4.5e-7 / 2.4e-7, so its matrix and dot2 instructions keep f16 subnormals)."""
    c = SC.case(L, SC.N_SMALL)
    exact = c.exact(0)
    ok = (~c.flagged_queries())[:, None] & (~c.flagged_rows())[None, :]
    err = np.abs(SC.split_model_level0(c.Q, c.C, c.m) - exact)[ok]
    ftz = np.abs(SC.split_model_level0(c.Q, c.C, c.m, ftz=True) - exact)[ok]
    print(f"\nlevel-0 split model, m = {c.m}: max |model - oracle| = {err.max():.3e} over {ok.sum()} pairs "
          f"(f16 subnormals flushed: {ftz.max():.3e})")
    assert err.max() <= SC.B_SCAN0


@pytest.mark.parametrize("L", [64, 32])
@pytest.mark.parametrize("n", [SC.N_SMALL, SC.N_LARGE])
def test_indeterminate_band_is_small(L, n):
    """The completeness test says nothing about a row whose exact score lies within EPS of the threshold.
    That exclusion must stay rare, or the test could hide failures behind it: at most 0.1% of the (query, row,
    threshold) triples of its sweep, for the level-0 and for the overall score.  The share leaves out the
    flagged queries: the split scans do not answer them at all (the GPU test checks that instead)."""
    c = SC.case(L, n)
    for mode in (0, 1):
        exact = c.exact(mode)[~c.flagged_queries(mode)]
        inside = sum(int((np.abs(exact - t) <= SC.EPS).sum()) for t in SC.THRESHOLDS)
        share = inside / (exact.size * len(SC.THRESHOLDS))
        print(f"\nL = {L}, N = {c.N}, mode {mode}: indeterminate share = {share:.3e}")
        assert share <= 1e-3


def test_case_layout():
    """What the GPU tests rely on: every family among queries and rows, flagged families where expected, the
    corpus sizes on both sides of the longest list."""
    small, large = SC.case(64, SC.N_SMALL), SC.case(64, SC.N_LARGE)
    assert small.N < max(SC.LIST_LENGTHS) < large.N
    assert sorted(set(small.q_fam)) == list(range(len(SC.FAMILIES)))
    m = small.m
    lv0 = small.C[:, :m]
    const = lv0.std(axis=1) == 0
    msq = (lv0 * lv0).mean(axis=1)
    unsafe = ~((msq >= 2.0 ** -60) & (msq <= 2.0 ** 60))
    assert np.array_equal(const | unsafe, small.flagged_rows())
    assert np.array_equal(small.Q[0], small.C[-1])  # the duplicates of query 0 close the corpus
    inside = small.q_rows >= 0
    assert np.array_equal(small.Q[inside], small.C[small.q_rows[inside]])
    assert np.array_equal(small.q_fam[inside], small.row_fam[small.q_rows[inside]])
    big = SC.case(64, 4, extra_gauss=100, derived=False)
    inside = big.q_rows >= 0
    assert np.array_equal(big.Q[inside], big.C[big.q_rows[inside]])


def test_resolved_rule_by_hand():
    # six rows; exact scores by row id
    exact = np.array([0.90, 0.80, 0.70, 0.60, 0.50, 0.40])
    eps = 0.01
    ok = SC.passes(exact, 0.0, 0)

    # complete: list of 4 (ids 0, 1, 2, 3), k = 2.  last approx 0.60 + 0.01 = 0.61 < 2nd exact 0.80 -> resolved
    r = SC.resolved_rule([0.90, 0.80, 0.70, 0.60], [0, 1, 2, 3], exact, ok, 2, 0.0, 0, eps)
    assert r[0] is True and r[1] == 2 and list(r[2]) == [0, 1] and list(r[3]) == [0.90, 0.80]

    # incomplete: k = 4 of the same list.  0.61 < 4th exact 0.60 is false: an unlisted row could score 0.605
    r = SC.resolved_rule([0.90, 0.80, 0.70, 0.60], [0, 1, 2, 3], exact, ok, 4, 0.0, 0, eps)
    assert r[0] is False and r[1] == 4 and list(r[2]) == [0, 1, 2, 3]

    # the approximate order is not the exact one: ranking is by exact score, then id
    r = SC.resolved_rule([0.805, 0.80, 0.70, 0.60], [1, 0, 2, 3], exact, ok, 2, 0.0, 0, eps)
    assert list(r[2]) == [0, 1]

    # not full, ending in (-inf, -1): every candidate was listed -> resolved, 3 entries, padded output
    r = SC.resolved_rule([0.90, 0.80, 0.70, -np.inf], [0, 1, 2, -1], exact, ok, 4, 0.0, 0, eps)
    assert r[0] is True and r[1] == 3 and list(r[2]) == [0, 1, 2, -1] and r[3][3] == -np.inf

    # truncated: the last slot is (+inf, -1) -> the scan cut the list, never resolved
    r = SC.resolved_rule([0.90, 0.80, 0.70, np.inf], [0, 1, 2, -1], exact, ok, 2, 0.0, 0, eps)
    assert r[0] is False and r[1] == 2

    # too few pass, threshold 0.75 (>=): rows 0 and 1 pass, k = 3.  Full list, last approx 0.60:
    # bound 0.61 < 0.75 -> nothing unlisted can pass -> resolved with 2 entries
    ok75 = SC.passes(exact, 0.75, 1)
    r = SC.resolved_rule([0.90, 0.80, 0.70, 0.60], [0, 1, 2, 3], exact, ok75, 3, 0.75, 1, eps)
    assert r[0] is True and r[1] == 2 and list(r[2]) == [0, 1, -1]
    # ... last approx 0.745: bound 0.755 >= 0.75 -> an unlisted row could pass -> unresolved
    r = SC.resolved_rule([0.90, 0.80, 0.75, 0.745], [0, 1, 2, 3], exact, ok75, 3, 0.75, 1, eps)
    assert r[0] is False
    # ... bound == thr exactly (0.5 + 0.25, binary fractions): mode 1 (>=) could still pass, mode 2 (>) cannot
    r1 = SC.resolved_rule([0.90, 0.80, 0.70, 0.5], [0, 1, 2, 3], exact, ok75, 3, 0.75, 1, 0.25)
    r2 = SC.resolved_rule([0.90, 0.80, 0.70, 0.5], [0, 1, 2, 3], exact, SC.passes(exact, 0.75, 2), 3, 0.75, 2, 0.25)
    assert r1[0] is False and r2[0] is True
    # ... no threshold (mode 0) and too few valid entries on a full list (ids out of range): never resolved
    r = SC.resolved_rule([0.90, 0.80, 0.70, 0.60], [0, 77, 88, 99], exact, ok, 3, 0.0, 0, eps)
    assert r[0] is False and r[1] == 1 and list(r[2]) == [0, -1, -1]

    assert SC.redo_count([True, False, True], [2, 0, 0], count_empty=False) == 1
    assert SC.redo_count([True, False, True], [2, 0, 0], count_empty=True) == 2
