"""The long-double model of the frame ordering (tests/order_cases.py) reproduces the reference's own outputs
(tests/golden/frame_ordering.npz: orders, insertion positions, metrics before and after sorting)."""
import numpy as np
import pytest

import order_cases as OC



@pytest.mark.parametrize("name", OC.CASES)
def test_model_reproduces_reference(golden, name):
    g = golden("frame_ordering")
    assert tuple(g["names"]) == OC.CASES
    rows = g[f"{name}_rows"]
    order, _, gap = OC.greedy(rows)
    assert gap >= 1e-9 and OC.start_gap(rows) >= 1e-9
    assert order.tolist() == g[f"{name}_order"].tolist()
    np.testing.assert_allclose(OC.metrics(rows), g[f"{name}_metrics"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(OC.metrics(rows, order), g[f"{name}_metrics_sorted"], rtol=0, atol=1e-12)
    pos = [OC.insertion(s)[0] for s in OC.sims(g[f"{name}_queries"], rows)]
    assert pos == g[f"{name}_pos"].tolist()
