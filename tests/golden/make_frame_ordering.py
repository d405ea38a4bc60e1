"""Golden data of the video store's frame ordering (core/video_storage.py:1203-1277, 1445-1522, 1751-1803)
-> tests/golden/frame_ordering.npz.  Build-container only, like make_progressive_rag.py (same inert cv2 stub, the
storage made with cls.__new__).

    python tests/golden/make_frame_ordering.py --ref /path/to/reference

names: the cases.  Per case <c>: <c>_rows [N, L] index rows, <c>_order [N] (the reference's sorted frames as
positions in the stored order), <c>_metrics / <c>_metrics_sorted [4] (order_cases.KEYS, stored / sorted order),
<c>_queries [Q, L] and <c>_pos [Q] (the reference's insertion positions).

Every store is asserted here to keep the model's smallest step gap (order_cases.greedy), its start gap and the gap of
every insertion score >= 1e-9, exact ties of bit-identical rows and of the constant-row branch aside; stores are
re-seeded until that holds, so the reference's own float64 rounding never decides an order."""
import argparse
import os
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def _reference(rows, queries):
    from hilbert_quantization.core.video_storage import VideoModelStorage as cls
    import order_cases as OC
    obj = cls.__new__(cls)
    frames = [SimpleNamespace(frame_index=i, hierarchical_indices=r.copy()) for i, r in enumerate(rows)]
    obj._video_index = {"v": SimpleNamespace(frame_metadata=frames)}
    obj._current_metadata = frames
    stored = obj.get_frame_ordering_metrics("v")
    pos = [obj._find_optimal_insertion_position(q) for q in queries]
    ids = {id(f): i for i, f in enumerate(frames)}
    out = obj._sort_frames_by_hierarchical_indices(frames)
    assert [f.frame_index for f in out] == list(range(len(out)))
    obj._video_index["v"].frame_metadata = out
    after = obj.get_frame_ordering_metrics("v")
    return (np.array([ids[id(f)] for f in out], np.int64), np.array([stored[k] for k in OC.KEYS]),
            np.array([after[k] for k in OC.KEYS]), np.array(pos, np.int64))


def fixtures():
    import order_cases as OC
    out, names = {}, []
    cases = (("gauss5", OC.gaussian, 12, 5), ("gauss32", OC.gaussian, 48, 32), ("gauss64", OC.gaussian, 33, 64),
             ("dups32", OC.with_duplicates, 24, 32), ("const5", OC.with_constants, 16, 5),
             ("const64", OC.with_constants, 17, 64))
    for name, build, N, L in cases:
        for seed in range(200):
            rng = np.random.default_rng(seed + sum(map(ord, name)))
            rows = build(rng, N, L)
            # queries: near a stored row, a copy of the first and of the last row, a constant row
            queries = np.stack([rows[N // 2] + 0.1 * rng.standard_normal(L), rows[0], rows[-1], np.full(L, 0.5)])
            gaps = [OC.greedy(rows)[2], OC.start_gap(rows)]
            for s in OC.sims(queries, rows):  # position scores: exact ties (np.unique merges them) go to the first
                sc = np.unique(np.concatenate([s[:1], (s[:-1] + s[1:]) / 2, s[-1:]]))
                gaps.append(float(sc[-1] - sc[-2]) if len(sc) > 1 else np.inf)
            if min(gaps) >= 1e-9:
                break
        else:
            raise AssertionError(f"{name}: no seed keeps every decision 1e-9 apart")
        order, m0, m1, pos = _reference(rows, queries)
        names.append(name)
        out[f"{name}_rows"], out[f"{name}_queries"] = rows, queries
        out[f"{name}_order"], out[f"{name}_metrics"], out[f"{name}_metrics_sorted"], out[f"{name}_pos"] = order, m0, m1, pos
        print(f"{name}: N = {N}, L = {L}, seed {seed}, smallest gap {min(gaps):.2e}, positions {pos.tolist()}")
    out["names"] = np.array(names)
    return out


def main():
    from make_golden import _import_reference
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of the reference checkout")
    a = ap.parse_args()
    _import_reference(a.ref)
    d = fixtures()
    path = os.path.join(HERE, "frame_ordering.npz")
    np.savez_compressed(path, **d)
    print(f"wrote {path}: {len(d)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
