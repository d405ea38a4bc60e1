"""Golden data of the RAG engine's comprehensive frame similarity (rag/search/engine.py:478-727, 994-1138)
-> tests/golden/comprehensive.npz.  Build-container only, like make_golden.py (same inert cv2 stub, the engine
made with cls.__new__: the scoring helpers use no instance state beyond each other).

    python tests/golden/make_comprehensive.py --ref /path/to/reference

Families (8 frames each, the RAG generator's index rows appended): base, base + noise, independent, -base,
|base|, |base| + 1, 3 base + 1, base with a 4 x 6 zero patch.  Per family <tag>: <tag>_enh [8, H, W],
<tag>_score [8, 8], <tag>_parts [8, 8, 3] (hierarchical, embedding, spatial), <tag>_desc [8, 3] (h, L, width),
<tag>_rank_keys / <tag>_rank_ids / <tag>_rank_scores (calculate_embedding_similarity of frame 1 against the
family under the frame numbers <tag>_rank_keys).
Edge frames e_<name>_<tag>: _enh [H, W], _desc [3], _score [2, 9] (row 0: the edge frame as the query against
the family's 8 frames and itself, row 1: as the candidate), _parts [2, 9, 3].  Stand-alone sets s_<name>:
_enh [n, H, W], _desc [n, 3], _score [n, n], _parts [n, n, 3].  e_width_enh [2, 9, 8] with e_width_raised = 1
when the reference raised ValueError for the pair.

shape_fixtures() -> tests/golden/comprehensive_shapes.npz: hand-built frames (tests/comp_sweep_cases.build_frame) at
the shapes the first file lacks, 5 frames each (full, noisy, independent, first index row dropped, zero patch), in
float64 (<set>) and float32 (<set>f): wide 12 x 100, odd 20 x 65, small 6 x 4 (ws < 2 with index rows), rows31
40 x 8 (31 index rows).  Per set g_<set>_enh / _desc / _score / _parts as for the stand-alone sets.  nonfinite: 9 x 8
frames, frame 1 with a NaN and frame 2 with an inf in the data block, frame 3 with a NaN in its index row;
g_<set>_raised [n, n] is 1 where the reference raised for the pair (its score and parts are then recorded as NaN)."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

FAMILIES = (("f9d", 8, np.float64), ("f18d", 16, np.float64), ("f9f", 8, np.float32), ("f34f", 32, np.float32),
            ("f67f", 64, np.float32))


def _engine():
    from hilbert_quantization.rag.search import engine as E
    cls = [v for v in vars(E).values() if isinstance(v, type) and hasattr(v, "_calculate_comprehensive_similarity")][0]
    return cls.__new__(cls)


def _desc(obj, e):
    h = int(obj._detect_original_embedding_height(e))
    lv = obj._extract_hierarchical_indices(e)
    return np.array([h, len(lv), max([len(x) for x in lv], default=0)], dtype=np.int64)


def _pair(obj, q, c):
    """(score, [hierarchical, embedding, spatial]) exactly as _calculate_comprehensive_similarity forms them."""
    qi, ci = obj._extract_hierarchical_indices(q), obj._extract_hierarchical_indices(c)
    if qi and ci:
        m = max(len(qi), len(ci))
        hier = obj.compare_hierarchical_indices(obj._pad_indices_to_length(qi, m), obj._pad_indices_to_length(ci, m))
    else:
        hier = 0.0
    emb = obj._calculate_embedding_cosine_similarity(obj._extract_original_embedding(q),
                                                     obj._extract_original_embedding(c))
    spa = obj._calculate_spatial_locality_similarity(q, c)
    score = obj._calculate_comprehensive_similarity(q, qi, c, 0)
    return float(score), [float(hier), float(emb), float(spa)]


def _matrix(obj, qs, cs):
    sc = np.zeros((len(qs), len(cs)))
    pt = np.zeros((len(qs), len(cs), 3))
    for a, q in enumerate(qs):
        for b, c in enumerate(cs):
            sc[a, b], pt[a, b] = _pair(obj, q, c)
    return sc, pt


def fixtures():
    from hilbert_quantization.rag.embedding_generation.hierarchical_index_generator import (
        HierarchicalIndexGenerator as RagGen)
    obj, rg = _engine(), RagGen()
    rng = np.random.default_rng(77)
    out = {}

    def enhance(im, dt):
        return np.asarray(rg.generate_multi_level_indices(im)).astype(dt)

    fams = {}
    for tag, n, dt in FAMILIES:
        base = rng.standard_normal((n, n)).astype(dt)
        patch = base.copy()
        patch[2:6, 2:8] = 0.0   # even offsets: whole 4 x 4 windows at stride 2 inside it
        imgs = [base, base + rng.normal(0, 0.3, (n, n)).astype(dt), rng.standard_normal((n, n)).astype(dt), -base,
                np.abs(base), np.abs(base) + dt(1.0), base * dt(3.0) + dt(1.0), patch]
        enh = np.stack([enhance(im, dt) for im in imgs])
        fams[tag] = enh
        out[f"{tag}_enh"] = enh
        out[f"{tag}_score"], out[f"{tag}_parts"] = _matrix(obj, enh, enh)
        out[f"{tag}_desc"] = np.stack([_desc(obj, e) for e in enh])
        keys = 100 + 7 * rng.permutation(8)
        rank = obj.calculate_embedding_similarity(enh[1], {int(k): enh[i] for i, k in enumerate(keys)})
        out[f"{tag}_rank_keys"] = keys.astype(np.int64)
        out[f"{tag}_rank_ids"] = np.array([r[0] for r in rank], dtype=np.int64)
        out[f"{tag}_rank_scores"] = np.array([float(r[1]) for r in rank])

    def edge(name, tag, e):
        enh = fams[tag]
        e = np.ascontiguousarray(e.astype(enh.dtype))
        cs = list(enh) + [e]
        s0, p0 = _matrix(obj, [e], cs)
        s1, p1 = _matrix(obj, cs, [e])
        out[f"e_{name}_{tag}_enh"] = e
        out[f"e_{name}_{tag}_desc"] = _desc(obj, e)
        out[f"e_{name}_{tag}_score"] = np.stack([s0[0], s1[:, 0]])
        out[f"e_{name}_{tag}_parts"] = np.stack([p0[0], p1[:, 0]])

    for tag, n, dt in FAMILIES:
        H = fams[tag].shape[1]
        edge("zero", tag, np.zeros((H, n), dt))
        base = fams[tag][0][:n]
        # the "short" frame of rag_score_fixtures, its last data row cut to the family's index width so that the
        # pair does not raise: where the first index row is sparse (9 x 8, 34 x 32) the row counts as an index
        # row, the detected height drops by one and L grows by one
        short = base.copy()
        short[n - 1, int(out[f"{tag}_desc"][0, 2]):] = 0.0
        edge("short", tag, enhance(short, dt))
        # every quarter zero-mean (small integers: the sums are exact) -> the g = 2 row is all zero and is dropped
        a = rng.integers(-8, 9, (2, 2, n // 2, n // 4)).astype(dt)
        zm = np.block([[np.concatenate([a[i, j], -a[i, j]], axis=1) for j in range(2)] for i in range(2)])
        edge("zeromean", tag, enhance(zm, dt))

    def standalone(name, frames):
        enh = np.stack(frames)
        out[f"s_{name}_enh"] = enh
        out[f"s_{name}_desc"] = np.stack([_desc(obj, e) for e in enh])
        out[f"s_{name}_score"], out[f"s_{name}_parts"] = _matrix(obj, enh, enh)

    # 15 x 16, one sparse index row: h = 14, ws = 3, stride 1
    b = rng.standard_normal((14, 16))
    fr = []
    for x in (b, b + rng.normal(0, 0.3, (14, 16)), rng.standard_normal((14, 16))):
        row = np.zeros((1, 16))
        row[0, :4] = x.reshape(2, 7, 2, 8).mean(axis=(1, 3)).reshape(-1)
        fr.append(np.concatenate([x, row]))
    standalone("ws3", fr)
    standalone("ws3f", [f.astype(np.float32) for f in fr])
    # 11 x 8 with three index rows of one width; frame 1 has its first, frame 2 its middle index row zeroed: the
    # row is dropped and the later rows move up (the generator's rows differ in width, so a dropped generator
    # row other than the last makes the reference raise)
    g = np.concatenate([rng.standard_normal((8, 8)), np.zeros((3, 8))])
    g[8:, :4] = rng.standard_normal((3, 4))
    g1, g2, g3 = g.copy(), g.copy(), g.copy()
    g1[8], g2[9] = 0.0, 0.0
    g3[8:, :4] += rng.normal(0, 0.5, (3, 4))
    standalone("gap", [g, g1, g2, g3])
    standalone("gapf", [x.astype(np.float32) for x in (g, g1, g2, g3)])
    # 5 x 4: ws < 2 (one cosine over the block), no index rows
    t = rng.standard_normal((5, 4))
    standalone("tiny", [t, t + rng.normal(0, 0.3, (5, 4)), rng.standard_normal((5, 4))])
    # index rows of different trimmed widths: the reference raises
    w = np.stack([fams["f9d"][0].copy(), fams["f9d"][1].copy()])
    w[1, 8, 3] = 0.0
    out["e_width_enh"] = w
    try:
        _pair(obj, w[0], w[1])
        out["e_width_raised"] = np.array(0, dtype=np.int64)
    except ValueError as e:
        assert "same shape" in str(e)
        out["e_width_raised"] = np.array(1, dtype=np.int64)
    out["e_width_desc"] = np.stack([_desc(obj, e) for e in w])
    out["weights"] = np.array([obj._get_similarity_weights()[k] for k in ("hierarchical", "embedding", "spatial")])
    return out


SHAPE_SETS = (("wide", 12, 100, 10), ("odd", 20, 65, 17), ("small", 6, 4, 4), ("rows31", 40, 8, 9))


def _matrix_recorded(obj, qs, cs):
    """_matrix that records what the reference does with a pair instead of assuming it: raised = 1 and NaN entries
    where it raised."""
    sc = np.full((len(qs), len(cs)), np.nan)
    pt = np.full((len(qs), len(cs), 3), np.nan)
    raised = np.zeros((len(qs), len(cs)), dtype=np.int64)
    for a, q in enumerate(qs):
        for b, c in enumerate(cs):
            try:
                sc[a, b], pt[a, b] = _pair(obj, q, c)
            except Exception:  # noqa: BLE001 - whatever it raises is the recorded behaviour
                raised[a, b] = 1
    return sc, pt, raised


def shape_fixtures():
    sys.path.insert(0, os.path.dirname(HERE))
    import comp_sweep_cases as SW
    obj = _engine()
    rng = np.random.default_rng(78)
    out = {}

    def record(name, frames):
        for tag, dt in ((name, np.float64), (name + "f", np.float32)):
            enh = np.stack(frames).astype(dt)
            out[f"g_{tag}_enh"] = enh
            out[f"g_{tag}_desc"] = np.stack([_desc(obj, e) for e in enh])
            out[f"g_{tag}_score"], out[f"g_{tag}_parts"], out[f"g_{tag}_raised"] = _matrix_recorded(obj, enh, enh)

    for name, H, W, h in SHAPE_SETS:
        base, _ = SW.build_frame(rng, H, W, h)
        record(name, [base, SW.build_frame(rng, H, W, h, "noisy", base)[0], SW.build_frame(rng, H, W, h)[0],
                      SW.build_frame(rng, H, W, h, "drop_first", base)[0],
                      SW.build_frame(rng, H, W, h, "zero_patch", base)[0]])
    base, _ = SW.build_frame(rng, 9, 8, 8)
    nan_block, inf_block, nan_row = base.copy(), base.copy(), base.copy()
    nan_block[3, 5] = np.nan
    inf_block[2, 1] = np.inf
    nan_row[8, 1] = np.nan
    record("nonfinite", [base, nan_block, inf_block, nan_row, SW.build_frame(rng, 9, 8, 8, "noisy", base)[0]])
    return out


def main():
    from make_golden import _import_reference
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of the reference checkout")
    a = ap.parse_args()
    _import_reference(a.ref)
    d = fixtures()
    path = os.path.join(HERE, "comprehensive.npz")
    np.savez_compressed(path, **d)
    print(f"wrote {path}: {len(d)} arrays, {os.path.getsize(path)} bytes")
    d = shape_fixtures()
    path = os.path.join(HERE, "comprehensive_shapes.npz")
    np.savez_compressed(path, **d)
    print(f"wrote {path}: {len(d)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
