"""Inputs of the pre-computed similarity scorer sweep (core/precomputed_hilbert_index.py:358-496), NumPy only.

One definition of the cases for three users: tests/golden/make_golden.py runs the real reference on them and
records value + result type in tests/golden/precomp_sim.npz, tests/test_precomp_sim_cpu.py pins the oracle to
those records, tests/test_gpu_precomp_sim.py runs the kernels on them.  `digest()` of every input array is
stored with the goldens, so a change of the seeded inputs is reported as such instead of as a wrong score.

Level lengths are the sizes that occur in real layouts (5, 25, 113, 481, 1985, 8065; 2610 = a whole 64 x 64
index) plus every edge of NumPy's pairwise summation: the n < 8 sequential sum, n % 8 remainders, the 128 / 129
split and splits whose halves are themselves odd.
"""
import hashlib

import numpy as np

LENGTHS = [1, 2, 3, 5, 7, 8, 9, 13, 25, 64, 113, 127, 128, 129, 136, 255, 256, 257, 321, 481, 1000, 1985, 2610, 8065]
CANDIDATES = ["same", "neg", "x3", "2x+5", "-x+100", "noisy", "const", "near_const"]
EDGE_LENGTHS = [7, 129]
CONST_PAIRS = [(0.5, 0.5), (1.0, 1.0 + 5e-7), (1.0, 1.0 + 2e-6), (0.0, 1e-6), (0.0, 0.0)]
LEGACY_LENGTHS = [1, 2, 3, 7, 64, 129, 1000]

TYPE_F32, TYPE_PY = 0, 1


def digest(a) -> bytes:
    """8-byte BLAKE2b of dtype.str + shape + bytes."""
    a = np.ascontiguousarray(a)
    h = hashlib.blake2b(digest_size=8)
    h.update(a.dtype.str.encode())
    h.update(repr(tuple(a.shape)).encode())
    h.update(a.tobytes())
    return h.digest()


def type_code(v) -> int:
    """0 for a numpy float32 result, 1 for a Python float (or any other scalar the reference returns)."""
    return TYPE_F32 if isinstance(v, np.float32) else TYPE_PY


def _f32(x):
    return np.asarray(x, dtype=np.float32)


def single_level_cases():
    """[(name, q, c)] float32 vectors of equal length for _compare_precomputed_levels."""
    rng = np.random.default_rng(20261021)
    out = []
    for m in LENGTHS:
        q = _f32(rng.standard_normal(m))
        cands = [q.copy(), -q, np.float32(3) * q, np.float32(2) * q + np.float32(5), -q + np.float32(100),
                 q + _f32(rng.normal(0, 0.1, m)), np.full(m, 0.5, np.float32),
                 _f32(1 + 1e-3 * rng.standard_normal(m))]
        for name, c in zip(CANDIDATES, cands):
            out.append((f"m{m}_{name}", q, _f32(c)))
    for m in EDGE_LENGTHS:
        q = _f32(rng.standard_normal(m))
        c = q + _f32(rng.normal(0, 0.3, m))
        for a, b in CONST_PAIRS:
            out.append((f"m{m}_const_{a!r}_{b!r}", np.full(m, a, np.float32), np.full(m, b, np.float32)))
        for tag, bad in (("nan", np.nan), ("inf", np.inf)):
            qb, cb = q.copy(), c.copy()
            qb[m // 2] = bad
            cb[m - 1] = bad
            out.append((f"m{m}_{tag}_q", qb, c))
            out.append((f"m{m}_{tag}_c", q, cb))
            out.append((f"m{m}_{tag}_both", qb, cb))
            out.append((f"m{m}_{tag}_vs_const", qb, np.full(m, 0.5, np.float32)))
        out.append((f"m{m}_1e30", q * np.float32(1e30), c * np.float32(1e30)))
        out.append((f"m{m}_1e30_same", q * np.float32(1e30), q * np.float32(1e30)))
    return out


def legacy_cases():
    """[(name, q, c)] float64 vectors for the legacy compare_indices_at_level (np.std branches, np.allclose,
    np.corrcoef).  The near-constant vectors 1 + 1e-9 N are the ones whose centred sums cancel nine digits."""
    rng = np.random.default_rng(77001)
    out = []
    for m in LEGACY_LENGTHS:
        q = rng.standard_normal(m)
        near = 1 + 1e-9 * rng.standard_normal(m)
        near2 = 1 + 1e-9 * rng.standard_normal(m)
        out += [(f"m{m}_const_equal", np.full(m, 2.0), np.full(m, 2.0)),
                (f"m{m}_const_close", np.full(m, 2.0), np.full(m, 2.0 + 2.0 ** -20)),    # np.allclose holds
                (f"m{m}_const_inexact", np.full(m, 2.0), np.full(m, 2.0 + 1e-6)),        # np.std may not be 0
                (f"m{m}_const_far", np.full(m, 2.0), np.full(m, 2.1)),
                (f"m{m}_one_const", np.full(m, 2.0), q),
                (f"m{m}_neg", q, -q),
                (f"m{m}_same", q, q.copy()),
                (f"m{m}_noisy", q, q + rng.normal(0, 0.5, m)),
                (f"m{m}_near_const_vs_q", near, q),
                (f"m{m}_near_const_pair", near, near2),
                (f"m{m}_near_const_noisy", near, 1 + (near - 1) + 3e-10 * rng.standard_normal(m))]
        if m >= 3:
            qn = q.copy()
            qn[1] = np.nan
            out.append((f"m{m}_nan", qn, q))
    return out


def layout_counts(n: int):
    """Averages per level of the default layout (max_levels 6, min_square_size 2): g^2 grid squares plus
    (g - 1)^2 overlapping squares for square sizes 2, 4, ... n / 2, then the whole image."""
    out, s = [], 2
    while s <= n // 2 and len(out) < 6:
        g = n // s
        out.append(g * g + (g - 1) * (g - 1))
        s *= 2
    out.append(1)
    return out


def _index_set(rng, n):
    """(queries, candidates): lists of per-level float32 arrays in the default layout of an n x n image."""
    cnt = layout_counts(n)

    def gen(scale=1.0):
        return [_f32(rng.standard_normal(c) * scale) for c in cnt]

    g0, g1 = gen(), gen(0.3)
    const = lambda v: [np.full(c, v, np.float32) for c in cnt]  # noqa: E731
    noisy = lambda s: [a + _f32(rng.normal(0, s, len(a))) for a in g0]  # noqa: E731
    cfirst = [a.copy() for a in g0]
    cfirst[0] = np.full(cnt[0], 0.25, np.float32)
    nanlvl = [a.copy() for a in g0]
    nanlvl[1][len(nanlvl[1]) // 3] = np.nan
    queries = [g0, g1, const(0.5)]
    cands = [[a.copy() for a in g0], noisy(0.02), noisy(0.2), noisy(1.0), [-a for a in g0], cfirst, const(0.5),
             const(0.7), nanlvl, gen()]
    return queries, cands


def multi_level_cases():
    """{name: (queries, candidates)}: every query x candidate pair is one case.  `q32_c16` pairs 32 x 32 queries
    (5 levels: 481, 113, 25, 5, 1) with 16 x 16 candidates (4 levels: 113, 25, 5, 1): the level offsets differ
    and every level compares the first min(count) averages."""
    rng = np.random.default_rng(3216)
    q32, c32 = _index_set(rng, 32)
    q16, c16 = _index_set(rng, 16)
    # 16 x 16 candidates related to the 32 x 32 query's leading averages, so the cross scores are spread out
    rel = [[q32[0][l][:c] + _f32(rng.normal(0, s, c)) for l, c in enumerate(layout_counts(16))]
           for s in (0.0, 0.05, 0.5)]
    return {"n32": (q32, c32), "n16": (q16, c16), "q32_c16": (q32, rel + c16)}


def pack(levels):
    """(row, offsets) of one index: the level arrays back to back."""
    offs, o = [], 0
    for a in levels:
        offs.append(o)
        o += len(a)
    return np.concatenate(levels).astype(np.float32), offs
