"""Shared inputs and comparisons of the mutable-corpus tests (tests/test_mutate_cpu.py, tests/test_gpu_mutate.py):
seeded index rows with the degenerate shapes the layouts flag, a fresh build of a row set, and the byte
comparison of every layout of two Prepared corpora (the standard hq_seg_append is held to, hq_mi355x.h)."""
import ctypes

import numpy as np

from oracle import hq_oracle as O

TOL = 1e-10
PAD0 = 48

# (rows, removed rows): the smallest shapes at which 16-row tiles, 4-row groups and pad extents can go wrong
REMOVALS = [
    (1, []),
    (2, [0]),
    (2, [1]),
    (4, [3]),
    (5, [0]),
    (16, [15]),
    (17, [0]),                        # loses a whole 16-row tile
    (17, [16]),
    (33, list(range(0, 33, 2))),      # every second row
    (64, list(range(16))),
    (65, list(range(64))),            # all but row 64
    (200, None),                      # 37 seeded rows
]

# (rows, replaced rows)
REPLACEMENTS = [(1, [0]), (5, [4]), (16, [0, 15]), (17, [16]), (63, [3, 4, 62]), (200, None)]   # None: 40 seeded rows


def seeded_rows(n, count, seed):
    return sorted(np.random.default_rng(seed).choice(n, size=count, replace=False).tolist())


def np_(x):
    from hq_mi355x._dev import to_np
    return to_np(x)


def dev(x):
    from hq_mi355x._dev import to_dev
    return to_dev(x)


def special_lengths(lib):
    """(an L without a split overall layout, an L whose level-0 segment exceeds 32 values), L <= 1024.
    The first prefers an L that still has the level-0 copies, so both halves of the kernels are told apart."""
    no_ov, big0 = [], []
    v = [ctypes.c_int() for _ in range(4)]
    for L in range(2, 1025, 2):
        if lib.hq_seg_count(L) <= 0:
            continue
        l0 = lib.hq_seg_level0_len(L)
        if l0 > 32:
            big0.append(L)
        elif lib.hq_seg_packov_info(L, *[ctypes.byref(x) for x in v]) != 0:
            no_ov.append(L)
    return (no_ov[0] if no_ov else None), (big0[0] if big0 else None)


def kind(i):
    """The shape rows() gives row i: 'const', 'zero', 'flat0' (zero-variance level-0 segment) or 'plain'."""
    if i % 7 == 3:
        return "const"
    if i % 11 == 5:
        return "zero"
    if i % 5 == 1:
        return "flat0"
    return "plain"


def rows(n, L, seed, f32=False):
    """Seeded index rows with the degenerate shapes the layouts flag: constant rows, zero rows, rows whose
    level-0 segment has zero variance."""
    rng = np.random.default_rng(seed)
    C = rng.standard_normal((n, L)) * 0.5 + 0.1
    a, b = O.segment_bounds(L)[0]
    for i in range(n):
        k = kind(i)
        if k == "const":
            C[i] = 0.25
        elif k == "zero":
            C[i] = 0.0
        elif k == "flat0":
            C[i, a:b] = -0.75
    if f32:
        C = C.astype(np.float32).astype(np.float64)
    return C


def swapped_rows(which, L, seed):
    """Replacement rows for the rows `which` of rows(n, L, .): an ordinary row where the old one was degenerate,
    and a constant / zero / zero-variance level-0 row (in turn) where it was ordinary — so the flagged-row list
    must both lose and gain entries."""
    rng = np.random.default_rng(seed)
    a, b = O.segment_bounds(L)[0]
    out = rng.standard_normal((len(which), L)) * 0.5 - 0.2
    turn = 0
    for j, i in enumerate(which):
        if kind(i) != "plain":
            continue
        if turn % 3 == 0:
            out[j] = 0.5
        elif turn % 3 == 1:
            out[j] = 0.0
        else:
            out[j, a:b] = 1.25
        turn += 1
    return out


def fresh(x, flags=None):
    from hq_mi355x import kernels as K
    return K.flag_rows(K.packov(K.pack0(K.seg_prepare(dev(x), row_f32=flags))))


def same_layouts(g, f):
    """Every valid extent of the Prepared g equals the freshly built f (hq_mi355x.h: hq_seg_gather)."""
    N = f.N
    assert g.N == N and g.R.shape[0] == N and g.Z.shape[0] == N and g.S.shape[0] == N
    assert (g.f32, g.all32) == (f.f32, f.all32)
    r16, r4 = (N + 15) // 16 * 16 + PAD0, (N + 3) // 4 * 4 + PAD0
    for name, nrows in (("R", N), ("Z", N), ("S", N), ("Z16", r16), ("S32", r4), ("Zov16", r16), ("Sov32", r4 // 4)):
        a, b = getattr(g, name), getattr(f, name)
        assert (a is None) == (b is None), name
        if b is None:
            continue
        assert b.shape[0] == nrows and a.shape[0] >= nrows, name
        assert np_(a[:nrows]).tobytes() == np_(b[:nrows]).tobytes(), name
    assert (g.F0 is None) == (f.F0 is None)
    if f.F0 is not None:
        ga, fa = np_(g.F0), np_(f.F0)
        assert ga[0] == fa[0]
        assert sorted(ga[1:1 + ga[0]]) == sorted(fa[1:1 + fa[0]])


def flagged(p):
    """The flagged-row list of a Prepared as a set."""
    a = np_(p.F0)
    return set(int(v) for v in a[1:1 + a[0]])
