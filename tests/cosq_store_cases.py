"""Inputs and the NumPy model of the mutable u8 frame store (hq_cosq_append / hq_cosq_replace / hq_cosq_gather):
seeded, NumPy only.

The model states the operand layout of include/hq_mi355x.h independently of the kernels.  An operand of `cap` rows
is a pair (X8 uint8 [cap * Kp] flat, stats float64 [cap, 4]); row r = 16 t + j owns the 4 KB pieces of 16 bytes at
(t KB + kb) 1024 + 16 (16 g + j), kb < KB = Kp / 64, g < 4 (bytes 64 kb + 16 g .. + 15 of the frame, u ^ 0x80, zero
past K), and stats row r = (A, B, S, ok) by the header's formulas.  fresh() writes what hq_cosq_prepare writes;
append() / replace() / gather() write only what the three calls may write.  The contract under test: after any of
them the first padded_rows(N) rows equal fresh() of the resulting frames bit for bit, and nothing else changed.

`mutate` breaks an operation in one named way (MUTATIONS), to show that the cases tell a right kernel from a wrong
one.  Buffers under test are pre-filled with FILL = 0x5A, a byte no pad row holds."""
from functools import lru_cache

import numpy as np

import cosq_cases as C

FILL = 0x5A
MUTATIONS = ("resident_rows", "tile_sums", "no_pad", "swap_gj", "gather_no_stats")

padded_k = C.padded_k
padded_rows = C.padded_rows


# ---- the layout ------------------------------------------------------------------------------------------


def piece_offsets(rows, K, swap_gj=False):
    """Byte offset of every byte of the operand rows `rows` [R] -> int64 [R, Kp]: column k of a row is byte
    k % 16 of piece (kb = k // 64, g = (k % 64) // 16)."""
    rows = np.asarray(rows, np.int64).reshape(-1, 1)
    Kp = padded_k(K)
    KB = Kp // 64
    k = np.arange(Kp, dtype=np.int64)[None, :]
    kb, g, b = k // 64, (k % 64) // 16, k % 16
    t, j = rows // 16, rows % 16
    lane = 4 * j + g if swap_gj else 16 * g + j
    return (t * KB + kb) * 1024 + 16 * lane + b


def signed_rows(U, K):
    """u ^ 0x80 of the frames' first K bytes, zero padded to Kp -> uint8 [R, Kp]."""
    U = np.asarray(U, np.uint8)
    W = np.zeros((U.shape[0], padded_k(K)), np.uint8)
    W[:, :K] = U[:, :K] ^ 0x80
    return W


def row_stats(S, T, MM, K):
    """(A, B, S, ok) float64 [R, 4] of the header: s = (mx - mn) / 255 (0 when mx == mn), m = mn + s (128 + S / K),
    V = K T - S^2, n^2 / K = m^2 + s^2 V / K^2, A = m / sqrt(n^2 / K), B = s / (K sqrt(n^2 / K)); (0, 0, S, 0) when
    n^2 == 0 or (mn, mx) is not finite."""
    mm = np.asarray(MM, np.float32).astype(np.float64)
    ok = np.isfinite(mm[:, 0]) & np.isfinite(mm[:, 1])
    mn, mx = np.where(ok, mm[:, 0], 0.0), np.where(ok, mm[:, 1], 0.0)
    S = np.asarray(S, np.int64)
    T = np.asarray(T, np.int64)
    Kd = float(K)
    with np.errstate(all="ignore"):
        s = np.where(mx == mn, 0.0, (mx - mn) / 255.0)
        m = mn + s * (128.0 + S.astype(np.float64) / Kd)
        V = (K * T - S * S).astype(np.float64)
        n2 = m * m + (s * s) * (V / (Kd * Kd))
        ok &= n2 > 0.0
        inv = np.where(ok, 1.0 / np.sqrt(np.where(ok, n2, 1.0)), 0.0)
        out = np.stack([np.where(ok, m * inv, 0.0), np.where(ok, (s * inv) / Kd, 0.0), S.astype(np.float64),
                        ok.astype(np.float64)], axis=1)
    return out


def sums(U, K):
    w = np.asarray(U, np.uint8)[:, :K].astype(np.int64) - 128
    return w.sum(axis=1), (w * w).sum(axis=1)


def empty(cap, K):
    """An operand of cap rows filled with FILL."""
    return np.full(cap * padded_k(K), FILL, np.uint8), np.full(cap * 32, FILL, np.uint8).view(np.float64).reshape(cap, 4)


def _write_rows(X8, st, rows, U, MM, K, swap_gj=False, S=None, T=None):
    rows = np.asarray(rows, np.int64)
    if rows.size == 0:
        return
    X8[piece_offsets(rows, K, swap_gj)] = signed_rows(U, K)
    s0, t0 = sums(U, K)
    st[rows] = row_stats(s0 if S is None else S, t0 if T is None else T, MM, K)


def _write_pad(X8, st, lo, hi, K):
    if hi > lo:
        rows = np.arange(lo, hi, dtype=np.int64)
        X8[piece_offsets(rows, K)] = 0
        st[rows] = 0.0


def fresh(U, MM, K, cap=None):
    """hq_cosq_prepare of the frames U [N, >= K] with MM [N, 2] into an operand of cap rows (padded_rows(N) by
    default); rows past padded_rows(N) keep FILL."""
    N = np.asarray(U).shape[0]
    X8, st = empty(padded_rows(N) if cap is None else cap, K)
    _write_rows(X8, st, np.arange(N), U, MM, K)
    _write_pad(X8, st, N, padded_rows(N), K)
    return X8, st


def append(X8, st, N0, U, MM, K, mutate=None):
    """hq_cosq_append in place: frames U [M] become rows [N0, N0 + M), rows up to padded_rows(N0 + M) pad rows."""
    M = np.asarray(U).shape[0]
    if M == 0:
        return N0
    N1 = N0 + M
    rows = np.arange(N0, N1)
    S = T = None
    if mutate == "tile_sums":  # the partial sums of a tile's new rows land in every one of them
        s0, t0 = sums(U, K)
        S, T = s0.copy(), t0.copy()
        for t in np.unique(rows // 16):
            sel = rows // 16 == t
            S[sel], T[sel] = s0[sel].sum(), t0[sel].sum()
    _write_rows(X8, st, rows, U, MM, K, swap_gj=mutate == "swap_gj", S=S, T=T)
    if mutate == "resident_rows":  # N0's whole tile written: its resident rows as if they were pad rows
        _write_pad(X8, st, N0 // 16 * 16, N0, K)
    if mutate != "no_pad":
        _write_pad(X8, st, N1, padded_rows(N1), K)
    return N1


def replace(X8, st, N, rows, U, MM, K, mutate=None):
    """hq_cosq_replace in place: frame i overwrites row rows[i]; ids outside [0, N) are skipped."""
    rows = np.asarray(rows, np.int64)
    ok = (rows >= 0) & (rows < N)
    _write_rows(X8, st, rows[ok], np.asarray(U)[ok], np.asarray(MM)[ok], K, swap_gj=mutate == "swap_gj")
    if mutate == "resident_rows":  # the other rows of the tile zeroed
        for r in rows[ok]:
            X8[piece_offsets(np.setdiff1d(np.arange(r // 16 * 16, r // 16 * 16 + 16), rows[ok]), K)] = 0
    return N


def gather(src, K, sel, cap=None, mutate=None):
    """hq_cosq_gather: a second operand of cap rows (padded_rows(M) by default) whose row i is row sel[i] of src."""
    X8s, sts = src
    sel = np.asarray(sel, np.int64)
    M = sel.size
    X8, st = empty(padded_rows(M) if cap is None else cap, K)
    if M:
        dst = np.arange(M)
        X8[piece_offsets(dst, K, mutate == "swap_gj")] = X8s[piece_offsets(sel, K)]
        if mutate != "gather_no_stats":
            st[dst] = sts[sel]
    if mutate != "no_pad":
        _write_pad(X8, st, M, padded_rows(M) if M else min(128, st.shape[0]), K)  # M = 0: an empty corpus's pad rows
    return X8, st


def same(a, b, rows, K):
    """The first `rows` rows of two operands agree bit for bit."""
    n = rows * padded_k(K)
    return bool(np.array_equal(a[0][:n], b[0][:n]) and
                np.array_equal(a[1][:rows].view(np.int64), b[1][:rows].view(np.int64)))


def untouched(a, rows, K):
    """Everything past the first `rows` rows still holds FILL."""
    return bool(np.all(a[0][rows * padded_k(K):] == FILL) and np.all(a[1][rows:].view(np.uint8) == FILL))


# ---- the cases -------------------------------------------------------------------------------------------

# (name, K, ld, base offset): every K edge of a 16-byte piece and a 64-byte step, KB = 17 (past the sixteen waves'
# first pass over the K steps), the pipeline's 65 x 64 frames searched on 64 rows, and a store with an odd base
# and an odd ld (byte loads)
STORES = (
    ("K1", 1, 1, 0),
    ("K15", 15, 15, 0),
    ("K16", 16, 16, 0),
    ("K17", 17, 17, 0),
    ("K63", 63, 63, 0),
    ("K64", 64, 64, 0),
    ("K65", 65, 65, 0),
    ("K1088", 1088, 1088, 0),
    ("K4096", 4096, 4096, 0),
    ("K4096-ld4160", 4096, 4160, 0),
    ("K64-ld67-base1", 64, 67, 1),
)
N0S = (0, 1, 15, 16, 17, 127, 128, 129, 383, 384, 385)
MS = (1, 15, 16, 17, 130)
STORE_IDS = [s[0] for s in STORES]


@lru_cache(maxsize=None)
def pool(K):
    """Rows to draw from: every family of cosq_cases (mn == mx and non-finite (min, max) among them), then seeded
    rows of mixed ranges.  Read-only."""
    Uf, Mf, names = C.all_families(K)
    Ur, Mr = C.random_rows(600, K, 91)
    U, MM = np.concatenate([Uf, Ur]), np.concatenate([Mf, Mr])
    U.setflags(write=False)
    MM.setflags(write=False)
    return U, MM, len(names)


def frames(K, first, count):
    """`count` frames (U [count, K], MM [count, 2]) starting at draw `first`: every second one walks the families,
    the others the seeded rows, so that short appends meet constant and non-finite frames too."""
    U, MM, F = pool(K)
    i = np.arange(first, first + count)
    idx = np.where(i % 2 == 0, (i // 2 * 3) % F, F + (i * 37) % (U.shape[0] - F))
    return U[idx], MM[idx]


def nonfinite_frame(K):
    U, MM, names = C.all_families(K)
    r = C.rows_of(names, {"nonfinite"})[0]
    return U[r:r + 1], MM[r:r + 1]


# replace: (N, row ids): first and last row, two rows of one tile, a whole tile, rows across tiles
REPLACES = (
    (17, (0,)),
    (17, (16,)),
    (129, (128, 3, 4)),
    (129, tuple(range(16, 32))),
    (385, (384, 0, 127, 128, 200, 383, 17)),
    (385, tuple(range(5, 385, 29))),
)


def gather_patterns(N):
    """(name, source row ids) over a source of N >= 145 rows."""
    a = np.arange(N)
    return (
        ("identity", a),
        ("reverse", a[::-1]),
        ("repeats", np.array([5, 5, 5, N - 1, 0, 0, 17, 16, 15, N - 1])),
        ("drop-first", a[1:]),
        ("drop-last", a[:-1]),
        ("drop-every-16th", a[a % 16 != 15]),
        ("drop-a-tile", np.concatenate([a[:32], a[48:]])),
        ("to-127", (a * 7 % N)[:127]),
        ("to-128", (a * 7 % N)[:128]),
        ("to-129", (a * 7 % N)[:129]),
        ("one", a[N // 2:N // 2 + 1]),
    )


GATHER_N = 145
