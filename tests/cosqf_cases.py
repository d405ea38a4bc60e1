"""Inputs and references of the float32-query tests of the compressed-domain frame search (hq_cosqf_*): seeded,
NumPy only.  Frames come from cosq_cases (K bytes u plus float32 (mn, mx), x = mn + (mx - mn) u / 255).

A query row q of K float32 values is rounded to 24-bit fixed point (include/hq_mi355x.h): amax = f 2^e with f in
[0.5, 1), v_i = min(rint(q_i 2^(23 - e)), 2^23 - 1).  References:

fix24          v (int64) and ok per row; ok = 0 for a zero row and for a row with a NaN or inf.
exact_scores   the long-double (cos + 1) / 2 of (v, dequantised frame): what the kernels must give within TOL.
true_scores    the same for the query's own float32 values: what the caller means; bound() is the contract's
               limit 2^(e - 24) sqrt(K) / |q| on the difference of the two.
model_scores   the contract's integer formula (three digit planes, D = 65536 P2 + 256 P1 + P0 + 32896 S_c,
               t = K D - Sv S_c in int64, cos = A_q A_c + (B_q B_c) t) in NumPy int64 / float64.  `mutate` breaks it
               in one named way, to show that the families tell a right implementation from a wrong one."""
from functools import lru_cache

import numpy as np

import cosq_cases as C

TOL = C.TOL
MUTATIONS = ("drop_plane", "digit_offset", "unclamped", "float_t", "padded_k")
ONE_M = np.float32(1.0 - 2.0 ** -24)  # the largest float32 below 1: f = 1 - 2^-24 rounds to +2^23, which the clamp takes


def fix24(q, clamp=True):
    """(v int64 [R, K], ok bool [R], e int [R]) of float32 rows q."""
    q = np.asarray(q, np.float32)
    q64 = q.astype(np.float64)
    finite = np.isfinite(q64).all(axis=1)
    amax = np.where(finite, np.abs(np.where(np.isfinite(q64), q64, 0.0)).max(axis=1), 0.0)
    ok = finite & (amax > 0)
    _, e = np.frexp(np.where(ok, amax, 1.0))
    v = np.rint(np.ldexp(np.where(ok[:, None], q64, 0.0), (23 - e)[:, None].astype(np.int64)))  # exact scaling
    v = v.astype(np.int64)
    assert np.abs(v).max(initial=0) <= 2 ** 23
    if clamp:
        v = np.minimum(v, 2 ** 23 - 1)
    return v, ok, e


def _scores_ld(x, okq, U, MM):
    ld = np.longdouble
    xc, okc = C.dequantize_ld(U, MM)
    x = np.asarray(x).astype(ld)
    nq = np.sqrt((x * x).sum(axis=1))
    nc = np.sqrt((xc * xc).sum(axis=1))
    okq = okq & (nq > 0)
    okc = okc & (nc > 0)
    den = np.outer(np.where(okq, nq, ld(1)), np.where(okc, nc, ld(1)))
    s = ((x @ xc.T) / den + ld(1)) / ld(2)
    s[~okq, :] = 0
    s[:, ~okc] = 0
    return s.astype(np.float64)


def exact_scores(v, U, MM, ok=None):
    """[Q, N] float64: the long-double (cos + 1) / 2 of the integer rows v and the dequantised frames."""
    v = np.asarray(v)
    return _scores_ld(v, np.ones(len(v), bool) if ok is None else ok, U, MM)


def true_scores(q, U, MM):
    """The same for the float32 values themselves (a zero or non-finite row scores 0)."""
    q = np.asarray(q, np.float32)
    ok = np.isfinite(q).all(axis=1)
    return _scores_ld(np.where(ok[:, None], q, 0).astype(np.longdouble), ok, U, MM)


def bound(q, K):
    """Per row: 2^(e - 24) sqrt(K) / |q| (0 for rows that are not ok)."""
    q = np.asarray(q, np.float32)
    _, ok, e = fix24(q)
    q64 = np.where(ok[:, None], q.astype(np.float64), 0.0)
    _, ea = np.frexp(np.where(ok, np.abs(q64).max(axis=1), 1.0))
    nrm = np.sqrt(((q64 * np.ldexp(1.0, -ea)[:, None]) ** 2).sum(axis=1))  # |q| / 2^e, no overflow or underflow
    return np.where(ok, 2.0 ** -24 * np.sqrt(float(K)) / np.where(ok, nrm, 1.0), 0.0)


def digits(v):
    """The three int8 planes of v: bytes 0 and 1 of the 24-bit two's complement minus 128, byte 2 signed."""
    u = np.asarray(v, np.int64) & 0xFFFFFF
    p2 = (u >> 16) & 0xFF
    return (u & 0xFF) - 128, ((u >> 8) & 0xFF) - 128, np.where(p2 >= 128, p2 - 256, p2)


def frame_stats(U, MM, K):
    """(w, S, A_c, B_c, ok_c) as hq_cosq_prepare stores them."""
    mm = np.asarray(MM, np.float32).astype(np.float64)
    ok = np.isfinite(mm[:, 0]) & np.isfinite(mm[:, 1])
    mn, mx = np.where(ok, mm[:, 0], 0.0), np.where(ok, mm[:, 1], 0.0)
    w = np.asarray(U).astype(np.int64) - 128
    S, T = w.sum(axis=1), (w * w).sum(axis=1)
    Kf = float(K)
    s = np.where(mx == mn, 0.0, (mx - mn) / 255.0)
    m = mn + s * (128.0 + S / Kf)
    V = (K * T - S * S).astype(np.float64)
    n2 = m * m + (s * s) * (V / (Kf * Kf))
    ok &= n2 > 0
    inv = np.where(ok, 1.0 / np.sqrt(np.where(ok, n2, 1.0)), 0.0)
    return w, S, m * inv, (s * inv) / Kf, ok


def model_scores(q, U, MM, mutate=None, with_t=False):
    """[Q, N] float64 by the contract's formula; mutate in MUTATIONS (or None: the contract itself).  with_t: also
    the exact int64 t and the t of plain float64 products."""
    q = np.asarray(q, np.float32)
    Kt = q.shape[1]
    K = C.padded_k(Kt) if mutate == "padded_k" else Kt
    v, okq, _ = fix24(q, clamp=mutate != "unclamped")
    Sv, Nv = v.sum(axis=1), (v * v).sum(axis=1)
    Bq = np.where(okq, 1.0 / np.sqrt(np.where(okq, float(K) * Nv.astype(np.float64), 1.0)), 0.0)
    Aq = Sv.astype(np.float64) * Bq
    w, Sc, Ac, Bc, okc = frame_stats(U, MM, K)
    p0, p1, p2 = digits(v)
    P0, P1, P2 = p0 @ w.T, p1 @ w.T, p2 @ w.T
    assert max(np.abs(P).max(initial=0) for P in (P0, P1, P2)) <= 2 ** 30
    if mutate == "drop_plane":
        P0 = 0 * P0
    D = 65536 * P2 + 256 * P1 + P0 + (32768 if mutate == "digit_offset" else 32896) * Sc[None, :]
    ti = K * D - np.outer(Sv, Sc)                              # exact in int64: |t| <= 2^62
    tf = float(K) * D.astype(np.float64) - np.outer(Sv.astype(np.float64), Sc.astype(np.float64))
    t = tf if mutate == "float_t" else ti.astype(np.float64)
    cos = np.outer(Aq, Ac) + np.outer(Bq, Bc) * t
    s = np.where(np.outer(okq, okc), (cos + 1.0) / 2.0, 0.0)
    return (s, ti, tf) if with_t else s


# ---- query families ------------------------------------------------------------------------------------

FAMILIES = ("gaussian", "relu", "constant", "spike", "1e30", "subnormal", "zero", "nonfinite", "grid", "pipeline")
DEAD = ("zero",)            # every row scores 0.0
SMOOTH = ("gaussian", "relu", "pipeline")   # the families the 1e-5 statement is made for


@lru_cache(maxsize=None)
def family(name, K, seed=1):
    """float32 [4, K], read-only: four query rows of one family."""
    rng = np.random.default_rng([seed, K, FAMILIES.index(name), 5])
    R = 4
    g = rng.standard_normal((R, K))
    if name == "gaussian":
        q = g * np.array([1.0, 0.02, 37.0, 1e-6])[:, None] + np.array([0.0, 0.0, 5.0, 0.0])[:, None]
    elif name == "relu":
        q = np.maximum(g, 0.0) * np.array([1.0, 0.1, 3.0, 250.0])[:, None]
        q[:, 0] = np.abs(g[:, 0]) + 0.5  # never a zero row, also at K = 1
    elif name == "constant":
        q = np.tile(np.array([2.5, -1e-3, ONE_M, -ONE_M])[:, None], (1, K))
    elif name == "spike":
        q = np.zeros((R, K))
        q[np.arange(R), rng.integers(0, K, R)] = [1.0, -3.0, ONE_M, 1e-3]
        q[3] += 1e-9 * g[3]          # a spike over noise 2^-20 of it
    elif name == "1e30":
        q = g * 1e30
    elif name == "subnormal":
        q = g * 1e-40
        q[3] = np.where(g[3] > 0, 1.4e-45, -1.4e-45)  # the smallest subnormal, both signs
        q[:, 0] = np.where(q[:, 0] == 0, 1e-40, q[:, 0])
    elif name == "zero":
        q = np.zeros((R, K))
        q[1] = -0.0
    elif name == "nonfinite":
        q = g.copy()               # rows 0 .. 2 are outside the domain, row 3 is finite
        q[0, rng.integers(0, K)] = np.nan
        q[1, rng.integers(0, K)] = np.inf
        q[2, rng.integers(0, K)] = -np.inf
    elif name == "grid":
        q = rng.integers(0, 256, (R, K)).astype(np.float64)
        q[:, 0] = 255.0
    elif name == "pipeline":       # parameters of length 3 K / 8 laid onto K cells, the rest zero padding
        q = np.zeros((R, K))
        d = max(1, 3 * K // 8)
        q[:, rng.permutation(K)[:d]] = g[:, :d] * np.array([1.0, 0.02, 2.0, 0.3])[:, None]
    else:
        raise KeyError(name)
    q = q.astype(np.float32)
    q.setflags(write=False)
    return q


@lru_cache(maxsize=None)
def all_families(K, seed=1):
    """Every family's rows stacked: (q [4 F, K] f32, names [4 F])."""
    q = np.concatenate([family(n, K, seed) for n in FAMILIES])
    q.setflags(write=False)
    return q, [n for n in FAMILIES for _ in range(4)]


def dead_rows(names):
    """Rows that must score 0.0: the zero family and the three non-finite rows."""
    nf = C.rows_of(names, {"nonfinite"})[:3]
    return np.concatenate([C.rows_of(names, set(DEAD)), nf])


def grid_rows(R, K, seed):
    """Integer rows 0 .. 255 (every row holds a 255): as float32 queries and as u8 rows with (mn, mx) = (0, 255)."""
    rng = np.random.default_rng([seed, R, K, 9])
    U = rng.integers(0, 256, (R, K), dtype=np.uint8)
    U[:, 0] = 255
    return U.astype(np.float32), U, np.tile(np.array([[0, 255]], np.float32), (R, 1))


def operand_map_queries(R, K):
    """Rows whose three digit planes all differ and are asymmetric in (row, k): 24-bit integers from a
    multiplicative hash, the row maximum pinned to 2^23 - 1 so that v = q exactly."""
    r = np.arange(R, dtype=np.int64)[:, None]
    k = np.arange(K, dtype=np.int64)[None, :]
    v = ((r * 2654435761 + k * 40503 + r * k * 977 + 12345) % (2 ** 24)) - 2 ** 23
    v[:, 0] = 2 ** 23 - 1
    return v.astype(np.float32), v   # every |v| <= 2^23 is a float32


@lru_cache(maxsize=None)
def random_queries(R, K, seed):
    rng = np.random.default_rng([seed, R, K, 7])
    q = (rng.standard_normal((R, K)) * rng.uniform(0.01, 30, (R, 1)) + rng.uniform(-1, 1, (R, 1))).astype(np.float32)
    q[:, 0] = np.where(q[:, 0] == 0, 1, q[:, 0])
    q.setflags(write=False)
    return q


# (name, Q, N, K, ld (floats), base offset (floats), frames): cosq_cases.SHAPES' K, N and ld edges with Q at the
# 64-query workgroup tile (one below, at, one above, two tiles and one); frames = (r, c): the queries are
# [Q, r, c] frames read on their leading K / c rows
SHAPES = (
    ("K1", 1, 1, 1, 1, 0, None),
    ("K15", 63, 383, 15, 15, 0, None),
    ("K63", 65, 385, 63, 63, 0, None),
    ("K64-ld72", 129, 769, 64, 72, 0, None),
    ("K64-base1", 127, 385, 64, 64, 1, None),
    ("K65", 128, 769, 65, 65, 0, None),
    ("K4096", 1, 385, 4096, 4096, 0, None),
    ("K4096-frames", 129, 383, 4096, 4160, 0, (65, 64)),
    ("Q64", 64, 385, 16, 20, 0, None),
)


def strided(q, ld, off):
    """The flat float32 buffer that holds q's rows ld floats apart starting at float `off`; the gaps hold 3e38,
    which a kernel reading outside its K values would fold into amax."""
    R, K = q.shape
    buf = np.full(off + R * ld + 4, 3e38, np.float32)
    for r in range(R):
        buf[off + r * ld: off + r * ld + K] = q[r]
    return buf


def accumulator_queries():
    """K = 65536: v = -2^23 everywhere, v = 2^23 - 1 everywhere (the clamp), half and half."""
    K = C.MAX_K
    q = np.empty((3, K), np.float32)
    q[0] = -ONE_M                 # e = 0, v = rint(-(2^23 - 0.5)) = -2^23 (ties to even)
    q[1] = ONE_M                  # +2^23, clamped to 2^23 - 1
    q[2, :K // 2], q[2, K // 2:] = -ONE_M, ONE_M
    return q


def accumulator_frames():
    """u = 0 everywhere, 255 everywhere, half-and-half frames (both phases), seeded rows: 16 frames."""
    K = C.MAX_K
    U = C.random_rows(16, K, 78)[0].copy()
    U[0], U[1] = 0, 255
    U[2, :K // 2], U[2, K // 2:] = 0, 255
    U[3, :K // 2], U[3, K // 2:] = 255, 0
    MM = np.array([(-1, 1), (0, 1), (-2, 0.5), (1, 3)] * 4, np.float32)
    return U, MM
