"""Inputs and references of the compressed-domain frame search tests (hq_cosq_*): seeded, NumPy only.

A row is K bytes u plus float32 (mn, mx); its values are x = mn + (mx - mn) u / 255.  Two references:

exact_scores   the definition, naively: x in np.longdouble (80-bit), dot and norms in long double, (cos + 1) / 2;
               0.0 for a zero row and for a row whose (mn, mx) is not finite.
model_scores   the contract's integer formula (include/hq_mi355x.h) stated independently in NumPy int64 / float64:
               a = m inv, b = s inv, cos = K a_q a_c + b_q b_c t / K.  `mutate` breaks it in one named way, to show
               that the row families below tell a right implementation from a wrong one.

TOL = 1e-13 is the bound every comparison against exact_scores uses: 300 times the largest difference the model
shows on these families (3.3e-16), eight orders of magnitude below what one wrong byte produces."""
from functools import lru_cache

import numpy as np

TOL = 1e-13
MAX_K = 65536
MUTATIONS = ("unsigned", "no_mean", "padded_k", "const_zero")

FLT_MAX = np.finfo(np.float32).max
SUBNORMAL = np.float32(1e-40)


def padded_k(K):
    return (K + 63) // 64 * 64


def padded_rows(N):
    return (N + 127) // 128 * 128


def _valid(mm):
    return np.isfinite(mm[:, 0]) & np.isfinite(mm[:, 1])


def dequantize_ld(U, MM):
    """x = mn + (mx - mn) u / 255 in long double from the float32 (mn, mx); rows with a non-finite pair: zeros."""
    ld = np.longdouble
    mm = np.asarray(MM, np.float32)
    ok = _valid(mm)
    mn = np.where(ok, mm[:, 0], 0).astype(ld)[:, None]
    mx = np.where(ok, mm[:, 1], 0).astype(ld)[:, None]
    return mn + (mx - mn) * np.asarray(U).astype(ld) / ld(255), ok


def exact_scores(Uq, MMq, Uc, MMc):
    """[Q, N] float64: the long-double (cos + 1) / 2 of the dequantised rows, rounded once."""
    ld = np.longdouble
    xq, okq = dequantize_ld(Uq, MMq)
    xc, okc = dequantize_ld(Uc, MMc)
    nq = np.sqrt((xq * xq).sum(axis=1))
    nc = np.sqrt((xc * xc).sum(axis=1))
    okq &= nq > 0
    okc &= nc > 0
    dot = xq @ xc.T
    den = np.outer(np.where(okq, nq, ld(1)), np.where(okc, nc, ld(1)))
    s = (dot / den + ld(1)) / ld(2)
    s[~okq, :] = 0
    s[:, ~okc] = 0
    return s.astype(np.float64)


def _row_stats(U, MM, K, mutate, operand):
    mm = np.asarray(MM, np.float32).astype(np.float64)
    ok = _valid(mm)
    mn, mx = np.where(ok, mm[:, 0], 0.0), np.where(ok, mm[:, 1], 0.0)
    w = np.asarray(U).astype(np.int64) - 128
    S, T = w.sum(axis=1), (w * w).sum(axis=1)
    Kf = float(padded_k(K) if mutate == "padded_k" else K)
    s = np.where(mx == mn, 0.0, (mx - mn) / 255.0)
    m = mn + s * (128.0 + (0.0 if mutate == "no_mean" else S / Kf))
    V = (int(Kf) * T - S * S).astype(np.float64)
    n2 = Kf * m * m + s * s * V / Kf
    if mutate == "const_zero":
        n2 = np.where(mx == mn, 0.0, n2)
    with np.errstate(divide="ignore"):
        inv = np.where(ok & (n2 > 0), 1.0 / np.sqrt(np.where(n2 > 0, n2, 1.0)), 0.0)
    if mutate == "unsigned" and operand == "q":
        w = w + 128
    return w, S, m * inv, s * inv, inv, Kf


def model_scores(Uq, MMq, Uc, MMc, mutate=None):
    """[Q, N] float64 by the contract's formula; mutate in MUTATIONS (or None: the contract itself)."""
    K = np.asarray(Uq).shape[1]
    wq, Sq, aq, bq, iq, Kf = _row_stats(Uq, MMq, K, mutate, "q")
    wc, Sc, ac, bc, ic, _ = _row_stats(Uc, MMc, K, mutate, "c")
    P = wq @ wc.T                                              # exact in int64
    t = (int(Kf) * P - np.outer(Sq, Sc)).astype(np.float64)    # |t| < 2^49: exact
    cos = Kf * np.outer(aq, ac) + np.outer(bq, bc) * t / Kf
    return np.where(np.outer(iq, ic) != 0, (cos + 1.0) / 2.0, 0.0)


# ---- row families --------------------------------------------------------------------------------------

FAMILIES = ("symmetric", "mn0", "negative", "one255", "narrow1000", "pm1e-30", "subnormal", "fltmax", "skewed",
            "const_pos", "const_neg", "const_zero", "nonfinite")


@lru_cache(maxsize=None)
def family(name, K, seed=1):
    """(U [4, K] u8, MM [4, 2] f32), read-only: four rows of one family."""
    rng = np.random.default_rng([seed, K, FAMILIES.index(name)])
    R = 4
    U = rng.integers(0, 256, (R, K), dtype=np.uint8)
    f = np.float32
    if name == "symmetric":
        MM = [(-1, 1), (-0.5, 0.5), (-3, 3), (-100, 100)]
    elif name == "mn0":
        MM = [(0, 1), (0, 255), (0, 1e-3), (0, 7.5)]
    elif name == "negative":
        MM = [(-2, -1), (-255, -1e-3), (-1e4, -9e3), (-1, -0.999)]
    elif name == "one255":
        U[:] = 0
        U[np.arange(R), rng.integers(0, K, R)] = 255
        MM = [(0, 1), (0, 255), (-1, 1), (0, 1e-20)]
    elif name == "narrow1000":
        MM = [(1000, 1000.001)] * R
    elif name == "pm1e-30":
        MM = [(-1e-30, 1e-30), (-1e30, 1e30), (0, 1e-30), (-1e30, 0)]
    elif name == "subnormal":
        MM = [(-SUBNORMAL, SUBNORMAL), (0, SUBNORMAL), (-SUBNORMAL, 0), (f(1e-45), f(3e-45))]
    elif name == "fltmax":
        MM = [(-FLT_MAX, FLT_MAX), (0, FLT_MAX), (-FLT_MAX, 0), (f(3e38), FLT_MAX)]
    elif name == "skewed":
        U = np.minimum(rng.geometric(0.2, (R, K)), 255).astype(np.uint8)   # mostly small bytes
        U[2:] = 255 - U[2:]                                                # mostly large bytes
        MM = [(-1, 1), (0, 1), (-1, 1), (-5, -1)]
    elif name == "const_pos":
        MM = [(2.5, 2.5), (1e-30, 1e-30), (FLT_MAX, FLT_MAX), (1, 1)]
    elif name == "const_neg":
        MM = [(-2.5, -2.5), (-1e-30, -1e-30), (-FLT_MAX, -FLT_MAX), (-1, -1)]
    elif name == "const_zero":
        MM = [(0, 0), (0.0, -0.0), (-0.0, 0.0), (0, 0)]
        U[3] = 128
    elif name == "nonfinite":
        MM = [(np.nan, 1), (0, np.inf), (-np.inf, np.inf), (np.nan, np.nan)]
    else:
        raise KeyError(name)
    MM = np.array(MM, dtype=np.float32)
    assert MM.shape == (R, 2)
    U.setflags(write=False)
    MM.setflags(write=False)
    return U, MM


@lru_cache(maxsize=None)
def all_families(K, seed=1):
    """Every family's rows stacked: (U [4 F, K], MM [4 F, 2], names [4 F])."""
    parts = [family(n, K, seed) for n in FAMILIES]
    U = np.concatenate([p[0] for p in parts])
    MM = np.concatenate([p[1] for p in parts])
    names = [n for n in FAMILIES for _ in range(4)]
    U.setflags(write=False)
    MM.setflags(write=False)
    return U, MM, names


def rows_of(names, fam):
    return np.array([i for i, n in enumerate(names) if n in fam], dtype=np.int64)


# ---- the GPU test's inputs -------------------------------------------------------------------------------


def operand_map_rows(R, K, which):
    """Asymmetric integer bytes, different for queries (which = 0) and frames (1); (mn, mx) = (0, 255): x = u."""
    r = np.arange(R, dtype=np.int64)[:, None]
    k = np.arange(K, dtype=np.int64)[None, :]
    U = ((7 * r + 3 * k + r * k + 1) % 256) if which == 0 else ((11 * r + 5 * k + 3 * r * k + 2 * (k // 16) + 9) % 256)
    MM = np.tile(np.array([[0, 255]], np.float32), (R, 1))
    return U.astype(np.uint8), MM


@lru_cache(maxsize=None)
def random_rows(R, K, seed):
    """Seeded rows of mixed ranges (symmetric, one-sided, shifted), read-only."""
    rng = np.random.default_rng([seed, R, K])
    U = rng.integers(0, 256, (R, K), dtype=np.uint8)
    lo = rng.uniform(-2, 1, R)
    MM = np.stack([lo, lo + rng.uniform(0.1, 3, R)], axis=1).astype(np.float32)
    U.setflags(write=False)
    MM.setflags(write=False)
    return U, MM


# (name, Q, N, K, ld, base offset): every K, N and Q edge (a step, a tile, a workgroup, one past each) appears at least once; ld > K twice,
# the unaligned generic path twice (ld = 20, and a base one byte off an aligned ld)
SHAPES = (
    ("K1", 1, 1, 1, 1, 0),
    ("K15", 127, 383, 15, 15, 0),
    ("K16-ld20", 128, 384, 16, 20, 0),
    ("K63", 129, 385, 63, 63, 0),
    ("K64-ld72", 129, 769, 64, 72, 0),
    ("K64-base1", 127, 385, 64, 64, 1),
    ("K65", 128, 769, 65, 65, 0),
    ("K4096", 1, 385, 4096, 4096, 0),
    ("K4096-ld4160", 129, 383, 4096, 4160, 0),
)


def strided(U, ld, off):
    """The flat buffer that holds U's rows ld bytes apart starting at byte `off` (gaps filled with 0xA5, which
    a kernel reading outside its K bytes would fold into the sums)."""
    R, K = U.shape
    buf = np.full(off + R * ld + 16, 0xA5, np.uint8)
    for r in range(R):
        buf[off + r * ld: off + r * ld + K] = U[r]
    return buf


def accumulator_rows():
    """K = 65536: all 0, all 255, alternating 0 / 255 (both phases), plus seeded rows; as queries and frames they
    give P = +-2^30 ((-128)^2 K = 2^30; 127 * -128 K the most negative sum)."""
    K, R = MAX_K, 16
    U = random_rows(R, K, 77)[0].copy()
    U[0] = 0
    U[1] = 255
    U[2, 0::2], U[2, 1::2] = 0, 255
    U[3, 0::2], U[3, 1::2] = 255, 0
    MM = np.array([(-1, 1), (0, 1), (-2, 0.5), (1, 3)] * 4, np.float32)
    return U, MM


def reference_topk(scores, k, thr, mode, id_base=0):
    """hq_select_topk's rule in NumPy: passing frames by (score desc, id asc), -inf / -1 padded."""
    scores = np.asarray(scores, np.float64)
    Q, N = scores.shape
    os_ = np.full((Q, k), -np.inf)
    oi = np.full((Q, k), -1, np.int64)
    for q in range(Q):
        row = scores[q]
        ok = np.ones(N, bool) if mode == 0 else (row >= thr if mode == 1 else row > thr)
        ids = np.flatnonzero(ok)
        ids = ids[np.lexsort((ids, -row[ids]))][:k]
        os_[q, :len(ids)] = row[ids]
        oi[q, :len(ids)] = ids + id_base
    return os_, oi
