"""Cases for the frame-cosine and RAG scoring stage: hq_cos_prepare + hq_cos_scores_mfma
(hq_cosine.hip), hq_cosine_scores / hq_cosine_scores_dt, hq_detect_heights, hq_spatial_locality and
hq_threshold_select (hq_rag.hip).  Plain NumPy, imported by test_cos_rag_cases_cpu.py (which proves that the
cases discriminate) and test_gpu_cos_rag_edges.py (which runs them on the kernels).

* exact references: float32 products are exact in float64 and math.fsum adds them exactly, so fsum_scores
  is the cosine to an ulp; exact_scores is the same contraction in np.longdouble (64-bit mantissa: every
  float32 product exact, K additions each within 2^-64), fast enough for 17 x 130 x 16384, and the CPU test
  checks it against fsum_scores pair by pair.  The zero rule is the reference's (rag/search/engine.py:654-660):
  0.0 iff a norm is 0, else (cos + 1) / 2, NaN propagated.
* model_scores: a NumPy model of the MFMA route's arithmetic (frexp scale, hi / lo f16 split, f64 inverse
  norm, per 32-K step hi.hi, hi.lo, lo.hi added to a float32 accumulator, epilogue) with switches for the
  mutations the CPU test applies.  GPU results are never compared with it.
* row families for the MFMA cosine, shapes and values for the four hq_rag.hip entry points."""
import math
import os
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_FILE = os.path.join(ROOT, "profiles", "cos_error_bounds.txt")

# ---------------------------------------------------------------------------------------------------------
# exact references
# ---------------------------------------------------------------------------------------------------------

_WIDE = np.finfo(np.longdouble).nmant >= 63


def _rule(dot, na2, nb2):
    """(cos + 1) / 2 from a dot product and two squared norms; 0.0 iff a norm is 0; NaN / inf propagate."""
    dot, na2, nb2 = np.broadcast_arrays(dot, na2, nb2)
    with np.errstate(all="ignore"):
        cs = dot / (np.sqrt(na2) * np.sqrt(nb2))
        return np.where((na2 == 0) | (nb2 == 0), 0.0, (cs + 1) / 2).astype(np.float64)


def fsum_scores(A, B, pairs=None):
    """Exact (cos + 1) / 2 of float32 rows: float64 products (exact), math.fsum.  pairs: [(q, n), ...] to
    compute (default all) -> {(q, n): score}.  Rows with a NaN or inf take NumPy's float64 sum (the result is
    NaN either way)."""
    assert A.dtype == np.float32 and B.dtype == np.float32
    a64, b64 = A.astype(np.float64), B.astype(np.float64)
    if pairs is None:
        pairs = [(q, n) for q in range(A.shape[0]) for n in range(B.shape[0])]
    out = {}
    for q, n in pairs:
        a, b = a64[q], b64[n]
        if np.isfinite(a).all() and np.isfinite(b).all():
            d, x, y = math.fsum((a * b).tolist()), math.fsum((a * a).tolist()), math.fsum((b * b).tolist())
        else:
            with np.errstate(all="ignore"):
                d, x, y = float(np.sum(a * b)), float(np.sum(a * a)), float(np.sum(b * b))
        out[(q, n)] = float(_rule(d, x, y))
    return out


def _fraction_scores(A, B):
    out = np.zeros((A.shape[0], B.shape[0]))
    fa = [[Fraction(float(v)) for v in r] for r in A]
    fb = [[Fraction(float(v)) for v in r] for r in B]
    na = [sum(v * v for v in r) for r in fa]
    nb = [sum(v * v for v in r) for r in fb]
    for q, ra in enumerate(fa):
        for n, rb in enumerate(fb):
            if na[q] == 0 or nb[n] == 0:
                continue
            d = sum(x * y for x, y in zip(ra, rb))
            # cos^2 as an exact fraction, one rounding, one square root
            c = math.sqrt(float(d * d / (na[q] * nb[n])))
            out[q, n] = ((c if d >= 0 else -c) + 1.0) / 2.0
    return out


def exact_scores(A, B):
    """(cos + 1) / 2 of every row of A [Q, K] against every row of B [N, K] (float32 or float64) -> f64 [Q, N],
    in np.longdouble (x87 extended: float32 products exact, sums within K 2^-64; float64 products within
    2^-64 each); where long double is no wider than double, exact rational arithmetic on finite rows."""
    A, B = np.asarray(A), np.asarray(B)
    if A.shape[1] == 0:
        return np.zeros((A.shape[0], B.shape[0]))
    if not _WIDE and np.isfinite(A).all() and np.isfinite(B).all():
        return _fraction_scores(A, B)
    a, b = A.astype(np.longdouble), B.astype(np.longdouble)
    with np.errstate(all="ignore"):
        dot = a @ b.T
        na2, nb2 = np.sum(a * a, axis=1), np.sum(b * b, axis=1)
    return _rule(dot, na2[:, None], nb2[None, :])


def detect_height_exact(img):
    """engine.py:134-162 in integers: the last row with 2 zeros < W ends the embedding; H if none."""
    H, W = img.shape
    ok = [r for r in range(H) if 2 * int(np.count_nonzero(img[r] == 0)) < W]
    return ok[-1] + 1 if ok else H


def spatial_exact(e1, e2):
    """engine.py:604-714 on two enhanced images: heights, window plan, exact window cosines, exact mean."""
    h1, h2 = detect_height_exact(e1), detect_height_exact(e2)
    if h1 != h2:
        return 0.0
    a, b = e1[:h1], e2[:h1]
    h, W = a.shape
    ws, st, nw = window_plan(h, W)
    if ws < 2:
        return float(exact_scores(a.reshape(1, -1), b.reshape(1, -1))[0, 0])
    s = [float(exact_scores(a[i:i + ws, j:j + ws].reshape(1, -1), b[i:i + ws, j:j + ws].reshape(1, -1))[0, 0])
         for i in range(0, h - ws + 1, st) for j in range(0, W - ws + 1, st)]
    assert len(s) == nw
    return math.fsum(s) / nw


# ---------------------------------------------------------------------------------------------------------
# NumPy model of the MFMA route (CPU test only)
# ---------------------------------------------------------------------------------------------------------


def model_prepare(X, scale="ldexp"):
    """k_cos_prepare's arithmetic: amax (NaN ignored, as fmaxf), e = frexp exponent (0 for a zero row),
    v = s x with s = 2^-e, hi = f16(v), lo = f16(v - hi), inv = 1 / (s |x|) from the f64 norm.
    scale "mul": x * ldexpf(1, -e) and 1 / (s sqrt(ss)), the expression before the fix (s overflows to inf for
    a subnormal amax); "ldexp": ldexpf(x, -e) and ldexp(1 / sqrt(ss), e).  -> hi, lo (float32 holding f16
    values), inv (f64)."""
    X = np.asarray(X, np.float32)
    with np.errstate(all="ignore"):
        amax = np.fmax.reduce(np.abs(X), axis=1, initial=np.float32(0))
        e = np.where(amax > 0, np.frexp(amax)[1], 0).astype(np.int32)
        ss = np.sum(X.astype(np.float64) ** 2, axis=1)
        if scale == "mul":
            s = np.ldexp(np.float32(1), -e).astype(np.float32)
            v = (X * s[:, None]).astype(np.float32)
            inv = np.where(ss > 0, 1.0 / (s.astype(np.float64) * np.sqrt(ss)), 0.0)
        else:
            v = np.ldexp(X, -e[:, None]).astype(np.float32)
            inv = np.where(ss > 0, np.ldexp(1.0 / np.sqrt(ss), e), 0.0)
        hi = v.astype(np.float16).astype(np.float32)
        lo = (v - hi).astype(np.float16).astype(np.float32)
    return hi, lo, inv


def _rtz32(t):
    """float64 -> float32 rounded toward zero."""
    r = t.astype(np.float32)
    over = np.abs(r.astype(np.float64)) > np.abs(t)
    return np.where(over, np.nextafter(r, np.float32(0)), r)


def model_scores(A, B, scale="ldexp", drop=(), zero_lo=False, trunc=False):
    """The MFMA route's scores in NumPy.  Per 32-K step the partial sums of hi.hi, hi.lo, lo.hi are formed in
    float64 and added, in that order, to one float32 accumulator (np.cumsum in float32: sequential adds);
    epilogue (acc inv_a inv_b + 1) / 2, 0 where an inverse norm is 0.  Mutations: drop = subset of
    ("hl", "lh") leaves those terms out, zero_lo clears both lo planes, trunc makes every accumulator add
    round toward zero."""
    ha, la, ia = model_prepare(A, scale)
    hb, lb, ib = model_prepare(B, scale)
    if zero_lo:
        la, lb = np.zeros_like(la), np.zeros_like(lb)
    Q, K = ha.shape
    N = hb.shape[0]
    S = (K + 31) // 32

    def steps(x):  # [rows, K] -> [S, rows, 32] float64, zero padded
        p = np.zeros((x.shape[0], S * 32))
        p[:, :K] = x
        return p.reshape(x.shape[0], S, 32).transpose(1, 0, 2)

    sa_h, sa_l, sb_h, sb_l = steps(ha), steps(la), steps(hb), steps(lb)
    terms = [("hh", sa_h, sb_h), ("hl", sa_h, sb_l), ("lh", sa_l, sb_h)]
    terms = [t for t in terms if t[0] not in drop]
    with np.errstate(all="ignore"):
        seq = np.stack([np.matmul(x, y.transpose(0, 2, 1)) for _, x, y in terms], axis=1)  # [S, T, Q, N]
        seq = seq.reshape(S * len(terms), Q, N)
        if trunc:
            acc = np.zeros((Q, N), np.float32)
            for p in seq:
                acc = _rtz32(acc.astype(np.float64) + p)
        else:
            acc = np.cumsum(seq, axis=0, dtype=np.float32)[-1]
        cs = acc.astype(np.float64) * ia[:, None] * ib[None, :]
        return np.where((ia[:, None] != 0) & (ib[None, :] != 0), (cs + 1.0) / 2.0, 0.0)


# ---------------------------------------------------------------------------------------------------------
# row families for the MFMA cosine: builder(Q, N, K, seed) -> A [Q, K], B [N, K] float32
# ---------------------------------------------------------------------------------------------------------

MFMA_Q, MFMA_N = 17, 130            # ragged against the 16-row fragment tile and the 128-row frame tile
MFMA_KS = (1000, 4096, 16384)       # not a multiple of 32; 64 x 64; the largest frame the docs name, 128 x 128
HARD_CAP = 1e-5                     # include/hq_mi355x.h, DESIGN.md §4.5
NAN_ROWS = {"nan_row": ((3,), (77,)), "inf_row": ((), (129,))}  # family -> (query rows, frame rows) affected


def _rng(seed, *salt):
    return np.random.default_rng([seed, *salt])


def _normal(Q, N, K, seed):
    r = _rng(seed, 1)
    return r.standard_normal((Q, K)).astype(np.float32), r.standard_normal((N, K)).astype(np.float32)


def _pos_uniform(Q, N, K, seed):
    r = _rng(seed, 2)
    return r.uniform(0.5, 1, (Q, K)).astype(np.float32), r.uniform(0.5, 1, (N, K)).astype(np.float32)


def _near_const(Q, N, K, seed):
    r = _rng(seed, 3)
    return ((0.7 + r.uniform(0, 1e-3, (Q, K))).astype(np.float32),
            (0.9 + r.uniform(0, 1e-3, (N, K))).astype(np.float32))


def _u8_frames(Q, N, K, seed):
    r = _rng(seed, 4)
    return r.integers(0, 256, (Q, K)).astype(np.float32), r.integers(0, 256, (N, K)).astype(np.float32)


def _antiparallel(Q, N, K, seed):
    r = _rng(seed, 5)
    A = r.standard_normal((Q, K)).astype(np.float32)
    c = r.uniform(0.5, 2.0, (N, 1)).astype(np.float32)
    return A, (-A[np.arange(N) % Q] * c).astype(np.float32)  # frame n = -c_n a_(n mod Q): score 0 on those pairs


def _orthogonal(Q, N, K, seed):
    r = _rng(seed, 6)
    A, B = r.standard_normal((Q, K)).astype(np.float32), r.standard_normal((N, K)).astype(np.float32)
    A[:, 1::2] = 0.0  # queries live on even k, frames on odd k: every dot product is exactly 0
    B[:, 0::2] = 0.0
    return A, B


def _spike(Q, N, K, seed):
    r = _rng(seed, 7)
    A, B = r.standard_normal((Q, K)).astype(np.float32), r.standard_normal((N, K)).astype(np.float32)
    for X, off in ((A, 0), (B, 5)):  # one element 2^12 (even rows) or 2^20 (odd rows) times the rest
        rows = np.arange(X.shape[0])
        pos = (37 * rows + off) % K
        mag = np.where(rows % 2 == 0, 2.0 ** 12, 2.0 ** 20) * r.uniform(1, 2, X.shape[0])
        X[rows, pos] = (mag * np.where(r.random(X.shape[0]) < 0.5, -1, 1)).astype(np.float32)
    return A, B


def _tiny_normal(Q, N, K, seed):
    r = _rng(seed, 8)
    return ((r.standard_normal((Q, K)) * 1e-30).astype(np.float32),
            (r.standard_normal((N, K)) * 1e-30).astype(np.float32))


SUB_LIMIT = 2.0 ** -128


def _subnormal(Q, N, K, seed):
    r = _rng(seed, 9)
    top = SUB_LIMIT - 2.0 ** -149

    def rows(n):  # every |x| < 2^-128 (subnormal: multiples of 2^-149)
        return np.clip(r.standard_normal((n, K)) * 2.0 ** -131, -top, top).astype(np.float32)

    return rows(Q), rows(N)


def _huge(Q, N, K, seed):
    r = _rng(seed, 10)

    def rows(n):  # amax in [2^127, 1.99 x 2^127) < FLT_MAX
        u = r.uniform(-1, 1, (n, K))
        return (u / np.max(np.abs(u), axis=1, keepdims=True) * r.uniform(1.0, 1.99, (n, 1)) * 2.0 ** 127).astype(np.float32)

    return rows(Q), rows(N)


def _nan_row(Q, N, K, seed):
    A, B = _normal(Q, N, K, seed + 100)
    (qa,), (nb,) = NAN_ROWS["nan_row"]
    A[qa % Q, 100 % K] = np.nan
    B[nb % N, 5 % K] = np.nan
    return A, B


def _inf_row(Q, N, K, seed):
    A, B = _normal(Q, N, K, seed + 200)
    B[NAN_ROWS["inf_row"][1][0] % N, 9 % K] = np.inf
    return A, B


FAMILIES = {
    "normal": _normal, "pos_uniform": _pos_uniform, "near_const": _near_const, "u8_frames": _u8_frames,
    "antiparallel": _antiparallel, "orthogonal": _orthogonal, "spike": _spike, "tiny_normal": _tiny_normal,
    "subnormal": _subnormal, "huge": _huge, "nan_row": _nan_row, "inf_row": _inf_row,
}
ROUTE_FAMILIES = ("tiny_normal", "subnormal", "huge", "pos_uniform")
ROUTE_SHAPE = (8, 128, 4096)  # Q N K = 2^22 = MFMA_COS_MIN_WORK; N = 127 is just below it


def build(family, Q=MFMA_Q, N=MFMA_N, K=4096, seed=0):
    A, B = FAMILIES[family](Q, N, K, seed)
    assert A.dtype == np.float32 and B.dtype == np.float32 and A.shape == (Q, K) and B.shape == (N, K)
    return A, B


def affected(family, Q, N):
    """Boolean [Q, N]: outputs of a row / column that holds a NaN or inf."""
    m = np.zeros((Q, N), bool)
    qa, nb = NAN_ROWS.get(family, ((), ()))
    for q in qa:
        m[q % Q, :] = True
    for n in nb:
        m[:, n % N] = True
    return m


# ---- measured per-family maxima (profiles/cos_error_bounds.txt) and the bounds derived from them ----------


def ceil_1sig(x):
    """x rounded up to one significant digit."""
    if x <= 0:
        return 0.0
    e = math.floor(math.log10(x))
    m = math.ceil(round(x / 10.0 ** e, 9))
    return float(f"{m}e{e}")


def measured():
    """{(family, K): measured max |MFMA score - exact score|} from profiles/cos_error_bounds.txt (lines
    '  family  K=nnn  value')."""
    out = {}
    with open(BOUNDS_FILE) as f:
        for line in f:
            p = line.split()
            if len(p) >= 3 and p[0] in FAMILIES and p[1].startswith("K="):
                out[(p[0], int(p[1][2:]))] = float(p[2])
    return out


def bound(family, K, table=None):
    """The asserted bound: twice the measured maximum rounded up to one significant digit (headroom for a kernel
    variant that associates differently; the kernel is deterministic), never above the contract's 1e-5."""
    table = measured() if table is None else table
    return min(HARD_CAP, ceil_1sig(2.0 * table[(family, K)]))


# ---------------------------------------------------------------------------------------------------------
# hq_spatial_locality: shapes and images
# ---------------------------------------------------------------------------------------------------------


def window_plan(h, W):
    """(ws, stride, windows) of engine.py:662-714 for an h x W embedding; ws < 2: one cosine over the block
    (stride 0, 0 windows)."""
    ws = min(4, h // 4, W // 4)
    if ws < 2:
        return ws, 0, 0
    st = ws // 2
    return ws, st, ((h - ws) // st + 1) * ((W - ws) // st + 1)


# (h, W, window side, stride, windows): the window side changes at h or W = 8, 12, 16; NumPy's pairwise sum
# changes path at 8 and at 128 elements.  With ws >= 2 both h and W are >= 8, so the smallest window count is
# (8, 8) -> 49 (the CPU test proves it): counts below 8, of 8 and of 9 do not exist, nor do 127 and 129;
# 126, 128 (twice) and 130 bracket the 128 split and 1192 is past 1024.
SPATIAL_SHAPES = (
    (1, 1, 0, 0, 0), (1, 8, 0, 0, 0), (3, 3, 0, 0, 0), (4, 19, 1, 0, 0), (7, 7, 1, 0, 0), (7, 16, 1, 0, 0),
    (8, 7, 1, 0, 0), (8, 8, 2, 1, 49), (8, 11, 2, 1, 70), (11, 8, 2, 1, 70), (11, 12, 2, 1, 110),
    (12, 11, 2, 1, 110), (12, 12, 3, 1, 100), (12, 15, 3, 1, 130), (15, 12, 3, 1, 130), (15, 16, 3, 1, 182),
    (16, 15, 3, 1, 182), (16, 16, 4, 2, 49), (16, 17, 4, 2, 49), (17, 16, 4, 2, 49), (17, 19, 4, 2, 56),
    (19, 17, 4, 2, 56), (19, 19, 4, 2, 64), (8, 19, 2, 1, 126), (9, 17, 2, 1, 128), (18, 34, 4, 2, 128),
    (11, 14, 2, 1, 130), (9, 150, 2, 1, 1192),
)


def index_rows(img, h):
    """Rows h.. of an enhanced image become index rows: two values, then zeros (more than half zeros wherever
    W >= 5; W < 5: all zeros)."""
    img[h:] = 0.0
    if img.shape[1] >= 5:
        img[h:, :2] = 0.25
    return img


def spatial_images(h, W, dtype, seed=0):
    """Queries [2, H, W] and stored images [4, H, W] with H = h + 2 index rows: stored 0 / 1 of height h, stored 2
    with a zero window at the top left (its windows with a zero norm score 0.0 inside the mean), stored 3 of
    another detected height (-> 0.0; h = 1: none lower exists, so it keeps h).  -> q, c, heights_q, heights_c."""
    r = _rng(seed, 20, h, W)
    H = h + 2
    q = r.standard_normal((2, H, W)).astype(dtype)
    c = r.standard_normal((4, H, W)).astype(dtype)
    c[1] = (q[0] + 0.1 * c[1]).astype(dtype)  # a near match
    ws = window_plan(h, W)[0]
    if ws >= 2:
        c[2, :ws, :ws] = 0.0
        q[1, :ws, -ws:] = -0.0
    hq, hc = [h, h], [h, h, h, h]
    for x in list(q) + list(c):
        index_rows(x, h)
    if h > 1:
        index_rows(c[3], h - 1)
        hc[3] = h - 1
    return q, c, hq, hc


def many_pair_images(dtype, seed=0):
    """6 distinct query and 5 distinct stored 8 x 8 images of differing detected height (8: 49 windows of side 2;
    7 and 4: the whole-block branch), and the index vectors that expand them to Q = 257 x N = 256 pairs: 65792
    pairs on 65536 workgroups, so workgroups 0 .. 255 score (0, n) and then (256, n).  Two query orders: in the
    first, queries 0 and 256 are different images of height 8 (two window lists in a row: a stale list shows); in
    the second, query 256 has height 4 (windows, then the whole-block branch).
    -> dq [6, 8, 8], dc [5, 8, 8], (iq, iq') [257] each, ic [256], heights."""
    r = _rng(seed, 21)
    hq, hc = (8, 7, 8, 4, 4, 7), (8, 7, 4, 8, 7)
    dq = r.standard_normal((6, 8, 8)).astype(dtype)
    dc = r.standard_normal((5, 8, 8)).astype(dtype)
    dc[3] = (dq[0] + 0.2 * dc[3]).astype(dtype)
    dc[0, :2, :2] = 0.0
    for x, h in list(zip(dq, hq)) + list(zip(dc, hc)):
        index_rows(x, h)
    iq2 = np.arange(257) % 6
    iq1 = iq2.copy()
    iq1[256] = 2
    return dq, dc, (iq1, iq2), (np.arange(256) * 3) % 5, hq, hc


# ---------------------------------------------------------------------------------------------------------
# hq_detect_heights: images whose rows sit on the zero-ratio boundary
# ---------------------------------------------------------------------------------------------------------

DETECT_H = (1, 2, 63, 64, 65, 200)  # 200 rows: more than the 64 threads
DETECT_W = (1, 2, 3, 7, 8, 64, 129)


def _zeros_in_row(r, W, z, dtype):
    row = (r.standard_normal(W) + 3.0).astype(dtype)  # no accidental zeros
    row[r.permutation(W)[:z]] = 0.0
    return row


def detect_images(H, W, dtype, seed=0):
    """[(name, image [H, W])]: z_no = ceil(W / 2) zeros is the fewest that does NOT end the embedding (exactly
    W / 2 at even W, (W + 1) / 2 at odd W), z_yes = z_no - 1 the most that does ((W - 1) / 2 at odd W)."""
    r = _rng(seed, 30, H, W)
    z_no = (W + 1) // 2
    z_yes = z_no - 1
    tiny = np.finfo(dtype).smallest_subnormal
    out = [("dense", (r.standard_normal((H, W)) + 3.0).astype(dtype)),
           ("all zero", np.zeros((H, W), dtype)),
           ("all -0.0", np.full((H, W), -0.0, dtype))]
    only0 = np.zeros((H, W), dtype)
    only0[0] = 1.0
    out.append(("only row 0", only0))
    for rs in sorted({0, H // 2, H - 1, min(H - 1, 150)}):
        img = (r.standard_normal((H, W)) + 3.0).astype(dtype)
        img[: rs][r.random(rs) < 0.3] = 0.0  # zero rows above the boundary do not matter
        img[rs] = _zeros_in_row(r, W, z_yes, dtype)
        for k in range(rs + 1, H):
            img[k] = _zeros_in_row(r, W, z_no if k % 2 else W, dtype)
        out.append((f"boundary row {rs}", img))
        neg = img.copy()
        neg[rs + 1:][neg[rs + 1:] == 0] = -0.0  # -0.0 counts as zero
        out.append((f"boundary row {rs}, -0.0", neg))
        sub = np.zeros((H, W), dtype)
        sub[rs] = tiny  # subnormals are not zero
        sub[rs, ::2] = -tiny
        out.append((f"subnormal row {rs}", sub))
        nan = np.zeros((H, W), dtype)
        nan[rs] = np.where(np.arange(W) < W - z_yes, np.nan, 0.0)  # NaN == 0 is false: exactly z_yes zeros
        out.append((f"nan row {rs}", nan))
    return out


# ---------------------------------------------------------------------------------------------------------
# hq_threshold_select
# ---------------------------------------------------------------------------------------------------------

SELECT_N = (1, 63, 64, 65, 128, 1000)
SELECT_THR = 0.5


def select_rows(N, seed=0):
    """[(name, scores [N] f64)] around SELECT_THR."""
    r = _rng(seed, 40, N)
    half = r.random(N)
    eq = np.where(r.random(N) < 0.5, SELECT_THR, np.nextafter(SELECT_THR, 0.0))  # equal passes, one ulp below fails
    odd = r.random(N)
    odd[r.random(N) < 0.3] = np.nan
    odd[r.random(N) < 0.1] = np.inf
    odd[r.random(N) < 0.1] = -np.inf
    sparse = np.where(r.random(N) < 0.05, 0.9, 0.1)
    return [("all pass", np.full(N, 0.75)), ("none pass", np.full(N, 0.25)), ("half", half), ("equal / ulp below", eq),
            ("nan and inf", odd), ("sparse", sparse), ("all nan", np.full(N, np.nan))]


def select_caps(N):
    """1; 37 and 100: the cut falls inside a 64-lane ballot word (all-pass rows: lanes 36 / 35); 64 and 128: on
    the last lane of one; N; past N."""
    return sorted({1, 37, 64, 100, 128, N, N + 5})


def select_expected(scores, ids, thr, cap):
    """The first `cap` positions (or ids) with score >= thr, -1 padded, and their number."""
    Q, N = scores.shape
    out = np.full((Q, cap), -1, np.int64)
    cnt = np.zeros(Q, np.int64)
    for q in range(Q):
        with np.errstate(invalid="ignore"):
            pos = np.nonzero(scores[q] >= thr)[0][:cap]
        out[q, : len(pos)] = pos if ids is None else ids[q, pos]
        cnt[q] = len(pos)
    return out, cnt
