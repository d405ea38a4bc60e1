"""Case tables of the scorer sweep over index length (the exact scorers and re-rank kernels of hq_search.hip),
NumPy and the CPU oracle's level structure only.

tests/golden/make_golden.py runs the real reference's compare_indices_at_level, _calculate_overall_similarity,
progressive_search and brute_force_search over these tables and writes tests/golden/scorer_sweep.npz;
tests/test_scorer_sweep_cpu.py pins the oracle to that file; tests/test_gpu_scorer_sweep.py compares the kernels
with the oracle over the same lengths.  The golden file keeps an 8-byte digest of every length's inputs, so a
generator that drifts fails loudly; score tables are digests too, full arrays at LS_FULL.

Lengths.  The exact scorers branch on the segment lengths of the level structure (O.segment_bounds):
NumPy's sum is a plain loop below 8 values, an eight-accumulator leaf up to 128, a recursive split above, and
the kernels take single-leaf forms while every segment has at most 128 values.  LS_SWEEP has every L in 2..140
(every segment length 1..70, both parities, the cooperative re-rank's piece counts 6 -> 10 at L = 76 / 78 and
10 -> none at 140 / 142).  LS_EDGE adds: the first length with a segment above 128 values (214: last segment
129), the level-0 segment crossing 128 (256 / 258), the fused f64 overall scan's 256 padded values (252 / 254),
the staged re-rank's 96 KiB of LDS (a list of 64: L = 160 / 162; of 28: L = 378 / 380), the fused level-0
scan's 256 values and the seventh segment (1022 / 1024: a record wider than the cooperative kernels take), and
4096 / 4098 on both sides of the append-in-place limit.  L = 1 has no level structure (one case of its own)."""
import numpy as np

from index_sweep_cases import digest, digest_row  # noqa: F401  (re-exported: one digest scheme for both sweeps)
from oracle import hq_oracle as O

SEED = 771903
LS_SWEEP = list(range(2, 141))
LS_EDGE = [141, 142, 143, 159, 160, 161, 162, 212, 213, 214, 215, 252, 253, 254, 255, 256, 257, 258, 259, 300, 378,
           379, 380, 511, 512, 513, 1000, 1022, 1023, 1024, 1025, 2048, 2050, 4095, 4096, 4097, 4098]
LS = LS_SWEEP + LS_EDGE
LS_FULL = [2, 7, 66, 214, 258, 1025]           # score tables stored in full
# one length per routing class of IndexCorpus: split level-0 + split overall scans (16, 64), one-value segments
# (2, 3), odd L (33, 255: f64 fused scans only), even L past the split level-0 scan (66, 142, 214), level 0
# above 128 values (258), dense only (1025), append by rebuild (4098)
LS_SEARCH = [2, 3, 16, 33, 64, 66, 142, 214, 255, 258, 1025, 4098]
N_ROWS, N_QUERIES, N_POOL, TOP_K, M_GOLDEN = 24, 6, 40, 10, 20
COMBOS = ("c64", "c32", "q64c32", "mix")     # q64 c64, q32 c32, q64 c32, q32 against odd rows widened


def _rows(L: int, dt, n: int, seed: int) -> np.ndarray:
    """n >= 24 index vectors of dtype dt: seeded N(0, 1) with the degenerate rows in front."""
    rng = np.random.default_rng(seed)
    f = dt
    C = rng.standard_normal((n, L)).astype(dt)
    b = O.segment_bounds(L)
    j = rng.integers(0, L, 3)
    C[20] = C[20] * f(3.0) + f(0.5)                    # (query 1 is a copy of this row)
    C[21] = C[21] * f(0.01)
    C[1] = 0.0
    C[2] = f(0.1)                                      # an inexact constant
    C[3] = f(0.5)                                      # an exact constant
    C[4] = C[10]                                       # a duplicate
    C[5] = -C[20]                                      # the negation of query 1: the clamp at 0
    C[6, b[0][0]:b[0][1]] = f(0.25)                    # a constant level-0 segment
    C[7, b[-1][0]:b[-1][1]] = f(-3.0)                  # a constant last segment
    C[8] = C[12] * f(2.0) + f(1.0)                     # an affine copy: correlation 1
    C[9] = f(1.7)
    C[9, j] = np.nextafter(f(1.7), f(2))               # a 1-ulp near-constant
    C[13] = (1000.0 + rng.standard_normal(L) * 1e-3).astype(dt)   # a large mean / std ratio
    C[14] = C[13] + f(0.001)
    C[15] = np.where(np.arange(L) % 2 == 0, f(1e-25), f(2e-25))   # d * d underflows in float32
    C[16] = (rng.standard_normal(L) * 1e-20).astype(dt)           # squares in the float32 denormal range
    C[17] = (rng.standard_normal(L) * 1e25).astype(dt)            # squares overflow in float32
    C[18] = C[9]
    C[18, 0] = np.nextafter(f(1.7), f(0))
    C[19] = f(0.1)
    C[19, ::5] = np.nextafter(f(0.1), f(1))
    # every square rounds to zero or to one subnormal unit u: t * t = u / 2.  In a segment of even length the mean
    # of squares is u / 2 -> 0 (ties to even) while every squared deviation rounds up to u: std != 0 with
    # np.mean(x ** 2) == 0, the `max_possible_mse > 0` test of the scorer failing in its general branch
    t = np.sqrt(float(np.finfo(dt).smallest_subnormal)) * np.sqrt(0.5)   # (u / 2 itself is not a float64)
    for r, (hi, lo) in ((22, (1.2, 0.9)), (23, (1.25, 0.85))):
        for (s, e) in b:
            C[r, s:e] = np.where(np.arange(e - s) % 2 == 0, f(hi * t), f(-lo * t))
    return C


def make_rows(L: int):
    """{"C64", "Q64", "C32", "Q32"}: 24 rows and 6 queries of length L in float64 and in float32."""
    out = {}
    for tag, dt, k in (("64", np.float64, 0), ("32", np.float32, 1)):
        C = _rows(L, dt, N_ROWS, SEED + 2 * L + k)
        rng = np.random.default_rng(SEED + 100003 * (k + 1) + L)
        Q = np.stack([C[10] + rng.normal(0, 0.01, L).astype(dt), C[20], np.full(L, 0.5, dt), C[22], C[2], C[6]])
        out["C" + tag], out["Q" + tag] = C, Q
    return out


def make_pool(L: int):
    """The search pools of length L: the 24 rows, 16 noisy copies of query rows behind them (so the level
    filter has something to rank), the 6 queries; float64 and float32."""
    out = {}
    for tag, dt, k in (("64", np.float64, 0), ("32", np.float32, 1)):
        C = _rows(L, dt, N_POOL, SEED + 2 * L + k)
        rng = np.random.default_rng(SEED + 200003 * (k + 1) + L)
        for i in range(N_ROWS, N_POOL):
            src = (10, 20, 0, 12)[i % 4]
            C[i] = C[src] + rng.normal(0, 0.02 * (1 + i - N_ROWS), L).astype(dt)
        C[N_POOL - 1] = C[N_POOL - 2]                      # a tie decided by the pool order
        Q = np.stack([C[10] + rng.normal(0, 0.01, L).astype(dt), C[20], np.full(L, 0.5, dt),
                      rng.standard_normal(L).astype(dt), C[2], C[12] + rng.normal(0, 0.05, L).astype(dt)])
        out["C" + tag], out["Q" + tag] = C, Q
    return out


def inputs_digest(rows) -> np.ndarray:
    return digest_row(np.concatenate([rows[k].astype(np.float64).ravel() for k in ("C64", "Q64", "C32", "Q32")]))


def combo_inputs(rows, combo: str):
    """(queries, [candidate row, ...]) of a dtype combination: what the reference's scorer is handed."""
    C32, C64 = rows["C32"], rows["C64"]
    if combo == "c64":
        return rows["Q64"], list(C64)
    if combo == "c32":
        return rows["Q32"], list(C32)
    if combo == "q64c32":
        return rows["Q32"].astype(np.float64), list(C32)
    if combo == "mix":
        return rows["Q32"], [C32[b] if b % 2 == 0 else C32[b].astype(np.float64) for b in range(len(C32))]
    raise KeyError(combo)


def mix_flags(n: int) -> np.ndarray:
    """Per-row float32 flags of the mixed pool: even rows float32, odd rows widened to float64."""
    return np.arange(n) % 2 == 0


def _by_dtype(fn, Q, rows):
    """fn(q, C) [N, ...] for every query against a row list of one length that may mix dtypes."""
    is32 = np.array([r.dtype == np.float32 for r in rows])
    outs = []
    for q in Q:
        res = None
        for flag, dt in ((True, np.float32), (False, np.float64)):
            sel = np.nonzero(is32 == flag)[0]
            if len(sel) == 0:
                continue
            v = fn(q, np.stack([rows[i] for i in sel]).astype(dt))
            if res is None:
                res = np.zeros((len(rows),) + v.shape[1:], dtype=v.dtype)
            res[sel] = v
        outs.append(res)
    return np.stack(outs)


def oracle_tables(Q, rows):
    """The oracle's score table of a combination: values f64 [Q, N, nseg + 2] = levels 0 .. nseg - 1, the level
    nseg (past the structure: 0.0) and the overall score; types u8 (1: the reference returns a numpy float32)."""
    L = len(rows[0])
    nseg = len(O.segment_bounds(L))
    with np.errstate(all="ignore"):
        lv = [_by_dtype(lambda q, C, l=l: O.level_similarity(q, C, l), Q, rows) for l in range(nseg + 1)]
        ov = _by_dtype(lambda q, C: O.overall_similarity(q, C)[0], Q, rows)
    val = np.stack(lv + [ov], axis=2)
    both32 = np.array([q.dtype == np.float32 for q in Q])[:, None] & np.array([r.dtype == np.float32 for r in rows])
    ty = np.zeros(val.shape, np.uint8)
    for l in range(nseg + 1):
        ty[:, :, l] = both32 & O.level_types(val[:, :, l], True)
    # the overall sum is float32 once a float32 level score entered it (O.overall_similarity); its clamp returns
    # the Python floats 0.0 / 1.0 (core/search_engine.py:228)
    ty[:, :, nseg + 1] = ty[:, :, :nseg].any(axis=2) & ~np.isin(val[:, :, nseg + 1], (0.0, 1.0))
    return val, ty


BRANCHES = ("both_equal", "both_differ", "one", "general", "clamp0", "maxmse0")


def branches(q, c, s: int, e: int):
    """The branches of compare_indices_at_level (core/search_engine.py:137-189) one pair takes on the segment
    [s, e), from NumPy's own statistics in each side's dtype: a set of BRANCHES names."""
    qv, cv = q[s:e], c[s:e]
    with np.errstate(all="ignore"):
        qs, cs = np.std(qv), np.std(cv)
        if qs == 0 and cs == 0:
            return {"both_equal" if abs(np.mean(qv) - np.mean(cv)) < 1e-6 else "both_differ"}
        if qs == 0 or cs == 0:
            return {"one"}
        out = {"general"}
        mx = np.mean(qv ** 2) + np.mean(cv ** 2)
        if not mx > 0:
            out.add("maxmse0")
        elif not 1.0 - np.mean((qv - cv) ** 2) / mx > 0.0:
            out.add("clamp0")
        return out


RAW_LENGTHS = list(range(1, 301)) + [659, 1024, 1025, 2731, 2733]


def raw_segment_rows(m: int, dt):
    """(q [m], C [14, m]) of dtype dt: one raw level segment and candidates of the same length (the raw-segment
    scorer of pools of mixed index length): random rows and the degenerate ones of the tables."""
    rng = np.random.default_rng(SEED + 7 * m + (1 if dt == np.float32 else 0))
    f = dt
    q = rng.standard_normal(m).astype(dt)
    C = rng.standard_normal((14, m)).astype(dt)
    C[1] = 0.0
    C[2] = f(0.1)
    C[3] = f(0.5)
    C[4] = q
    C[5] = -q
    C[6] = q * f(2.0) + f(1.0)
    C[7] = f(1.7)
    C[7, rng.integers(0, m, 2)] = np.nextafter(f(1.7), f(2))
    C[8] = (1000.0 + rng.standard_normal(m) * 1e-3).astype(dt)
    C[9] = np.where(np.arange(m) % 2 == 0, f(1e-25), f(2e-25))
    C[10] = (rng.standard_normal(m) * 1e-20).astype(dt)
    C[11] = (rng.standard_normal(m) * 1e25).astype(dt)
    return q, C


def raw_pair_scores(q, C) -> np.ndarray:
    """compare_indices_at_level on raw segments, pair by pair in NumPy's own operations (each side's statistics in
    its dtype, Python's max / min): float64 [N]."""
    with np.errstate(all="ignore"):
        return np.array([float(O.precomputed_level_similarity(q, c)) for c in C])


def seg_class(m: int) -> str:
    """NumPy's summation form for m values: a plain loop, one eight-accumulator leaf, a recursive split."""
    return "lt8" if m < 8 else ("leaf" if m <= 128 else "split")
