"""Shared helpers of the scan contract tests (test_scan_contract_cpu.py, test_gpu_scan_contract.py).

Plain NumPy plus the CPU oracle; nothing here touches the GPU package.  Three things live here:

* `families` / `build_case`: adversarial level-0 segments and the corpora built from them.  Every family
  stresses one term of the error budget in the comment above kMarginF (hq_search.hip).
* `split_model_level0`: a NumPy emulation of the level-0 split-f16 scan as designed (second reference, for
  diagnosis: did a kernel leave its design, or is the design bound wrong?).
* `resolved_rule`: the re-rank's contract (hq_mi355x.h: hq_refine_topk; the comment above k_refine) written
  down once more, independently of the four kernels that implement it.
"""
import numpy as np

from oracle import hq_oracle as O

EPS = 2e-5            # IndexCorpus.EPS (the GPU tests assert the two are the same number)
B_SCAN0 = 5.5e-6      # documented bound of hq_scan0_topk_split (hq_mi355x.h)
B_SCANOV = 6e-6       # documented bound of hq_scanov_topk_split
B_F64_SHORT = 1e-12   # hq_scan_topk, L <= 64 (hq_mi355x.h)
B_F64_LONG = 1e-10    # hq_scan_topk, longer L: the suite's TOL (nothing tighter is documented)

FAMILIES = ("gauss", "outlier", "twoval", "bigmean", "cauchy", "lognorm", "sparse", "ramp", "tiny", "huge",
            "unsafe_tiny", "unsafe_huge", "const")
# level-0 segments the split scans flag: zero variance (bit 1), mean of squares outside [2^-60, 2^60] (bit 2)
FLAGGED = ("unsafe_tiny", "unsafe_huge", "const")
UNFLAGGED = tuple(f for f in FAMILIES if f not in FLAGGED)

# the completeness sweep: 0.3499 / 0.35 / 0.3501 put R = T' - 0.35 of gstar0 on both sides of zero
THRESHOLDS = (0.0, 0.1, 0.2, 0.3499, 0.35, 0.3501, 0.36, 0.5, 0.65, 0.8, 0.95, 0.999, 1.0)
LIST_LENGTHS = (8, 28, 64, 108, 1024)

# constant rows: a few values, so that constant pairs give both 1.0 (|mean difference| < 1e-6) and 0.0
_CONST_VALUES = np.array([0.0, 0.25, 0.25 + 5e-7, -3.0, 1000.0])


def families(m, n, rng):
    """{family: [n, m]} level-0 segments (any m >= 1)."""
    out = {}
    out["gauss"] = rng.standard_normal((n, m))
    x = 1e-3 * rng.standard_normal((n, m))
    x[np.arange(n), rng.integers(0, m, n)] = 10.0
    out["outlier"] = x                                   # one z ~ sqrt(m - 1), the others ~ -0.18
    a = rng.uniform(0.1, 5.0, (n, 1))
    sign = np.where(np.arange(m) < m // 2, 1.0, -1.0)
    out["twoval"] = a * rng.permuted(np.tile(sign, (n, 1)), axis=1)   # m even: z = +-1 exactly, lo = 0
    out["bigmean"] = 1000.0 + 1e-2 * rng.standard_normal((n, m))      # the qB * mn term dominates num
    out["cauchy"] = rng.standard_cauchy((n, m))
    out["lognorm"] = np.exp(3.0 * rng.standard_normal((n, m)))
    x = np.zeros((n, m))
    for i in range(n):
        pos = rng.choice(m, size=min(2, m), replace=False)
        x[i, pos] = rng.standard_normal(len(pos)) + np.sign(rng.standard_normal(len(pos)))
    out["sparse"] = x                                    # near-constant z plus two spikes
    # rising ramps: the same z in every row, scores near 1 (-q below covers the anti-correlated side)
    out["ramp"] = (0.05 + np.abs(rng.standard_normal((n, 1)))) * np.arange(m)[None, :] + 10.0 * rng.standard_normal((n, 1))
    out["tiny"] = rng.standard_normal((n, m)) * 2.0 ** -25           # msq near 2^-50: still unflagged
    out["huge"] = rng.standard_normal((n, m)) * 2.0 ** 25
    out["unsafe_tiny"] = rng.standard_normal((n, m)) * 2.0 ** -35    # msq ~ 2^-70: flag bit 2
    out["unsafe_huge"] = rng.standard_normal((n, m)) * 2.0 ** 35
    out["const"] = np.repeat(rng.choice(_CONST_VALUES, (n, 1)), m, axis=1)   # std 0: flag bit 1
    assert tuple(out) == FAMILIES
    return out


class Case:
    """A corpus C [N, L], its queries Q [nq, L] and the family of every row / query.  q_rows: the corpus row
    a query is a copy of (-1: the query is not in the corpus)."""

    def __init__(self, L, C, row_fam, Q, q_fam, q_rows):
        self.L, self.C, self.row_fam, self.Q, self.q_fam, self.q_rows = L, C, row_fam, Q, q_fam, q_rows
        self.N = C.shape[0]
        self.m = O.segment_bounds(L)[0][1]
        self._exact = {}

    def exact(self, mode, dtype=np.float64):
        """Oracle scores [nq, N] (mode 0: level 0, mode 1: overall), computed once and never written to."""
        key = (mode, np.dtype(dtype).name)
        if key not in self._exact:
            C, Q = self.C.astype(dtype), self.Q.astype(dtype)
            if mode == 0:
                e = np.stack([O.level_similarity(q, C, 0) for q in Q])
            else:
                e = np.stack([O.overall_similarity(q, C)[0] for q in Q])
            e.setflags(write=False)
            self._exact[key] = e
        return self._exact[key]

    def flagged_rows(self):
        return np.isin(self.row_fam, [FAMILIES.index(f) for f in FLAGGED])

    def flagged_queries(self, mode=0):
        """Queries the split scans do not answer (their lists are (+inf, -1) throughout: the dense exact path):
        level 0 (mode 0) the zero-variance and f32-unsafe ones, overall (mode 1) the f32-unsafe ones."""
        return np.isin(self.q_fam, [FAMILIES.index(f) for f in (FLAGGED if mode == 0 else FLAGGED[:2])])


def build_case(L, n, seed, nq=8, n_unsafe=None, n_const=2, derived=True, extra_gauss=0):
    """The corpus of the contract tests for index length L.

    Queries: the first nq rows of every family.  Corpus rows: n of every unflagged family, n_unsafe (default
    nq) of the two f32-unsafe ones and n_const constant rows.  Flagged rows are scored by a path of their own,
    so a handful is enough; and a constant row scores exactly 0.1 against every other row, so each one puts
    a whole column of the threshold-0.1 sweep into the indeterminate band (test_scan_contract_cpu.py), which
    is why there are only two.  For each query q in the corpus: q + 1e-3 max|q| N (near-duplicates: scores
    ~ 1, the clamp), 1.5 q and q + std(q) (the same z, other statistics), -q (anti-correlation: the
    max(0, .) branch), and 5 exact duplicates of query 0 at the end (ties broken by id).  The columns behind
    level 0 are N(0, 1); every third row gets one of the later segments replaced by a sample of its own
    family, so the overall scan sees hard short segments too (8, 3, 1 and 20 values at L = 64).
    extra_gauss: that many Gaussian rows in front (the large corpus of the sampled-threshold case)."""
    rng = np.random.default_rng(seed)
    bounds = O.segment_bounds(L)
    m = bounds[0][1]
    n_unsafe = nq if n_unsafe is None else n_unsafe
    fam = families(m, max(n, n_unsafe, n_const, nq), rng)
    rows, labels, Q, q_fam, q_rows = [], [], [], [], []
    at = extra_gauss
    for fi, f in enumerate(FAMILIES):
        cnt = n_const if f == "const" else (n_unsafe if f in FLAGGED else n)
        tot = max(cnt, nq)
        x = np.concatenate([fam[f][:tot], rng.standard_normal((tot, L - m))], axis=1)
        for i in range(0, tot, 3):  # every third row: one later segment in the family's own way
            s, e = bounds[1 + (i // 3) % (len(bounds) - 1)] if len(bounds) > 1 else (m, m)
            if e > s:
                x[i, s:e] = families(e - s, 1, rng)[f][0]
        rows.append(x[:cnt])
        labels += [fi] * cnt
        Q.append(x[:nq])
        q_fam += [fi] * nq
        q_rows += [at + i if i < cnt else -1 for i in range(nq)]
        at += cnt
    C, Q = np.concatenate(rows), np.concatenate(Q)
    if derived:
        extra, elab = [], []
        for q, fi, r in zip(Q, q_fam, q_rows):
            if r < 0 or FAMILIES[fi] == "const":  # a constant row's variants are constant rows again
                continue
            sd = np.std(q[:m])
            # the noise scale per part: level 0 and the N(0, 1) columns behind it differ by 2^35 in some families
            scale = np.concatenate([np.full(m, np.abs(q[:m]).max()), np.full(L - m, np.abs(q[m:]).max())])
            extra += [q + 1e-3 * scale * rng.standard_normal(L), 1.5 * q, q + sd, -q]
            elab += [fi] * 4
        extra += [Q[0].copy() for _ in range(5)]
        elab += [q_fam[0]] * 5
        C = np.concatenate([C, np.stack(extra)])
        labels += elab
    if extra_gauss:
        C = np.concatenate([rng.standard_normal((extra_gauss, L)), C])
        labels = [FAMILIES.index("gauss")] * extra_gauss + labels
    return Case(L, C, np.array(labels), Q, np.array(q_fam), np.array(q_rows))


_CASES = {}


def case(L, n, seed=20, **kw):
    """build_case, built once per argument set and shared by the tests."""
    key = (L, n, seed, tuple(sorted(kw.items())))
    if key not in _CASES:
        _CASES[key] = build_case(L, n, seed, **kw)
    return _CASES[key]


# rows per unflagged family of the two corpus sizes of the bound and completeness tests:
# N below the longest list (1024: every row must be listed) and above it
N_SMALL, N_LARGE = 58, 90


def split_model_level0(Q, C, m, ftz=False):
    """The level-0 split scan as designed, in NumPy: z = hi + lo in f16, G = hi.hi + hi.lo + lo.hi accumulated
    in f32, then k_scan0g's f32 epilogue.  Q [nq, >= m], C [N, >= m] -> scores [nq, N] (meaningful for pairs of
    unflagged rows only).  ftz: f16 subnormals flushed to zero (what the bound would be on hardware that does)."""
    def side(X):
        X = np.asarray(X, dtype=np.float64)[:, :m]
        mean = X.mean(axis=1)
        d = X - mean[:, None]
        std = np.sqrt((d * d).mean(axis=1))
        msq = (X * X).mean(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            z = d / std[:, None]
        z = np.where(np.isfinite(z), z, 0.0)
        hi = z.astype(np.float16)
        lo = (z - hi.astype(np.float64)).astype(np.float16)
        if ftz:
            hi = np.where(np.abs(hi) < 2.0 ** -14, np.float16(0), hi)
            lo = np.where(np.abs(lo) < 2.0 ** -14, np.float16(0), lo)
        return (hi.astype(np.float32), lo.astype(np.float32), std.astype(np.float32), mean.astype(np.float32),
                msq.astype(np.float32))
    qh, ql, sq, mq, msq_q = side(Q)
    ch, cl, sc, mc, msq_c = side(C)
    f = np.float32
    G = qh @ ch.T + qh @ cl.T + ql @ ch.T
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        base = f(0.35) + f(0.35 / m) * G
        num = G * (f(0.6 / m) * sq)[:, None] * sc[None, :] + (f(0.6) * mq)[:, None] * mc[None, :]
        t = np.maximum(f(0), num / (msq_q[:, None] + msq_c[None, :]))
        s = np.clip(base + t, f(0), f(1))
    return s.astype(np.float64)


def passes(exact, thr, thr_mode):
    """The exact threshold test of an f64 pool."""
    exact = np.asarray(exact)
    if thr_mode == 0:
        return np.ones(exact.shape, dtype=bool)
    return exact >= thr if thr_mode == 1 else exact > thr


def resolved_rule(cand_score, cand_id, exact, passing, k, thr, thr_mode, eps):
    """One query's re-rank, from the contract alone (f64 pools, HQ_THR_KEY32 off).

    cand_score / cand_id [kp]: the list (approximate scores; id -1 = empty slot); exact / passing [N]: the
    query's exact score against every row and whether it passes the exact threshold test.
    Returns (resolved, count, out_id [k], out_score [k]): the exact top-k (score desc, id asc) of the valid
    entries, padded with (-1, -inf), and whether the list proves it complete."""
    cand_score, cand_id = np.asarray(cand_score, dtype=np.float64), np.asarray(cand_id, dtype=np.int64)
    N = len(exact)
    listed = (cand_id >= 0) & (cand_id < N)
    ids = cand_id[listed]
    ids = ids[passing[ids]]                    # valid: listed and passing the exact threshold test
    n = len(ids)
    count = min(n, k)
    order = np.lexsort((ids, -exact[ids]))     # score desc, id asc
    top = ids[order][:k]
    out_id = np.full(k, -1, dtype=np.int64)
    out_score = np.full(k, -np.inf)
    out_id[:count] = top
    out_score[:count] = exact[top]
    full = cand_id[-1] >= 0
    if not full:
        resolved = cand_score[-1] != np.inf    # +inf in the last slot: the scan cut the list short
    else:
        bound = cand_score[-1] + eps
        if n >= k:
            resolved = bound < out_score[k - 1]
        elif thr_mode == 0:
            resolved = False
        else:
            resolved = bound < thr if thr_mode == 1 else bound <= thr
    return bool(resolved), count, out_id, out_score


def redo_count(resolved, count, count_empty):
    """Queries that need the dense path: unresolved, or (count_empty) with no candidate passing."""
    resolved, count = np.asarray(resolved, dtype=bool), np.asarray(count)
    return int((~resolved | ((count == 0) if count_empty else False)).sum())
