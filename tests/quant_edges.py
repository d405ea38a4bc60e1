"""Shared helpers of the quantiser edge tests (test_quant_edges_cpu.py, test_gpu_quant_edges.py).

Plain NumPy plus the CPU oracle; nothing here touches the GPU package.  Every frame byte of the project
is trunc((x - mn) / (mx - mn) * 255) in float32 (oracle.normalize_u8), so a kernel can only be wrong at
the few inputs that sit next to a byte boundary, and only a kernel that replaces the division can be
wrong at all.  This module builds exactly those inputs:

* `level_edges`: for a float32 range, the values on both sides of every byte boundary;
* `RANGES_F32` / `RANGES_F16`: the ranges the tests run, from ordinary ones to subnormal and near-FLT_MAX
  ones; every range keeps mx - mn finite and holds no NaN or Inf (the documented input domain);
* `f16_sweep`: every f16 value of a range, packed so that every chunk has exactly that range;
* `recip_model`: the reciprocal form of the fast kernels (qfast of hq_common.h and the packed form of
  k_chunk_np / process_emb) WITHOUT its exact-division fallback, as a second reference: the CPU tests use
  it to prove that the inputs above land where the unguarded form is wrong.
"""
import numpy as np

from oracle import hq_oracle as O

F32 = np.float32

# ------------------------------------------------------------------------------------ float32 ordinals


def _ordinal(x):
    """float32 -> int64, monotone in the value (-0.0 and +0.0 both give 0)."""
    b = np.asarray(x, F32).view(np.int32).astype(np.int64)
    return np.where(b >= 0, b, -(b & 0x7FFFFFFF))


def _from_ordinal(o):
    o = np.asarray(o, np.int64)
    bits = np.where(o >= 0, o, (-o) | 0x80000000).astype(np.uint32)
    return bits.view(F32)


def oracle_bytes(x, mn, mx):
    """oracle.normalize_u8 bytes of the float32 values x inside an image whose range is [mn, mx]."""
    x = np.asarray(x, F32).reshape(-1)
    img = np.concatenate([np.array([mn, mx], F32), x])[None]
    u8, rmn, rmx = O.normalize_u8(img)               # one 1 x (len + 2) image
    assert rmn == F32(mn) and rmx == F32(mx), "values outside [mn, mx]"
    return u8[0, 2:]


# --------------------------------------------------------------------------------------- level edges


def boundaries(mn, mx):
    """[(k, x)]: for every byte boundary k = 1..255 the range has, the smallest float32 x in [mn, mx] whose
    oracle byte is >= k (bisection over the float32 ordinals: the byte is monotone in x).  A boundary is
    missing when no value of the range has byte k - 1 (fewer than 256 distinct bytes)."""
    mn, mx = F32(mn), F32(mx)
    assert np.isfinite(mn) and np.isfinite(mx) and mn < mx and np.isfinite(mx - mn)
    ks = np.arange(1, 256)
    lo = np.full(255, _ordinal(mn))          # byte(lo) = 0 < k
    hi = np.full(255, _ordinal(mx))          # byte(hi) = 255 >= k
    while np.any(hi - lo > 1):
        mid = (lo + hi) // 2
        ge = oracle_bytes(_from_ordinal(mid), mn, mx) >= ks
        hi = np.where(ge, mid, hi)
        lo = np.where(ge, lo, mid)
    below = oracle_bytes(_from_ordinal(hi - 1), mn, mx)
    return [(int(k), F32(x)) for k, x, b in zip(ks, _from_ordinal(hi), below) if b == k - 1]


def level_edges(mn, mx):
    """Sorted distinct float32 values of [mn, mx]: for every byte boundary the first value of the upper byte,
    its predecessor, one more neighbour on each side, plus mn and mx."""
    mn, mx = F32(mn), F32(mx)
    first = np.unique(np.array([_ordinal(x) for _, x in boundaries(mn, mx)], np.int64))
    o = np.concatenate([first - 2, first - 1, first, first + 1, [_ordinal(mn), _ordinal(mx)]])
    o = np.unique(np.clip(o, _ordinal(mn), _ordinal(mx)))
    return _from_ordinal(o)


RANGES_F32 = {
    "pm1": (F32(-1.0), F32(1.0)),
    "unit": (F32(0.0), F32(1.0)),
    "offset": (F32(-0.3), F32(0.7)),
    "wide": (F32(-7.25), F32(1000.125)),
    "big_offset": (F32(1e8), F32(1e8) + F32(800.0)),          # 101 distinct values
    "few_ulps": (F32(3.0), F32(3.0) + F32(2.0 ** -20)),       # 5 distinct values
    "huge": (F32(-1.5e38), F32(1.5e38)),                       # 1 / rng is subnormal
    "small_normal": (F32(0.0), F32(1e-37)),                    # fl(fl(1 / rng) * 255) overflows
    "small_normal_signed": (F32(-3e-38), F32(4e-38)),
    "subnormal": (F32(0.0), F32(1e-40)),
    "subnormal_signed": (F32(-2e-41), F32(5e-41)),
}
# the ranges whose fl(fl(1 / rng) * 255) is inf (rng below about 7.5e-37)
RECIP_OVERFLOW = ("small_normal", "small_normal_signed", "subnormal", "subnormal_signed")
# ranges that contain 0.0 (a zero-padded image, d < n * n, keeps their min / max)
HOLDS_ZERO = tuple(k for k, (a, b) in RANGES_F32.items() if a <= 0 <= b)


def full_range(name):
    """True when the family has all 256 bytes."""
    return len(boundaries(*RANGES_F32[name])) == 255


_EDGES = {}


def edges(name):
    """level_edges of a family, computed once and never written to."""
    if name not in _EDGES:
        e = level_edges(*RANGES_F32[name])
        e.setflags(write=False)
        _EDGES[name] = e
    return _EDGES[name]


def cycled(vals, count, first=()):
    """`count` values: `first`, then `vals` over and over."""
    vals = np.asarray(vals)
    head = np.asarray(first, vals.dtype)
    reps = -(-max(count - len(head), 0) // len(vals))
    return np.concatenate([head, np.tile(vals, reps)])[:count]


# ---------------------------------------------------------------------------------------------- f16

_F16_MAXSUB = np.float16(2.0 ** -14 - 2.0 ** -24)


def _f16_bits(a, b):
    v = np.array([a, b], np.uint16).view(np.float16)
    return v[0], v[1]


RANGES_F16 = {
    "full": (np.float16(-65504.0), np.float16(65504.0)),
    "subnormal": (np.float16(0.0), _F16_MAXSUB),
    "tiny": (np.float16(2.0 ** -24), np.float16(2.0 ** -14)),
    "cfg5": (np.float16(-0.07), np.float16(0.07)),
    # found by search_f16_pairs(seed=2024): both unguarded forms give a wrong byte for at least one f16 value
    # of the range, with the correctly rounded reciprocal and with it moved one ulp either way
    # (test_quant_edges_cpu.py re-runs the search and re-checks this)
    "searched0": _f16_bits(0xA24D, 0x23F7),     # (-0.01231, 0.01556)
    "searched1": _f16_bits(0xB484, 0x306F),     # (-0.2822, 0.1385)
    "searched2": _f16_bits(0xDC4B, 0x5CD4),     # (-274.8, 309.0)
    "searched3": _f16_bits(0xD289, 0x501A),     # (-52.28, 32.8)
}
SEARCHED_F16 = ("searched0", "searched1", "searched2", "searched3")


def f16_values(mn, mx):
    """Every finite f16 value in [mn, mx], ascending (both zeros when the range holds 0)."""
    allv = np.arange(0x10000, dtype=np.uint32).astype(np.uint16).view(np.float16)
    allv = allv[np.isfinite(allv)]
    v = allv[(allv >= mn) & (allv <= mx)]
    return v[np.argsort(v.astype(F32), kind="stable")]


def f16_sweep(mn, mx, chunk):
    """Every finite f16 value of [mn, mx] in chunks of `chunk` values that each start with mn, mx; the last
    chunk is filled up with mn.  Every chunk therefore has exactly the range [mn, mx]."""
    assert chunk > 2
    v = f16_values(mn, mx)
    per = chunk - 2
    nch = -(-len(v) // per)
    body = np.full(nch * per, mn, np.float16)
    body[:len(v)] = v
    out = np.empty((nch, chunk), np.float16)
    out[:, 0], out[:, 1] = mn, mx
    out[:, 2:] = body.reshape(nch, per)
    return out.reshape(-1)


def chunk_frame_range(mn, mx):
    """Range of a chunk encoder frame whose f16 data has the range [mn, mx]: the traditional index row of a
    32 x 32 or 64 x 64 chunk has zero-filled slots (and block means and samples inside [mn, mx]), so the
    frame's range always holds 0.0."""
    return min(F32(mn), F32(0.0)), max(F32(mx), F32(0.0))


# --------------------------------------------------------------------------------- the reciprocal form


def recip_model(x, mn, mx, ulp=0, form="packed"):
    """The fast kernels' reciprocal quantiser without the exact-division fallback, in float32 NumPy.

    form "qfast":  y = fl(fl(fl(x - mn) * r) * 255), fallback wanted where frac(y) < 1e-4 or > 0.9999;
    form "packed": y = fl(fl(x - mn) * fl(r * 255)), fallback wanted where |frac(y) - 0.5| > 0.4999;
    r = fl(1 / rng) moved by `ulp` (-1, 0, +1) float32 steps, which covers the 1-ulp hardware reciprocal.
    Returns (bytes, guard): the byte the unguarded form stores (saturating conversion: NaN -> 0, above
    255 -> 255) and the mask of values for which the kernel would redo the exact division.  The guard
    compares false on NaN, as the kernels' comparisons do."""
    x = np.asarray(x, F32)
    mn, mx = F32(mn), F32(mx)
    with np.errstate(all="ignore"):
        rng = F32(mx - mn)
        r = F32(1.0) / rng
        if ulp:
            r = _from_ordinal(_ordinal(r) + int(ulp))[()]
        d = (x - mn).astype(F32)
        if form == "qfast":
            y = ((d * r).astype(F32) * F32(255.0)).astype(F32)
        else:
            y = (d * F32(r * F32(255.0))).astype(F32)
        fl = np.floor(y)
        f = (y - fl).astype(F32)
        if form == "qfast":
            guard = (f < F32(1e-4)) | (f > F32(0.9999))
        else:
            guard = np.abs((f - F32(0.5)).astype(F32)) > F32(0.4999)
        b = np.where(np.isnan(fl), F32(0.0), np.clip(fl, 0.0, 255.0)).astype(np.uint8)
    return b, guard


def guarded_model(x, mn, mx, ulp=0, form="packed"):
    """recip_model with the fallback applied: the oracle byte wherever the guard asks for it."""
    b, g = recip_model(x, mn, mx, ulp, form)
    return np.where(g, oracle_bytes(x, mn, mx), b)


def search_f16_pairs(seed=2024, want=4, tries=4000):
    """The seeded search behind RANGES_F16's searched pairs: random f16 (mn, mx) whose sweep holds a value
    at which both unguarded forms give a wrong byte, whichever way the reciprocal is rounded."""
    rng = np.random.default_rng(seed)
    found = []
    for _ in range(tries):
        a, b = np.sort((rng.standard_normal(2) * 10.0 ** rng.uniform(-3, 3)).astype(np.float16))
        if not (np.isfinite(a) and np.isfinite(b) and a < b):
            continue
        v = f16_values(a, b).astype(F32)
        ref = oracle_bytes(v, a, b)
        if all(np.any(recip_model(v, a, b, u, f)[0] != ref) for f in ("qfast", "packed") for u in (-1, 0, 1)):
            found.append((a, b))
            if len(found) == want:
                break
    return found
