"""Float64 NumPy model and frame families of the video-feature tests (tests/test_gpu_vfeat.py, tests/test_vfeat_cpu.py)
and of tools/ab_vfeat.py: the contract of include/hq_mi355x.h (hq_vfeat_*) written with NumPy's own routines."""
import numpy as np

PARTS = (slice(0, 32), slice(32, 48), slice(48, 55))
WEIGHTS = (0.3, 0.2, 0.1)
FAMILIES = ("random", "zeros", "const", "ramp", "narrow", "spike", "checker")
EXACT = list(range(32)) + list(range(40, 48)) + [50, 51]  # histogram, magnitude counts, min, max


def sobel(g):
    p = np.pad(g.astype(np.float64), 1, mode="reflect")
    gx = (p[:-2, 2:] + 2 * p[1:-1, 2:] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[1:-1, :-2] + p[2:, :-2])
    gy = (p[2:, :-2] + 2 * p[2:, 1:-1] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[:-2, 1:-1] + p[:-2, 2:])
    return gx, gy, np.sqrt(gx ** 2 + gy ** 2)


def features(g):
    """[55] float64: histogram, texture, stats of one gray u8 frame."""
    gx, gy, m = sobel(g)
    tex = [m.mean(), m.std(), gx.mean(), gx.std(), gy.mean(), gy.std(), np.abs(gx).mean(), np.abs(gy).mean(),
           *np.histogram(m.ravel(), bins=8)[0]]
    st = [np.mean(g), np.std(g), np.min(g), np.max(g), np.median(g), np.percentile(g, 25), np.percentile(g, 75)]
    return np.concatenate([np.bincount(g.ravel() >> 3, minlength=32), tex, st]).astype(np.float64)


def bin_rule(m):
    """The 8 magnitude counts as the header states them: bin(x) = #{j in 1 .. 7 : x >= edge_j}."""
    lo, hi = m.min(), m.max()
    if lo == hi:
        lo, hi = lo - 0.5, hi + 0.5
    edges = np.arange(1, 8) * ((hi - lo) / 8) + lo
    return np.bincount((m.ravel()[:, None] >= edges).sum(1), minlength=8)


def score(fa, fb, w=WEIGHTS, hist32=False):
    """_calculate_feature_similarity without its ORB part; hist32: the histogram part in float32, as cv2.calcHist
    returns it."""
    tot = 0.0
    for i, (sl, wt) in enumerate(zip(PARTS, w)):
        a, b = (v[sl].astype(np.float32) if hist32 and i == 0 else v[sl] for v in (fa, fb))
        na, nb = np.linalg.norm(a), np.linalg.norm(b)
        if na > 0 and nb > 0:
            tot += wt * max(0, np.dot(a, b) / (na * nb))
    return tot


def combine(h, v):
    return np.where(v > 0.5, 0.3 * h + 0.7 * v, 0.8 * h + 0.2 * v)


def make(family, H, W, n=8, seed=0):
    """[n, H, W] u8 frames of one family."""
    rng = np.random.default_rng([seed, H, W])
    r, c, i = np.ogrid[:H, :W, :n]
    f = {"random": lambda: rng.integers(0, 256, (H, W, n)),
         "zeros": lambda: np.zeros((H, W, n)),
         "const": lambda: np.broadcast_to(np.array([7, 200, 255, 8, 7, 1, 128, 64])[i % 8], (H, W, n)),
         "ramp": lambda: np.minimum(3 * r + 2 * c + 5 * i, 255),
         "narrow": lambda: rng.integers(100, 104, (H, W, n)),
         "spike": lambda: 255 * ((r == (2 * i) % H) & (c == (3 * i) % W)),
         "checker": lambda: 40 + 150 * ((r + c + (r * i) // 2) % 2)}[family]()
    return np.ascontiguousarray(np.moveaxis(np.asarray(f), 2, 0).astype(np.uint8))
