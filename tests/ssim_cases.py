"""Float64 model and seeded frame families of the SSIM tests (tests/test_gpu_ssim.py) and of tools/ab_ssim.py.

The model is the contract of include/hq_mi355x.h written out in NumPy float64: min-max normalisation, the 7-tap
Gaussian (sigma 1.5) applied along both axes with mirrored borders, the SSIM map, its mean."""
import numpy as np
from scipy.ndimage import correlate1d

G7 = np.exp(-(np.arange(7) - 3.0) ** 2 / 4.5)
G7 /= G7.sum()


def _F(a):
    return correlate1d(correlate1d(a, G7, axis=0, mode="mirror"), G7, axis=1, mode="mirror")


def ssim_model(x, y):
    x, y = x.astype(np.float64), y.astype(np.float64)
    x = (x - x.min()) / (x.max() - x.min() + 1e-8)
    y = (y - y.min()) / (y.max() - y.min() + 1e-8)
    m1, m2 = _F(x), _F(y)
    v1, v2, cov = _F(x * x) - m1 * m1, _F(y * y) - m2 * m2, _F(x * y) - m1 * m2
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    return float(np.mean((2 * m1 * m2 + c1) * (2 * cov + c2) / ((m1 * m1 + m2 * m2 + c1) * (v1 + v2 + c2) + 1e-8)))


def ncc_model(x, y):
    """Pearson correlation of the raw pixels from exact integer sums; 0.0 when a frame is constant."""
    x, y, n = x.astype(np.int64).ravel(), y.astype(np.int64).ravel(), x.size
    vx, vy = n * int(x @ x) - int(x.sum()) ** 2, n * int(y @ y) - int(y.sum()) ** 2
    return 0.0 if vx == 0 or vy == 0 else (n * int(x @ y) - int(x.sum()) * int(y.sum())) / np.sqrt(float(vx) * float(vy))


def _flat(rng, n, H, W):
    f = np.full((n, H, W), 254, np.uint8)
    f[:, ::2, ::2] = 255
    f[:, 1::2, 1::2] = 255
    for i in range(n):
        f[i, rng.integers(H), rng.integers(W)] = 0
    return f


def make(family, H, W, Q=3, N=5, seed=0):
    """(queries [Q, H, W], corpus [N, H, W]) u8 of one family."""
    rng = np.random.default_rng([seed, H, W])
    q = rng.integers(0, 256, (Q, H, W), dtype=np.uint8)
    c = rng.integers(0, 256, (N, H, W), dtype=np.uint8)
    if family == "identical":
        c[:] = q[np.arange(N) % Q]
    elif family == "negated":
        c[:] = 255 - q[np.arange(N) % Q]
    elif family == "flat":  # 254 / 255 checkerboard with one 0 pixel; the corpus frames also hold some 253s
        q = _flat(rng, Q, H, W)
        c = q[np.arange(N) % Q].copy()
        c[rng.random(c.shape) < 0.1] = 253
        c[0] = q[0]
    elif family == "const_random":
        q[:] = np.array([0, 7, 255], np.uint8)[np.arange(Q) % 3, None, None]
    elif family == "const_const":
        q[:] = np.array([0, 7, 255], np.uint8)[np.arange(Q) % 3, None, None]
        c[:] = np.array([7, 200], np.uint8)[np.arange(N) % 2, None, None]
    elif family == "ranges":  # every frame has its own (min, max)
        q = (10 + q // 5).astype(np.uint8)
        c = np.stack([(40 * i + c[i] // (2 + i)).astype(np.uint8) for i in range(N)])
    elif family != "random":
        raise ValueError(family)
    return q, c


FAMILIES = ("random", "identical", "negated", "flat", "const_random", "const_const", "ranges")
