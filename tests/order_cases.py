"""Long-double NumPy model of the frame ordering (reference core/video_storage.py:762-781, 1203-1277, 1445-1522,
1751-1803) and the input builders shared by test_order_cpu.py, test_gpu_order.py and golden/make_frame_ordering.py."""
import numpy as np

LD = np.longdouble
KEYS = ("average_neighbor_similarity", "similarity_variance", "temporal_coherence", "ordering_efficiency")
CASES = ("gauss5", "gauss32", "gauss64", "dups32", "const5", "const64")  # stores of golden/frame_ordering.npz


def _unit(X):
    c = X.astype(LD)
    c = c - c.mean(1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        return c / np.sqrt((c * c).sum(1, keepdims=True))


def sims(Q, C):
    """S[i][j] = similarity of query row i and candidate row j in long double; constant-row entries exact."""
    Q, C = np.atleast_2d(np.asarray(Q, np.float64)), np.atleast_2d(np.asarray(C, np.float64))
    s = np.clip((np.clip(_unit(Q) @ _unit(C).T, -1, 1) + 1) / 2, 0, 1)
    cq, cc = Q.std(1) == 0, C.std(1) == 0
    for i, j in zip(*np.nonzero(cq[:, None] | cc[None, :])):
        s[i, j] = 1.0 if np.allclose(Q[i], C[j]) else 0.0
    return s


def start_gap(rows):
    """Relative gap between the two smallest distances to the centroid, in long double (inf for one row).  Two rows
    are always equidistant from their midpoint: there the reference's own start row is rounding noise of np.mean."""
    x = np.asarray(rows, np.float64).astype(LD)
    d = np.sort(np.sqrt(((x - x.mean(0)) ** 2).sum(1)))
    return np.inf if len(d) < 2 else float((d[1] - d[0]) / d[1])


def greedy(rows, start=None):
    """(order, step_sims, smallest gap): the chain on the model's matrix from the row nearest the centroid (or from
    `start`).  The gap of a step is the best remaining similarity minus the best one that does not tie with it by
    construction (bit-identical rows, or both values from the exact constant-row branch); inf when no such step
    exists."""
    rows = np.asarray(rows, np.float64)
    N = len(rows)
    S = sims(rows, rows)
    const = rows.std(1) == 0
    cls = np.unique(rows, axis=0, return_inverse=True)[1].reshape(-1)
    last = int(np.argmin(np.sqrt(((rows - rows.mean(0)) ** 2).sum(1)))) if start is None else int(start)
    order, steps, gap, left = [last], [], np.inf, np.ones(N, bool)
    left[last] = False
    for _ in range(N - 1):
        s = np.where(left, S[last], -np.inf)
        b = int(np.argmax(s))
        key = np.where(const[last] | const, -1 - (S[last] >= 0.5), cls)
        rest = s[left & (key != key[b])]
        if len(rest):
            gap = min(gap, float(s[b] - rest.max()))
        order.append(b)
        steps.append(float(s[b]))
        left[b] = False
        last = b
    return np.array(order, np.int64), np.array(steps), gap


def metrics(rows, order=None):
    """The four metrics (KEYS order) of the rows taken in `order`."""
    rows = np.asarray(rows, np.float64)
    if order is not None:
        rows = rows[np.asarray(order)]
    if len(rows) < 2:
        return np.array([1.0, 0.0, 1.0, 1.0])
    s = np.array([sims(rows[i], rows[i + 1])[0, 0] for i in range(len(rows) - 1)], LD)
    avg, var = s.mean(), ((s - s.mean()) ** 2).mean()
    return np.array([avg, var, avg * (1 - min(var, 1)), max(0, 1 - (1 - s).mean())], np.float64)


def insertion(s):
    """(position, score) for one row of similarities: head, between neighbours, tail; the first maximum wins."""
    s = np.asarray(s, LD)
    sc = np.concatenate([s[:1], (s[:-1] + s[1:]) / 2, s[-1:]])
    return int(np.argmax(sc)), float(sc.max())


def gaussian(rng, N, L, shift=3.0):
    """Gaussian rows with |mean| <= 10 std (per-row offset of up to `shift` standard deviations)."""
    return rng.standard_normal((N, L)) + shift * rng.uniform(-1, 1, (N, 1))


def with_duplicates(rng, N, L):
    """Gaussian rows where every third row is a bit-identical copy of an earlier one."""
    x = gaussian(rng, N, L)
    for i in range(2, N, 3):
        x[i] = x[rng.integers(0, i - 1)]
    return x


def with_constants(rng, N, L):
    """Gaussian rows with constant rows of the dyadic values 0.0, 0.5, 2.0 (two of each 0.5) mixed in."""
    x = gaussian(rng, N, L)
    for i, v in zip(rng.choice(N, 4, replace=False), (0.0, 0.5, 2.0, 0.5)):
        x[i] = v
    return x


def anticorrelated(rng, N, L):
    """N <= L rows, every pair negatively correlated (noisy indicator rows): every similarity is below 0.5."""
    return np.eye(N, L) + 0.01 * rng.standard_normal((N, L))
