#!/usr/bin/env python3
"""Float32 queries against the u8 frame store: the asymmetric route against decode-then-search, one process.

The store: map_index_quantize of seeded float32 parameters -> u8 frames [N, n + 1, n] + (min, max) [N, 2]; the
queries: noisy copies of stored parameters, laid onto n x n along the curve (map_to_2d) and kept in float32.
Every route searches the n leading rows.

(a)  the full-precision route there was: dequantize_u8 -> cos_prepare (once, not timed) -> cos_prepare of the
     query batch + cosine_topk (split-f16 MFMA) on the decoded store;
(b)  cosqf_prepare of the query batch + cosqf_topk on the resident u8 corpus (three exact int8 MFMA planes);
(c)  the floor: the queries quantised to u8 (once, not timed) and cosq_topk, one plane, a third of (b)'s K loop.

Every variant runs once per repetition, in turn, each between two HIP events on the launch stream, after warm-up
rounds of every variant.  Checked first: (b) equals select_topk(cosqf_scores) bit for bit, and (a)'s scores are
within 1e-5 of (b)'s at equal rank.  Also timed: the prepare calls and the dense cosqf_scores; reported: the
resident bytes of each corpus and the share of top-k positions where (b) and (c) list different ids (the ranking
effect of quantising the query to 8 bits).

usage: ab_cosqf.py [--queries 1000] [--frames 250000] [--n 64] [--k 10 64] [--reps 9] [--warmup 2]
Needs an MI355X."""
import argparse
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--queries", type=int, default=1000)
ap.add_argument("--frames", type=int, default=250_000)
ap.add_argument("--n", type=int, default=64)
ap.add_argument("--k", type=int, nargs="+", default=[10, 64])
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hilbert-quantization_amd")]

import torch  # noqa: E402
from hq_mi355x import kernels as K  # noqa: E402

assert torch.cuda.is_available(), "ab_cosqf.py needs the GPU"
Q, N, n = args.queries, args.frames, args.n
Kd = n * n

g = torch.Generator(device="cuda").manual_seed(0)
frames = torch.empty((N, n + 1, n), dtype=torch.uint8, device="cuda")
minmax = torch.empty((N, 2), dtype=torch.float32, device="cuda")
pick = torch.randint(0, N, (Q,), generator=g, device="cuda")
xq = torch.empty((Q, Kd), dtype=torch.float32, device="cuda")
CH = 25_000
for c0 in range(0, N, CH):  # the parameters, a chunk at a time: only the store stays
    c1 = min(N, c0 + CH)
    x = torch.randn((c1 - c0, Kd), generator=g, dtype=torch.float32, device="cuda")
    K.map_index_quantize(x, n, want_idx=False, out=(frames[c0:c1], None, minmax[c0:c1]))
    m = (pick >= c0) & (pick < c1)
    xq[m] = x[pick[m] - c0]
    del x
xq += 0.5 * torch.randn((Q, Kd), generator=g, dtype=torch.float32, device="cuda")
qf32 = K.map_to_2d(xq, n)  # the float32 query frames [Q, n, n]
qframes, _, qminmax = K.map_index_quantize(xq, n, want_idx=False)
del xq
print(f"== float32 queries against the u8 frame store A/B: {Q} queries x {N} frames x K = {Kd} (u8 store of {n + 1} x {n} "
      f"frames), {args.reps} alternating repetitions after {args.warmup} warm-up rounds, HIP events; "
      f"{torch.cuda.get_device_name(0)} ==", flush=True)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    del r
    return e0.elapsed_time(e1) * 1e-3


def line(name, ts):
    print(f"{name:<52} median {statistics.median(ts) * 1e3:9.3f} ms  (min {min(ts) * 1e3:9.3f} - max {max(ts) * 1e3:9.3f})",
          flush=True)
    return statistics.median(ts)


def f16_corpus():
    return K.cos_prepare(K.dequantize_u8(frames, minmax)[:, :n].reshape(N, -1))


def f16_queries():
    return K.cos_prepare(qf32.reshape(Q, -1))


prep = {"a  dequantize_u8 + cos_prepare, corpus": f16_corpus,
        "b  cosq_prepare, corpus (serves b and c)": lambda: K.cosq_prepare(frames, minmax, n),
        "a  cos_prepare, float32 query batch": f16_queries,
        "b  cosqf_prepare, float32 query batch": lambda: K.cosqf_prepare(qf32),
        "c  cosq_prepare, u8 query batch": lambda: K.cosq_prepare(qframes, qminmax, n)}
for name, fn in prep.items():
    fn()
    torch.cuda.synchronize()
    line(name, [timed(fn) for _ in range(max(3, args.reps // 2))])
pc16 = f16_corpus()
pc8 = K.cosq_prepare(frames, minmax, n)
pq8 = K.cosq_prepare(qframes, qminmax, n)
b16 = pc16.X16.numel() * 2 + pc16.inv.numel() * 8
b8 = pc8.nbytes
print(f"resident corpus: (a) split-f16 fragments + inverse norms {b16} B = {b16 / 2 ** 30:.3f} GiB; "
      f"(b), (c) signed bytes + statistics {b8} B = {b8 / 2 ** 30:.3f} GiB ({b16 / b8:.2f}x less); "
      f"the u8 store itself {frames.numel() + minmax.numel() * 4} B", flush=True)

pqf = K.cosqf_prepare(qf32)
sc = K.cosqf_scores(pqf, pc8)
torch.cuda.synchronize()
del sc
df = line("b  cosqf_scores (dense [Q, N] f64)", [timed(lambda: K.cosqf_scores(pqf, pc8)) for _ in range(args.reps)])
d8 = line("c  cosq_scores (dense [Q, N] f64)", [timed(lambda: K.cosq_scores(pq8, pc8)) for _ in range(args.reps)])
ops = 2.0 * Q * N * Kd
print(f"dense: (b) {3 * ops / df / 1e12:.1f} TOP/s over its three planes ({ops / df / 1e12:.1f} algorithmic), "
      f"(c) {ops / d8 / 1e12:.1f} TOP/s; (b) / (c) = {df / d8:.2f}x", flush=True)

for k in args.k:
    limit = 1 << 40  # one query block

    def route_a():
        return K.cosine_topk(f16_queries(), pc16, k, workspace_limit=limit)

    def route_b():
        return K.cosqf_topk(K.cosqf_prepare(qf32), pc8, k, workspace_limit=limit)

    def route_c():
        return K.cosq_topk(pq8, pc8, k, workspace_limit=limit)

    VARIANTS = [("a  cos_prepare + cosine_topk on the decoded store", route_a),
                ("b  cosqf_prepare + cosqf_topk on the u8 store", route_b),
                ("c  cosq_topk, u8 queries (the floor)", route_c)]
    ra, rb, rc = route_a(), route_b(), route_c()
    want = K.select_topk(K.cosqf_scores(pqf, pc8), k)[:2]
    assert torch.equal(rb[1], want[1]) and torch.equal(rb[0].view(torch.int64), want[0].view(torch.int64)), \
        "cosqf_topk differs from select_topk(cosqf_scores)"
    same = float((ra[1] == rb[1]).double().mean())
    gap = float((ra[0] - rb[0]).abs().max())
    assert gap < 1e-5, gap
    moved = float((rb[1] != rc[1]).double().mean())
    qgap = float((rb[0] - rc[0]).abs().max())
    print(f"-- k = {k}: (b) bit-identical to select_topk(cosqf_scores); (a) lists the same id at {same * 100:.2f} % of the "
          f"positions, largest score difference at equal rank {gap:.2e}; quantising the query (c) lists a different id "
          f"at {moved * 100:.2f} % of the positions, largest score difference at equal rank {qgap:.2e}")
    del ra, rb, rc, want
    for _ in range(args.warmup):
        for _, fn in VARIANTS:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in VARIANTS}
    for _ in range(args.reps):
        for name, fn in VARIANTS:
            times[name].append(timed(fn))
    a, b, c = (line(name, times[name]) for name, _ in VARIANTS)
    spread = max(max(t) - min(t) for t in times.values())
    print(f"(a) / (b): {a / b:5.3f}x   (a) - (b) = {(a - b) * 1e3:.3f} ms;   (b) / (c): {b / c:5.3f}x;   largest spread of "
          f"the repetitions {spread * 1e3:.3f} ms", flush=True)
