#!/usr/bin/env python3
"""Compressed-domain frame search against the decode-then-search route, on the same u8 store, one process.

The store: map_index_quantize of seeded float32 parameters -> u8 frames [N, n + 1, n] + (min, max) [N, 2]; the
queries: noisy copies of stored parameters, quantised the same way.  Both routes search the n leading rows.

(a)  the existing route: dequantize_u8 -> cos_prepare (once, not timed) -> cosine_topk (split-f16 MFMA);
(b)  cosq_prepare (once, not timed) -> cosq_topk (exact int8 MFMA).

Every variant runs once per repetition, in turn, each between two HIP events on the launch stream, after warm-up
rounds of every variant.  Checked first: (b) equals select_topk(cosq_scores) bit for bit, and (a)'s scores are
within 1e-5 of (b)'s for the frames (b) lists.  Also timed: both prepare calls (corpus and query batch), the dense
cosq_scores, and reported: the resident bytes of each corpus, and the dense int8 GEMM (its float64 score stores
included) as a fraction of the int8 matrix ceiling, twice bench.py's dense-f16 figure.

usage: ab_cosq.py [--queries 1000] [--frames 250000] [--n 64] [--k 10 64] [--reps 9] [--warmup 2]
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

assert torch.cuda.is_available(), "ab_cosq.py needs the GPU"
Q, N, n = args.queries, args.frames, args.n
Kd = n * n
I8_PEAK_TOPS = 2.0 * 2500.0  # twice bench.py's FP16_MATRIX_PEAK_TFS

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
qframes, _, qminmax = K.map_index_quantize(xq, n, want_idx=False)
del xq
print(f"== compressed-domain frame search A/B: {Q} queries x {N} frames x K = {Kd} (u8 store of {n + 1} x {n} frames), "
      f"{args.reps} alternating repetitions after {args.warmup} warm-up rounds, HIP events; "
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


def f16_prepare(fr, mm):
    return K.cos_prepare(K.dequantize_u8(fr, mm)[:, :n].reshape(fr.shape[0], -1))


# prepare: both routes, corpus and query batch, timed on their own (first calls are warm-up)
prep = {"a  dequantize_u8 + cos_prepare, corpus": lambda: f16_prepare(frames, minmax),
        "b  cosq_prepare, corpus": lambda: K.cosq_prepare(frames, minmax, n),
        "a  dequantize_u8 + cos_prepare, query batch": lambda: f16_prepare(qframes, qminmax),
        "b  cosq_prepare, query batch": lambda: K.cosq_prepare(qframes, qminmax, n)}
for name, fn in prep.items():
    fn()
    torch.cuda.synchronize()
    line(name, [timed(fn) for _ in range(max(3, args.reps // 2))])
pc16, pq16 = f16_prepare(frames, minmax), f16_prepare(qframes, qminmax)
pc8, pq8 = K.cosq_prepare(frames, minmax, n), K.cosq_prepare(qframes, qminmax, n)
b16 = pc16.X16.numel() * 2 + pc16.inv.numel() * 8
b8 = pc8.nbytes
print(f"resident corpus: (a) split-f16 fragments + inverse norms {b16} B = {b16 / 2 ** 30:.3f} GiB; "
      f"(b) signed bytes + statistics {b8} B = {b8 / 2 ** 30:.3f} GiB ({b16 / b8:.2f}x less); "
      f"the u8 store itself {frames.numel() + minmax.numel() * 4} B", flush=True)

# the dense int8 GEMM (float64 score stores included) and the dense split-f16 one
sc = K.cosq_scores(pq8, pc8)
torch.cuda.synchronize()
del sc
d8 = line("b  cosq_scores (dense [Q, N] f64)", [timed(lambda: K.cosq_scores(pq8, pc8)) for _ in range(args.reps)])
d16 = line("a  cosine_scores_mfma (dense [Q, N] f64)", [timed(lambda: K.cosine_scores_mfma(pq16, pc16)) for _ in range(args.reps)])
ops = 2.0 * Q * N * Kd
print(f"int8 GEMM: {ops / d8 / 1e12:.1f} TOP/s = {ops / d8 / 1e12 / I8_PEAK_TOPS:.3f} of the int8 ceiling "
      f"({I8_PEAK_TOPS:.0f} TOP/s); split-f16 GEMM: {ops / d16 / 1e12:.1f} TFLOP/s algorithmic = "
      f"{3 * ops / d16 / 1e12 / 2500.0:.3f} of the f16 ceiling at three MFMAs per block", flush=True)

for k in args.k:
    limit = 1 << 40  # one query block

    def route_a():
        return K.cosine_topk(pq16, pc16, k, workspace_limit=limit)

    def route_b():
        return K.cosq_topk(pq8, pc8, k, workspace_limit=limit)

    VARIANTS = [("a  cosine_topk on the decoded store", route_a), ("b  cosq_topk on the u8 store", route_b)]
    ra, rb = route_a(), route_b()
    want = K.select_topk(K.cosq_scores(pq8, pc8), k)[:2]
    assert torch.equal(rb[1], want[1]) and torch.equal(rb[0].view(torch.int64), want[0].view(torch.int64)), \
        "cosq_topk differs from select_topk(cosq_scores)"
    # (a) scores the same frames within the split-f16 bound; where the lists differ, the scores at that rank do not
    same = float((ra[1] == rb[1]).double().mean())
    gap = float((ra[0] - rb[0]).abs().max())
    assert gap < 1e-5, gap
    print(f"-- k = {k}: (b) bit-identical to select_topk(cosq_scores); (a) lists the same id at {same * 100:.2f} % of the "
          f"positions, largest score difference at equal rank {gap:.2e}")
    del ra, rb, want
    for _ in range(args.warmup):
        for _, fn in VARIANTS:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in VARIANTS}
    for _ in range(args.reps):
        for name, fn in VARIANTS:
            times[name].append(timed(fn))
    a, b = (line(name, times[name]) for name, _ in VARIANTS)
    spread = max(max(t) - min(t) for t in times.values())
    print(f"(a) / (b): {a / b:5.3f}x   (a) - (b) = {(a - b) * 1e3:.3f} ms, largest spread of the repetitions "
          f"{spread * 1e3:.3f} ms", flush=True)
