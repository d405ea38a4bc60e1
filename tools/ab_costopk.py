#!/usr/bin/env python3
"""Fused frame-cosine top-k against the dense route, device resident, one process.

(a)  K.cosine_scores_mfma (the [Q, N] float64 matrix) + K.select_topk: what a frame ranking cost before
     hq_cos_topk, with the corpus already prepared (a1 / a2: the two halves on their own);
(b)  K.cosine_topk with the running threshold between tiles (option cos_topk_hint 1);
(b') the same without it (cos_topk_hint 0).

Every variant runs once per repetition, in turn (a, b, b', a, ...), each between two HIP events on the launch
stream, after warm-up rounds of every variant; the outputs are compared bit for bit first.  Prints the median
(min - max) per variant, the kernel times of the fused call's two stages (k_cos_t's top-k epilogue form and
k_cos_topk_merge, from the profiler's kernel records of one extra call), and the workspace bytes against the
Q N 8 bytes of the score matrix.

usage: ab_costopk.py [--queries 1000] [--frames 250000] [--K 4096] [--k 10 64] [--reps 9] [--warmup 2]
Needs an MI355X."""
import argparse
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--queries", type=int, default=1000)
ap.add_argument("--frames", type=int, default=250_000)
ap.add_argument("--K", type=int, default=4096)
ap.add_argument("--k", type=int, nargs="+", default=[10, 64])
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--no-kernel-times", action="store_true")
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hilbert-quantization_amd")]

import torch  # noqa: E402
from hq_mi355x import _lib, kernels as K  # noqa: E402

assert torch.cuda.is_available(), "ab_costopk.py needs the GPU"
Q, N, Kd = args.queries, args.frames, args.K

g = torch.Generator(device="cuda").manual_seed(0)
frames = torch.randn((N, Kd), generator=g, dtype=torch.float32, device="cuda")
queries = frames[torch.randint(0, N, (Q,), generator=g, device="cuda")] + \
    0.5 * torch.randn((Q, Kd), generator=g, dtype=torch.float32, device="cuda")
pc = K.cos_prepare(frames)
pq = K.cos_prepare(queries)
del frames, queries
print(f"== frame cosine top-k A/B: {Q} queries x {N} frames x K = {Kd}, {args.reps} alternating repetitions after "
      f"{args.warmup} warm-up rounds, HIP events; {torch.cuda.get_device_name(0)} ==", flush=True)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    del r
    return e0.elapsed_time(e1) * 1e-3


for k in args.k:
    limit = 1 << 40  # one query block: the whole workspace is reported

    def dense():
        return K.select_topk(K.cosine_scores_mfma(pq, pc), k)[:2]

    def fused(hint):
        def run():
            with _lib.option("cos_topk_hint", hint):
                return K.cosine_topk(pq, pc, k, workspace_limit=limit)
        return run

    VARIANTS = [("a  cosine_scores_mfma + select_topk", dense),
                ("b  cosine_topk, hint on", fused(1)),
                ("b' cosine_topk, hint off", fused(0))]
    # same bits first (and the first launches: code objects, allocator blocks)
    ref = dense()
    for name, fn in VARIANTS[1:]:
        got = fn()
        assert torch.equal(got[1], ref[1]) and torch.equal(got[0].view(torch.int64), ref[0].view(torch.int64)), name
    del ref, got
    for _ in range(args.warmup):
        for _, fn in VARIANTS:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in VARIANTS}
    halves = {"a1 cosine_scores_mfma alone": [], "a2 select_topk alone": []}
    for _ in range(args.reps):
        for name, fn in VARIANTS:
            times[name].append(timed(fn))
        sc = K.cosine_scores_mfma(pq, pc)
        halves["a1 cosine_scores_mfma alone"].append(timed(lambda: K.cosine_scores_mfma(pq, pc)))
        halves["a2 select_topk alone"].append(timed(lambda: K.select_topk(sc, k)))
        del sc
    ws = int(_lib.load().hq_cos_topk_workspace_size(Q, N, k))
    print(f"-- k = {k}: outputs bit-identical; workspace {ws} B = {ws / 2 ** 20:.1f} MiB against Q N 8 = "
          f"{Q * N * 8} B = {Q * N * 8 / 2 ** 20:.1f} MiB ({Q * N * 8 / ws:.1f}x)")
    med = {}
    for name, ts in list(times.items()) + list(halves.items()):
        med[name] = statistics.median(ts)
        print(f"{name:<40} median {med[name] * 1e3:9.3f} ms  (min {min(ts) * 1e3:9.3f} - max {max(ts) * 1e3:9.3f})")
    a, b, b0 = (med[n] for n, _ in VARIANTS)
    print(f"(a) / (b): {a / b:5.3f}x   (a) / (b'): {a / b0:5.3f}x   (b') / (b): {b0 / b:5.3f}x (> 1: the hint is faster)",
          flush=True)
    if not args.no_kernel_times:
        # the two stages of one fused call per hint setting, from the profiler's kernel records
        from torch.profiler import ProfilerActivity, profile
        for hint in (1, 0):
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fused(hint)()
                torch.cuda.synchronize()
            rows = [(e.key, e.count, getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0))
                    for e in prof.key_averages()
                    if "k_cos_t" in e.key or "k_cos_topk_merge" in e.key]
            for key, cnt, us in rows:
                stage = "stage 2 k_cos_topk_merge" if "merge" in key else "stage 1 k_cos_t<3, 1, 1, 4>"
                print(f"hint {hint}: {stage:<28} {cnt} launch(es), {us * 1e-3:9.3f} ms in all", flush=True)
