#!/usr/bin/env python3
"""Append against rebuild: what growing a resident corpus costs.

1. Registry search: HilbertQuantizer.search(q) over a registry of N models (L = 64).  Every call quantizes
   its query into the registry first, so the pool grows by one row per call; the per-call wall time
   (the call ends in a device-to-host copy of the results, so the host clock sees the whole search).
2. IndexCorpus.append of M = 1, 1,000 and N rows to a resident corpus of N rows against a fresh
   IndexCorpus of the N + M rows, both from host arrays, a device synchronise before each clock read.

usage: ab_append.py [--tree DIR] [--sizes 10000,100000] [--calls 20] [--reps 5]
  --tree DIR   measure the checkout at DIR (with its library built) instead of this one: the parent commit
               for an A/B.  A tree without IndexCorpus.append reports its part 2 appends as n/a.
Needs an MI355X; prints one block of lines (append the blocks of both commits to a profile file)."""
import argparse
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--sizes", default="10000,100000")
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--label", default=None)
args = ap.parse_args()
TREE = os.path.abspath(args.tree)
sys.path[:0] = [TREE, os.path.join(TREE, "hilbert-quantization_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
from hq_mi355x.api import HilbertQuantizer  # noqa: E402
from hq_mi355x.core.search_engine import IndexCorpus  # noqa: E402
from hq_mi355x.models import ModelMetadata, QuantizedModel  # noqa: E402

assert torch.cuda.is_available(), "ab_append.py needs the GPU"
L, D = 64, 4096  # a 64 x 64 parameter image gives index vectors of 64 values
HAS_APPEND = hasattr(IndexCorpus, "append")


def sync():
    torch.cuda.synchronize()


def ms(xs):
    return f"median {statistics.median(xs) * 1e3:9.3f} ms  (min {min(xs) * 1e3:9.3f}, max {max(xs) * 1e3:9.3f}, n={len(xs)})"


def registry(n, seed):
    rng = np.random.default_rng(seed)
    C = rng.standard_normal((n, L)) * 0.05
    return [QuantizedModel(b"x", (L, L), D, 0.8, C[i].copy(), ModelMetadata(f"m{i}", 4 * D, 1, 1.0, "t"))
            for i in range(n)]


def registry_search(n):
    hq = HilbertQuantizer(use_precomputed_indexing=False)
    hq._model_registry.extend(registry(n, n))
    rng = np.random.default_rng(1)
    qs = (rng.standard_normal((3 + args.calls, D)) * 0.02).astype(np.float32)
    ts = []
    for i, q in enumerate(qs):
        sync()
        t0 = time.perf_counter()
        res = hq.search(q)
        sync()
        t1 = time.perf_counter()
        assert res and res[0].model is hq._model_registry[-1]
        if i >= 3:  # three warm-up calls: code objects, the first build, pinned buffers
            ts.append(t1 - t0)
    stats = getattr(hq.search_engine, "pool_stats", None)
    print(f"registry search  N={n:>7}  per call {ms(ts)}  pool_stats={stats}")


def append_vs_build(n):
    rng = np.random.default_rng(n + 7)
    C = rng.standard_normal((2 * n, L)) * 0.05
    IndexCorpus(C[:1000]).progressive(C[:4], 10, 0.1, 20)  # warm-up
    for m in (1, 1000, n):
        tb, ta = [], []
        for _ in range(args.reps):
            sync()
            t0 = time.perf_counter()
            fresh = IndexCorpus(C[:n + m])
            sync()
            tb.append(time.perf_counter() - t0)
            del fresh
            if HAS_APPEND:
                corpus = IndexCorpus(C[:n])
                sync()
                t0 = time.perf_counter()
                corpus.append(C[n:n + m])
                sync()
                ta.append(time.perf_counter() - t0)
                del corpus
        print(f"fresh build      N+M={n + m:>7}           {ms(tb)}")
        print(f"append           N={n:>7} M={m:>7}   " + (ms(ta) if ta else "n/a (no IndexCorpus.append)"))
    if HAS_APPEND:  # steady state of one-row appends (reallocations included)
        corpus = IndexCorpus(C[:n])
        corpus.append(C[n:n + 1])
        sync()
        t0 = time.perf_counter()
        for i in range(1, 201):
            corpus.append(C[n + i:n + i + 1])
        sync()
        print(f"append           N={n:>7} M=1 x 200 in a row: {(time.perf_counter() - t0) / 200 * 1e3:9.3f} ms per call")


print(f"== {args.label or TREE}  (IndexCorpus.append: {'yes' if HAS_APPEND else 'no'}) ==")
for n in (int(s) for s in args.sizes.split(",")):
    registry_search(n)
for n in (int(s) for s in args.sizes.split(",")):
    append_vs_build(n)
