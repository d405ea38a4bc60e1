#!/usr/bin/env python3
"""Mutating the resident u8 frame corpus against rebuilding it.

On a resident rag.QuantizedFrameCorpus of N = 250,000 frames of 65 x 64 bytes (searched on 64 rows: K = 4096), in one
process, each of
  append of M = 1, 1,000 and 100,000 frames (capacity reserved ahead; M = 1,000 also with the reallocation it causes
  on a corpus built to size), 200 single-frame appends in a row from a corpus built to size (one reallocation among
  them), remove of 1 row and of 1 % of the rows, replace of 1 and 1,000 rows, insert of 1 frame
is timed against the only way a tree without the mutable store has: kernels.cosq_prepare of the resulting frames,
which needs the raw store resident next to the operand (the raw frames of the result are laid out before the clock
starts, so the rebuild is charged its kernel and its output allocation only).  Every timed call starts from a freshly
built corpus (built, and reserved where stated, before the clock starts) and runs between two device synchronises on
the host's wall clock.  After the last repetition of every operation the mutated operand is compared with the rebuilt
one (torch.equal on the padded rows of X8 and on the bits of stats).  One search row (kernels.cosq_topk, k = 10, 1000
queries) runs on a mutated corpus and on a fresh one of the same frames.

usage: ab_cosq_store.py [--n 250000] [--reps 7] [--label TEXT]
Needs an MI355X; prints one block of lines (profiles/cosq_store_vs_rebuild.txt holds two runs)."""
import argparse
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=250_000)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--label", default=None)
args = ap.parse_args()
TREE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [TREE, os.path.join(TREE, "hilbert-quantization_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
from hq_mi355x import kernels as K, rag  # noqa: E402

assert torch.cuda.is_available(), "ab_cosq_store.py needs the GPU"
N, n, WARM = args.n, 64, 2
BIG = min(100_000, N)


def sync():
    torch.cuda.synchronize()


def ms(xs):
    return f"median {statistics.median(xs) * 1e3:9.3f} ms  (min {min(xs) * 1e3:9.3f}, max {max(xs) * 1e3:9.3f}, n={len(xs)})"


def padded(rows):
    return (rows + 127) // 128 * 128


gen = torch.Generator(device="cuda").manual_seed(1)
F = torch.randint(0, 256, (N + BIG + 256, n + 1, n), dtype=torch.uint8, device="cuda", generator=gen)
lo = torch.rand(F.shape[0], device="cuda", generator=gen) * 3 - 2
MM = torch.stack([lo, lo + 0.1 + 3 * torch.rand(F.shape[0], device="cuda", generator=gen)], dim=1).float()


def timed(label, mutate, result, reserve=0):
    """mutate(corpus) on a fresh corpus of the first N frames, `reps` times after WARM warm-ups, against
    cosq_prepare of result() = (frames, minmax) of the corpus it leaves."""
    rF, rM = result()
    ta, tb = [], []
    for i in range(WARM + args.reps):
        c = rag.QuantizedFrameCorpus(F[:N], MM[:N])
        if reserve:
            c.reserve(reserve)
        sync()
        t0 = time.perf_counter()
        mutate(c)
        sync()
        t1 = time.perf_counter()
        fresh = K.cosq_prepare(rF, rM, n)
        sync()
        t2 = time.perf_counter()
        if i >= WARM:
            ta.append(t1 - t0)
            tb.append(t2 - t1)
        if i == WARM + args.reps - 1:
            rows = padded(fresh.N)
            same = c.N == fresh.N and torch.equal(c._rows.X8[:rows], fresh.X8[:rows]) and \
                torch.equal(c._rows.stats[:rows].view(torch.int64), fresh.stats[:rows].view(torch.int64))
        del c, fresh
    print(f"{label:<44} {ms(ta)}  identical to the rebuild: {'yes' if same else 'NO'}")
    print(f"{'  rebuild: cosq_prepare of ' + str(rF.shape[0]) + ' frames':<44} {ms(tb)}")


def cat(*parts):
    return torch.cat([F[a:b] for a, b in parts]), torch.cat([MM[a:b] for a, b in parts])


print(f"== {args.label or TREE}  N={N} frames of {n + 1} x {n}, K={n * n}, reps={args.reps} after {WARM} warm-ups ==")
for M in (1, 1000, BIG):
    timed(f"append M={M} (capacity reserved)", lambda c, M=M: c.append(F[N:N + M], MM[N:N + M]),
          lambda M=M: (F[:N + M], MM[:N + M]), reserve=N + BIG)
timed("append M=1000 (built to size: reallocation)", lambda c: c.append(F[N:N + 1000], MM[N:N + 1000]),
      lambda: (F[:N + 1000], MM[:N + 1000]))

c = rag.QuantizedFrameCorpus(F[:N], MM[:N])
c.append(F[N:N + 1], MM[N:N + 1])
sync()
t0 = time.perf_counter()
for i in range(1, 201):
    c.append(F[N + i:N + i + 1], MM[N + i:N + i + 1])
sync()
per = (time.perf_counter() - t0) / 200
fresh = K.cosq_prepare(F[:N + 201], MM[:N + 201], n)
rows = padded(N + 201)
same = torch.equal(c._rows.X8[:rows], fresh.X8[:rows]) and \
    torch.equal(c._rows.stats[:rows].view(torch.int64), fresh.stats[:rows].view(torch.int64))
print(f"{'append M=1 x 200 in a row':<44} {per * 1e3:9.3f} ms per call  identical to the rebuild: {'yes' if same else 'NO'}")
del c, fresh

one = N // 2
timed("remove 1 row", lambda c: c.remove([one]), lambda: cat((0, one), (one + 1, N)))
drop = np.random.default_rng(2).choice(N, N // 100, replace=False)
keep = torch.from_numpy(np.setdiff1d(np.arange(N), drop)).cuda()
timed(f"remove {drop.size} rows (1 %)", lambda c: c.remove(drop), lambda: (F[:N][keep], MM[:N][keep]))
# the launch alone: the survivors' row numbers already on the device (remove() builds them on the host and uploads them)
src = K.cosq_prepare(F[:N], MM[:N], n)
ts = []
for i in range(WARM + args.reps):
    sync()
    t0 = time.perf_counter()
    g = K.cosq_gather(src, keep, checked=True)
    sync()
    if i >= WARM:
        ts.append(time.perf_counter() - t0)
    del g
print(f"{'  kernels.cosq_gather, device row numbers':<44} {ms(ts)}")
del src


def replaced(rows):
    rF, rM = F[:N].clone(), MM[:N].clone()
    idx = torch.from_numpy(rows).cuda()
    rF[idx], rM[idx] = F[N:N + rows.size], MM[N:N + rows.size]
    return rF, rM


for M in (1, 1000):
    rows = np.random.default_rng(3).choice(N, M, replace=False)
    timed(f"replace {M} row{'s' if M > 1 else ''}", lambda c, rows=rows, M=M: c.replace(rows, F[N:N + M], MM[N:N + M]),
          lambda rows=rows: replaced(rows))
timed("insert 1 frame", lambda c: c.insert(one, F[N:N + 1], MM[N:N + 1]), lambda: cat((0, one), (N, N + 1), (one, N)))

# the search does not care how the corpus was built
c = rag.QuantizedFrameCorpus(F[:N], MM[:N])
c.append(F[N:N + 1000], MM[N:N + 1000])
c.remove(drop)
c.insert(one, F[N + 1000:N + 1001], MM[N + 1000:N + 1001])
cur = torch.cat([keep, torch.arange(N, N + 1000, device="cuda")])
cur = torch.cat([cur[:one], torch.tensor([N + 1000], device="cuda"), cur[one:]])
fresh = K.cosq_prepare(F[cur], MM[cur], n)
q = K.cosq_prepare(F[N + BIG:N + BIG + 250].repeat(4, 1, 1), MM[N + BIG:N + BIG + 250].repeat(4, 1), n)
out = {}
for name, rows_ in (("mutated", c._rows), ("fresh", fresh)):
    ts = []
    for i in range(WARM + 5):
        sync()
        t0 = time.perf_counter()
        out[name] = K.cosq_topk(q, rows_, 10)
        sync()
        if i >= WARM:
            ts.append(time.perf_counter() - t0)
    print(f"{'cosq_topk k=10 Q=1000 on the ' + name + ' corpus (N=' + str(rows_.N) + ')':<58} {ms(ts)}")
print("search results identical (ids and score bits): " + ("yes" if torch.equal(out["mutated"][1], out["fresh"][1]) and
      torch.equal(out["mutated"][0].view(torch.int64), out["fresh"][0].view(torch.int64)) else "NO"))
