#!/usr/bin/env python3
"""Remove / replace against rebuild: what editing a resident corpus costs.

One process; the variants of a comparison alternate inside one loop; medians of host-clock times with a
device synchronise before each clock read; every variant's output is compared bit for bit with the others'
before anything is timed.

(a) Registry search: HilbertQuantizer.search(q) over a registry of N models (L = 64) straight after one
    remove_model_from_registry, with shrink_resident off (the resident corpus is rebuilt) and on (one gather,
    one append).  Per call: the search alone (the removal is outside the clock).
(b) IndexCorpus.remove of 1 row, 1,000 rows and half the rows of N resident rows against
      (i)   a fresh IndexCorpus of the surviving rows from a host array (the host gather of the rows not timed),
      (ii)  a fresh IndexCorpus from the surviving rows already on the device (their device gather not timed),
      (iii) the unfused device sequence Prepared.rows(sel) + flag_rows (three index_select copies, two pack
            launches, one list launch).
    Also kernels.seg_gather alone with the row numbers already on the device (allocations + the one launch),
    which is what the bandwidth figure of DESIGN 4.10 is taken from.
(c) IndexCorpus.replace of 1 row and of 1,000 rows against a fresh IndexCorpus of the updated host rows.

usage: ab_remove.py [--registry 10000,100000] [--sizes 100000,1000000] [--replace 100000] [--calls 10] [--reps 7]
Needs an MI355X; prints one block of lines (profiles/remove_vs_rebuild.txt)."""
import argparse
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--registry", default="10000,100000")
ap.add_argument("--sizes", default="100000,1000000")
ap.add_argument("--replace", default="100000")
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--reps", type=int, default=7)
args = ap.parse_args()
TREE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [TREE, os.path.join(TREE, "hilbert-quantization_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
from hq_mi355x import kernels as K  # noqa: E402
from hq_mi355x._dev import to_dev, to_np  # noqa: E402
from hq_mi355x.api import HilbertQuantizer  # noqa: E402
from hq_mi355x.core.search_engine import IndexCorpus  # noqa: E402
from hq_mi355x.models import ModelMetadata, QuantizedModel  # noqa: E402

assert torch.cuda.is_available(), "ab_remove.py needs the GPU"
L, D = 64, 4096  # a 64 x 64 parameter image gives index vectors of 64 values


def sync():
    torch.cuda.synchronize()


def ms(xs):
    return f"median {statistics.median(xs) * 1e3:9.3f} ms  (min {min(xs) * 1e3:9.3f}, max {max(xs) * 1e3:9.3f}, n={len(xs)})"


def timed(fn):
    sync()
    t0 = time.perf_counter()
    out = fn()
    sync()
    return time.perf_counter() - t0, out


def ints(s):
    return [int(v) for v in s.split(",") if v]


def same_bytes(a, b, what):
    """Every layout of the Prepared a equals that of b over the valid extents of their N rows (hq_mi355x.h);
    the flagged-row lists as sets."""
    N = b.N
    assert a.N == N and (a.f32, a.all32) == (b.f32, b.all32), what
    r16, r4 = (N + 15) // 16 * 16 + K.PAD0, (N + 3) // 4 * 4 + K.PAD0
    for name, rows in (("R", N), ("Z", N), ("S", N), ("Z16", r16), ("S32", r4), ("Zov16", r16), ("Sov32", r4 // 4)):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), (what, name)
        if y is not None:
            assert torch.equal(x[:rows].view(torch.uint8), y[:rows].view(torch.uint8)), (what, name)
    fa, fb = to_np(a.F0), to_np(b.F0)
    assert fa[0] == fb[0] and sorted(fa[1:1 + fa[0]]) == sorted(fb[1:1 + fb[0]]), (what, "F0")


# ---- (a) -----------------------------------------------------------------------------------------
def registry(n, seed):
    rng = np.random.default_rng(seed)
    C = rng.standard_normal((n, L)) * 0.05
    return [QuantizedModel(b"x", (L, L), D, 0.8, C[i].copy(), ModelMetadata(f"m{i}", 4 * D, 1, 1.0, "t"))
            for i in range(n)]


def registry_search(n):
    hqs = {}
    for name, on in (("rebuild (switch off)", False), ("shrink  (switch on) ", True)):
        hq = HilbertQuantizer(use_precomputed_indexing=False, shrink_resident=on)
        hq._model_registry.extend(registry(n, n))
        hqs[name] = hq
    rng = np.random.default_rng(1)
    qs = (rng.standard_normal((3 + args.calls, D)) * 0.02).astype(np.float32)
    ts = {name: [] for name in hqs}
    victims = np.random.default_rng(2).choice(np.arange(n // 4, 3 * n // 4), len(qs), replace=False)
    for i, q in enumerate(qs):
        outs = []
        for name, hq in hqs.items():
            if i >= 2:  # two plain warm-up calls (code objects, the first build), then one removal before every call
                assert hq.remove_model_from_registry(f"m{victims[i]}")
            dt, res = timed(lambda: hq.search(q))
            assert res and res[0].model is hq._model_registry[-1]
            pos = {id(m): j for j, m in enumerate(hq._model_registry)}  # the two registries hold equal rows in order
            outs.append([(pos[id(r.model)], r.similarity_score) for r in res])
            if i >= 3:
                ts[name].append(dt)
        assert outs[0] == outs[1], "the two variants answer differently"
    for name, hq in hqs.items():
        eng = hq.search_engine
        print(f"registry search after one removal  N={n:>7}  {name}  per call {ms(ts[name])}  "
              f"pool_stats={eng.pool_stats} shrinks={eng.pool_shrinks}")


# ---- (b) -----------------------------------------------------------------------------------------
def remove_vs_build(n):
    rng = np.random.default_rng(n + 7)
    C = rng.standard_normal((n, L)) * 0.05
    C[rng.choice(n, 50, replace=False)] = 0.25  # a few flagged rows, so the lists are not empty
    IndexCorpus(C[:1000]).progressive(C[:4], 10, 0.1, 20)  # warm-up
    corpus = IndexCorpus(C)
    prep0 = corpus.prep
    nseg, Lp = prep0.nseg, prep0.Lp
    for m in (1, 1000, n // 2):
        gone = np.sort(rng.choice(n, m, replace=False))
        keep = np.setdiff1d(np.arange(n), gone)
        host_rows = np.ascontiguousarray(C[keep])
        sel = to_dev(keep)
        dev_rows = prep0.R.index_select(0, sel)

        def v_remove():
            corpus.prep, corpus.N = prep0, n  # remove gathers out of place: the full corpus is still there
            corpus.remove(gone)
            return corpus.prep

        variants = [
            ("IndexCorpus.remove", v_remove),
            ("(i)   fresh corpus, host rows", lambda: IndexCorpus(host_rows).prep),
            ("(ii)  fresh corpus, device rows", lambda: IndexCorpus(dev_rows).prep),
            ("(iii) Prepared.rows + flag_rows", lambda: K.flag_rows(prep0.rows(sel))),
            ("kernels.seg_gather alone", lambda: K.seg_gather(prep0, sel, checked=True)),
        ]
        outs = [fn() for _, fn in variants]
        sync()
        for (name, _), o in zip(variants[1:], outs[1:]):
            same_bytes(outs[0], o, name)
        del outs
        ts = {name: [] for name, _ in variants}
        for _ in range(args.reps):
            for name, fn in variants:
                dt, out = timed(fn)
                ts[name].append(dt)
                del out
        print(f"-- remove {m} of N={n} rows ({len(keep)} survive)")
        for name, _ in variants:
            print(f"   {name:<34} {ms(ts[name])}")
        # algorithmic traffic of the gather per surviving row: the row number read, R, Z, S read
        # and written, the split copies and their statistics written
        per_row = 8 + 2 * 8 * (L + Lp + 4 * nseg) + 2 * 2 * 32 + 16 + (prep0.Zov16.shape[1] * 2) + prep0.Sov32.shape[1]
        t = statistics.median(ts["kernels.seg_gather alone"])
        print(f"   gather traffic {per_row} B/row x {len(keep)} rows = {per_row * len(keep) / 1e6:.1f} MB -> "
              f"{per_row * len(keep) / t / 1e12:.3f} TB/s of 8 TB/s ({per_row * len(keep) / t / 8e12 * 100:.1f} %)")
    corpus.prep, corpus.N = prep0, n


# ---- (c) -----------------------------------------------------------------------------------------
def replace_vs_build(n):
    rng = np.random.default_rng(n + 11)
    C = rng.standard_normal((n, L)) * 0.05
    corpus = IndexCorpus(C)
    corpus.replace([0], C[:1])  # the one-off move into the corpus's own buffers
    for m in (1, 1000):
        rows = np.sort(rng.choice(n, m, replace=False))
        new = rng.standard_normal((m, L)) * 0.05
        new[::7] = 0.5
        C2 = C.copy()
        C2[rows] = new
        corpus.replace(rows, new)
        same_bytes(corpus.prep, IndexCorpus(C2).prep, "replace")
        tr, tb = [], []
        for _ in range(args.reps):
            tr.append(timed(lambda: corpus.replace(rows, new))[0])
            dt, fresh = timed(lambda: IndexCorpus(C2))
            tb.append(dt)
            del fresh
        print(f"-- replace {m} of N={n} rows")
        print(f"   {'IndexCorpus.replace':<34} {ms(tr)}")
        print(f"   {'fresh corpus, host rows':<34} {ms(tb)}")
        corpus.replace(rows, C[rows])


print(f"== remove / replace against rebuild, L = {L} ==")
for n in ints(args.registry):
    registry_search(n)
for n in ints(args.sizes):
    remove_vs_build(n)
for n in ints(args.replace):
    replace_vs_build(n)
